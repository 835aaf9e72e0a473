// C-ABI entry points that touch the device (declared in include/koemorph.h).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <cstring>
#include <vector>

#include "km_context.h"
#include "km_device.h"
#include "km_gemm.h"

using namespace km;

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                                                                        \
            (void)hipGetLastError(); /* the runtime keeps a failed call as its last error: do not leave it to the next launch check */ \
            return fail(KM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));                                                           \
        }                                                                                                                              \
    } while (0)

static int free_streams(Context* c);
static int free_train(Context* c);
static int free_pipeline(Context* c);
static int free_legacy_streams(Context* c);

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int need_ready(Context* c) {
    if (!c) return fail(KM_ERR_INVALID_ARG, "NULL handle");
    if (!c->dev_finalized) return fail(KM_ERR_NOT_FINALIZED, "call km_finalize after loading the state dict");
    return KM_OK;
}

static int need_dual(Context* c) {
    if (int rc = need_ready(c)) return rc;
    if (c->kind != 0) return fail(KM_ERR_INVALID_ARG, "this entry point needs a dual-stream handle (km_create), not a legacy one");
    return KM_OK;
}

static int need_legacy_train(Context* c, int64_t B) {
    if (int rc = need_ready(c)) return rc;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "this entry point needs a legacy handle (km_legacy_create)");
    if (!c->tr_params || !c->ltr_ws) return fail(KM_ERR_NOT_FINALIZED, "call km_legacy_train_init first");
    if (B <= 0 || B > c->tr_windows) return fail(KM_ERR_WORKSPACE, "km_legacy_train_init sized the step for %lld windows, got %lld",
                                                 (long long)c->tr_windows, (long long)B);
    return KM_OK;
}

namespace km { LogParams plan_log_params(MelPlan* p); }

extern "C" {

int km_finalize(km_handle h, void* stream) {
    if (!h) return fail(KM_ERR_INVALID_ARG, "NULL handle");
    Context* c = h;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(KM_ERR_HIP, "no HIP device: libkoemorph_hip has no CPU fallback");
    HIP_TRY(hipGetDevice(&c->device));
    if (!c->host_finalized)
        if (int rc = finalize_host(c)) return rc;
    for (auto& kv : c->packed) {
        Packed& p = kv.second;
        if (!p.dev) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p.dev), p.host.size() * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(p.dev, p.host.data(), p.host.size() * sizeof(float), hipMemcpyHostToDevice,
                               (hipStream_t)stream));
    }
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (MelPlan* p : c->mel_plans)
        if (int rc = upload_mel_plan(p)) return rc;
    if (c->kind != 2)                                   // the front end's chunk counters exist before any launch could be captured
        if (int rc = ensure_chunk_counters(c, 4096, stream)) return rc;
    c->dev_finalized = true;
    return KM_OK;
}

static int free_ws(Context* c) {
    if (c->ws_zemo) HIP_TRY(hipFree(c->ws_zemo));
    if (c->ws_zemo_win) HIP_TRY(hipFree(c->ws_zemo_win));
    if (c->ws_melpow) HIP_TRY(hipFree(c->ws_melpow));
    if (c->ws_melmax) HIP_TRY(hipFree(c->ws_melmax));
    if (c->ws_mel) HIP_TRY(hipFree(c->ws_mel));
    if (c->ws_short) HIP_TRY(hipFree(c->ws_short));
    if (c->ws_generic) HIP_TRY(hipFree(c->ws_generic));
    c->ws_zemo = c->ws_zemo_win = c->ws_melpow = c->ws_mel = c->ws_short = c->ws_generic = nullptr;
    c->ws_melmax = nullptr;
    c->ws_windows = c->ws_samples = c->ws_frames = 0;
    c->ws_mels = 0;
    return KM_OK;
}

int km_reserve(km_handle h, int64_t max_windows, int64_t max_samples) {
    if (!h || max_windows <= 0 || max_samples < 0) return fail(KM_ERR_INVALID_ARG, "km_reserve: bad argument");
    Context* c = h;
    if (c->kind == 2) return fail(KM_ERR_INVALID_ARG, "KoeMorphModel handles take no audio: use km_koemorph_reserve");
    // frames for the smallest hop among the registered plans (upper bound for all of them)
    int min_hop = c->cfg.mel.hop_length, max_mels = c->cfg.mel.n_mels;
    for (MelPlan* p : c->mel_plans) {
        if (p->cfg.hop_length < min_hop) min_hop = p->cfg.hop_length;
        if (p->cfg.n_mels > max_mels) max_mels = p->cfg.n_mels;
    }
    const int64_t frames = max_samples > 0 ? 1 + max_samples / min_hop : 0;
    const bool need_generic = c->host_finalized && !c->fused_ok;
    if (max_windows <= c->ws_windows && frames <= c->ws_frames && max_mels <= c->ws_mels && (c->ws_generic || !need_generic)) return KM_OK;
    const int64_t W = max_windows > c->ws_windows ? max_windows : c->ws_windows;
    const int64_t F = frames > c->ws_frames ? frames : c->ws_frames;
    const int64_t S = max_samples > c->ws_samples ? max_samples : c->ws_samples;
    if (int rc = free_ws(c)) return rc;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ws_zemo), (size_t)W * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ws_zemo_win), (size_t)W * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ws_melmax), (size_t)W * sizeof(unsigned)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ws_short), (size_t)W * 3 * max_mels * sizeof(float)));
    if (F > 0) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ws_melpow), (size_t)W * F * max_mels * sizeof(float)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ws_mel), (size_t)W * F * max_mels * sizeof(float)));
    }
    if (need_generic) {
        const int64_t per = c->kind == 1 ? legacy_ws_floats(c, F > 0 ? F : 1) : generic_ws_floats(c);
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ws_generic), (size_t)W * per * sizeof(float)));
    }
    c->ws_windows = W; c->ws_frames = F; c->ws_samples = S; c->ws_mels = max_mels;
    c->melmax_dirty = true;
    return ensure_chunk_counters(c, W, nullptr);
}

int km_destroy(km_handle h) {
    if (!h) return KM_OK;
    Context* c = h;
    for (auto& kv : c->packed)
        if (kv.second.dev) (void)hipFree(kv.second.dev);
    (void)free_ws(c);
    if (c->ws_chunkctr) (void)hipFree(c->ws_chunkctr);
    (void)free_streams(c);
    (void)free_legacy_streams(c);
    (void)free_train(c);
    (void)free_pipeline(c);
    for (void* q : {(void*)c->seq_pow, (void*)c->seq_fmax, (void*)c->seq_edge, (void*)c->seq_emax, (void*)c->seq_ztrack, (void*)c->seq_zwin, (void*)c->seq_attn, (void*)c->fwd_span, (void*)c->fwd_edge})
        if (q) (void)hipFree(q);
    if (c->pipe_s1) {
        (void)hipStreamDestroy((hipStream_t)c->pipe_s1); (void)hipStreamDestroy((hipStream_t)c->pipe_s2);
        for (int i = 0; i < 2; ++i) {
            (void)hipEventDestroy((hipEvent_t)c->pipe_ev_in[i]); (void)hipEventDestroy((hipEvent_t)c->pipe_ev_mel[i]);
            (void)hipEventDestroy((hipEvent_t)c->pipe_ev_core[i]);
        }
    }
    for (MelPlan* p : c->mel_plans) free_mel_plan(p);
    for (void* e : c->stage_ev)
        if (e) (void)hipEventDestroy((hipEvent_t)e);
    delete h;
    return KM_OK;
}

int64_t km_mel_num_frames(km_handle h, int64_t L) {
    if (!h || L < 0) return -1;
    return 1 + L / h->cfg.mel.hop_length;    // librosa center=True: 1 + len(y) // hop
}

int km_mel_batch(km_handle h, const float* audio_dev, int64_t B, int64_t L, float* mel_long_dev,
                 float* mel_short_dev, void* stream) {
    if (int rc = need_ready(h)) return rc;
    if (!audio_dev || !mel_long_dev || B <= 0 || L <= 0) return fail(KM_ERR_INVALID_ARG, "km_mel_batch: bad argument");
    return launch_mel(h, h->mel_plans[0], mel_windows(audio_dev, B, L), 0, mel_long_dev, mel_short_dev, stream);
}

int km_mel_extract(km_handle h, const km_mel_config* cfg, const float* audio_dev, int64_t B, int64_t L,
                   int64_t out_frames, float* mel_dev, void* stream) {
    if (int rc = need_ready(h)) return rc;
    if (!cfg || !audio_dev || !mel_dev || B <= 0 || L <= 0 || out_frames < 0)
        return fail(KM_ERR_INVALID_ARG, "km_mel_extract: bad argument");
    if (cfg->n_fft != 512 && cfg->n_fft != 1024) return fail(KM_ERR_UNSUPPORTED, "n_fft must be 512 or 1024");
    if (cfg->hop_length <= 0 || cfg->n_mels <= 0 || cfg->n_mels > 128) return fail(KM_ERR_INVALID_ARG, "bad hop_length / n_mels");
    MelPlan* p = nullptr;
    for (MelPlan* q : h->mel_plans)
        if (std::memcmp(&q->cfg, cfg, sizeof(*cfg)) == 0) p = q;
    if (!p) {   // first use of this configuration: build + upload (allocates; not capturable)
        p = find_or_add_plan(h, *cfg);
        if (int rc = upload_mel_plan(p)) return rc;
        if (cfg->n_mels > h->ws_mels && h->ws_windows > 0) {
            // the workspace rows were sized for narrower plans: regrow it now (this first-use path allocates anyway)
            HIP_TRY(hipDeviceSynchronize());
            if (int rc = km_reserve(h, h->ws_windows, h->ws_samples)) return rc;
        }
    }
    return launch_mel(h, p, mel_windows(audio_dev, B, L), out_frames, mel_dev, nullptr, stream);
}

int km_core_forward(km_handle h, const float* mel_dev, int64_t B, int64_t T_in, const float* mel_short_dev,
                    const float* emotion_dev, float* out_dev, float* raw_dev, float* attn_mel_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (!mel_dev || !mel_short_dev || !emotion_dev || !out_dev || B <= 0 || T_in <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_core_forward: bad argument");
    if (!aligned16(mel_dev) || !aligned16(mel_short_dev))
        return fail(KM_ERR_INVALID_ARG, "km_core_forward: mel pointers must be 16-byte aligned");
    if (B > c->ws_windows) return fail(KM_ERR_WORKSPACE, "workspace holds %lld windows, need %lld: call km_reserve",
                                       (long long)c->ws_windows, (long long)B);
    if (int rc = launch_emotion(c, emotion_dev, B, c->ws_zemo, stream)) return rc;
    if (!c->fused_ok) {
        if (!c->ws_generic) return fail(KM_ERR_WORKSPACE, "generic workspace missing: call km_reserve after km_finalize");
        return launch_core_generic(c, mel_dev, B, T_in, mel_short_dev, c->ws_zemo, out_dev, raw_dev, attn_mel_dev, stream);
    }
    return launch_core_fused(c, mel_dev, B, T_in, mel_short_dev, c->ws_zemo, out_dev, raw_dev, attn_mel_dev,
                             nullptr, 1, stream);
}

int km_emotion_logit(km_handle h, const float* emotion_dev, int64_t B, float* z_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    if (!emotion_dev || !z_dev || B <= 0) return fail(KM_ERR_INVALID_ARG, "km_emotion_logit: bad argument");
    return launch_emotion(h, emotion_dev, B, z_dev, stream);
}

int km_core_forward_z(km_handle h, const float* mel_dev, int64_t B, int64_t T_in, const float* mel_short_dev,
                      const float* z_dev, float* out_dev, float* raw_dev, float* attn_mel_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (!mel_dev || !mel_short_dev || !z_dev || !out_dev || B <= 0 || T_in <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_core_forward_z: bad argument");
    if (!aligned16(mel_dev) || !aligned16(mel_short_dev))
        return fail(KM_ERR_INVALID_ARG, "km_core_forward_z: mel pointers must be 16-byte aligned");
    if (!c->fused_ok) {
        if (B > c->ws_windows || !c->ws_generic) return fail(KM_ERR_WORKSPACE, "generic workspace missing or too small: call km_reserve after km_finalize");
        return launch_core_generic(c, mel_dev, B, T_in, mel_short_dev, z_dev, out_dev, raw_dev, attn_mel_dev, stream);
    }
    return launch_core_fused(c, mel_dev, B, T_in, mel_short_dev, z_dev, out_dev, raw_dev, attn_mel_dev, nullptr, 1, stream);
}

static int free_train(Context* c) {
    void* ptrs[] = {c->tr_params, c->tr_m, c->tr_v, c->tr_part, c->tr_gnorm, c->tr_loss, c->tr_steps};
    for (void* p : ptrs)
        if (p) HIP_TRY(hipFree(p));
    c->tr_params = c->tr_m = c->tr_v = c->tr_part = c->tr_gnorm = c->tr_loss = nullptr;
    c->tr_steps = nullptr;
    if (c->clip_span) { HIP_TRY(hipFree(c->clip_span)); c->clip_span = c->clip_edge = nullptr; c->clip_span_cap = c->clip_edge_cap = 0; }
    if (c->trp_act) { HIP_TRY(hipFree(c->trp_act)); c->trp_act = nullptr; c->trp_act_floats = 0; }
    if (c->trp_split) { HIP_TRY(hipFree(c->trp_split)); c->trp_split = nullptr; c->trp_split_floats = 0; }
    if (c->trp_wcep) { HIP_TRY(hipFree(c->trp_wcep)); c->trp_wcep = nullptr; }
    if (c->trp_tail_part) { HIP_TRY(hipFree(c->trp_tail_part)); c->trp_tail_part = nullptr; }
    if (c->trp_tail_ctr) { HIP_TRY(hipFree(c->trp_tail_ctr)); c->trp_tail_ctr = nullptr; }
    if (c->trp_masks) { HIP_TRY(hipFree(c->trp_masks)); c->trp_masks = nullptr; }
    if (c->trp_drop_ctr) { HIP_TRY(hipFree(c->trp_drop_ctr)); c->trp_drop_ctr = nullptr; }
    if (c->ltr_ws) { HIP_TRY(hipFree(c->ltr_ws)); c->ltr_ws = nullptr; c->ltr_ws_floats = 0; }
    if (c->ltr_part) { HIP_TRY(hipFree(c->ltr_part)); c->ltr_part = nullptr; }
    if (c->ltr_masks) { HIP_TRY(hipFree(c->ltr_masks)); c->ltr_masks = nullptr; c->ltr_mask_bytes = 0; }
    if (c->tr_early_ev) { (void)hipEventDestroy((hipEvent_t)c->tr_early_ev); c->tr_early_ev = nullptr; }
    c->tr_windows = 0;
    return KM_OK;
}

static int upload_train_params(Context* c, void* stream) {
    std::vector<float> flat((size_t)c->tr_nparams);
    for (const auto& k : c->param_order) {
        const HostParam& hp = c->params.at(k);
        std::memcpy(flat.data() + c->tr_offset.at(k), hp.data.data(), hp.data.size() * sizeof(float));
    }
    HIP_TRY(hipMemcpyAsync(c->tr_params, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
    if (int rc = train_refresh_padded_weights(c, stream)) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return KM_OK;
}

// where km_train_step_audio lets the front end write the packed encoder input itself (MelPack) for windows of n_frames frames
static bool train_fe_packs(Context* c, int64_t n_frames) {
    MelPlan* p = c->mel_plans[0];
    return !c->opt.train_no_fe_pack && !c->opt.train_no_dma && mel_packs(c, p, n_frames, c->T) && p->cfg.n_mels == c->NK;
}

// km_train_step_clip: the windows share the clip's STFT frames, and the step behind them is km_train_step_audio's packing
// branch at a window of T hop samples
static bool train_clip_ok(Context* c) {
    return !c->mel_plans.empty() && clip_frames_shared(c, c->mel_plans[0]) && train_fe_packs(c, c->T + 1);
}

// span image (span_rows, NK) and edge image (tr_windows, 2, NK) of km_train_step_clip in ONE allocation: the pack kernel
// addresses both with 32-bit offsets from one base
static int alloc_clip_images(Context* c, int64_t span_rows) {
    if (c->clip_span) HIP_TRY(hipFree(c->clip_span));
    c->clip_span = c->clip_edge = nullptr; c->clip_span_cap = c->clip_edge_cap = 0;
    if ((span_rows + 2 * c->tr_windows) * c->NK >= (1ll << 31)) return fail(KM_ERR_WORKSPACE, "km_train_step_clip: span of %lld frames is too wide", (long long)span_rows);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->clip_span), (size_t)(span_rows + 2 * c->tr_windows) * c->NK * sizeof(float)));
    c->clip_edge = c->clip_span + span_rows * c->NK;
    c->clip_span_cap = span_rows; c->clip_edge_cap = c->tr_windows;
    return KM_OK;
}

int km_train_init(km_handle h, int64_t max_windows, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (max_windows <= 0) return fail(KM_ERR_INVALID_ARG, "km_train_init: bad max_windows");
    if (int rc = free_train(c)) return rc;
    c->tr_offset.clear();
    // Flat layout: state-dict order within two groups; every offset a multiple of 4 floats (16 B).  The second group holds
    // the tensors whose gradients the backward pass finishes LAST (channel encoder, LayerNorm parameters, emotion encoder,
    // mouth queries: 17 % of the bucket), so the all-reduce of the first 83 % can start while they are still being
    // computed (km_train_grad_split / km_train_wait_early).
    auto late = [](const std::string& k) {
        return k == "mouth_queries" || k.rfind("mel_channel_encoder.", 0) == 0 || k.rfind("mel_norm.", 0) == 0 ||
               k.rfind("emotion_norm.", 0) == 0 || k.rfind("emotion_encoder.", 0) == 0;
    };
    int64_t off = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) c->tr_early = off;
        for (const auto& k : c->param_order) {
            if (late(k) != (pass == 1)) continue;
            c->tr_offset[k] = off;
            off += ((int64_t)c->params.at(k).data.size() + 3) / 4 * 4;
        }
    }
    c->tr_nparams = off;
    const size_t nb = (size_t)off * sizeof(float);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->tr_params), nb));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->tr_m), nb));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->tr_v), nb));
    HIP_TRY(hipMemsetAsync(c->tr_params, 0, nb, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(c->tr_m, 0, nb, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(c->tr_v, 0, nb, (hipStream_t)stream));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->tr_part), 256 * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->tr_gnorm), sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->tr_loss), sizeof(float)));
    {
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->tr_early_ev = ev;
    }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->tr_steps), 2 * sizeof(int)));
    HIP_TRY(hipMemsetAsync(c->tr_steps, 0, 2 * sizeof(int), (hipStream_t)stream));
    c->tr_windows = max_windows;
    {   // the step's workspace (km_trainp.hip): packed input first, then a fixed part, then per-window activations; dropout masks
        int64_t fixed = 0;
        const int64_t per = trainp_act_floats(c, &fixed);
        const int64_t KP = trainp_kp(c);
        c->trp_act_floats = max_windows * (per + 2 * KP * c->NK) + fixed + 4096;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->trp_act), (size_t)c->trp_act_floats * sizeof(float)));
        // the packed input's columns beyond T + 3 are written by nobody when the front end packs: zeros (they meet zero weights)
        HIP_TRY(hipMemsetAsync(c->trp_act, 0, (size_t)c->trp_act_floats * sizeof(float), (hipStream_t)stream));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->trp_wcep), (size_t)c->d * KP * sizeof(float)));
        // split-K partials: up to 16 partial outputs of every weight / bias gradient that is a product over the rows of the batch
        c->trp_split_floats = 16 * (5 * (int64_t)c->d * c->d + 2 * (int64_t)c->DH * c->d + 16 * (int64_t)c->d + (int64_t)c->d * c->KT) + 1024;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->trp_split), (size_t)c->trp_split_floats * sizeof(float)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->trp_tail_part), (size_t)1024 * 64 * sizeof(float)));      // one row of sums per tail workgroup
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->trp_tail_ctr), sizeof(unsigned)));
        HIP_TRY(hipMemsetAsync(c->trp_tail_ctr, 0, sizeof(unsigned), (hipStream_t)stream));
        HIP_TRY(hipMalloc(&c->trp_masks, (size_t)trainp_mask_alloc_bytes(c)));
        HIP_TRY(hipMemsetAsync(c->trp_masks, 1, (size_t)trainp_mask_alloc_bytes(c), (hipStream_t)stream));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->trp_drop_ctr), sizeof(int)));
        HIP_TRY(hipMemsetAsync(c->trp_drop_ctr, 0, sizeof(int), (hipStream_t)stream));
    }
    if (train_clip_ok(c))       // km_train_step_clip: the span of a dense (stride 1) batch; a wider span grows the image on first use
        if (int rc = alloc_clip_images(c, max_windows + c->T + 1)) return rc;
    return upload_train_params(c, stream);
}

int64_t km_train_num_params(km_handle h) { return h ? h->tr_nparams : -1; }

int64_t km_train_param_offset(km_handle h, const char* key) {
    if (!h || !key) return -1;
    auto it = h->tr_offset.find(key);
    return it == h->tr_offset.end() ? -1 : it->second;
}

static int need_train(Context* c, int64_t B) {
    if (int rc = need_dual(c)) return rc;
    if (!c->tr_params) return fail(KM_ERR_NOT_FINALIZED, "call km_train_init first");
    if (B <= 0 || B > c->tr_windows) return fail(KM_ERR_WORKSPACE, "km_train_init sized the step for %lld windows, got %lld",
                                                 (long long)c->tr_windows, (long long)B);
    return KM_OK;
}

int km_train_step(km_handle h, const float* mel_dev, int64_t B, int64_t T_in, const float* mel_short_dev,
                  const float* emotion_dev, const float* target_dev, float mse_weight, float l1_weight,
                  float* flat_grad_dev, float* loss_dev, float* out_dev, float* ema_state_dev, int32_t ema_first,
                  void* stream) {
    if (int rc = need_train(h, B)) return rc;
    if (!mel_dev || !mel_short_dev || !emotion_dev || !target_dev || !flat_grad_dev || !loss_dev || T_in <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_train_step: bad argument");
    const TrainStepArgs sa{emotion_dev, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, ema_state_dev, ema_first, stream};
    return train_forward_backward(h, mel_dev, B, T_in, mel_short_dev, nullptr, nullptr, sa);
}

int km_train_step_audio(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                        const float* target_dev, float mse_weight, float l1_weight, float* flat_grad_dev,
                        float* loss_dev, float* out_dev, float* ema_state_dev, int32_t ema_first, void* stream) {
    if (int rc = need_train(h, B)) return rc;
    Context* c = h;
    if (!audio_dev || !emotion_dev || !target_dev || !flat_grad_dev || !loss_dev || L <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_train_step_audio: bad argument");
    const int64_t n_frames = 1 + L / c->cfg.mel.hop_length;
    if (B > c->ws_windows || n_frames > c->ws_frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve", (long long)B, (long long)L);
    // front end -> power-mel; phase 0 of the program converts and packs it into the encoder input (B, KP, n_mels) at the
    // head of the step's workspace
    // (round 4: the front end writes the packed dB input itself -- MelPack -- where it can; option train_no_fe_pack)
    const bool fe_packs = train_fe_packs(c, n_frames);
    const MelPack pack{c->trp_act, (int)c->T, (int)trainp_kp(c)};
    if (int rc = launch_mel_power(c, c->mel_plans[0], mel_windows(audio_dev, B, L), stream, fe_packs ? mel_to_pack(&pack) : MelCarry{})) return rc;
    c->melmax_dirty = true;      // until phase 1 / 2 has re-zeroed the maxima
    const LogParams lp = plan_log_params(c->mel_plans[0]);
    const TrainAudioSrc asrc{c->ws_melpow, c->ws_melmax, (int)n_frames, &lp, fe_packs};
    const TrainStepArgs sa{emotion_dev, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, ema_state_dev, ema_first, stream};
    return train_forward_backward(c, nullptr, B, n_frames, nullptr, c->trp_act, &asrc, sa);
}

int km_train_clip_supported(km_handle h) {
    if (!h || !h->dev_finalized || h->kind != 0 || !h->tr_params) return 0;
    return train_clip_ok(h) ? 1 : 0;
}

int km_train_step_clip(km_handle h, const float* clip_dev, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                       int32_t min_start_frame, int32_t max_start_frame, const float* emotion_dev, const float* target_dev,
                       float mse_weight, float l1_weight, float* flat_grad_dev, float* loss_dev, float* out_dev,
                       float* ema_state_dev, int32_t ema_first, void* stream) {
    if (int rc = need_train(h, B)) return rc;
    Context* c = h;
    if (!clip_dev || !start_frames_dev || !emotion_dev || !target_dev || !flat_grad_dev || !loss_dev || clip_len <= 0 ||
        min_start_frame < 0 || max_start_frame < min_start_frame)
        return fail(KM_ERR_INVALID_ARG, "km_train_step_clip: bad argument");
    const km_mel_config& m = c->mel_plans[0]->cfg;
    if (!train_clip_ok(c))
        return fail(KM_ERR_UNSUPPORTED, "km_train_step_clip: windows share STFT frames only with the packing 1024-point front end, constant "
                    "padding and hop >= n_fft / 2 (hop %d, n_fft %d): gather the windows (km_gather_windows) and call km_train_step_audio",
                    m.hop_length, m.n_fft);
    const int64_t T = c->T, hop = m.hop_length;
    const int64_t n_span = (int64_t)(max_start_frame - min_start_frame) + T + 1;
    if (clip_len >= (1ll << 31) || ((int64_t)max_start_frame + T + 2) * hop >= (1ll << 31))
        return fail(KM_ERR_INVALID_ARG, "km_train_step_clip: clip or start frame beyond 2^31 samples");
    if (B > c->ws_windows)
        return fail(KM_ERR_WORKSPACE, "workspace holds %lld windows, need %lld: call km_reserve", (long long)c->ws_windows, (long long)B);
    if (n_span > c->clip_span_cap) {     // grow-only, both images in one allocation (the edge image holds tr_windows >= B windows)
        if (int rc = growth_refused(stream, "km_train_step_clip: span frames", n_span, c->clip_span_cap)) return rc;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if (int rc = alloc_clip_images(c, n_span)) return rc;
    }
    // (the pack kernel STORES the maxima of windows 0 .. B - 1: no zeroed slots needed, no memset whatever ran before)
    const int KP = (int)trainp_kp(c);
    if (int rc = launch_mel_clip_span(c, c->mel_plans[0], clip_dev, clip_len, start_frames_dev, B, min_start_frame, n_span, (int)T,
                                      c->clip_span, c->clip_edge, stream)) return rc;
    if (int rc = launch_train_clip_pack(c, c->mel_plans[0], c->clip_span, c->clip_edge, start_frames_dev, B, min_start_frame, n_span,
                                        (int)T, KP, c->trp_act, stream)) return rc;
    c->melmax_dirty = true;      // until phase 3 / 4 has re-zeroed the maxima
    const LogParams lp = plan_log_params(c->mel_plans[0]);
    const TrainAudioSrc asrc{c->ws_melpow, c->ws_melmax, (int)(T + 1), &lp, true};
    const TrainStepArgs sa{emotion_dev, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, ema_state_dev, ema_first, stream};
    return train_forward_backward(c, nullptr, B, T + 1, nullptr, c->trp_act, &asrc, sa);
}

int km_linear(const float* x_dev, const float* w_dev, const float* b_dev, int64_t B, int64_t K, int64_t N, float* out_dev, void* stream) {
    if (!x_dev || !w_dev || !out_dev || B <= 0 || K <= 0 || N <= 0) return fail(KM_ERR_INVALID_ARG, "km_linear: bad argument");
    GemmArgs g{};
    g.alpha = 1.f; g.batch2 = 1; g.kb_count = 1;
    g.A = x_dev; g.a_rs = K; g.a_cs = 1; g.B = w_dev; g.b_rs = 1; g.b_cs = K; g.C = out_dev; g.c_rs = N;
    g.M = (int)B; g.N = (int)N; g.K = (int)K; g.bias = b_dev; g.bias_mode = b_dev ? 1 : 0;
    return launch_gemm(g, 1, stream);
}

int km_train_grad_split(km_handle h, int64_t* early_floats) {
    if (int rc = need_train(h, 1)) return rc;
    if (!early_floats) return fail(KM_ERR_INVALID_ARG, "km_train_grad_split: NULL argument");
    *early_floats = h->tr_early;
    return KM_OK;
}

int km_train_wait_early(km_handle h, void* stream) {
    if (int rc = need_train(h, 1)) return rc;
    if (!h->tr_early_recorded) return fail(KM_ERR_NOT_READY, "km_train_wait_early: no training step has run yet");
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)h->tr_early_ev, 0));
    return KM_OK;
}

static int train_set_dropout_impl(km_handle h, float p, uint64_t seed, int32_t external_masks) {
    if (!(p >= 0.f && p < 1.f)) return fail(KM_ERR_INVALID_ARG, "dropout probability has to be in [0, 1), but got %g", (double)p);
    h->tr_dropout_p = p; h->tr_dropout_seed = seed; h->tr_dropout_mode = external_masks ? 1 : 0;
    return KM_OK;
}
int km_train_set_dropout(km_handle h, float p, uint64_t seed, int32_t external_masks) {
    if (int rc = need_train(h, 1)) return rc;
    return train_set_dropout_impl(h, p, seed, external_masks);
}
int km_legacy_train_set_dropout(km_handle h, float p, uint64_t seed, int32_t external_masks) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_set_dropout_impl(h, p, seed, external_masks);
}

static int train_get_dropout_step_impl(const char* fn, km_handle h, int64_t* step) {
    if (!step) return fail(KM_ERR_INVALID_ARG, "%s: NULL argument", fn);
    int v = 0;
    if (h->trp_drop_ctr) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&v, h->trp_drop_ctr, sizeof(int), hipMemcpyDeviceToHost));
    }
    *step = v;
    return KM_OK;
}
int km_train_get_dropout_step(km_handle h, int64_t* step) {
    if (int rc = need_train(h, 1)) return rc;
    return train_get_dropout_step_impl("km_train_get_dropout_step", h, step);
}
int km_legacy_train_get_dropout_step(km_handle h, int64_t* step) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_get_dropout_step_impl("km_legacy_train_get_dropout_step", h, step);
}

static int train_set_dropout_step_impl(const char* fn, km_handle h, int64_t step) {
    if (step < 0 || step > 0x7fffffff) return fail(KM_ERR_INVALID_ARG, "%s: step out of range", fn);
    if (!h->trp_drop_ctr) return fail(KM_ERR_NOT_READY, "%s: the training step is not initialised", fn);
    const int v = (int)step;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->trp_drop_ctr, &v, sizeof(int), hipMemcpyHostToDevice));
    return KM_OK;
}
int km_train_set_dropout_step(km_handle h, int64_t step) {
    if (int rc = need_train(h, 1)) return rc;
    return train_set_dropout_step_impl("km_train_set_dropout_step", h, step);
}
int km_legacy_train_set_dropout_step(km_handle h, int64_t step) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_set_dropout_step_impl("km_legacy_train_set_dropout_step", h, step);
}

int km_train_get_dropout_masks(km_handle h, int64_t B, uint8_t* mel_host, uint8_t* emo_host, uint8_t* dec_host, void* stream) {
    if (int rc = need_train(h, B)) return rc;
    if (!mel_host || !emo_host || !dec_host) return fail(KM_ERR_INVALID_ARG, "km_train_get_dropout_masks: NULL argument");
    return trainp_copy_masks(h, B, mel_host, emo_host, dec_host, 0, stream);
}

int km_train_set_dropout_masks(km_handle h, int64_t B, const uint8_t* mel_host, const uint8_t* emo_host, const uint8_t* dec_host,
                               void* stream) {
    if (int rc = need_train(h, B)) return rc;
    if (!mel_host || !emo_host || !dec_host) return fail(KM_ERR_INVALID_ARG, "km_train_set_dropout_masks: NULL argument");
    return trainp_copy_masks(h, B, const_cast<uint8_t*>(mel_host), const_cast<uint8_t*>(emo_host), const_cast<uint8_t*>(dec_host), 1, stream);
}

int km_audio_energy(const float* features_dev, int64_t B, int64_t T, int64_t D, float* energy_dev, void* stream) {
    if (!features_dev || !energy_dev || B <= 0 || T <= 0 || D <= 0) return fail(KM_ERR_INVALID_ARG, "km_audio_energy: bad argument");
    return launch_audio_energy(features_dev, B, T, D, energy_dev, stream);
}

static int train_set_loss_impl(km_handle h, const km_loss_config* cfg) {
    Context* c = h;
    // the struct has grown since ABI version 1 and holds device pointers the loss tail dereferences: a caller built against
    // an older header must be refused, not read past
    if (cfg && cfg->abi_version != KM_ABI_VERSION)
        return fail(KM_ERR_INVALID_ARG, "km_loss_config.abi_version %d != %d", cfg->abi_version, KM_ABI_VERSION);
    if (cfg) c->tr_loss_cfg = *cfg; else c->tr_loss_cfg = km_loss_config{};
    return KM_OK;
}
int km_train_set_loss(km_handle h, const km_loss_config* cfg) {
    if (int rc = need_train(h, 1)) return rc;
    return train_set_loss_impl(h, cfg);
}
int km_legacy_train_set_loss(km_handle h, const km_loss_config* cfg) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    if (cfg && (cfg->audio_energy_dev || cfg->ds_velocity_weight != 0.f || cfg->ds_separation_weight != 0.f))
        return fail(KM_ERR_UNSUPPORTED, "km_legacy_train_set_loss: the audio-visual and DualStreamLoss terms belong to the dual-stream step");
    return train_set_loss_impl(h, cfg);
}

static int train_adamw_impl(const char* fn, km_handle h, const float* flat_grad_dev, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float max_grad_norm, int64_t step, void* stream) {
    if (!flat_grad_dev || step < 1) return fail(KM_ERR_INVALID_ARG, "%s: bad argument", fn);
    return train_adamw(h, flat_grad_dev, lr, beta1, beta2, eps, weight_decay, max_grad_norm, step, stream);
}
int km_train_adamw(km_handle h, const float* flat_grad_dev, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float max_grad_norm, int64_t step, void* stream) {
    if (int rc = need_train(h, 1)) return rc;
    return train_adamw_impl("km_train_adamw", h, flat_grad_dev, lr, beta1, beta2, eps, weight_decay, max_grad_norm, step, stream);
}
int km_legacy_train_adamw(km_handle h, const float* flat_grad_dev, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float max_grad_norm, int64_t step, void* stream) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_adamw_impl("km_legacy_train_adamw", h, flat_grad_dev, lr, beta1, beta2, eps, weight_decay, max_grad_norm, step, stream);
}

static int train_get_params_impl(const char* fn, km_handle h, float* flat_host, int64_t n) {
    if (!flat_host || n != h->tr_nparams) return fail(KM_ERR_INVALID_ARG, "%s: size mismatch", fn);
    HIP_TRY(hipMemcpy(flat_host, h->tr_params, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return KM_OK;
}
int km_train_get_params(km_handle h, float* flat_host, int64_t n) {
    if (int rc = need_train(h, 1)) return rc;
    return train_get_params_impl("km_train_get_params", h, flat_host, n);
}
int km_legacy_train_get_params(km_handle h, float* flat_host, int64_t n) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_get_params_impl("km_legacy_train_get_params", h, flat_host, n);
}

static int train_set_params_impl(const char* fn, km_handle h, const float* flat_host, int64_t n) {
    if (!flat_host || n != h->tr_nparams) return fail(KM_ERR_INVALID_ARG, "%s: size mismatch", fn);
    HIP_TRY(hipMemcpy(h->tr_params, flat_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = train_refresh_padded_weights(h, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return KM_OK;
}
int km_train_set_params(km_handle h, const float* flat_host, int64_t n) {
    if (int rc = need_train(h, 1)) return rc;
    return train_set_params_impl("km_train_set_params", h, flat_host, n);
}
int km_legacy_train_set_params(km_handle h, const float* flat_host, int64_t n) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_set_params_impl("km_legacy_train_set_params", h, flat_host, n);
}

static int train_get_optimizer_state_impl(const char* fn, km_handle h, float* exp_avg_host, float* exp_avg_sq_host, int64_t n, int32_t* steps2_host) {
    if (!exp_avg_host || !exp_avg_sq_host || !steps2_host || n != h->tr_nparams)
        return fail(KM_ERR_INVALID_ARG, "%s: bad argument", fn);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(exp_avg_host, h->tr_m, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(exp_avg_sq_host, h->tr_v, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(steps2_host, h->tr_steps, 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return KM_OK;
}
int km_train_get_optimizer_state(km_handle h, float* exp_avg_host, float* exp_avg_sq_host, int64_t n, int32_t* steps2_host) {
    if (int rc = need_train(h, 1)) return rc;
    return train_get_optimizer_state_impl("km_train_get_optimizer_state", h, exp_avg_host, exp_avg_sq_host, n, steps2_host);
}
int km_legacy_train_get_optimizer_state(km_handle h, float* exp_avg_host, float* exp_avg_sq_host, int64_t n, int32_t* steps2_host) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_get_optimizer_state_impl("km_legacy_train_get_optimizer_state", h, exp_avg_host, exp_avg_sq_host, n, steps2_host);
}

static int train_set_optimizer_state_impl(const char* fn, km_handle h, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t n,
                                 const int32_t* steps2_host) {
    if (!exp_avg_host || !exp_avg_sq_host || !steps2_host || n != h->tr_nparams)
        return fail(KM_ERR_INVALID_ARG, "%s: bad argument", fn);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->tr_m, exp_avg_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->tr_v, exp_avg_sq_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->tr_steps, steps2_host, 2 * sizeof(int32_t), hipMemcpyHostToDevice));
    return KM_OK;
}
int km_train_set_optimizer_state(km_handle h, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t n,
                                 const int32_t* steps2_host) {
    if (int rc = need_train(h, 1)) return rc;
    return train_set_optimizer_state_impl("km_train_set_optimizer_state", h, exp_avg_host, exp_avg_sq_host, n, steps2_host);
}
int km_legacy_train_set_optimizer_state(km_handle h, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t n,
                                 const int32_t* steps2_host) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_set_optimizer_state_impl("km_legacy_train_set_optimizer_state", h, exp_avg_host, exp_avg_sq_host, n, steps2_host);
}

static int train_sync_impl(km_handle h, void* stream) {
    Context* c = h;
    std::vector<float> flat((size_t)c->tr_nparams);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(flat.data(), c->tr_params, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (const auto& k : c->param_order) {
        HostParam& hp = c->params.at(k);
        std::memcpy(hp.data.data(), flat.data() + c->tr_offset.at(k), hp.data.size() * sizeof(float));
    }
    c->host_finalized = false;
    return km_finalize(h, stream);
}
int km_train_sync(km_handle h, void* stream) {
    if (int rc = need_train(h, 1)) return rc;
    return train_sync_impl(h, stream);
}
int km_legacy_train_sync(km_handle h, void* stream) {
    if (int rc = need_legacy_train(h, 1)) return rc;
    return train_sync_impl(h, stream);
}

// ---- training step of the legacy model (kernels: km_legacy_train.hip; optimizer, parameter and state transfers: the
// implementations of the km_train_* twins above) ----
int km_legacy_train_init(km_handle h, int64_t max_windows, int64_t max_frames, void* stream) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "km_legacy_train_init needs a legacy handle (km_legacy_create)");
    if (!legacy_train_supported(c))
        return fail(KM_ERR_UNSUPPORTED, "km_legacy_train_init: the training step exists for d_model 256, 8 heads, decoder hidden 128, "
                    "52 blendshapes and 80 mel bins only (got d_model %d, %d heads, hidden %d)", (int)c->d, (int)c->H, c->legacy_hidden);
    if (max_windows <= 0 || max_frames <= 0) return fail(KM_ERR_INVALID_ARG, "km_legacy_train_init: bad argument");
    if (int rc = free_train(c)) return rc;
    return legacy_train_init(c, max_windows, max_frames, stream);
}

int64_t km_legacy_train_num_params(km_handle h) { return h && h->kind == 1 ? h->tr_nparams : -1; }

int64_t km_legacy_train_param_offset(km_handle h, const char* key) {
    if (!h || !key || h->kind != 1) return -1;
    auto it = h->tr_offset.find(key);
    return it == h->tr_offset.end() ? -1 : it->second;
}

int km_legacy_train_step_mel(km_handle h, const float* mel_dev, int64_t B, int64_t T, const float* target_dev, float mse_weight,
                             float l1_weight, float* flat_grad_dev, float* loss_dev, float* out_dev, void* stream) {
    if (int rc = need_legacy_train(h, B)) return rc;
    if (!mel_dev || !target_dev || !flat_grad_dev || !loss_dev || T <= 0) return fail(KM_ERR_INVALID_ARG, "km_legacy_train_step_mel: bad argument");
    if (T > h->ltr_frames) return fail(KM_ERR_WORKSPACE, "km_legacy_train_init sized the step for %lld frames, got %lld",
                                       (long long)h->ltr_frames, (long long)T);
    return legacy_train_step(h, mel_dev, B, T, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, stream);
}

int km_legacy_train_step_audio(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* target_dev, float mse_weight,
                               float l1_weight, float* flat_grad_dev, float* loss_dev, float* out_dev, void* stream) {
    if (int rc = need_legacy_train(h, B)) return rc;
    Context* c = h;
    if (!audio_dev || !target_dev || !flat_grad_dev || !loss_dev || L <= 0) return fail(KM_ERR_INVALID_ARG, "km_legacy_train_step_audio: bad argument");
    const int64_t T = 1 + L / c->cfg.mel.hop_length;
    if (T > c->ltr_frames) return fail(KM_ERR_WORKSPACE, "km_legacy_train_init sized the step for %lld frames, got %lld",
                                       (long long)c->ltr_frames, (long long)T);
    if (B > c->ws_windows || T > c->ws_frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve", (long long)B, (long long)L);
    // km_mel_batch into the step's own mel image, then the step from mel: the same launches, the same bits
    float* mel = legacy_train_mel_buffer(c);
    if (int rc = launch_mel(c, c->mel_plans[0], mel_windows(audio_dev, B, L), 0, mel, nullptr, stream)) return rc;
    return legacy_train_step(c, mel, B, T, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, stream);
}

int km_legacy_train_get_dropout_masks(km_handle h, int64_t B, int64_t T, uint8_t* enc1_host, uint8_t* enc2_host, uint8_t* attn_host,
                                      uint8_t* dec1_host, uint8_t* dec2_host, void* stream) {
    if (int rc = need_legacy_train(h, B)) return rc;
    if (!enc1_host || !enc2_host || !attn_host || !dec1_host || !dec2_host || T <= 0 || T > h->ltr_frames)
        return fail(KM_ERR_INVALID_ARG, "km_legacy_train_get_dropout_masks: bad argument");
    unsigned char* const hp[5] = {enc1_host, enc2_host, attn_host, dec1_host, dec2_host};
    return legacy_train_copy_masks(h, B, T, hp, 0, stream);
}

int km_legacy_train_set_dropout_masks(km_handle h, int64_t B, int64_t T, const uint8_t* enc1_host, const uint8_t* enc2_host,
                                      const uint8_t* attn_host, const uint8_t* dec1_host, const uint8_t* dec2_host, void* stream) {
    if (int rc = need_legacy_train(h, B)) return rc;
    if (!enc1_host || !enc2_host || !attn_host || !dec1_host || !dec2_host || T <= 0 || T > h->ltr_frames)
        return fail(KM_ERR_INVALID_ARG, "km_legacy_train_set_dropout_masks: bad argument");
    unsigned char* const hp[5] = {const_cast<uint8_t*>(enc1_host), const_cast<uint8_t*>(enc2_host), const_cast<uint8_t*>(attn_host),
                                  const_cast<uint8_t*>(dec1_host), const_cast<uint8_t*>(dec2_host)};
    return legacy_train_copy_masks(h, B, T, hp, 1, stream);
}

int km_legacy_forward_mel(km_handle h, const float* mel_dev, int64_t B, int64_t T_mel, float* out_dev, void* stream) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "not a legacy handle (km_legacy_create)");
    if (!mel_dev || !out_dev || B <= 0 || T_mel <= 0) return fail(KM_ERR_INVALID_ARG, "km_legacy_forward_mel: bad argument");
    if (B > c->ws_windows || T_mel > c->ws_frames || !c->ws_generic)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld frames: call km_reserve",
                    (long long)B, (long long)T_mel);
    return launch_legacy(c, mel_dev, B, T_mel, out_dev, stream);
}

int km_koemorph_reserve(km_handle h, int64_t max_batch, int64_t max_frames) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 2) return fail(KM_ERR_INVALID_ARG, "not a KoeMorphModel handle (km_koemorph_create)");
    if (max_batch <= 0 || max_frames <= 0) return fail(KM_ERR_INVALID_ARG, "km_koemorph_reserve: bad argument");
    if (max_batch <= c->kmm_batch && max_frames <= c->kmm_frames) return KM_OK;
    const int64_t Bm = max_batch > c->kmm_batch ? max_batch : c->kmm_batch, Tm = max_frames > c->kmm_frames ? max_frames : c->kmm_frames;
    if (c->ws_generic) { HIP_TRY(hipFree(c->ws_generic)); c->ws_generic = nullptr; c->kmm_batch = c->kmm_frames = 0; }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ws_generic), (size_t)(Bm * koemorph_ws_floats(c, Tm)) * sizeof(float)));
    c->kmm_batch = Bm; c->kmm_frames = Tm;
    return KM_OK;
}

int km_koemorph_forward(km_handle h, const float* mel_dev, const float* emotion_dev, int64_t B, int64_t T,
                        const uint8_t* audio_mask_dev, const float* prev_dev, float* smoother_state_dev,
                        int32_t apply_constraints, float* out_dev, float* raw_dev, float* attn_dev, void* stream) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 2) return fail(KM_ERR_INVALID_ARG, "not a KoeMorphModel handle (km_koemorph_create)");
    if (!mel_dev || !emotion_dev || !out_dev || B <= 0 || T <= 0) return fail(KM_ERR_INVALID_ARG, "km_koemorph_forward: bad argument");
    // the workspace is carved per call for (B, T): B * ws(T) floats must fit what km_koemorph_reserve allocated
    if (!c->ws_generic || B * koemorph_ws_floats(c, T) > c->kmm_batch * koemorph_ws_floats(c, c->kmm_frames))
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld x %lld frames: call km_koemorph_reserve", (long long)B, (long long)T);
    return launch_koemorph(c, mel_dev, emotion_dev, B, T, audio_mask_dev, prev_dev, smoother_state_dev, apply_constraints, out_dev, raw_dev,
                           attn_dev, stream);
}

int km_legacy_forward(km_handle h, const float* audio_dev, int64_t B, int64_t L, float* out_dev, void* stream) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "not a legacy handle (km_legacy_create)");
    if (!audio_dev || !out_dev || B <= 0 || L <= 0) return fail(KM_ERR_INVALID_ARG, "km_legacy_forward: bad argument");
    const int64_t n_frames = 1 + L / c->cfg.mel.hop_length;
    if (B > c->ws_windows || n_frames > c->ws_frames || !c->ws_generic)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve",
                    (long long)B, (long long)L);
    if (legacy_pow_ok(c)) {
        // front end -> power-mel + window maxima; the fused encoder converts to dB while it stages its rows and the attention
        // kernel re-zeroes the maxima: no mel_log_kernel launch, no memset (round 4; 18 us of the 460 per 256 windows)
        if (int rc = launch_mel_power(c, c->mel_plans[0], mel_windows(audio_dev, B, L), stream)) return rc;
        const LogParams lp = plan_log_params(c->mel_plans[0]);
        const LegacyPowSrc src{c->ws_melpow, c->ws_melmax, &lp};
        return launch_legacy(c, nullptr, B, n_frames, out_dev, stream, &src);
    }
    if (int rc = launch_mel(c, c->mel_plans[0], mel_windows(audio_dev, B, L), 0, c->ws_mel, nullptr, stream)) return rc;
    return launch_legacy(c, c->ws_mel, B, n_frames, out_dev, stream);
}

int km_ema_scan(km_handle h, float* x_dev, int64_t B, int64_t N, void* stream) {
    if (int rc = need_ready(h)) return rc;
    if (h->kind != 0) return fail(KM_ERR_INVALID_ARG, "this entry point needs a dual-stream handle (km_create)");
    if (!x_dev || B <= 0 || N <= 0) return fail(KM_ERR_INVALID_ARG, "km_ema_scan: bad argument");
    return launch_ema_scan(h, x_dev, B, N, stream);
}

int km_smooth(km_handle h, float* x_dev, float* state_dev, int64_t B, int32_t first, void* stream) {
    if (int rc = need_ready(h)) return rc;
    if (!x_dev || !state_dev || B <= 0) return fail(KM_ERR_INVALID_ARG, "km_smooth: bad argument");
    return launch_smooth(h, x_dev, state_dev, B, first, stream);
}

// The fused core's attention-map output exists for the plain fp32 instantiations only: refused before anything is launched
static int attn_refused(Context* c, const char* who) {
    if (c->fused_ok && (c->opt.core_split == 3 || c->opt.core_split == 6))
        return fail(KM_ERR_UNSUPPORTED, "%s: the split-bf16 core (core_split %d) has no attention-map output", who, c->opt.core_split);
    return KM_OK;
}

// km_forward_audio and km_forward_audio_attn (raw_dev / attn_dev: null in the former, which makes the launches it always made)
static int forward_audio(km_handle h, const char* who, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                         float* out_dev, float* state_dev, int32_t first, float* raw_dev, float* attn_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (!audio_dev || !emotion_dev || !out_dev || B <= 0 || L <= 0)
        return fail(KM_ERR_INVALID_ARG, "%s: bad argument", who);
    if (attn_dev)
        if (int rc = attn_refused(c, who)) return rc;
    const int64_t n_frames = 1 + L / c->cfg.mel.hop_length;
    if (B > c->ws_windows || n_frames > c->ws_frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve",
                    (long long)B, (long long)L);
    MelPlan* plan = c->mel_plans[0];
    const MelSrc src = mel_windows(audio_dev, B, L);
    if (!c->fused_ok) {     // generic shapes: staged front end, GEMM-chain core, stand-alone EMA
        if (!c->ws_generic) return fail(KM_ERR_WORKSPACE, "generic workspace missing: call km_reserve after km_finalize");
        const bool power_path = generic_core_takes_power(c) && !c->opt.generic_staged;
        const bool fuse_emo = power_path && mel_fuses_emotion(c, plan);   // emotion logits inside the front-end kernel
        if (!fuse_emo)
            if (int rc = launch_emotion(c, emotion_dev, B, c->ws_zemo, stream)) return rc;
        if (power_path) {
            // power-mel -> dB conversion inside the encoder's tile staging: no log-mel image at all
            if (int rc = launch_mel_power(c, plan, src, stream, fuse_emo ? mel_emotion(emotion_dev, c->ws_zemo) : MelCarry{})) return rc;
            if (int rc = launch_core_generic_power(c, plan, B, n_frames, c->ws_zemo, out_dev, raw_dev, attn_dev, stream)) return rc;
        } else if (c->NK == 80 && !c->opt.generic_staged) {
            // log-mel written straight into the packed encoder input; long + short-term rows in one contraction
            float* xp = generic_packed_x(c, B);
            if (int rc = launch_mel_packed(c, plan, src, xp, c->T, (c->KT + 15) / 16 * 16, stream)) return rc;
            if (int rc = launch_core_generic_packed(c, xp, B, c->ws_zemo, out_dev, raw_dev, attn_dev, stream)) return rc;
        } else {
            if (int rc = launch_mel(c, plan, src, 0, c->ws_mel, c->ws_short, stream)) return rc;
            if (int rc = launch_core_generic(c, c->ws_mel, B, n_frames, c->ws_short, c->ws_zemo, out_dev, raw_dev, attn_dev, stream)) return rc;
        }
        if (state_dev) return launch_smooth(c, out_dev, state_dev, B, first, stream);
        return KM_OK;
    }
    // three launches: emotion logits, power-mel + window maxima, fused core (dB conversion on load)
    hipStream_t st = (hipStream_t)stream;
    const bool tm = c->stage_timing;
    const bool fuse_emo = mel_fuses_emotion(c, plan);   // emotion logits computed inside the front-end kernel
    if (tm) HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[0], st));
    if (!fuse_emo)
        if (int rc = launch_emotion(c, emotion_dev, B, c->ws_zemo, stream)) return rc;
    if (tm) HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[1], st));
    if (int rc = launch_mel_power(c, plan, src, stream, fuse_emo ? mel_emotion(emotion_dev, c->ws_zemo) : MelCarry{})) return rc;
    if (tm) { HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[2], st)); HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[3], st)); }
    if (int rc = launch_core_fused_db(c, plan, B, n_frames, c->ws_zemo, out_dev, stream,
                                      with_outputs(core_workspace(state_dev, first), raw_dev, attn_dev))) return rc;
    if (tm) HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[4], st));
    return KM_OK;
}

int km_forward_audio(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                     float* out_dev, float* state_dev, int32_t first, void* stream) {
    return forward_audio(h, "km_forward_audio", audio_dev, B, L, emotion_dev, out_dev, state_dev, first, nullptr, nullptr, stream);
}

int km_forward_audio_attn(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                          float* out_dev, float* state_dev, int32_t first, float* raw_dev, float* attn_dev, void* stream) {
    return forward_audio(h, "km_forward_audio_attn", audio_dev, B, L, emotion_dev, out_dev, state_dev, first, raw_dev, attn_dev, stream);
}

// km_forward_clip shares STFT frames between the windows of a batch exactly as km_train_step_clip does; behind the span
// front end runs the fused core's table variant.  The experimental split-bf16 core has no table variant: with it switched on
// km_forward_audio computes something else.
static bool forward_clip_ok(Context* c) {
    if (c->mel_plans.empty() || !c->fused_ok || c->opt.core_split == 3 || c->opt.core_split == 6) return false;
    return mel_rp_ok(c, c->mel_plans[0]) && clip_frames_shared(c, c->mel_plans[0]);
}

int km_forward_clip_supported(km_handle h) {
    if (!h || !h->dev_finalized || h->kind != 0) return 0;
    return forward_clip_ok(h) ? 1 : 0;
}

static int forward_clip(km_handle h, const float* clip_dev, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                        int32_t min_start_frame, int32_t max_start_frame, const float* emotion_dev, float* out_dev,
                        float* state_dev, int32_t first, float* raw_dev, float* attn_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (!clip_dev || !start_frames_dev || !emotion_dev || !out_dev || B <= 0 || clip_len <= 0 || min_start_frame < 0 ||
        max_start_frame < min_start_frame)
        return fail(KM_ERR_INVALID_ARG, "km_forward_clip: bad argument");
    const km_mel_config& m = c->mel_plans[0]->cfg;
    if (!forward_clip_ok(c))
        return fail(KM_ERR_UNSUPPORTED, "km_forward_clip: needs the fused core (d_model 256, window 256, 8 heads) behind the 1024-point "
                    "front end with constant padding and hop >= n_fft / 2 (hop %d, n_fft %d): gather the windows (km_gather_windows) "
                    "and call km_forward_audio", m.hop_length, m.n_fft);
    const int64_t T = c->T, hop = m.hop_length;
    const int64_t n_span = (int64_t)(max_start_frame - min_start_frame) + T + 1;
    if (clip_len >= (1ll << 31) || ((int64_t)max_start_frame + T + 2) * hop >= (1ll << 31) || n_span * c->NK >= (1ll << 31))
        return fail(KM_ERR_INVALID_ARG, "km_forward_clip: clip or start frame beyond 2^31 samples");
    if (B > c->ws_windows)
        return fail(KM_ERR_WORKSPACE, "workspace holds %lld windows, need %lld: call km_reserve", (long long)c->ws_windows, (long long)B);
    // grow-only; allocates, so not inside a stream capture
    if (int rc = grow_buffer(&c->fwd_span, &c->fwd_span_cap, n_span, c->NK * sizeof(float), stream, "km_forward_clip: span frames")) return rc;
    if (int rc = grow_buffer(&c->fwd_edge, &c->fwd_edge_cap, B, 2 * c->NK * sizeof(float), stream, "km_forward_clip: windows")) return rc;
    // four launches: emotion logits (emotion_kernel_d256: bit-identical to the rider inside km_forward_audio's front end), the
    // span + edge images, the window maxima, the fused core reading its rows through the table
    if (int rc = launch_emotion(c, emotion_dev, B, c->ws_zemo, stream)) return rc;
    if (int rc = launch_mel_clip_span(c, c->mel_plans[0], clip_dev, clip_len, start_frames_dev, B, min_start_frame, n_span, (int)T,
                                      c->fwd_span, c->fwd_edge, stream)) return rc;
    if (int rc = launch_clip_window_max(c, c->fwd_span, c->fwd_edge, start_frames_dev, B, min_start_frame, n_span, (int)(T + 1),
                                        stream)) return rc;
    const ClipTable tab{c->fwd_span, c->fwd_edge, (int)n_span, start_frames_dev, min_start_frame};
    return launch_core_fused_db(c, c->mel_plans[0], B, T + 1, c->ws_zemo, out_dev, stream,
                                with_outputs(core_table(&tab, state_dev, first), raw_dev, attn_dev));
}

int km_forward_clip(km_handle h, const float* clip_dev, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                    int32_t min_start_frame, int32_t max_start_frame, const float* emotion_dev, float* out_dev,
                    float* state_dev, int32_t first, void* stream) {
    return forward_clip(h, clip_dev, clip_len, start_frames_dev, B, min_start_frame, max_start_frame, emotion_dev, out_dev, state_dev, first,
                        nullptr, nullptr, stream);
}

int km_forward_clip_attn(km_handle h, const float* clip_dev, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                         int32_t min_start_frame, int32_t max_start_frame, const float* emotion_dev, float* out_dev,
                         float* state_dev, int32_t first, float* raw_dev, float* attn_dev, void* stream) {
    return forward_clip(h, clip_dev, clip_len, start_frames_dev, B, min_start_frame, max_start_frame, emotion_dev, out_dev, state_dev, first,
                        raw_dev, attn_dev, stream);
}

static int free_streams(Context* c) {
    void* ptrs[] = {c->ring, c->ring_wptr, c->ring_frames, c->ring_ready, c->ring_started, c->ring_state, c->sfifo, c->sfifo_state, c->ring_fire};
    for (void* p : ptrs)
        if (p) HIP_TRY(hipFree(p));
    c->ring = nullptr; c->ring_wptr = nullptr; c->ring_frames = nullptr; c->ring_ready = nullptr;
    c->ring_started = nullptr; c->ring_state = nullptr; c->n_streams = 0;
    c->sfifo = nullptr; c->sfifo_state = nullptr; c->ring_fire = nullptr; c->sfifo_len = 0; c->sfifo_frame = 0;
    return KM_OK;
}

int km_stream_reset(km_handle h, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_reset: no streams (km_stream_create first)");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(c->ring, 0, (size_t)c->n_streams * c->ring_len * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(c->ring_wptr, 0, (size_t)c->n_streams * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(c->ring_frames, 0, (size_t)c->n_streams * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(c->ring_ready, 0, (size_t)c->n_streams, st));
    HIP_TRY(hipMemsetAsync(c->ring_started, 0, (size_t)c->n_streams, st));
    HIP_TRY(hipMemsetAsync(c->ring_state, 0, (size_t)c->n_streams * c->NB * sizeof(float), st));
    if (c->sfifo_len > 0) {     // empty FIFOs: their samples are not read below `available` (stream_reset_masked_kernel)
        HIP_TRY(hipMemsetAsync(c->sfifo_state, 0, 3 * (size_t)c->n_streams * sizeof(int), st));
        HIP_TRY(hipMemsetAsync(c->ring_fire, 0, (size_t)c->n_streams, st));
    }
    return KM_OK;
}

int km_stream_create(km_handle h, int64_t n_streams, double context_window_s, double update_interval_s,
                     const km_mel_config* mel_cfg) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (n_streams <= 0 || !(context_window_s > 0) || !(update_interval_s > 0) || !mel_cfg)
        return fail(KM_ERR_INVALID_ARG, "km_stream_create: bad argument");
    if (mel_cfg->n_fft != 512 && mel_cfg->n_fft != 1024) return fail(KM_ERR_UNSUPPORTED, "n_fft must be 512 or 1024");
    if (mel_cfg->n_mels != c->NK) return fail(KM_ERR_INVALID_ARG, "stream front end must produce %d mel channels", c->NK);
    if (int rc = free_streams(c)) return rc;
    const int sr = mel_cfg->sample_rate;
    c->ring_len = (int64_t)(context_window_s * sr);                                // mel_sliding_window.py:46
    const double target_fps = 1.0 / update_interval_s;
    c->ring_hop = (int)((double)sr / target_fps);                                   // :49-50 (532 for 0.0333)
    c->stream_out_frames = (int64_t)(context_window_s / update_interval_s);         // :300
    if (c->ring_hop <= 0 || c->ring_len <= mel_cfg->n_fft / 2) return fail(KM_ERR_INVALID_ARG, "context window too short");
    c->n_streams = n_streams;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ring), (size_t)n_streams * c->ring_len * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ring_wptr), (size_t)n_streams * sizeof(int)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ring_frames), (size_t)n_streams * sizeof(int)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ring_ready), (size_t)n_streams));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ring_started), (size_t)n_streams));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ring_state), (size_t)n_streams * c->NB * sizeof(float)));
    c->stream_plan = find_or_add_plan(c, *mel_cfg);
    if (int rc = upload_mel_plan(c->stream_plan)) return rc;
    if (int rc = km_reserve(h, n_streams, c->ring_len)) return rc;
    if (int rc = km_stream_reset(h, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return KM_OK;
}

int km_stream_push(km_handle h, const float* samples_dev, int64_t n_per_stream, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_push: no streams (km_stream_create first)");
    if (!samples_dev) return fail(KM_ERR_INVALID_ARG, "km_stream_push: NULL samples");
    const int64_t diff = n_per_stream - c->ring_hop;
    if (diff > 1 || diff < -1)                                                      // :80-82
        return fail(KM_ERR_INVALID_ARG, "Frame size mismatch: expected ~%d, got %lld", c->ring_hop, (long long)n_per_stream);
    return launch_ring_push(c, samples_dev, n_per_stream, stream);
}

// what asking for raw / the map adds to the refusals of tick and step, before anything is launched or popped
static int stream_outputs_ok(Context* c, const float* attn_dev) {
    if (attn_dev && (c->opt.core_split == 3 || c->opt.core_split == 6))
        return fail(KM_ERR_UNSUPPORTED, "streams: the split-bf16 variant (core_split %d) has no attention-map output", c->opt.core_split);
    if ((uintptr_t)attn_dev & 15) return fail(KM_ERR_INVALID_ARG, "streams: the attention maps must be 16-byte aligned");
    return KM_OK;
}

static int stream_tick(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* ready_dev, float* raw_dev, float* attn_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_tick: no streams (km_stream_create first)");
    if (!emotion_dev || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_stream_tick: NULL argument");
    // two shapes have a streaming core: the fused one (d_model 256, 8 heads, window 256) and core512's (512, 8 or 16 heads, window 512)
    if (!c->fused_ok && !core512_stream_ok(c))
        return fail(KM_ERR_UNSUPPORTED, "no kernel for d_model=%d, mel_sequence_length=%d, heads=%d", c->d, c->T, c->H);
    const int64_t S = c->n_streams, L = c->ring_len;
    const int64_t n_frames = 1 + L / c->stream_plan->cfg.hop_length;
    if (S > c->ws_windows || n_frames > c->ws_frames) return fail(KM_ERR_WORKSPACE, "stream workspace too small");
    if (int rc = stream_outputs_ok(c, attn_dev)) return rc;
    const bool fuse_emo = mel_fuses_emotion(c, c->stream_plan);
    if (!fuse_emo)
        if (int rc = launch_emotion(c, emotion_dev, S, c->ws_zemo, stream)) return rc;
    if (int rc = launch_mel_power(c, c->stream_plan, mel_rings(c), stream, fuse_emo ? mel_emotion(emotion_dev, c->ws_zemo) : MelCarry{})) return rc;
    if (c->fused_ok) {
        if (int rc = launch_core_fused_db(c, c->stream_plan, S, n_frames, c->ws_zemo, out_dev, stream,
                                          with_outputs(core_stream(c), raw_dev, attn_dev))) return rc;
    } else {
        if (int rc = launch_core512_stream(c, c->stream_plan, S, n_frames, c->ws_zemo, out_dev, stream, nullptr, raw_dev, attn_dev)) return rc;
    }
    if (ready_dev)
        HIP_TRY(hipMemcpyAsync(ready_dev, c->ring_ready, (size_t)S, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return KM_OK;
}

int km_stream_tick(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* ready_dev, void* stream) {
    return stream_tick(h, emotion_dev, out_dev, ready_dev, nullptr, nullptr, stream);
}

int km_stream_tick_attn(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* ready_dev, float* raw_dev, float* attn_dev,
                        void* stream) {
    return stream_tick(h, emotion_dev, out_dev, ready_dev, raw_dev, attn_dev, stream);
}

// ---- streams out of phase: a chunk FIFO per stream in front of its ring (kernels: km_legacy_stream.hip) ----
static int need_stream_fifos(Context* c, const char* who) {
    if (int rc = need_dual(c)) return rc;
    if (c->n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "%s: no streams (km_stream_create first)", who);
    if (c->sfifo_len <= 0) return fail(KM_ERR_INVALID_ARG, "%s: no FIFOs (km_stream_fifo_create first)", who);
    return KM_OK;
}

// the launches of a step behind the pop: what km_stream_tick launches, gated on the step's fire flags instead of is_full
static int stream_step_launches(Context* c, const float* emotion_dev, float* out_dev, void* stream, float* raw_dev = nullptr,
                                float* attn_dev = nullptr) {
    const int64_t S = c->n_streams, n_frames = 1 + c->ring_len / c->stream_plan->cfg.hop_length;
    const bool fuse_emo = mel_fuses_emotion(c, c->stream_plan);
    if (!fuse_emo)
        if (int rc = launch_emotion(c, emotion_dev, S, c->ws_zemo, stream)) return rc;
    if (int rc = launch_mel_power(c, c->stream_plan, mel_rings(c, c->ring_fire), stream,
                                  fuse_emo ? mel_emotion(emotion_dev, c->ws_zemo) : MelCarry{})) return rc;
    if (c->fused_ok)
        return launch_core_fused_db(c, c->stream_plan, S, n_frames, c->ws_zemo, out_dev, stream,
                                    with_outputs(core_stream(c, c->ring_fire), raw_dev, attn_dev));
    return launch_core512_stream(c, c->stream_plan, S, n_frames, c->ws_zemo, out_dev, stream, c->ring_fire, raw_dev, attn_dev);
}

int km_stream_fifo_create(km_handle h, int64_t fifo_samples, int64_t frame_samples) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_fifo_create: no streams (km_stream_create first)");
    if (fifo_samples <= 0 || frame_samples <= 0 || fifo_samples >= (1ll << 30))
        return fail(KM_ERR_INVALID_ARG, "km_stream_fifo_create: bad argument (FIFOs of %lld samples, frames of %lld)", (long long)fifo_samples,
                    (long long)frame_samples);
    const int64_t diff = frame_samples - c->ring_hop;
    if (diff > 1 || diff < -1)                                                      // mel_sliding_window.py:80-82
        return fail(KM_ERR_INVALID_ARG, "Frame size mismatch: expected ~%d, got %lld", c->ring_hop, (long long)frame_samples);
    if (fifo_samples < frame_samples)
        return fail(KM_ERR_INVALID_ARG, "km_stream_fifo_create: frames of %lld samples exceed the FIFO of %lld: no read could ever succeed",
                    (long long)frame_samples, (long long)fifo_samples);
    if (c->ring_hop > c->ring_len) return fail(KM_ERR_INVALID_ARG, "km_stream_fifo_create: the ring hop exceeds the ring");
    HIP_TRY(hipDeviceSynchronize());
    void* old[] = {c->sfifo, c->sfifo_state, c->ring_fire};
    for (void* p : old)
        if (p) HIP_TRY(hipFree(p));
    c->sfifo = nullptr; c->sfifo_state = nullptr; c->ring_fire = nullptr; c->sfifo_len = 0; c->sfifo_frame = 0;
    const size_t S = (size_t)c->n_streams;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->sfifo), S * fifo_samples * sizeof(float)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->sfifo_state), 3 * S * sizeof(int)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ring_fire), S));
    HIP_TRY(hipMemset(c->sfifo, 0, S * fifo_samples * sizeof(float)));
    HIP_TRY(hipMemset(c->sfifo_state, 0, 3 * S * sizeof(int)));
    HIP_TRY(hipMemset(c->ring_fire, 0, S));
    c->sfifo_len = fifo_samples; c->sfifo_frame = (int)frame_samples;
    // the launches of one step over a gate of zeros: no workgroup passes it, so nothing is read or written (the emotion rows and
    // the result pointer are dummies), but every kernel of a step has had its attributes set before a capture sees its first launch
    if (c->fused_ok || core512_stream_ok(c)) {
        float* emo = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&emo), S * c->ED * sizeof(float)));
        HIP_TRY(hipMemset(emo, 0, S * c->ED * sizeof(float)));
        int rc = launch_sfifo_pop_ring(c, nullptr, nullptr, nullptr, nullptr);
        if (!rc) rc = stream_step_launches(c, emo, c->ring_state, nullptr);
        const hipError_t e = hipDeviceSynchronize();
        (void)hipFree(emo);
        if (rc) return rc;
        HIP_TRY(e);
    }
    return KM_OK;
}

int km_stream_feed(km_handle h, const float* samples_dev, int64_t n_per_stream, const int32_t* counts_dev, void* stream) {
    if (int rc = need_stream_fifos(h, "km_stream_feed")) return rc;
    if (!samples_dev || n_per_stream <= 0 || n_per_stream >= (1ll << 30)) return fail(KM_ERR_INVALID_ARG, "km_stream_feed: bad argument");
    return launch_sfifo_push(h, samples_dev, n_per_stream, counts_dev, stream);
}

static int stream_step(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* fired_dev, uint8_t* ready_dev, int32_t* backlog_dev,
                       float* raw_dev, float* attn_dev, void* stream) {
    if (int rc = need_stream_fifos(h, "km_stream_step")) return rc;
    Context* c = h;
    if (!emotion_dev || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_stream_step: NULL argument");
    if (!c->fused_ok && !core512_stream_ok(c))                                      // as km_stream_tick, before anything is popped
        return fail(KM_ERR_UNSUPPORTED, "no kernel for d_model=%d, mel_sequence_length=%d, heads=%d", c->d, c->T, c->H);
    const int64_t S = c->n_streams;
    if (S > c->ws_windows || 1 + c->ring_len / c->stream_plan->cfg.hop_length > c->ws_frames)
        return fail(KM_ERR_WORKSPACE, "stream workspace too small");
    if (int rc = stream_outputs_ok(c, attn_dev)) return rc;
    // pop + ring advance (fire, ready, backlog), then the launches of a tick gated on fire: one linear chain
    if (int rc = launch_sfifo_pop_ring(c, fired_dev, ready_dev, backlog_dev, stream)) return rc;
    return stream_step_launches(c, emotion_dev, out_dev, stream, raw_dev, attn_dev);
}

int km_stream_step(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* fired_dev, uint8_t* ready_dev, int32_t* backlog_dev,
                   void* stream) {
    return stream_step(h, emotion_dev, out_dev, fired_dev, ready_dev, backlog_dev, nullptr, nullptr, stream);
}

int km_stream_step_attn(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* fired_dev, uint8_t* ready_dev, int32_t* backlog_dev,
                        float* raw_dev, float* attn_dev, void* stream) {
    return stream_step(h, emotion_dev, out_dev, fired_dev, ready_dev, backlog_dev, raw_dev, attn_dev, stream);
}

int km_stream_reset_streams(km_handle h, const uint8_t* mask_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_reset_streams: no streams (km_stream_create first)");
    if (!mask_dev) return fail(KM_ERR_INVALID_ARG, "km_stream_reset_streams: NULL mask");
    return launch_stream_reset_masked(c, mask_dev, stream);
}

// ---- streams of the legacy model: device-resident consuming FIFOs + the one-launch model (kernels: km_legacy_stream.hip,
//      legacy_stream_kernel in km_kmmf.hip) ----
static int free_legacy_streams(Context* c) {
    void* ptrs[] = {c->lfifo, c->lfifo_state, c->lfifo_stage, c->lfifo_ready, c->lfifo_attn};
    for (void* p : ptrs)
        if (p) HIP_TRY(hipFree(p));
    c->lfifo = nullptr; c->lfifo_state = nullptr; c->lfifo_stage = nullptr; c->lfifo_ready = nullptr; c->lfifo_attn = nullptr;
    c->lfifo_cap = c->lfifo_state_cap = c->lfifo_stage_cap = c->lfifo_ready_cap = c->lfifo_attn_cap = 0;
    c->lfifo_streams = c->lfifo_len = c->lfifo_window = 0;
    return KM_OK;
}

// the shape legacy_stream_kernel is written for, behind the front end that leaves power-mel + window maxima
static bool legacy_stream_ok(Context* c) {
    return c->legacy_fused && c->legacy_tail_fused && c->d == 256 && c->H == 8 && c->legacy_hidden == 128 && c->NB == 52 && c->NK == 80 &&
           !c->mel_plans.empty() && c->mel_plans[0]->cfg.n_fft == 1024 && legacy_pow_ok(c);
}

static int need_legacy_stream(Context* c, const char* who) {
    if (int rc = need_ready(c)) return rc;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "%s needs a legacy handle (km_legacy_create)", who);
    if (c->lfifo_streams <= 0) return fail(KM_ERR_INVALID_ARG, "%s: no streams (km_legacy_stream_create first)", who);
    return KM_OK;
}

int km_legacy_stream_reset(km_handle h, void* stream) {
    if (int rc = need_legacy_stream(h, "km_legacy_stream_reset")) return rc;
    Context* c = h;
    hipStream_t st = (hipStream_t)stream;
    const size_t S = (size_t)c->lfifo_streams;
    HIP_TRY(hipMemsetAsync(c->lfifo, 0, S * c->lfifo_len * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(c->lfifo_stage, 0, S * c->lfifo_window * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(c->lfifo_state, 0, 3 * S * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(c->lfifo_ready, 0, S, st));
    return KM_OK;
}

int km_legacy_stream_create(km_handle h, int64_t n_streams, int64_t buffer_samples, int64_t audio_length) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "km_legacy_stream_create needs a legacy handle (km_legacy_create)");
    if (n_streams <= 0 || buffer_samples <= 0 || audio_length <= 0 || audio_length > buffer_samples || n_streams >= (1ll << 24) ||
        buffer_samples >= (1ll << 30))
        return fail(KM_ERR_INVALID_ARG, "km_legacy_stream_create: bad argument (%lld streams, buffer of %lld samples, windows of %lld)",
                    (long long)n_streams, (long long)buffer_samples, (long long)audio_length);
    const int64_t T = 1 + audio_length / c->cfg.mel.hop_length;                      // simplified_model.py:40
    if (!legacy_stream_ok(c))
        return fail(KM_ERR_UNSUPPORTED, "km_legacy_stream_create: windows of %lld frames are served for d_model 256, 8 heads, decoder hidden 128 "
                    "behind the 1024-point front end only (got d_model %d, %d heads, hidden %d, n_fft %d)", (long long)T, c->d, c->H,
                    c->legacy_hidden, c->mel_plans.empty() ? 0 : c->mel_plans[0]->cfg.n_fft);
    if (T > 32)
        return fail(KM_ERR_UNSUPPORTED, "km_legacy_stream_create: windows of %lld samples are %lld frames, the stream kernel holds at most 32 "
                    "(use km_legacy_forward for longer windows)", (long long)audio_length, (long long)T);
    c->lfifo_streams = 0;
    const char* what = "km_legacy_stream_create";
    if (int rc = grow_buffer(&c->lfifo, &c->lfifo_cap, n_streams * buffer_samples, sizeof(float), nullptr, what)) return rc;
    if (int rc = grow_buffer(&c->lfifo_state, &c->lfifo_state_cap, 3 * n_streams, sizeof(int), nullptr, what)) return rc;
    if (int rc = grow_buffer(&c->lfifo_stage, &c->lfifo_stage_cap, n_streams * audio_length, sizeof(float), nullptr, what)) return rc;
    if (int rc = grow_buffer(&c->lfifo_ready, &c->lfifo_ready_cap, n_streams, 1, nullptr, what)) return rc;
    if (int rc = grow_buffer(&c->lfifo_attn, &c->lfifo_attn_cap, n_streams * c->NB * c->d, sizeof(float), nullptr, what)) return rc;
    if (int rc = km_reserve(h, n_streams, audio_length)) return rc;                  // power-mel, window maxima, chunk counters
    if (!legacy_stream_ok(c)) return fail(KM_ERR_UNSUPPORTED, "km_legacy_stream_create: the power-mel workspace is not 16-byte aligned");
    c->lfifo_streams = n_streams; c->lfifo_len = buffer_samples; c->lfifo_window = audio_length;
    HIP_TRY(hipMemset(c->ws_melmax, 0, (size_t)c->ws_windows * sizeof(unsigned)));
    c->melmax_dirty = false;
    if (int rc = km_legacy_stream_reset(h, nullptr)) return rc;
    // one tick over the empty FIFOs: no stream is ready, so nothing is consumed or written (the result pointer is a dummy), but
    // every kernel of a tick has had its attributes set before a capture can see its first launch
    if (int rc = km_legacy_stream_tick(h, c->lfifo_attn, nullptr, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return KM_OK;
}

int km_legacy_stream_push(km_handle h, const float* samples_dev, int64_t n_per_stream, const int32_t* counts_dev, void* stream) {
    if (int rc = need_legacy_stream(h, "km_legacy_stream_push")) return rc;
    if (!samples_dev || n_per_stream <= 0 || n_per_stream >= (1ll << 30))
        return fail(KM_ERR_INVALID_ARG, "km_legacy_stream_push: bad argument");
    return launch_lfifo_push(h, samples_dev, n_per_stream, counts_dev, stream);
}

int km_legacy_stream_tick(km_handle h, float* out_dev, uint8_t* ready_dev, void* stream) {
    if (int rc = need_legacy_stream(h, "km_legacy_stream_tick")) return rc;
    Context* c = h;
    if (!out_dev) return fail(KM_ERR_INVALID_ARG, "km_legacy_stream_tick: NULL argument");
    const int64_t S = c->lfifo_streams, W = c->lfifo_window, T = 1 + W / c->cfg.mel.hop_length;
    if (S > c->ws_windows || T > c->ws_frames) return fail(KM_ERR_WORKSPACE, "stream workspace too small");
    if (!legacy_stream_ok(c)) return fail(KM_ERR_UNSUPPORTED, "km_legacy_stream_tick: the fused legacy kernels are switched off (km_set_option)");
    // three launches: pop (ready flags + the claimed windows, chronological), the plain front end over the staging image,
    // the model for every ready stream (which also puts every stream's window maximum back to zero)
    if (int rc = launch_lfifo_pop(c, ready_dev, stream)) return rc;
    if (int rc = launch_mel_power(c, c->mel_plans[0], mel_windows(c->lfifo_stage, S, W), stream)) return rc;
    const LogParams lp = plan_log_params(c->mel_plans[0]);
    return launch_legacy_stream_model(c, c->ws_melpow, c->ws_melmax, c->lfifo_ready, S, (int)T, lp, c->lfifo_attn, out_dev, stream);
}

int km_enable_stage_timing(km_handle h, int32_t enable) {
    if (!h) return fail(KM_ERR_INVALID_ARG, "NULL handle");
    Context* c = h;
    if (enable && !c->stage_ev[0])
        for (int i = 0; i < 5; ++i) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            c->stage_ev[i] = e;
        }
    c->stage_timing = enable != 0;
    return KM_OK;
}

int km_stage_times(km_handle h, float* ms3) {
    if (!h || !ms3) return fail(KM_ERR_INVALID_ARG, "km_stage_times: NULL argument");
    Context* c = h;
    if (!c->stage_ev[0]) return fail(KM_ERR_INVALID_ARG, "stage timing was never enabled");
    HIP_TRY(hipEventSynchronize((hipEvent_t)c->stage_ev[4]));
    HIP_TRY(hipEventElapsedTime(&ms3[0], (hipEvent_t)c->stage_ev[0], (hipEvent_t)c->stage_ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms3[1], (hipEvent_t)c->stage_ev[1], (hipEvent_t)c->stage_ev[2]));
    HIP_TRY(hipEventElapsedTime(&ms3[2], (hipEvent_t)c->stage_ev[3], (hipEvent_t)c->stage_ev[4]));
    return KM_OK;
}

static int free_pipeline(Context* c) {
    for (int i = 0; i < 2; ++i) {
        if (c->pipe_melpow[i]) HIP_TRY(hipFree(c->pipe_melpow[i]));
        if (c->pipe_melmax[i]) HIP_TRY(hipFree(c->pipe_melmax[i]));
        if (c->pipe_zemo[i]) HIP_TRY(hipFree(c->pipe_zemo[i]));
        c->pipe_melpow[i] = nullptr; c->pipe_melmax[i] = nullptr; c->pipe_zemo[i] = nullptr; c->pipe_dirty[i] = true;
    }
    c->pipe_windows = c->pipe_frames = 0;
    return KM_OK;
}

static int ensure_pipeline(Context* c, int64_t B, int64_t n_frames) {
    if (!c->pipe_s1) {
        hipStream_t s;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); c->pipe_s1 = s;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); c->pipe_s2 = s;
        for (int i = 0; i < 2; ++i) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->pipe_ev_in[i] = e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->pipe_ev_mel[i] = e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->pipe_ev_core[i] = e;
        }
    }
    if (B <= c->pipe_windows && n_frames <= c->pipe_frames) return KM_OK;
    HIP_TRY(hipDeviceSynchronize());                       // growing the slots: nothing may be in flight
    if (int rc = free_pipeline(c)) return rc;
    const int64_t W = B, F = n_frames;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->pipe_melpow[i]), (size_t)W * F * c->NK * sizeof(float)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->pipe_melmax[i]), (size_t)W * sizeof(unsigned)));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->pipe_zemo[i]), (size_t)W * sizeof(float)));
    }
    c->pipe_windows = W; c->pipe_frames = F; c->pipe_seq = 0;
    return KM_OK;
}

int km_forward_audio_pipelined(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                               float* out_dev, float* state_dev, int32_t first, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (!audio_dev || !emotion_dev || !out_dev || B <= 0 || L <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_forward_audio_pipelined: bad argument");
    if (!c->fused_ok) return fail(KM_ERR_UNSUPPORTED, "the pipelined mode needs the fused kernel shape (d_model 256, window 256, 8 heads)");
    const int64_t n_frames = 1 + L / c->cfg.mel.hop_length;
    if (B > c->ws_windows || n_frames > c->ws_frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve", (long long)B, (long long)L);
    if (int rc = ensure_pipeline(c, B > c->ws_windows ? B : c->ws_windows, n_frames > c->ws_frames ? n_frames : c->ws_frames)) return rc;
    const int slot = (int)(c->pipe_seq & 1);
    hipStream_t caller = (hipStream_t)stream, s1 = (hipStream_t)c->pipe_s1, s2 = (hipStream_t)c->pipe_s2;
    const bool tm = c->stage_timing;
    // redirect the workspace pointers the launchers read to this call's slot
    float* keep_pow = c->ws_melpow; unsigned* keep_max = c->ws_melmax; float* keep_z = c->ws_zemo; const bool keep_dirty = c->melmax_dirty;
    c->ws_melpow = c->pipe_melpow[slot]; c->ws_melmax = c->pipe_melmax[slot]; c->ws_zemo = c->pipe_zemo[slot];
    c->melmax_dirty = c->pipe_dirty[slot];
    int rc = KM_OK;
    do {
        if (hipEventRecord((hipEvent_t)c->pipe_ev_in[slot], caller) != hipSuccess) { rc = fail(KM_ERR_HIP, "hipEventRecord failed"); break; }
        if (hipStreamWaitEvent(s1, (hipEvent_t)c->pipe_ev_in[slot], 0) != hipSuccess) { rc = fail(KM_ERR_HIP, "hipStreamWaitEvent failed"); break; }
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[0], s1);
        const bool fuse_emo = mel_fuses_emotion(c, c->mel_plans[0]);
        if (!fuse_emo && (rc = launch_emotion(c, emotion_dev, B, c->ws_zemo, s1))) break;
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[1], s1);
        if ((rc = launch_mel_power(c, c->mel_plans[0], mel_windows(audio_dev, B, L), s1, fuse_emo ? mel_emotion(emotion_dev, c->ws_zemo) : MelCarry{}))) break;
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[2], s1);
        (void)hipEventRecord((hipEvent_t)c->pipe_ev_mel[slot], s1);
        (void)hipStreamWaitEvent(s2, (hipEvent_t)c->pipe_ev_mel[slot], 0);
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[3], s2);
        if ((rc = launch_core_fused_db(c, c->mel_plans[0], B, n_frames, c->ws_zemo, out_dev, s2, core_workspace(state_dev, first)))) break;
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[4], s2);
        (void)hipEventRecord((hipEvent_t)c->pipe_ev_core[slot], s2);
        // stream-order visibility of the PREVIOUS call's result (and release of its slot for the next call)
        if (c->pipe_seq > 0) (void)hipStreamWaitEvent(caller, (hipEvent_t)c->pipe_ev_core[slot ^ 1], 0);
    } while (0);
    c->pipe_dirty[slot] = c->melmax_dirty;
    c->ws_melpow = keep_pow; c->ws_melmax = keep_max; c->ws_zemo = keep_z; c->melmax_dirty = keep_dirty;
    if (rc == KM_OK) c->pipe_seq += 1;
    return rc;
}

int km_pipeline_flush(km_handle h, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->pipe_seq > 0 && c->pipe_s1)
        HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)c->pipe_ev_core[(c->pipe_seq - 1) & 1], 0));
    return KM_OK;
}

int64_t km_sequence_num_outputs(km_handle h, int64_t L, int32_t stride_frames) {
    if (!h || L < 0 || stride_frames <= 0) return -1;
    const int64_t num_frames = L / h->cfg.mel.hop_length;                       // sequential_dual_stream_model.py:84
    const int64_t n = (num_frames - h->T) / stride_frames + 1;                   // :96 (floor division)
    const int64_t nn = (num_frames - h->T) >= 0 ? n : ((num_frames - h->T - (stride_frames - 1)) / stride_frames + 1);
    return nn > 1 ? nn : 1;
}

// Where a window's emotion logit comes from in km_sequence_forward_track: the rows of every clip's track and the closed-form
// window -> row map (SeqTrackMap).  Null: one vector per clip (km_sequence_forward).
struct SeqTrack { const float* track; int64_t K, first, interval, sample_offset, clip_len; };

// What km_sequence_forward_attn adds to a sequence call: the pre-weight sigmoid values (B, N, 52) and the head-averaged maps
// (B, N, 28, NK) of every window, indexed like out_dev, and / or an accumulator (km_attn_stats_*) that takes every tile's maps.
// With an accumulator and no caller's map the maps of a tile live in seq_attn and are overwritten by the next tile.
struct SeqOutputs { float* raw; float* attn; void* stats; };

static int sequence_forward(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev, const SeqTrack* trk,
                            int32_t stride_frames, int32_t smooth, float* out_dev, void* stream, const SeqOutputs& xo = SeqOutputs{nullptr, nullptr, nullptr}) {
    Context* c = h;
    if (!c->fused_ok && !c->ws_generic)
        return fail(KM_ERR_WORKSPACE, "generic workspace missing: call km_reserve after km_finalize");
    const int hop = c->cfg.mel.hop_length;
    const int64_t N = km_sequence_num_outputs(h, L, stride_frames);
    const int64_t W = (int64_t)c->T * hop;                 // window_samples (sequential_dual_stream_model.py:54)
    const int64_t step = (int64_t)stride_frames * hop;     // stride_samples (:55)
    const int64_t n_frames = 1 + W / hop;
    if (c->ws_windows < B || c->ws_windows < 1 || n_frames > c->ws_frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld clips / %lld-frame windows: call km_reserve",
                    (long long)B, (long long)n_frames);
    if (N > 0x7fffffff) return fail(KM_ERR_INVALID_ARG, "too many output frames");
    const int64_t total = B * N, tile = c->ws_windows;
    // Shared-frame path.  Windows start at multiples of the hop (:101-117), so frame f of window i IS clip frame
    // i*stride + f for f = 1 .. T-1; only frame 0 and frame T see the zero padding at the window boundary.  The STFT
    // of the clip is computed once (N-1)*stride + T + 1 frames instead of N * (T+1)), the two edge frames per window
    // separately, and the core reads its rows from both images.  Results are bit-identical to the per-window path.
    const bool dedup = !c->opt.seq_per_window;       // km_set_option: tests compare both paths
    MelPlan* plan = c->mel_plans[0];
    const bool shared = c->fused_ok && dedup && mel_rp_ok(c, plan) && N < (1 << 24);
    const int64_t nfc = (N - 1) * stride_frames + n_frames;                     // clip frames any window touches
    if (shared) {     // grow-only images and their per-row maxima; allocates, so refused inside a stream capture, before any launch
        const char* what = "km_sequence_forward: clip frames / windows";
        if (int rc = grow_buffer(&c->seq_pow, &c->seq_pow_cap, B * nfc, c->NK * sizeof(float), stream, what)) return rc;
        if (int rc = grow_buffer(&c->seq_fmax, &c->seq_fmax_cap, B * nfc, sizeof(unsigned), stream, what)) return rc;
        if (int rc = grow_buffer(&c->seq_edge, &c->seq_edge_cap, total, 2 * c->NK * sizeof(float), stream, what)) return rc;
        if (int rc = grow_buffer(&c->seq_emax, &c->seq_emax_cap, total, 2 * sizeof(unsigned), stream, what)) return rc;
    }
    const int64_t map_floats = (int64_t)28 * c->NK;
    const bool tile_maps = xo.stats && !xo.attn;     // the maps of one tile at a time, for the accumulator alone
    if (tile_maps)
        if (int rc = grow_buffer(&c->seq_attn, &c->seq_attn_cap, tile, map_floats * sizeof(float), stream, "km_sequence_forward_attn: maps of one tile")) return rc;
    // rows of tile w0: the caller's arrays at w0, or the tile buffer
    auto raw_at = [&](int64_t w0) { return xo.raw ? xo.raw + w0 * c->NB : nullptr; };
    auto attn_at = [&](int64_t w0) { return xo.attn ? xo.attn + w0 * map_floats : (tile_maps ? c->seq_attn : nullptr); };
    auto stats_take = [&](int64_t w0, int64_t nw) { return xo.stats ? km_attn_stats_update(xo.stats, attn_at(w0), nw, stream) : KM_OK; };
    const float* zemo = c->ws_zemo;
    if (trk) {
        // a logit per track ROW (about nine windows share one), then one per window by the closed-form map: the core launches
        // below read zwin[win0 + b]
        const char* what = "km_sequence_forward_track: track rows / windows";
        if (int rc = grow_buffer(&c->seq_ztrack, &c->seq_ztrack_cap, B * trk->K, sizeof(float), stream, what)) return rc;
        if (int rc = grow_buffer(&c->seq_zwin, &c->seq_zwin_cap, total, sizeof(float), stream, what)) return rc;
        if (int rc = launch_emotion(c, trk->track, B * trk->K, c->seq_ztrack, stream)) return rc;
        const SeqTrackMap map{trk->K, trk->first, trk->interval, trk->sample_offset, trk->clip_len, step, W};
        if (int rc = launch_seq_track_logits(c, c->seq_ztrack, c->seq_zwin, total, (int)N, map, stream)) return rc;
        zemo = c->seq_zwin;
    } else {
        // emotion features ONCE for the entire audio (:88): one logit per clip
        if (int rc = launch_emotion(c, emotion_dev, B, c->ws_zemo, stream)) return rc;
    }
    if (shared) {
        hipStream_t st = (hipStream_t)stream;
        HIP_TRY(hipMemsetAsync(c->seq_fmax, 0, (size_t)B * nfc * sizeof(unsigned), st));
        HIP_TRY(hipMemsetAsync(c->seq_emax, 0, (size_t)total * 2 * sizeof(unsigned), st));
        // (1) every clip as one long "window" of nfc frames, zero beyond the clip end
        const SeqFrames clip_img{c->seq_pow, c->seq_fmax, nfc, 1};
        if (int rc = launch_mel_power(c, plan, mel_clip_windows(audio_dev, L, B, (nfc - 1) * hop, 0, 0, 1), stream, mel_to_frames(&clip_img))) return rc;
        // (2) the first and last frame of every window (rows 0 and 1 = frames 0 and T of the window)
        const SeqFrames edge_img{c->seq_edge, c->seq_emax, 2, (int)(n_frames - 1)};
        if (int rc = launch_mel_power(c, plan, mel_clip_windows(audio_dev, L, total, W, step, 0, (int)N), stream, mel_to_frames(&edge_img))) return rc;
        // (3) per tile: window maxima, then the fused core reading rows from both images
        const SeqCore sc{c->seq_pow, c->seq_edge, (int)nfc, (int)stride_frames, (int)N};
        for (int64_t w0 = 0; w0 < total; w0 += tile) {
            const int64_t nw = (total - w0) < tile ? (total - w0) : tile;
            if (int rc = launch_seq_window_max(c, c->seq_fmax, c->seq_emax, nw, w0, (int)nfc, (int)stride_frames, (int)N,
                                               (int)n_frames, stream)) return rc;
            if (int rc = launch_core_fused_db(c, plan, nw, n_frames, zemo, out_dev + w0 * c->NB, stream,
                                              with_outputs(trk ? core_strided_win(&sc, w0) : core_strided(&sc, w0), raw_at(w0), attn_at(w0)))) return rc;
            if (int rc = stats_take(w0, nw)) return rc;
        }
        if (smooth) return launch_ema_scan(c, out_dev, B, N, stream);
        return KM_OK;
    }
    for (int64_t w0 = 0; w0 < total; w0 += tile) {
        const int64_t nw = (total - w0) < tile ? (total - w0) : tile;
        const MelSrc src = mel_clip_windows(audio_dev, L, nw, W, step, w0, (int)N);
        if (c->fused_ok) {
            if (int rc = launch_mel_power(c, plan, src, stream)) return rc;
            if (int rc = launch_core_fused_db(c, plan, nw, n_frames, zemo, out_dev + w0 * c->NB, stream,
                                              with_outputs(trk ? core_workspace_seq_win(w0) : core_workspace_seq(w0, (int)N), raw_at(w0), attn_at(w0)))) return rc;
        } else {
            // generic shapes: staged log-mel, per-window logits gathered from the per-clip ones, GEMM-chain core
            if (int rc = launch_mel(c, plan, src, 0, c->ws_mel, c->ws_short, stream)) return rc;
            if (!trk)
                if (int rc = launch_gather_clip_logits(c, c->ws_zemo, c->ws_zemo_win, nw, w0, (int)N, stream)) return rc;
            if (int rc = launch_core_generic(c, c->ws_mel, nw, n_frames, c->ws_short, trk ? zemo + w0 : c->ws_zemo_win, out_dev + w0 * c->NB,
                                             raw_at(w0), attn_at(w0), stream)) return rc;
        }
        if (int rc = stats_take(w0, nw)) return rc;
    }
    if (smooth) return launch_ema_scan(c, out_dev, B, N, stream);
    return KM_OK;
}

int km_sequence_forward(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                        int32_t stride_frames, int32_t smooth, float* out_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    if (!audio_dev || !emotion_dev || !out_dev || B <= 0 || L <= 0 || stride_frames <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward: bad argument");
    return sequence_forward(h, audio_dev, B, L, emotion_dev, nullptr, stride_frames, smooth, out_dev, stream);
}

int km_sequence_forward_track(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* track_dev, int64_t K,
                              int64_t first_samples, int64_t interval_samples, int64_t sample_offset, int64_t clip_len,
                              int32_t stride_frames, int32_t smooth, float* out_dev, void* stream) {
    // the argument checks need no handle state and come first: they hold on a handle that is not finalized yet
    if (!h || !audio_dev || !track_dev || !out_dev || B <= 0 || L <= 0 || stride_frames <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_track: bad argument");
    const int64_t lim = (int64_t)1 << 62;                  // keeps sample_offset + (window index) * step + window inside int64
    if (K < 1 || interval_samples < 1 || first_samples < 0 || sample_offset < 0 || clip_len > lim || clip_len < L ||
        clip_len - L < sample_offset)
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_track: K %lld, first %lld, interval %lld, offset %lld, clip_len %lld for a chunk of %lld",
                    (long long)K, (long long)first_samples, (long long)interval_samples, (long long)sample_offset, (long long)clip_len,
                    (long long)L);
    if (K > 0x7fffffff / B) return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_track: %lld x %lld track rows, at most 2^31 - 1", (long long)B, (long long)K);
    if (int rc = need_dual(h)) return rc;
    const SeqTrack trk{track_dev, K, first_samples, interval_samples, sample_offset, clip_len};
    return sequence_forward(h, audio_dev, B, L, nullptr, &trk, stride_frames, smooth, out_dev, stream);
}

int km_sequence_forward_attn(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                             const float* track_dev, int64_t K, int64_t first_samples, int64_t interval_samples,
                             int64_t sample_offset, int64_t clip_len, int32_t stride_frames, int32_t smooth,
                             float* out_dev, float* raw_dev, float* attn_dev, void* stats, void* stream) {
    // as in km_sequence_forward_track, the argument checks need no handle state and come first
    if (!h || !audio_dev || !out_dev || B <= 0 || L <= 0 || stride_frames <= 0 || (emotion_dev != nullptr) == (track_dev != nullptr))
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: bad argument (exactly one of emotion_dev and track_dev)");
    if (track_dev) {
        const int64_t lim = (int64_t)1 << 62;
        if (K < 1 || interval_samples < 1 || first_samples < 0 || sample_offset < 0 || clip_len > lim || clip_len < L ||
            clip_len - L < sample_offset)
            return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: K %lld, first %lld, interval %lld, offset %lld, clip_len %lld for a chunk of %lld",
                        (long long)K, (long long)first_samples, (long long)interval_samples, (long long)sample_offset, (long long)clip_len,
                        (long long)L);
        if (K > 0x7fffffff / B) return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: %lld x %lld track rows, at most 2^31 - 1", (long long)B, (long long)K);
    }
    if (stats && attn_dev && !aligned16(attn_dev))
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: with an accumulator attn_dev must be 16-byte aligned");
    if (int rc = need_dual(h)) return rc;
    if (stats) {
        int32_t q = 0, k = 0;
        if (int rc = km_attn_stats_shape(stats, &q, &k)) return rc;
        if (q != 28 || k != h->NK)
            return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: the accumulator holds %d x %d maps, the model's are 28 x %d", q, k, h->NK);
    }
    if (attn_dev || stats)
        if (int rc = attn_refused(h, "km_sequence_forward_attn")) return rc;
    const SeqOutputs xo{raw_dev, attn_dev, stats};
    if (track_dev) {
        const SeqTrack trk{track_dev, K, first_samples, interval_samples, sample_offset, clip_len};
        return sequence_forward(h, audio_dev, B, L, nullptr, &trk, stride_frames, smooth, out_dev, stream, xo);
    }
    return sequence_forward(h, audio_dev, B, L, emotion_dev, nullptr, stride_frames, smooth, out_dev, stream, xo);
}

}  // extern "C"
