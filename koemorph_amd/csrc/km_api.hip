// C-ABI entry points that touch the device (declared in include/koemorph.h): handle lifecycle, front end, core, forward calls.
// Training: km_api_train.hip; streams: km_api_stream.hip; sequence mode: km_api_seq.hip.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "km_api_internal.h"
#include "km_context.h"
#include "km_device.h"
#include "km_gemm.h"

using namespace km;

namespace km {

int reserve_koemorph(Context* c, int64_t max_batch, int64_t max_frames) {
    if (max_batch <= c->kmm_batch && max_frames <= c->kmm_frames) return KM_OK;
    const int64_t Bm = max_batch > c->kmm_batch ? max_batch : c->kmm_batch, Tm = max_frames > c->kmm_frames ? max_frames : c->kmm_frames;
    c->kmm_batch = c->kmm_frames = 0;
    if (int rc = c->ws.generic.alloc(Bm * koemorph_ws_floats(c, Tm), "km_koemorph_reserve")) return rc;
    c->kmm_batch = Bm; c->kmm_frames = Tm;
    return KM_OK;
}

}  // namespace km

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
        if (!p.dev)
            if (int rc = p.dev.alloc((int64_t)p.host.size(), "km_finalize")) return rc;
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
    if (max_windows <= c->ws.windows && frames <= c->ws.frames && max_mels <= c->ws.mels && (c->ws.generic || !need_generic)) return KM_OK;
    const int64_t W = max_windows > c->ws.windows ? max_windows : c->ws.windows;
    const int64_t F = frames > c->ws.frames ? frames : c->ws.frames;
    const int64_t S = max_samples > c->ws.samples ? max_samples : c->ws.samples;
    c->ws = Workspace{};         // the old workspace goes first; the sizes are written when the new one is whole
    Workspace ws;
    const char* what = "km_reserve";
    if (int rc = ws.zemo.alloc(W, what)) return rc;
    if (int rc = ws.zemo_win.alloc(W, what)) return rc;
    if (int rc = ws.melmax.alloc(W, what)) return rc;
    // zero from the start, not only through the memset the first front-end launch issues (melmax_dirty): where that launch is
    // recorded into a stream capture the memset is a node of the graph and does not run, and the eager launches that follow
    // raised their maxima over whatever the allocation held (km_stream_tick captured before its first eager tick)
    HIP_TRY(hipMemset(ws.melmax, 0, (size_t)W * sizeof(unsigned)));
    if (int rc = ws.mel_short.alloc(W * 3 * max_mels, what)) return rc;
    if (F > 0) {
        if (int rc = ws.melpow.alloc(W * F * max_mels, what)) return rc;
        if (int rc = ws.mel.alloc(W * F * max_mels, what)) return rc;
    }
    if (need_generic) {
        const int64_t per = c->kind == 1 ? legacy_ws_floats(c, F > 0 ? F : 1) : generic_ws_floats(c);
        if (int rc = ws.generic.alloc(W * per, what)) return rc;
    }
    ws.windows = W; ws.frames = F; ws.samples = S; ws.mels = max_mels;
    c->ws = std::move(ws);
    c->melmax_dirty = true;
    return ensure_chunk_counters(c, W, nullptr);
}

int km_destroy(km_handle h) {
    delete h;      // every buffer, event and stream frees itself (km_devbuf.h)
    return KM_OK;
}

int64_t km_live_device_bytes(void) { return g_live_device_bytes.load(); }

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
        if (cfg->n_mels > h->ws.mels && h->ws.windows > 0) {
            // the workspace rows were sized for narrower plans: regrow it now (this first-use path allocates anyway)
            HIP_TRY(hipDeviceSynchronize());
            if (int rc = km_reserve(h, h->ws.windows, h->ws.samples)) return rc;
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
    if (B > c->ws.windows) return fail(KM_ERR_WORKSPACE, "workspace holds %lld windows, need %lld: call km_reserve",
                                       (long long)c->ws.windows, (long long)B);
    if (int rc = launch_emotion(c, emotion_dev, B, c->ws.zemo, stream)) return rc;
    if (!c->fused_ok) {
        if (!c->ws.generic) return fail(KM_ERR_WORKSPACE, "generic workspace missing: call km_reserve after km_finalize");
        return launch_core_generic(c, mel_dev, B, T_in, mel_short_dev, c->ws.zemo, out_dev, raw_dev, attn_mel_dev, stream);
    }
    return launch_core_fused(c, mel_dev, B, T_in, mel_short_dev, c->ws.zemo, out_dev, raw_dev, attn_mel_dev,
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
        if (B > c->ws.windows || !c->ws.generic) return fail(KM_ERR_WORKSPACE, "generic workspace missing or too small: call km_reserve after km_finalize");
        return launch_core_generic(c, mel_dev, B, T_in, mel_short_dev, z_dev, out_dev, raw_dev, attn_mel_dev, stream);
    }
    return launch_core_fused(c, mel_dev, B, T_in, mel_short_dev, z_dev, out_dev, raw_dev, attn_mel_dev, nullptr, 1, stream);
}

static GemmArgs linear_args(const float* x_dev, const float* w_dev, const float* b_dev, int64_t B, int64_t K, int64_t N, float* out_dev) {
    GemmArgs g{};
    g.alpha = 1.f; g.batch2 = 1; g.kb_count = 1;
    g.A = x_dev; g.a_rs = K; g.a_cs = 1; g.B = w_dev; g.b_rs = 1; g.b_cs = K; g.C = out_dev; g.c_rs = N;
    g.M = (int)B; g.N = (int)N; g.K = (int)K; g.bias = b_dev; g.bias_mode = b_dev ? 1 : 0;
    return g;
}

int km_linear(const float* x_dev, const float* w_dev, const float* b_dev, int64_t B, int64_t K, int64_t N, float* out_dev, void* stream) {
    if (!x_dev || !w_dev || !out_dev || B <= 0 || K <= 0 || N <= 0) return fail(KM_ERR_INVALID_ARG, "km_linear: bad argument");
    return launch_gemm(linear_args(x_dev, w_dev, b_dev, B, K, N, out_dev), 1, stream);
}

int km_gemm_kernel_choice(int64_t M, int64_t N, int64_t K, int64_t batch) {
    if (M <= 0 || N <= 0 || K <= 0 || batch <= 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX || batch > INT32_MAX) return -1;
    return gemm_kernel_choice(linear_args(nullptr, nullptr, nullptr, M, K, N, nullptr), (int)batch);
}

int km_mel_role_table(int64_t windows, int32_t per_window, int32_t group, int64_t n_ids, int32_t* out) {
    return mel_role_table(windows, per_window, group, n_ids, out);
}

int km_audio_energy(const float* features_dev, int64_t B, int64_t T, int64_t D, float* energy_dev, void* stream) {
    if (!features_dev || !energy_dev || B <= 0 || T <= 0 || D <= 0) return fail(KM_ERR_INVALID_ARG, "km_audio_energy: bad argument");
    return launch_audio_energy(features_dev, B, T, D, energy_dev, stream);
}

int km_legacy_forward_mel(km_handle h, const float* mel_dev, int64_t B, int64_t T_mel, float* out_dev, void* stream) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "not a legacy handle (km_legacy_create)");
    if (!mel_dev || !out_dev || B <= 0 || T_mel <= 0) return fail(KM_ERR_INVALID_ARG, "km_legacy_forward_mel: bad argument");
    if (B > c->ws.windows || T_mel > c->ws.frames || !c->ws.generic)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld frames: call km_reserve",
                    (long long)B, (long long)T_mel);
    return launch_legacy(c, mel_dev, B, T_mel, out_dev, stream);
}

int km_koemorph_reserve(km_handle h, int64_t max_batch, int64_t max_frames) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 2) return fail(KM_ERR_INVALID_ARG, "not a KoeMorphModel handle (km_koemorph_create)");
    if (max_batch <= 0 || max_frames <= 0) return fail(KM_ERR_INVALID_ARG, "km_koemorph_reserve: bad argument");
    return reserve_koemorph(c, max_batch, max_frames);
}

int km_koemorph_forward(km_handle h, const float* mel_dev, const float* emotion_dev, int64_t B, int64_t T,
                        const uint8_t* audio_mask_dev, const float* prev_dev, float* smoother_state_dev,
                        int32_t apply_constraints, float* out_dev, float* raw_dev, float* attn_dev, void* stream) {
    if (int rc = need_ready(h)) return rc;
    Context* c = h;
    if (c->kind != 2) return fail(KM_ERR_INVALID_ARG, "not a KoeMorphModel handle (km_koemorph_create)");
    if (!mel_dev || !emotion_dev || !out_dev || B <= 0 || T <= 0) return fail(KM_ERR_INVALID_ARG, "km_koemorph_forward: bad argument");
    // the workspace is carved per call for (B, T): B * ws(T) floats must fit what km_koemorph_reserve allocated
    if (!c->ws.generic || B * koemorph_ws_floats(c, T) > c->kmm_batch * koemorph_ws_floats(c, c->kmm_frames))
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
    if (B > c->ws.windows || n_frames > c->ws.frames || !c->ws.generic)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve",
                    (long long)B, (long long)L);
    if (legacy_pow_ok(c)) {
        // front end -> power-mel + window maxima; the fused encoder converts to dB while it stages its rows and the attention
        // kernel re-zeroes the maxima: no mel_log_kernel launch, no memset (round 4; 18 us of the 460 per 256 windows)
        if (int rc = launch_mel_power(c, c->mel_plans[0], mel_windows(audio_dev, B, L), stream)) return rc;
        const LogParams lp = plan_log_params(c->mel_plans[0]);
        const LegacyPowSrc src{c->ws.melpow, c->ws.melmax, &lp};
        return launch_legacy(c, nullptr, B, n_frames, out_dev, stream, &src);
    }
    if (int rc = launch_mel(c, c->mel_plans[0], mel_windows(audio_dev, B, L), 0, c->ws.mel, nullptr, stream)) return rc;
    return launch_legacy(c, c->ws.mel, B, n_frames, out_dev, stream);
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
    if (B > c->ws.windows || n_frames > c->ws.frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve",
                    (long long)B, (long long)L);
    MelPlan* plan = c->mel_plans[0];
    const MelSrc src = mel_windows(audio_dev, B, L);
    if (!c->fused_ok && !c->ws.generic) return fail(KM_ERR_WORKSPACE, "generic workspace missing: call km_reserve after km_finalize");
    if (core_takes_power(c, attn_dev != nullptr)) {
        // emotion logits (inside the front-end kernel where it can carry them), power-mel + window maxima, then the fused core or
        // a generic one, either converting to dB as it loads its rows: no log-mel image at all.  Stage events on the fused shape alone
        hipStream_t st = (hipStream_t)stream;
        const bool tm = c->fused_ok && c->stage_timing;
        if (tm) HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[0], st));
        if (int rc = launch_mel_power_with_logits(c, plan, src, emotion_dev, c->ws.zemo, stream, tm ? (hipEvent_t)c->stage_ev[1] : nullptr)) return rc;
        if (tm) { HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[2], st)); HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[3], st)); }
        if (int rc = launch_core_power(c, plan, B, n_frames, c->ws.zemo, out_dev, stream,
                                       with_outputs(core_workspace(state_dev, first), raw_dev, attn_dev))) return rc;
        if (tm) HIP_TRY(hipEventRecord((hipEvent_t)c->stage_ev[4], st));
        return KM_OK;
    }
    // generic shapes without a power path: staged front end, GEMM-chain core, stand-alone EMA
    if (int rc = launch_emotion(c, emotion_dev, B, c->ws.zemo, stream)) return rc;
    if (c->NK == 80 && !c->opt.generic_staged) {
        // log-mel written straight into the packed encoder input; long + short-term rows in one contraction
        float* xp = generic_packed_x(c, B);
        if (int rc = launch_mel_packed(c, plan, src, xp, c->T, (c->KT + 15) / 16 * 16, stream)) return rc;
        if (int rc = launch_core_generic_packed(c, xp, B, c->ws.zemo, out_dev, raw_dev, attn_dev, stream)) return rc;
    } else {
        if (int rc = launch_mel(c, plan, src, 0, c->ws.mel, c->ws.mel_short, stream)) return rc;
        if (int rc = launch_core_generic(c, c->ws.mel, B, n_frames, c->ws.mel_short, c->ws.zemo, out_dev, raw_dev, attn_dev, stream)) return rc;
    }
    if (state_dev) return launch_smooth(c, out_dev, state_dev, B, first, stream);
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
    return forward_clip_ok(h) || clip_plan(h, 1, 0, 0, 0).route == 2 ? 1 : 0;      // (the route does not depend on the batch)
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
    // option clip_assemble: a handle refused here by default takes the assembled route (km_clip_plan route 2); one accepted keeps its route
    const ClipPlan cp = clip_plan(c, B, min_start_frame, max_start_frame, attn_dev ? 2 : 0);
    const bool assembled = !forward_clip_ok(c) && cp.route == 2;
    if (!forward_clip_ok(c) && !assembled)
        return fail(KM_ERR_UNSUPPORTED, "km_forward_clip: needs the fused core (d_model 256, window 256, 8 heads) behind the 1024-point "
                    "front end with constant padding and hop >= n_fft / 2 (hop %d, n_fft %d): gather the windows (km_gather_windows) "
                    "and call km_forward_audio", m.hop_length, m.n_fft);
    const int64_t T = c->T, hop = m.hop_length;
    const int64_t n_span = (int64_t)(max_start_frame - min_start_frame) + T + 1;
    if (clip_len >= (1ll << 31) || ((int64_t)max_start_frame + T + 2) * hop >= (1ll << 31) || n_span * c->NK >= (1ll << 31))
        return fail(KM_ERR_INVALID_ARG, "km_forward_clip: clip or start frame beyond 2^31 samples");
    if (B > c->ws.windows)
        return fail(KM_ERR_WORKSPACE, "workspace holds %lld windows, need %lld: call km_reserve", (long long)c->ws.windows, (long long)B);
    if (assembled) {
        if (attn_dev)
            if (int rc = attn_refused(c, "km_forward_clip_attn")) return rc;
        if (!c->fused_ok && !c->ws.generic) return fail(KM_ERR_WORKSPACE, "generic workspace missing: call km_reserve after km_finalize");
        if (T + 1 > c->ws.frames)
            return fail(KM_ERR_WORKSPACE, "workspace holds %lld frames a window, need %lld: call km_reserve", (long long)c->ws.frames, (long long)(T + 1));
        // emotion logits, the span and edge images, the windows' rows and maxima into the workspace, then the core km_forward_audio
        // runs on its power path (the assemble kernel stores the maxima it needs; the slots of a fresh workspace beyond the batch
        // are cleared as launch_mel_power clears them, because the core launches below declare the maxima clean)
        MelPlan* plan = c->mel_plans[0];
        // The logits have to be the ones km_forward_audio computes.  At d_model 256 its rider and emotion_kernel_d256 are
        // bit-identical; at the other shapes the rider sums in another order than emotion_kernel, so the rider itself runs: an
        // ordinary front-end launch over B windows of one zero sample (one frame each, rows and maxima the assemble kernel
        // overwrites; the pointer stays inside the clip).
        if (mel_fuses_emotion(c, plan) && !(c->d == 256 && c->DH == 128)) {
            if (int rc = launch_mel_power(c, plan, mel_clip_windows(clip_dev, 0, B, 1, 0, 0, 1), stream, mel_emotion(emotion_dev, c->ws.zemo))) return rc;
        } else {
            if (int rc = launch_emotion(c, emotion_dev, B, c->ws.zemo, stream)) return rc;
        }
        if (int rc = launch_clip_images(c, plan, clip_dev, clip_len, start_frames_dev, B, min_start_frame, n_span, cp.E, stream)) return rc;
        if (int rc = clear_stale_maxima(c, stream)) return rc;
        if (int rc = launch_clip_assemble(c, start_frames_dev, B, min_start_frame, n_span, cp.E, stream)) return rc;
        return launch_core_power(c, plan, B, T + 1, c->ws.zemo, out_dev, stream, with_outputs(core_workspace(state_dev, first), raw_dev, attn_dev));
    }
    // grow-only; allocates, so not inside a stream capture
    if (int rc = c->seq.fwd_span.grow(n_span * c->NK, stream, "km_forward_clip: floats of the span image")) return rc;
    if (int rc = c->seq.fwd_edge.grow(B * 2 * c->NK, stream, "km_forward_clip: floats of the edge image")) return rc;
    // four launches: emotion logits (emotion_kernel_d256: bit-identical to the rider inside km_forward_audio's front end), the
    // span + edge images, the window maxima, the fused core reading its rows through the table
    if (int rc = launch_emotion(c, emotion_dev, B, c->ws.zemo, stream)) return rc;
    if (int rc = launch_mel_clip_span(c, c->mel_plans[0], clip_dev, clip_len, start_frames_dev, B, min_start_frame, n_span, (int)T,
                                      c->seq.fwd_span, c->seq.fwd_edge, stream)) return rc;
    if (int rc = launch_clip_window_max(c, c->seq.fwd_span, c->seq.fwd_edge, start_frames_dev, B, min_start_frame, n_span, (int)(T + 1),
                                        stream)) return rc;
    const ClipTable tab{c->seq.fwd_span, c->seq.fwd_edge, (int)n_span, start_frames_dev, min_start_frame};
    return launch_core_fused_db(c, c->mel_plans[0], B, T + 1, c->ws.zemo, out_dev, stream,
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

static int ensure_pipeline(Context* c, int64_t B, int64_t n_frames) {
    if (!c->pipe.s1) {
        hipStream_t s;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); c->pipe.s1 = s;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); c->pipe.s2 = s;
        for (int i = 0; i < 2; ++i) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->pipe.ev_in[i] = e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->pipe.ev_mel[i] = e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->pipe.ev_core[i] = e;
        }
    }
    if (B <= c->pipe.windows && n_frames <= c->pipe.frames) return KM_OK;
    HIP_TRY(hipDeviceSynchronize());                       // growing the slots: nothing may be in flight
    c->pipe.windows = c->pipe.frames = 0;
    for (PipeSlot& s : c->pipe.slot) s = PipeSlot{};
    const int64_t W = B, F = n_frames;
    for (PipeSlot& s : c->pipe.slot) {
        if (int rc = s.melpow.alloc(W * F * c->NK, "km_forward_audio_pipelined")) return rc;
        if (int rc = s.melmax.alloc(W, "km_forward_audio_pipelined")) return rc;
        if (int rc = s.zemo.alloc(W, "km_forward_audio_pipelined")) return rc;
    }
    c->pipe.windows = W; c->pipe.frames = F; c->pipe.seq = 0;
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
    if (B > c->ws.windows || n_frames > c->ws.frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve", (long long)B, (long long)L);
    if (int rc = ensure_pipeline(c, B > c->ws.windows ? B : c->ws.windows, n_frames > c->ws.frames ? n_frames : c->ws.frames)) return rc;
    const int slot = (int)(c->pipe.seq & 1);
    hipStream_t caller = (hipStream_t)stream, s1 = (hipStream_t)c->pipe.s1, s2 = (hipStream_t)c->pipe.s2;
    const bool tm = c->stage_timing;
    // the launchers read the workspace: for the length of this call its buffers and this call's slot change places
    PipeSlot& ps = c->pipe.slot[slot];
    auto swap_slot = [&] { std::swap(c->ws.melpow, ps.melpow); std::swap(c->ws.melmax, ps.melmax); std::swap(c->ws.zemo, ps.zemo); };
    const bool keep_dirty = c->melmax_dirty;
    swap_slot();
    c->melmax_dirty = ps.dirty;
    int rc = KM_OK;
    do {
        if (hipEventRecord((hipEvent_t)c->pipe.ev_in[slot], caller) != hipSuccess) { rc = fail(KM_ERR_HIP, "hipEventRecord failed"); break; }
        if (hipStreamWaitEvent(s1, (hipEvent_t)c->pipe.ev_in[slot], 0) != hipSuccess) { rc = fail(KM_ERR_HIP, "hipStreamWaitEvent failed"); break; }
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[0], s1);
        if ((rc = launch_mel_power_with_logits(c, c->mel_plans[0], mel_windows(audio_dev, B, L), emotion_dev, c->ws.zemo, s1,
                                               tm ? (hipEvent_t)c->stage_ev[1] : nullptr))) break;
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[2], s1);
        (void)hipEventRecord((hipEvent_t)c->pipe.ev_mel[slot], s1);
        (void)hipStreamWaitEvent(s2, (hipEvent_t)c->pipe.ev_mel[slot], 0);
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[3], s2);
        if ((rc = launch_core_fused_db(c, c->mel_plans[0], B, n_frames, c->ws.zemo, out_dev, s2, core_workspace(state_dev, first)))) break;
        if (tm) (void)hipEventRecord((hipEvent_t)c->stage_ev[4], s2);
        (void)hipEventRecord((hipEvent_t)c->pipe.ev_core[slot], s2);
        // stream-order visibility of the PREVIOUS call's result (and release of its slot for the next call)
        if (c->pipe.seq > 0) (void)hipStreamWaitEvent(caller, (hipEvent_t)c->pipe.ev_core[slot ^ 1], 0);
    } while (0);
    ps.dirty = c->melmax_dirty;
    swap_slot();
    c->melmax_dirty = keep_dirty;
    if (rc == KM_OK) c->pipe.seq += 1;
    return rc;
}

int km_pipeline_flush(km_handle h, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->pipe.seq > 0 && c->pipe.s1)
        HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)c->pipe.ev_core[(c->pipe.seq - 1) & 1], 0));
    return KM_OK;
}

}  // extern "C"
