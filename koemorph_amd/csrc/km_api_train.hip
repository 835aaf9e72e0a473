// C-ABI entry points of the training steps: km_train_* and km_legacy_train_* (declared in include/koemorph.h).
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

static int need_legacy_train(Context* c, int64_t B) {
    if (int rc = need_ready(c)) return rc;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "this entry point needs a legacy handle (km_legacy_create)");
    if (!c->tr.params || !c->tr.l_ws) return fail(KM_ERR_NOT_FINALIZED, "call km_legacy_train_init first");
    if (B <= 0 || B > c->tr.windows) return fail(KM_ERR_WORKSPACE, "km_legacy_train_init sized the step for %lld windows, got %lld",
                                                 (long long)c->tr.windows, (long long)B);
    return KM_OK;
}

extern "C" {

static int upload_train_params(Context* c, void* stream) {
    std::vector<float> flat((size_t)c->tr.nparams);
    for (const auto& k : c->param_order) {
        const HostParam& hp = c->params.at(k);
        std::memcpy(flat.data() + c->tr.offset.at(k), hp.data.data(), hp.data.size() * sizeof(float));
    }
    HIP_TRY(hipMemcpyAsync(c->tr.params, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
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

// span image (span_rows, NK) and edge image (windows, 2, NK) of km_train_step_clip in ONE allocation: the pack kernel
// addresses both with 32-bit offsets from one base
static int alloc_clip_images(Context* c, int64_t span_rows, int64_t windows) {
    c->tr.clip_span.release();
    c->tr.clip_edge = nullptr; c->tr.clip_span_rows = 0;
    if ((span_rows + 2 * windows) * c->NK >= (1ll << 31)) return fail(KM_ERR_WORKSPACE, "km_train_step_clip: span of %lld frames is too wide", (long long)span_rows);
    if (int rc = c->tr.clip_span.alloc((span_rows + 2 * windows) * c->NK, "km_train_step_clip: span and edge images")) return rc;
    c->tr.clip_edge = c->tr.clip_span + span_rows * c->NK;
    c->tr.clip_span_rows = span_rows;
    return KM_OK;
}

// fills the fresh c->tr; tr.windows, the guard of every km_train_* call, is written when everything exists
static int train_init(Context* c, int64_t max_windows, void* stream) {
    const char* what = "km_train_init";
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
        if (pass == 1) c->tr.early = off;
        for (const auto& k : c->param_order) {
            if (late(k) != (pass == 1)) continue;
            c->tr.offset[k] = off;
            off += ((int64_t)c->params.at(k).data.size() + 3) / 4 * 4;
        }
    }
    c->tr.nparams = off;
    const size_t nb = (size_t)off * sizeof(float);
    if (int rc = c->tr.params.alloc(off, what)) return rc;
    if (int rc = c->tr.m.alloc(off, what)) return rc;
    if (int rc = c->tr.v.alloc(off, what)) return rc;
    HIP_TRY(hipMemsetAsync(c->tr.params, 0, nb, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(c->tr.m, 0, nb, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(c->tr.v, 0, nb, (hipStream_t)stream));
    if (int rc = c->tr.part.alloc(256, what)) return rc;
    if (int rc = c->tr.gnorm.alloc(1, what)) return rc;
    if (int rc = c->tr.loss.alloc(1, what)) return rc;
    {
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->tr.early_ev = ev;
    }
    if (int rc = c->tr.steps.alloc(2, what)) return rc;
    HIP_TRY(hipMemsetAsync(c->tr.steps, 0, 2 * sizeof(int), (hipStream_t)stream));
    {   // the step's workspace (km_trainp.hip): packed input first, then a fixed part, then per-window activations; dropout masks
        int64_t fixed = 0;
        const int64_t per = trainp_act_floats(c, &fixed);
        const int64_t KP = trainp_kp(c);
        if (int rc = c->tr.act.alloc(max_windows * (per + 2 * KP * c->NK) + fixed + 4096, what)) return rc;
        // the packed input's columns beyond T + 3 are written by nobody when the front end packs: zeros (they meet zero weights)
        HIP_TRY(hipMemsetAsync(c->tr.act, 0, (size_t)c->tr.act.bytes(), (hipStream_t)stream));
        if (int rc = c->tr.wcep.alloc((int64_t)c->d * KP, what)) return rc;
        // split-K partials: up to 16 partial outputs of every weight / bias gradient that is a product over the rows of the batch
        if (int rc = c->tr.split.alloc(16 * (5 * (int64_t)c->d * c->d + 2 * (int64_t)c->DH * c->d + 16 * (int64_t)c->d + (int64_t)c->d * c->KT) + 1024, what)) return rc;
        if (int rc = c->tr.tail_part.alloc((int64_t)1024 * 64, what)) return rc;      // one row of sums per tail workgroup
        if (int rc = c->tr.tail_ctr.alloc(1, what)) return rc;
        HIP_TRY(hipMemsetAsync(c->tr.tail_ctr, 0, sizeof(unsigned), (hipStream_t)stream));
        if (int rc = c->tr.masks.alloc(trainp_mask_alloc_bytes(c, max_windows), what)) return rc;
        HIP_TRY(hipMemsetAsync(c->tr.masks, 1, (size_t)c->tr.masks.n, (hipStream_t)stream));
        if (int rc = c->tr.drop_ctr.alloc(1, what)) return rc;
        HIP_TRY(hipMemsetAsync(c->tr.drop_ctr, 0, sizeof(int), (hipStream_t)stream));
    }
    if (train_clip_ok(c))       // km_train_step_clip: the span of a dense (stride 1) batch; a wider span grows the image on first use
        if (int rc = alloc_clip_images(c, max_windows + c->T + 1, max_windows)) return rc;
    if (int rc = upload_train_params(c, stream)) return rc;
    c->tr.windows = max_windows;
    return KM_OK;
}

int km_train_init(km_handle h, int64_t max_windows, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (max_windows <= 0) return fail(KM_ERR_INVALID_ARG, "km_train_init: bad max_windows");
    c->tr = TrainState{};
    const int rc = train_init(c, max_windows, stream);
    if (rc) c->tr = TrainState{};      // no half-built training state
    return rc;
}

int64_t km_train_num_params(km_handle h) { return h ? h->tr.nparams : -1; }

int64_t km_train_param_offset(km_handle h, const char* key) {
    if (!h || !key) return -1;
    auto it = h->tr.offset.find(key);
    return it == h->tr.offset.end() ? -1 : it->second;
}

static int need_train(Context* c, int64_t B) {
    if (int rc = need_dual(c)) return rc;
    if (!c->tr.params) return fail(KM_ERR_NOT_FINALIZED, "call km_train_init first");
    if (B <= 0 || B > c->tr.windows) return fail(KM_ERR_WORKSPACE, "km_train_init sized the step for %lld windows, got %lld",
                                                 (long long)c->tr.windows, (long long)B);
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
    if (B > c->ws.windows || n_frames > c->ws.frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve", (long long)B, (long long)L);
    // front end -> power-mel; phase 0 of the program converts and packs it into the encoder input (B, KP, n_mels) at the
    // head of the step's workspace
    // (round 4: the front end writes the packed dB input itself -- MelPack -- where it can; option train_no_fe_pack)
    const bool fe_packs = train_fe_packs(c, n_frames);
    const MelPack pack{c->tr.act, (int)c->T, (int)trainp_kp(c)};
    if (int rc = launch_mel_power(c, c->mel_plans[0], mel_windows(audio_dev, B, L), stream, fe_packs ? mel_to_pack(&pack) : MelCarry{})) return rc;
    c->melmax_dirty = true;      // until phase 1 / 2 has re-zeroed the maxima
    const LogParams lp = plan_log_params(c->mel_plans[0]);
    const TrainAudioSrc asrc{c->ws.melpow, c->ws.melmax, (int)n_frames, &lp, fe_packs};
    const TrainStepArgs sa{emotion_dev, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, ema_state_dev, ema_first, stream};
    return train_forward_backward(c, nullptr, B, n_frames, nullptr, c->tr.act, &asrc, sa);
}

int km_train_clip_supported(km_handle h) {
    if (!h || !h->dev_finalized || h->kind != 0 || !h->tr.params) return 0;
    return train_clip_ok(h) || clip_plan(h, 1, 0, 0, 1).route == 2 ? 1 : 0;      // (the route does not depend on the batch)
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
    // option clip_assemble: a handle refused here by default takes the assembled route (km_clip_plan route 2); one accepted keeps its route
    const ClipPlan cp = clip_plan(c, B, min_start_frame, max_start_frame, 1);
    const bool assembled = !train_clip_ok(c) && cp.route == 2;
    if (!train_clip_ok(c) && !assembled)
        return fail(KM_ERR_UNSUPPORTED, "km_train_step_clip: windows share STFT frames only with the packing 1024-point front end, constant "
                    "padding and hop >= n_fft / 2 (hop %d, n_fft %d): gather the windows (km_gather_windows) and call km_train_step_audio",
                    m.hop_length, m.n_fft);
    const int64_t T = c->T, hop = m.hop_length;
    const int64_t n_span = (int64_t)(max_start_frame - min_start_frame) + T + 1;
    if (clip_len >= (1ll << 31) || ((int64_t)max_start_frame + T + 2) * hop >= (1ll << 31))
        return fail(KM_ERR_INVALID_ARG, "km_train_step_clip: clip or start frame beyond 2^31 samples");
    if (B > c->ws.windows)
        return fail(KM_ERR_WORKSPACE, "workspace holds %lld windows, need %lld: call km_reserve", (long long)c->ws.windows, (long long)B);
    if (assembled) {
        // the span and the 2 B snippets through the front end as it is, then the packed input and the window maxima (stored: no
        // zeroed slots needed); behind them the step of km_train_step_audio's packing branch
        if (int rc = launch_clip_images(c, c->mel_plans[0], clip_dev, clip_len, start_frames_dev, B, min_start_frame, n_span, cp.E, stream)) return rc;
        if (int rc = launch_clip_pack_edges(c, c->mel_plans[0], start_frames_dev, B, min_start_frame, n_span, cp.E, (int)trainp_kp(c), c->tr.act,
                                            stream)) return rc;
        c->melmax_dirty = true;      // until phase 3 / 4 has re-zeroed the maxima
        const LogParams lp = plan_log_params(c->mel_plans[0]);
        const TrainAudioSrc asrc{c->ws.melpow, c->ws.melmax, (int)(T + 1), &lp, true};
        const TrainStepArgs sa{emotion_dev, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, ema_state_dev, ema_first, stream};
        return train_forward_backward(c, nullptr, B, T + 1, nullptr, c->tr.act, &asrc, sa);
    }
    if (n_span > c->tr.clip_span_rows) {     // grow-only, both images in one allocation (the edge image holds tr.windows >= B windows)
        if (int rc = growth_refused(stream, "km_train_step_clip: span frames", n_span, c->tr.clip_span_rows)) return rc;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if (int rc = alloc_clip_images(c, n_span, c->tr.windows)) return rc;
    }
    // (the pack kernel STORES the maxima of windows 0 .. B - 1: no zeroed slots needed, no memset whatever ran before)
    const int KP = (int)trainp_kp(c);
    if (int rc = launch_mel_clip_span(c, c->mel_plans[0], clip_dev, clip_len, start_frames_dev, B, min_start_frame, n_span, (int)T,
                                      c->tr.clip_span, c->tr.clip_edge, stream)) return rc;
    if (int rc = launch_train_clip_pack(c, c->mel_plans[0], c->tr.clip_span, c->tr.clip_edge, start_frames_dev, B, min_start_frame, n_span,
                                        (int)T, KP, c->tr.act, stream)) return rc;
    c->melmax_dirty = true;      // until phase 3 / 4 has re-zeroed the maxima
    const LogParams lp = plan_log_params(c->mel_plans[0]);
    const TrainAudioSrc asrc{c->ws.melpow, c->ws.melmax, (int)(T + 1), &lp, true};
    const TrainStepArgs sa{emotion_dev, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, ema_state_dev, ema_first, stream};
    return train_forward_backward(c, nullptr, B, T + 1, nullptr, c->tr.act, &asrc, sa);
}

int km_train_grad_split(km_handle h, int64_t* early_floats) {
    if (int rc = need_train(h, 1)) return rc;
    if (!early_floats) return fail(KM_ERR_INVALID_ARG, "km_train_grad_split: NULL argument");
    *early_floats = h->tr.early;
    return KM_OK;
}

int km_train_wait_early(km_handle h, void* stream) {
    if (int rc = need_train(h, 1)) return rc;
    if (!h->tr.early_recorded) return fail(KM_ERR_NOT_READY, "km_train_wait_early: no training step has run yet");
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)h->tr.early_ev, 0));
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
    if (h->tr.drop_ctr) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&v, h->tr.drop_ctr, sizeof(int), hipMemcpyDeviceToHost));
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
    if (!h->tr.drop_ctr) return fail(KM_ERR_NOT_READY, "%s: the training step is not initialised", fn);
    const int v = (int)step;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->tr.drop_ctr, &v, sizeof(int), hipMemcpyHostToDevice));
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
    if (!flat_host || n != h->tr.nparams) return fail(KM_ERR_INVALID_ARG, "%s: size mismatch", fn);
    HIP_TRY(hipMemcpy(flat_host, h->tr.params, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
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
    if (!flat_host || n != h->tr.nparams) return fail(KM_ERR_INVALID_ARG, "%s: size mismatch", fn);
    HIP_TRY(hipMemcpy(h->tr.params, flat_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
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
    if (!exp_avg_host || !exp_avg_sq_host || !steps2_host || n != h->tr.nparams)
        return fail(KM_ERR_INVALID_ARG, "%s: bad argument", fn);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(exp_avg_host, h->tr.m, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(exp_avg_sq_host, h->tr.v, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(steps2_host, h->tr.steps, 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
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
    if (!exp_avg_host || !exp_avg_sq_host || !steps2_host || n != h->tr.nparams)
        return fail(KM_ERR_INVALID_ARG, "%s: bad argument", fn);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->tr.m, exp_avg_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->tr.v, exp_avg_sq_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->tr.steps, steps2_host, 2 * sizeof(int32_t), hipMemcpyHostToDevice));
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
    std::vector<float> flat((size_t)c->tr.nparams);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(flat.data(), c->tr.params, flat.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (const auto& k : c->param_order) {
        HostParam& hp = c->params.at(k);
        std::memcpy(hp.data.data(), flat.data() + c->tr.offset.at(k), hp.data.size() * sizeof(float));
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
    c->tr = TrainState{};
    const int rc = legacy_train_init(c, max_windows, max_frames, stream);
    if (rc) c->tr = TrainState{};      // no half-built training state
    return rc;
}

int64_t km_legacy_train_num_params(km_handle h) { return h && h->kind == 1 ? h->tr.nparams : -1; }

int64_t km_legacy_train_param_offset(km_handle h, const char* key) {
    if (!h || !key || h->kind != 1) return -1;
    auto it = h->tr.offset.find(key);
    return it == h->tr.offset.end() ? -1 : it->second;
}

int km_legacy_train_step_mel(km_handle h, const float* mel_dev, int64_t B, int64_t T, const float* target_dev, float mse_weight,
                             float l1_weight, float* flat_grad_dev, float* loss_dev, float* out_dev, void* stream) {
    if (int rc = need_legacy_train(h, B)) return rc;
    if (!mel_dev || !target_dev || !flat_grad_dev || !loss_dev || T <= 0) return fail(KM_ERR_INVALID_ARG, "km_legacy_train_step_mel: bad argument");
    if (T > h->tr.l_frames) return fail(KM_ERR_WORKSPACE, "km_legacy_train_init sized the step for %lld frames, got %lld",
                                       (long long)h->tr.l_frames, (long long)T);
    return legacy_train_step(h, mel_dev, B, T, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, stream);
}

int km_legacy_train_step_audio(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* target_dev, float mse_weight,
                               float l1_weight, float* flat_grad_dev, float* loss_dev, float* out_dev, void* stream) {
    if (int rc = need_legacy_train(h, B)) return rc;
    Context* c = h;
    if (!audio_dev || !target_dev || !flat_grad_dev || !loss_dev || L <= 0) return fail(KM_ERR_INVALID_ARG, "km_legacy_train_step_audio: bad argument");
    const int64_t T = 1 + L / c->cfg.mel.hop_length;
    if (T > c->tr.l_frames) return fail(KM_ERR_WORKSPACE, "km_legacy_train_init sized the step for %lld frames, got %lld",
                                       (long long)c->tr.l_frames, (long long)T);
    if (B > c->ws.windows || T > c->ws.frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld windows x %lld samples: call km_reserve", (long long)B, (long long)L);
    // km_mel_batch into the step's own mel image, then the step from mel: the same launches, the same bits
    float* mel = legacy_train_mel_buffer(c);
    if (int rc = launch_mel(c, c->mel_plans[0], mel_windows(audio_dev, B, L), 0, mel, nullptr, stream)) return rc;
    return legacy_train_step(c, mel, B, T, target_dev, mse_weight, l1_weight, flat_grad_dev, loss_dev, out_dev, stream);
}

int km_legacy_train_get_dropout_masks(km_handle h, int64_t B, int64_t T, uint8_t* enc1_host, uint8_t* enc2_host, uint8_t* attn_host,
                                      uint8_t* dec1_host, uint8_t* dec2_host, void* stream) {
    if (int rc = need_legacy_train(h, B)) return rc;
    if (!enc1_host || !enc2_host || !attn_host || !dec1_host || !dec2_host || T <= 0 || T > h->tr.l_frames)
        return fail(KM_ERR_INVALID_ARG, "km_legacy_train_get_dropout_masks: bad argument");
    unsigned char* const hp[5] = {enc1_host, enc2_host, attn_host, dec1_host, dec2_host};
    return legacy_train_copy_masks(h, B, T, hp, 0, stream);
}

int km_legacy_train_set_dropout_masks(km_handle h, int64_t B, int64_t T, const uint8_t* enc1_host, const uint8_t* enc2_host,
                                      const uint8_t* attn_host, const uint8_t* dec1_host, const uint8_t* dec2_host, void* stream) {
    if (int rc = need_legacy_train(h, B)) return rc;
    if (!enc1_host || !enc2_host || !attn_host || !dec1_host || !dec2_host || T <= 0 || T > h->tr.l_frames)
        return fail(KM_ERR_INVALID_ARG, "km_legacy_train_set_dropout_masks: bad argument");
    unsigned char* const hp[5] = {const_cast<uint8_t*>(enc1_host), const_cast<uint8_t*>(enc2_host), const_cast<uint8_t*>(attn_host),
                                  const_cast<uint8_t*>(dec1_host), const_cast<uint8_t*>(dec2_host)};
    return legacy_train_copy_masks(h, B, T, hp, 1, stream);
}

}  // extern "C"
