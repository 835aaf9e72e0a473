// C-ABI entry points of the streams: km_stream_* and km_legacy_stream_* (declared in include/koemorph.h).
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

extern "C" {

// every stream empty: rings, flags, EMA state and, where they exist, the chunk FIFOs
static int zero_streams(Streams& s, int NB, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(s.ring, 0, (size_t)s.n_streams * s.ring_len * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(s.ring_wptr, 0, (size_t)s.n_streams * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(s.ring_frames, 0, (size_t)s.n_streams * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(s.ring_ready, 0, (size_t)s.n_streams, st));
    HIP_TRY(hipMemsetAsync(s.ring_started, 0, (size_t)s.n_streams, st));
    HIP_TRY(hipMemsetAsync(s.ring_state, 0, (size_t)s.n_streams * NB * sizeof(float), st));
    if (s.fifo.len > 0) {     // empty FIFOs: their samples are not read below `available` (stream_reset_masked_kernel)
        HIP_TRY(hipMemsetAsync(s.fifo.state, 0, 3 * (size_t)s.n_streams * sizeof(int), st));
        HIP_TRY(hipMemsetAsync(s.fifo.fire, 0, (size_t)s.n_streams, st));
    }
    return KM_OK;
}

int km_stream_reset(km_handle h, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->st.n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_reset: no streams (km_stream_create first)");
    return zero_streams(c->st, c->NB, (hipStream_t)stream);
}

int km_stream_create(km_handle h, int64_t n_streams, double context_window_s, double update_interval_s,
                     const km_mel_config* mel_cfg) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (n_streams <= 0 || !(context_window_s > 0) || !(update_interval_s > 0) || !mel_cfg)
        return fail(KM_ERR_INVALID_ARG, "km_stream_create: bad argument");
    if (mel_cfg->n_fft != 512 && mel_cfg->n_fft != 1024) return fail(KM_ERR_UNSUPPORTED, "n_fft must be 512 or 1024");
    if (mel_cfg->n_mels != c->NK) return fail(KM_ERR_INVALID_ARG, "stream front end must produce %d mel channels", c->NK);
    c->st = Streams{};           // the old streams go first; the handle has none until the new ones are whole
    Streams s;
    const int sr = mel_cfg->sample_rate;
    s.ring_len = (int64_t)(context_window_s * sr);                                  // mel_sliding_window.py:46
    const double target_fps = 1.0 / update_interval_s;
    s.ring_hop = (int)((double)sr / target_fps);                                    // :49-50 (532 for 0.0333)
    s.out_frames = (int64_t)(context_window_s / update_interval_s);                 // :300
    if (s.ring_hop <= 0 || s.ring_len <= mel_cfg->n_fft / 2) return fail(KM_ERR_INVALID_ARG, "context window too short");
    s.n_streams = n_streams;
    const char* what = "km_stream_create";
    if (int rc = s.ring.alloc(n_streams * s.ring_len, what)) return rc;
    if (int rc = s.ring_wptr.alloc(n_streams, what)) return rc;
    if (int rc = s.ring_frames.alloc(n_streams, what)) return rc;
    if (int rc = s.ring_ready.alloc(n_streams, what)) return rc;
    if (int rc = s.ring_started.alloc(n_streams, what)) return rc;
    if (int rc = s.ring_state.alloc(n_streams * c->NB, what)) return rc;
    s.plan = find_or_add_plan(c, *mel_cfg);
    if (int rc = upload_mel_plan(s.plan)) return rc;
    if (int rc = km_reserve(h, n_streams, s.ring_len)) return rc;
    if (int rc = zero_streams(s, c->NB, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    c->st = std::move(s);
    return KM_OK;
}

int km_stream_push(km_handle h, const float* samples_dev, int64_t n_per_stream, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->st.n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_push: no streams (km_stream_create first)");
    if (!samples_dev) return fail(KM_ERR_INVALID_ARG, "km_stream_push: NULL samples");
    const int64_t diff = n_per_stream - c->st.ring_hop;
    if (diff > 1 || diff < -1)                                                      // :80-82
        return fail(KM_ERR_INVALID_ARG, "Frame size mismatch: expected ~%d, got %lld", c->st.ring_hop, (long long)n_per_stream);
    return launch_ring_push(c, samples_dev, n_per_stream, stream);
}

// what asking for raw / the map adds to the refusals of tick and step, before anything is launched or popped
static int stream_outputs_ok(Context* c, const float* attn_dev) {
    if (attn_dev && (c->opt.core_split == 3 || c->opt.core_split == 6))
        return fail(KM_ERR_UNSUPPORTED, "streams: the split-bf16 variant (core_split %d) has no attention-map output", c->opt.core_split);
    if ((uintptr_t)attn_dev & 15) return fail(KM_ERR_INVALID_ARG, "streams: the attention maps must be 16-byte aligned");
    return KM_OK;
}

// the launches of a tick or a step: emotion logits (where the front end does not carry them), the front end over the rings, the
// streaming core, all three skipping the streams whose gate flag is zero (is_full for km_stream_tick, this step's fire flags for
// km_stream_step)
static int stream_launches(Context* c, const unsigned char* gate, const float* emotion_dev, float* out_dev, float* raw_dev, float* attn_dev,
                           void* stream) {
    const int64_t S = c->st.n_streams, n_frames = 1 + c->st.ring_len / c->st.plan->cfg.hop_length;
    if (int rc = launch_mel_power_with_logits(c, c->st.plan, mel_rings(c, gate), emotion_dev, c->ws.zemo, stream)) return rc;
    return launch_core_power(c, c->st.plan, S, n_frames, c->ws.zemo, out_dev, stream, with_outputs(core_stream(c, gate), raw_dev, attn_dev));
}

static int stream_tick(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* ready_dev, float* raw_dev, float* attn_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->st.n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_tick: no streams (km_stream_create first)");
    if (!emotion_dev || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_stream_tick: NULL argument");
    // the shapes with a streaming core: the fused one (d_model 256, 8 heads, window 256), core512's (512, 8 or 16 heads, window 512),
    // core256w's (256, 8 heads, window 512) and core128's (128, 4 heads, window 128 or 256)
    if (!stream_core_ok(c))
        return fail(KM_ERR_UNSUPPORTED, "no kernel for d_model=%d, mel_sequence_length=%d, heads=%d", c->d, c->T, c->H);
    const int64_t S = c->st.n_streams, L = c->st.ring_len;
    const int64_t n_frames = 1 + L / c->st.plan->cfg.hop_length;
    if (S > c->ws.windows || n_frames > c->ws.frames) return fail(KM_ERR_WORKSPACE, "stream workspace too small");
    if (int rc = stream_outputs_ok(c, attn_dev)) return rc;
    if (int rc = stream_launches(c, c->st.ring_ready, emotion_dev, out_dev, raw_dev, attn_dev, stream)) return rc;
    if (ready_dev)
        HIP_TRY(hipMemcpyAsync(ready_dev, c->st.ring_ready, (size_t)S, hipMemcpyDeviceToDevice, (hipStream_t)stream));
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
    if (c->st.n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "%s: no streams (km_stream_create first)", who);
    if (c->st.fifo.len <= 0) return fail(KM_ERR_INVALID_ARG, "%s: no FIFOs (km_stream_fifo_create first)", who);
    return KM_OK;
}

int km_stream_fifo_create(km_handle h, int64_t fifo_samples, int64_t frame_samples) {
    if (int rc = need_dual(h)) return rc;
    Context* c = h;
    if (c->st.n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_fifo_create: no streams (km_stream_create first)");
    if (fifo_samples <= 0 || frame_samples <= 0 || fifo_samples >= (1ll << 30))
        return fail(KM_ERR_INVALID_ARG, "km_stream_fifo_create: bad argument (FIFOs of %lld samples, frames of %lld)", (long long)fifo_samples,
                    (long long)frame_samples);
    const int64_t diff = frame_samples - c->st.ring_hop;
    if (diff > 1 || diff < -1)                                                      // mel_sliding_window.py:80-82
        return fail(KM_ERR_INVALID_ARG, "Frame size mismatch: expected ~%d, got %lld", c->st.ring_hop, (long long)frame_samples);
    if (fifo_samples < frame_samples)
        return fail(KM_ERR_INVALID_ARG, "km_stream_fifo_create: frames of %lld samples exceed the FIFO of %lld: no read could ever succeed",
                    (long long)frame_samples, (long long)fifo_samples);
    if (c->st.ring_hop > c->st.ring_len) return fail(KM_ERR_INVALID_ARG, "km_stream_fifo_create: the ring hop exceeds the ring");
    HIP_TRY(hipDeviceSynchronize());
    c->st.fifo = ChunkFifos{};   // the old FIFOs go first
    ChunkFifos f;
    const size_t S = (size_t)c->st.n_streams;
    const char* what = "km_stream_fifo_create";
    if (int rc = f.samples.alloc(S * fifo_samples, what)) return rc;
    if (int rc = f.state.alloc(3 * S, what)) return rc;
    if (int rc = f.fire.alloc(S, what)) return rc;
    HIP_TRY(hipMemset(f.samples, 0, S * fifo_samples * sizeof(float)));
    HIP_TRY(hipMemset(f.state, 0, 3 * S * sizeof(int)));
    HIP_TRY(hipMemset(f.fire, 0, S));
    f.len = fifo_samples; f.frame = (int)frame_samples;
    if (!stream_core_ok(c)) { c->st.fifo = std::move(f); return KM_OK; }
    // the launches of one step over a gate of zeros: no workgroup passes it, so nothing is read or written (the emotion rows and
    // the result pointer are dummies), but every kernel of a step has had its attributes set before a capture sees its first launch
    DevBuf<float> emo;
    if (int rc = emo.alloc(S * c->ED, what)) return rc;
    HIP_TRY(hipMemset(emo, 0, S * c->ED * sizeof(float)));
    c->st.fifo = std::move(f);   // every allocation has succeeded
    int rc = launch_sfifo_pop_ring(c, nullptr, nullptr, nullptr, nullptr);
    if (!rc) rc = stream_launches(c, c->st.fifo.fire, emo, c->st.ring_state, nullptr, nullptr, nullptr);
    const hipError_t e = hipDeviceSynchronize();
    if (rc) return rc;
    HIP_TRY(e);
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
    if (!stream_core_ok(c))                                                         // as km_stream_tick, before anything is popped
        return fail(KM_ERR_UNSUPPORTED, "no kernel for d_model=%d, mel_sequence_length=%d, heads=%d", c->d, c->T, c->H);
    const int64_t S = c->st.n_streams;
    if (S > c->ws.windows || 1 + c->st.ring_len / c->st.plan->cfg.hop_length > c->ws.frames)
        return fail(KM_ERR_WORKSPACE, "stream workspace too small");
    if (int rc = stream_outputs_ok(c, attn_dev)) return rc;
    // pop + ring advance (fire, ready, backlog), then the launches of a tick gated on fire: one linear chain
    if (int rc = launch_sfifo_pop_ring(c, fired_dev, ready_dev, backlog_dev, stream)) return rc;
    return stream_launches(c, c->st.fifo.fire, emotion_dev, out_dev, raw_dev, attn_dev, stream);
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
    if (c->st.n_streams <= 0) return fail(KM_ERR_INVALID_ARG, "km_stream_reset_streams: no streams (km_stream_create first)");
    if (!mask_dev) return fail(KM_ERR_INVALID_ARG, "km_stream_reset_streams: NULL mask");
    return launch_stream_reset_masked(c, mask_dev, stream);
}

// ---- streams of the legacy model: device-resident consuming FIFOs + the one-launch model (kernels: km_legacy_stream.hip,
//      legacy_stream_kernel in km_kmmf.hip) ----
// the shape legacy_stream_kernel is written for, behind the front end that leaves power-mel + window maxima
static bool legacy_stream_ok(Context* c) {
    return c->legacy_fused && c->legacy_tail_fused && c->d == 256 && c->H == 8 && c->legacy_hidden == 128 && c->NB == 52 && c->NK == 80 &&
           !c->mel_plans.empty() && c->mel_plans[0]->cfg.n_fft == 1024 && legacy_pow_ok(c);
}

static int need_legacy_stream(Context* c, const char* who) {
    if (int rc = need_ready(c)) return rc;
    if (c->kind != 1) return fail(KM_ERR_INVALID_ARG, "%s needs a legacy handle (km_legacy_create)", who);
    if (c->lf.streams <= 0) return fail(KM_ERR_INVALID_ARG, "%s: no streams (km_legacy_stream_create first)", who);
    return KM_OK;
}

int km_legacy_stream_reset(km_handle h, void* stream) {
    if (int rc = need_legacy_stream(h, "km_legacy_stream_reset")) return rc;
    Context* c = h;
    hipStream_t st = (hipStream_t)stream;
    const size_t S = (size_t)c->lf.streams;
    HIP_TRY(hipMemsetAsync(c->lf.fifo, 0, S * c->lf.len * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(c->lf.stage, 0, S * c->lf.window * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(c->lf.state, 0, 3 * S * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(c->lf.ready, 0, S, st));
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
    c->lf.streams = 0;
    const char* what = "km_legacy_stream_create";
    if (int rc = c->lf.fifo.grow(n_streams * buffer_samples, nullptr, what)) return rc;
    if (int rc = c->lf.state.grow(3 * n_streams, nullptr, what)) return rc;
    if (int rc = c->lf.stage.grow(n_streams * audio_length, nullptr, what)) return rc;
    if (int rc = c->lf.ready.grow(n_streams, nullptr, what)) return rc;
    if (int rc = c->lf.attn.grow(n_streams * c->NB * c->d, nullptr, what)) return rc;
    if (int rc = km_reserve(h, n_streams, audio_length)) return rc;                  // power-mel, window maxima, chunk counters
    if (!legacy_stream_ok(c)) return fail(KM_ERR_UNSUPPORTED, "km_legacy_stream_create: the power-mel workspace is not 16-byte aligned");
    c->lf.streams = n_streams; c->lf.len = buffer_samples; c->lf.window = audio_length;
    HIP_TRY(hipMemset(c->ws.melmax, 0, (size_t)c->ws.windows * sizeof(unsigned)));
    c->melmax_dirty = false;
    if (int rc = km_legacy_stream_reset(h, nullptr)) return rc;
    // one tick over the empty FIFOs: no stream is ready, so nothing is consumed or written (the result pointer is a dummy), but
    // every kernel of a tick has had its attributes set before a capture can see its first launch
    if (int rc = km_legacy_stream_tick(h, c->lf.attn, nullptr, nullptr)) return rc;
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
    const int64_t S = c->lf.streams, W = c->lf.window, T = 1 + W / c->cfg.mel.hop_length;
    if (S > c->ws.windows || T > c->ws.frames) return fail(KM_ERR_WORKSPACE, "stream workspace too small");
    if (!legacy_stream_ok(c)) return fail(KM_ERR_UNSUPPORTED, "km_legacy_stream_tick: the fused legacy kernels are switched off (km_set_option)");
    // three launches: pop (ready flags + the claimed windows, chronological), the plain front end over the staging image,
    // the model for every ready stream (which also puts every stream's window maximum back to zero)
    if (int rc = launch_lfifo_pop(c, ready_dev, stream)) return rc;
    if (int rc = launch_mel_power(c, c->mel_plans[0], mel_windows(c->lf.stage, S, W), stream)) return rc;
    const LogParams lp = plan_log_params(c->mel_plans[0]);
    return launch_legacy_stream_model(c, c->ws.melpow, c->ws.melmax, c->lf.ready, S, (int)T, lp, c->lf.attn, out_dev, stream);
}

}  // extern "C"
