// Stream engine of the legacy KoeMorphModel (km_koemorph_stream_*, include/koemorph.h): N independent streams, out of phase, each with
// its last rows resident on the device.
//
// The law: stream s has a frame counter c_s (0 after creation and after a reset).  A step that gives it n_s rows (0 <= n_s <=
// max_rows) renders n_s frames; frame i = c_s + j is km_koemorph_forward at B = 1 on the DENSE window of the stream's rows
// i - T_i + 1 .. i, T_i = min(i + 1, T), no audio mask, prev = the stream's previous rendered frame (none for i == 0: that frame runs
// unconditioned), the stream's own smoother state (zeros after a reset) updated by every frame.  Streams share nothing; a stream
// with n_s == 0 keeps ring, counter, previous frame and state, and no row of an output is written for it.
//
// A step is FOUR launches whatever N, max_rows and the streams' phases are: kms_advance_kernel (rows into the rings, counters, the
// step's window table), kmmf_encoder_kernel<true, true> and <false, true> over all N x max_rows table entries each (km_kmmf.hip: one
// window per workgroup, T_i from the table, rows from the ring with wrap) and kmmf_chain_kernel (one workgroup per stream walks its
// n_s frames).  Nothing allocates, synchronises or reads back outside create, so a step can be captured.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_api_internal.h"
#include "km_context.h"
#include "km_kmmf.h"

namespace km {

#include "km_kmm_tail.h"

// km_kmmf.hip
int64_t kmmf_chain_lds_bytes();
int kmmf_stream_prepare(Context* c);
int launch_kmmf_encoder_ragged(Context* c, const float* ring_mel, const float* ring_emo, const int4* table, int64_t entries, int64_t T,
                               int64_t cap, float* xm, float* xe, void* stream);
int launch_kmmf_chain(Context* c, const float* xm, const float* xe, int64_t streams, int64_t max_rows, int64_t T, const KmmTail& tail,
                      const int* nstep, const long long* counter, float* prev, void* stream);
// km_koemorph.hip
KmmTail koemorph_tail(Context* c, const float* prev, float* state, int apply_constraints, float* out, float* raw);

// One workgroup per stream: the n = clamp(counts[s], 0, R) pushed rows go to ring positions (c + j) mod cap (16-byte moves: both row
// widths are multiples of 16 floats and the callers' pointers are checked), the table gets the stream's R entries, the counter moves
// on.  cap = T - 1 + R: the rows a step's windows read (c - T + 1 .. c + n - 1) and the rows it writes never share a position.
struct AdvArgs {
    const float* mel; const float* emo; const int* counts;     // (N, R, dim) rows; counts (N) or null = R for every stream
    float* ring_mel; float* ring_emo; int mel_dim, emo_dim;
    long long* counter; int* nstep; int4* table; int* rendered;   // rendered (N) or null
    int T, R, cap;
};

__global__ __launch_bounds__(256) void kms_advance_kernel(AdvArgs a) {
    const int s = blockIdx.x, tid = threadIdx.x;
    int n = a.counts ? a.counts[s] : a.R;
    n = n < 0 ? 0 : (n > a.R ? a.R : n);
    const long long c = a.counter[s];
    const int p0 = (int)(c % a.cap);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        const int dq = (st ? a.emo_dim : a.mel_dim) >> 2;
        const float4* src = reinterpret_cast<const float4*>(st ? a.emo : a.mel) + (int64_t)s * a.R * dq;
        float4* dst = reinterpret_cast<float4*>(st ? a.ring_emo : a.ring_mel) + (int64_t)s * a.cap * dq;
        for (int i = tid; i < n * dq; i += 256) {
            const int j = i / dq, cq = i - j * dq;
            int p = p0 + j;                                   // j < R <= cap
            p = p >= a.cap ? p - a.cap : p;
            dst[(int64_t)p * dq + cq] = src[i];
        }
    }
    for (int j = tid; j < a.R; j += 256) {
        int4 e = make_int4(s, j, 0, 0);
        if (j < n) {
            const long long i = c + j;
            const int Ti = i + 1 < (long long)a.T ? (int)(i + 1) : a.T;
            e.z = Ti; e.w = (int)((i - Ti + 1) % a.cap);
        }
        a.table[(int64_t)s * a.R + j] = e;
    }
    __syncthreads();                                          // every thread has read the counter
    if (tid == 0) {
        a.counter[s] = c + n;
        a.nstep[s] = n;
        if (a.rendered) a.rendered[s] = n;
    }
}

// the masked streams (mask null: all) become freshly created ones: counter 0, state and previous frame zero
__global__ __launch_bounds__(256) void kms_reset_kernel(const unsigned char* __restrict__ mask, long long* counter, int* nstep, float* prev,
                                                        float* state, int state_floats, int NB) {
    const int s = blockIdx.x, tid = threadIdx.x;
    if (mask && !mask[s]) return;
    if (tid == 0) { counter[s] = 0; nstep[s] = 0; }
    for (int i = tid; i < NB; i += 256) prev[(int64_t)s * NB + i] = 0.f;
    for (int i = tid; i < state_floats; i += 256) state[(int64_t)s * state_floats + i] = 0.f;
}

struct KmsPlan { int64_t cap, launches, device_floats, lds_bytes, state_floats; };

// why a handle cannot serve streams with a context of T frames, or KM_OK: the engine runs the fused kernels only (rollout route 1)
static int kms_refusal(Context* c, int64_t T, const char* who) {
    const km_koemorph_config& k = c->kmm;
    if (k.d_model != kmmf::D) return fail(KM_ERR_UNSUPPORTED, "%s: d_model %d, the stream engine serves d_model %d", who, k.d_model, kmmf::D);
    if (k.num_heads != kmmf::HEADS) return fail(KM_ERR_UNSUPPORTED, "%s: %d heads, the stream engine serves %d", who, k.num_heads, kmmf::HEADS);
    if (k.decoder_hidden_dim != kmmf::HID)
        return fail(KM_ERR_UNSUPPORTED, "%s: decoder width %d, the stream engine serves %d", who, k.decoder_hidden_dim, kmmf::HID);
    if (k.mel_dim % 16 != 0) return fail(KM_ERR_UNSUPPORTED, "%s: mel_dim %d is not a multiple of 16", who, k.mel_dim);
    if (k.emotion_dim % 16 != 0) return fail(KM_ERR_UNSUPPORTED, "%s: emotion_dim %d is not a multiple of 16", who, k.emotion_dim);
    if (k.num_attention_layers < 1) return fail(KM_ERR_UNSUPPORTED, "%s: %d attention layers, at least one", who, k.num_attention_layers);
    if (T > kmmf::TMAX) return fail(KM_ERR_UNSUPPORTED, "%s: context_frames %lld, at most %d", who, (long long)T, kmmf::TMAX);
    if (k.use_temporal_smoothing && k.smoothing_method != 0 && k.smoothing_window > 16)
        return fail(KM_ERR_UNSUPPORTED, "%s: smoothing window %d, at most 16", who, k.smoothing_window);
    if (c->opt.kmm_no_fuse) return fail(KM_ERR_UNSUPPORTED, "%s: option kmm_no_fuse is %d: the stream engine has no launch-per-op route", who, c->opt.kmm_no_fuse);
    if (!c->kmm_fused) return fail(KM_ERR_UNSUPPORTED, "%s: the model is outside the width of the fused kernels (%d blendshapes)", who, c->NB);
    return KM_OK;
}

static int64_t kms_state_floats(Context* c) {
    const km_koemorph_config& k = c->kmm;
    return !k.use_temporal_smoothing ? 0 : (k.smoothing_method == 0 ? c->NB : (int64_t)k.smoothing_window * c->NB + 1);
}

// The one function behind km_koemorph_stream_plan and km_koemorph_stream_create
static KmsPlan kms_plan(Context* c, int64_t N, int64_t T, int64_t R) {
    KmsPlan p{};
    p.cap = T - 1 + R;
    p.launches = 4;
    p.state_floats = kms_state_floats(c);
    p.lds_bytes = kmmf_chain_lds_bytes();
    p.device_floats = N * p.cap * (c->kmm.mel_dim + c->kmm.emotion_dim)   // rings
                      + 2 * N + N                                         // counters (64-bit), frames of the step
                      + N * c->NB + N * p.state_floats                    // previous frames, smoother states
                      + 4 * N * R                                         // window table
                      + 2 * N * R * T * kmmf::D;                          // encodings of the step's windows
    return p;
}

static int kms_guard(km_handle h, const char* who, bool created) {
    if (!h) return fail(KM_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (h->kind != 2) return fail(KM_ERR_INVALID_ARG, "%s: not a KoeMorphModel handle (km_koemorph_create), kind %d", who, h->kind);
    if (created && h->ks.streams == 0) return fail(KM_ERR_INVALID_ARG, "%s: no stream engine: call km_koemorph_stream_create", who);
    return KM_OK;
}

static int kms_sizes(const char* who, int64_t N, int64_t T, int64_t R) {
    if (N < 1) return fail(KM_ERR_INVALID_ARG, "%s: n_streams %lld < 1", who, (long long)N);
    if (T < 1) return fail(KM_ERR_INVALID_ARG, "%s: context_frames %lld < 1", who, (long long)T);
    if (R < 1) return fail(KM_ERR_INVALID_ARG, "%s: max_rows %lld < 1", who, (long long)R);
    if (N > (1 << 20) || R > (1 << 10)) return fail(KM_ERR_INVALID_ARG, "%s: %lld streams x %lld rows per step, at most 2^20 x 2^10", who, (long long)N, (long long)R);
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" {

int km_koemorph_stream_plan(km_handle h, int64_t n_streams, int64_t context_frames, int64_t max_rows, int64_t out[6]) {
    const char* who = "km_koemorph_stream_plan";
    if (int rc = kms_guard(h, who, false)) return rc;
    if (!out) return fail(KM_ERR_INVALID_ARG, "%s: out is NULL", who);
    Context* c = h;
    if (!c->host_finalized) return fail(KM_ERR_NOT_FINALIZED, "%s: call km_finalize_host or km_finalize first", who);
    if (int rc = kms_sizes(who, n_streams, context_frames, max_rows)) return rc;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (kms_refusal(c, context_frames, who) != KM_OK) return KM_OK;       // out[0] = 0; km_last_error holds the reason
    const KmsPlan p = kms_plan(c, n_streams, context_frames, max_rows);
    out[0] = 1; out[1] = p.cap; out[2] = p.launches; out[3] = p.device_floats; out[4] = p.lds_bytes; out[5] = p.state_floats;
    return KM_OK;
}

int km_koemorph_stream_create(km_handle h, int64_t n_streams, int64_t context_frames, int64_t max_rows, int32_t apply_smoothing,
                              int32_t apply_constraints) {
    const char* who = "km_koemorph_stream_create";
    if (int rc = kms_guard(h, who, false)) return rc;
    Context* c = h;
    if (!c->host_finalized) return fail(KM_ERR_NOT_FINALIZED, "%s: call km_finalize first", who);
    if (int rc = kms_sizes(who, n_streams, context_frames, max_rows)) return rc;
    if (int rc = kms_refusal(c, context_frames, who)) return rc;
    if (int rc = need_ready(c)) return rc;
    const KmsPlan p = kms_plan(c, n_streams, context_frames, max_rows);
    const int64_t N = n_streams, R = max_rows, T = context_frames;
    HIP_TRY(hipDeviceSynchronize());                // a second create replaces the first: nothing of it may be in flight
    c->ks = KoeMorphStreams{};
    KoeMorphStreams ks;
    if (int rc = ks.ring_mel.alloc(N * p.cap * c->kmm.mel_dim, who)) return rc;
    if (int rc = ks.ring_emo.alloc(N * p.cap * c->kmm.emotion_dim, who)) return rc;
    if (int rc = ks.counter.alloc(N, who)) return rc;
    if (int rc = ks.nstep.alloc(N, who)) return rc;
    if (int rc = ks.prev.alloc(N * c->NB, who)) return rc;
    if (p.state_floats > 0)
        if (int rc = ks.state.alloc(N * p.state_floats, who)) return rc;
    if (int rc = ks.table.alloc(4 * N * R, who)) return rc;
    if (int rc = ks.xm.alloc(N * R * T * kmmf::D, who)) return rc;
    if (int rc = ks.xe.alloc(N * R * T * kmmf::D, who)) return rc;
    // a fresh engine: every counter 0, every state zero; the rings need no value (a window never reaches behind its stream's frame 0)
    HIP_TRY(hipMemset(ks.counter, 0, (size_t)ks.counter.bytes()));
    HIP_TRY(hipMemset(ks.nstep, 0, (size_t)ks.nstep.bytes()));
    HIP_TRY(hipMemset(ks.prev, 0, (size_t)ks.prev.bytes()));
    if (ks.state) HIP_TRY(hipMemset(ks.state, 0, (size_t)ks.state.bytes()));
    HIP_TRY(hipMemset(ks.table, 0, (size_t)ks.table.bytes()));
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = kmmf_stream_prepare(c)) return rc;
    ks.context = T; ks.max_rows = R; ks.cap = p.cap; ks.state_floats = p.state_floats;
    ks.smoothing = apply_smoothing ? 1 : 0; ks.constraints = apply_constraints ? 1 : 0;
    ks.streams = N;
    c->ks = std::move(ks);
    return KM_OK;
}

int km_koemorph_stream_step(km_handle h, const float* mel_dev, const float* emotion_dev, const int32_t* counts_dev, float* out_dev,
                            float* raw_dev, int32_t* rendered_dev, void* stream) {
    const char* who = "km_koemorph_stream_step";
    if (int rc = kms_guard(h, who, true)) return rc;
    Context* c = h;
    if (!mel_dev) return fail(KM_ERR_INVALID_ARG, "%s: mel_dev is NULL", who);
    if (!emotion_dev) return fail(KM_ERR_INVALID_ARG, "%s: emotion_dev is NULL", who);
    if (!out_dev) return fail(KM_ERR_INVALID_ARG, "%s: out_dev is NULL", who);
    if (!aligned16(mel_dev)) return fail(KM_ERR_INVALID_ARG, "%s: mel_dev %p is not 16-byte aligned", who, (const void*)mel_dev);
    if (!aligned16(emotion_dev)) return fail(KM_ERR_INVALID_ARG, "%s: emotion_dev %p is not 16-byte aligned", who, (const void*)emotion_dev);
    if (int rc = need_ready(c)) return rc;
    KoeMorphStreams& ks = c->ks;
    if (int rc = kms_refusal(c, ks.context, who)) return rc;               // an option set after create
    hipStream_t st = (hipStream_t)stream;
    AdvArgs a{};
    a.mel = mel_dev; a.emo = emotion_dev; a.counts = counts_dev; a.ring_mel = ks.ring_mel; a.ring_emo = ks.ring_emo;
    a.mel_dim = c->kmm.mel_dim; a.emo_dim = c->kmm.emotion_dim; a.counter = ks.counter; a.nstep = ks.nstep;
    a.table = reinterpret_cast<int4*>(ks.table.p); a.rendered = rendered_dev; a.T = (int)ks.context; a.R = (int)ks.max_rows; a.cap = (int)ks.cap;
    hipLaunchKernelGGL(kms_advance_kernel, dim3((unsigned)ks.streams), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (int rc = launch_kmmf_encoder_ragged(c, ks.ring_mel, ks.ring_emo, a.table, ks.streams * ks.max_rows, ks.context, ks.cap, ks.xm, ks.xe, stream))
        return rc;
    const KmmTail ta = koemorph_tail(c, nullptr, ks.smoothing ? ks.state.p : nullptr, ks.constraints, out_dev, raw_dev);
    return launch_kmmf_chain(c, ks.xm, ks.xe, ks.streams, ks.max_rows, ks.context, ta, ks.nstep, ks.counter, ks.prev, stream);
}

int km_koemorph_stream_reset(km_handle h, const uint8_t* mask_dev, void* stream) {
    const char* who = "km_koemorph_stream_reset";
    if (int rc = kms_guard(h, who, true)) return rc;
    Context* c = h;
    KoeMorphStreams& ks = c->ks;
    hipLaunchKernelGGL(kms_reset_kernel, dim3((unsigned)ks.streams), dim3(256), 0, (hipStream_t)stream, mask_dev, ks.counter.p, ks.nstep.p,
                       ks.prev.p, ks.state.p, (int)ks.state_floats, c->NB);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_koemorph_stream_destroy(km_handle h) {
    if (int rc = kms_guard(h, "km_koemorph_stream_destroy", false)) return rc;
    if (h->ks.streams == 0) return KM_OK;
    HIP_TRY(hipDeviceSynchronize());
    h->ks = KoeMorphStreams{};
    return KM_OK;
}

int km_koemorph_stream_frames(km_handle h, int64_t* frames_dev, void* stream) {
    const char* who = "km_koemorph_stream_frames";
    if (int rc = kms_guard(h, who, true)) return rc;
    if (!frames_dev) return fail(KM_ERR_INVALID_ARG, "%s: frames_dev is NULL", who);
    HIP_TRY(hipMemcpyAsync(frames_dev, h->ks.counter.p, (size_t)h->ks.streams * sizeof(int64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return KM_OK;
}

int km_koemorph_stream_state(km_handle h, float* state_dev, float* prev_dev, void* stream) {
    const char* who = "km_koemorph_stream_state";
    if (int rc = kms_guard(h, who, true)) return rc;
    KoeMorphStreams& ks = h->ks;
    if (state_dev && ks.state_floats > 0)
        HIP_TRY(hipMemcpyAsync(state_dev, ks.state.p, (size_t)(ks.streams * ks.state_floats) * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (prev_dev)
        HIP_TRY(hipMemcpyAsync(prev_dev, ks.prev.p, (size_t)(ks.streams * h->NB) * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return KM_OK;
}

}  // extern "C"
