// The emotion track of a resident clip: what one emotion stream (km_emotion_stream.hip) would hold after t samples of the clip,
// for every update time t_k = MIN + k U at once -- the offline producer of the model's 256-D emotion input.  A training window's
// emotion vector is the row of the update a live stream would last have made when the window ends, so a clip has ONE track and a
// step gathers rows from it by start frame.
//   ec_plan_kernel       the window of row k in closed form (AudioBuffer.get_window after t_k samples, src/features/
//                        opensmile_extractor.py:111-130) as an EgmSlot: the clip is the one "ring", ring_len = clip_len, no wrap
//   km_egemaps.hip       the five ragged eGeMAPS kernels, as the streams launch them (egm_ragged_functionals)
//   ec_epilogue_kernel   NaN / Inf -> 0 (:450-452), features[k], and W concat(features[k], features[0], features[0]) + b for all rows
//                        of the pass: the 300 / 600 ms slots are filled once per life (:478-490) and a clip is one life
//   ecb_plan_kernel /    the same two for B clips of one length at once (km_emotion_clip_build_batch): rows numbered g = c K + k fill the
//   ecb_epilogue_kernel  passes across clip boundaries, the clips are the B "rings", and a row takes its OWN clip's features[0]
//   ec_rows_kernel       window -> row: e = min(n, (s + T) h), k = clamp((e - MIN) / U, 0, K - 1), a 256-float copy per window
// build and rows neither allocate, synchronise nor read back; rows' grid depends on the batch alone, so it captures into a hipGraph.
//
// The `basic` back end (km_emotion_clip_create_basic): the same slot law and the same row mapping, but a row is the nine raw prosodic
// values of its window as km_emotion_stream_create_basic's streams hold them.  ec_plan_kernel / ecb_plan_kernel write the table,
// prosody_ragged (km_prosody.hip) reads the windows in place from the clip and writes slot i to row i of the pointer it is handed --
// which is track row k0 (or g0) of the caller's output, since it skips empty slots: no staging copy, no epilogue.
//   ec_rows9_kernel      ec_rows_kernel's mapping at width 9: sixteen windows per workgroup, sixteen lanes a window (nine of them copy)
#include <hip/hip_runtime.h>

#include <new>

#include <memory>

#include "km_context.h"
#include "km_egemaps_ragged.h"
#include "km_prosody_ragged.h"

namespace km {


namespace ec {
constexpr int SR = 16000, NFEAT = 88, NCAT = 3 * NFEAT, NEMO = 256, REC = 36, MAXF = 2048;
constexpr int TN = 16, TM = 16;          // the epilogue's tile: output columns per workgroup, rows per turn (TN * TM = 256 threads)
constexpr int WS = NCAT + 1;             // LDS stride of a weight row: 265 is odd, so the 16 columns of a half wave hit 16 banks
constexpr int64_t MAX_CLIP = (int64_t)1 << 30;     // egm_ragged_functionals' ring limit; EgmSlot.start is an int32
constexpr int NBASIC = 9, BASIC_REC = 4, BASIC_HOP = 512, BASIC_MAX_WINDOW = 1 << 20;   // the `basic` back end (km_prosody.hip)
constexpr int RW = 16;                   // ec_rows9_kernel: windows per workgroup, and the lanes a window takes
}  // namespace ec

struct EmotionClip {
    int64_t max_slots = 0;
    int ring_len = 0, window_len = 0, update_samples = 0, min_samples = 0, max_nf = 0;
    void* plan = nullptr;
    DevBuf<char> blob;         // one allocation, carved below
    EgmSlot* table = nullptr;  // (max_slots)
    float* scale = nullptr;    // (max_slots)
    float* rec = nullptr;      // (max_slots, max_nf, 36)
    float* fout = nullptr;     // (max_slots, 88)
    float* f0 = nullptr;       // (88): features[0] of the clip being built, written by pass 0
    float* w = nullptr;        // (256, 264) as nn.Linear stores it
    float* bias = nullptr;     // (256)
    bool has_compression = false;
    bool basic = false;        // the `basic` back end: rows of 9, rec is (max_slots, max_nf, 4), no scale / fout / f0 / w / bias
    void* prosody = nullptr;
    ~EmotionClip() { (void)km_egemaps_plan_destroy(plan); (void)km_prosody_plan_destroy(prosody); }
};

static int64_t ec_num_rows(const EmotionClip* e, int64_t clip_len) {
    return clip_len < e->min_samples ? 0 : (clip_len - e->min_samples) / e->update_samples + 1;
}

// ---- rows k0 .. k0 + max_slots - 1 as slots: [0, min(t, C)) while t < R (the OLDEST C samples, as get_window returns them before
// the ring has wrapped), [t - C, t) from t >= R on ----
__global__ __launch_bounds__(256) void ec_plan_kernel(int64_t k0, int64_t K, int max_slots, int ring_len, int window_len, int update_samples,
                                                      int min_samples, EgmSlot* __restrict__ table) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= max_slots) return;
    const int64_t k = k0 + i;
    EgmSlot sl{-1, 0, 0, 0};
    if (k < K) {
        const int64_t t = min_samples + k * update_samples;                      // <= clip_len <= 2^30
        sl.stream = 0;
        if (t < ring_len) { sl.start = 0; sl.len = t < window_len ? (int)t : window_len; }
        else { sl.start = (int)(t - window_len); sl.len = window_len; }
        sl.nf = (sl.len - 960) / 160 + 1;                                        // km_egemaps_num_frames; len >= min_samples = 8000
    }
    table[i] = sl;
}

__device__ __forceinline__ float ec_scrub(float f) { return fabsf(f) <= 3.4028234663852886e38f ? f : 0.f; }    // NaN, +Inf, -Inf -> 0

// ---- the pass's rows: scrub, features[k0 + m], emotion[k0 + m] = W (f_m | f_0 | f_0) + b.  Workgroup j owns output columns
// 16 j .. 16 j + 15: their 16 x 264 weights go to LDS once and serve every row of the pass, 16 rows per turn (thread = column x row).
// A row's sum is one fmaf chain over k = 0 .. 263 from zero, then + bias: the order of es_epilogue_kernel, whatever the pass holds.
__global__ __launch_bounds__(256) void ec_epilogue_kernel(const float* __restrict__ fout, int rows, int64_t k0, float* __restrict__ f0,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ features, float* __restrict__ emotion) {
    using namespace ec;
    __shared__ float wl[TN * WS];
    __shared__ float xl[TM * NFEAT];
    __shared__ float f0l[NFEAT];
    const int tid = threadIdx.x, c = tid % TN, r = tid / TN, col0 = blockIdx.x * TN;
    const float* wsrc = w + (int64_t)col0 * NCAT;                                // rows col0 .. col0 + 15 of W: one contiguous piece
    for (int i = tid; i < TN * NCAT; i += 256) wl[(i / NCAT) * WS + i % NCAT] = wsrc[i];
    if (tid < NFEAT) {
        float f;
        if (k0 == 0) { f = ec_scrub(fout[tid]); if (blockIdx.x == 0) f0[tid] = f; }      // pass 0 holds row 0; later passes read f0
        else f = f0[tid];
        f0l[tid] = f;
    }
    const float bc = bias[col0 + c];
    for (int m0 = 0; m0 < rows; m0 += TM) {
        __syncthreads();                                                         // the turn before is done with xl; wl and f0l are written
        for (int i = tid; i < TM * NFEAT; i += 256) {
            const int m = m0 + i / NFEAT, j = i % NFEAT;
            float f = 0.f;
            if (m < rows) {
                f = ec_scrub(fout[(int64_t)m * NFEAT + j]);
                if (features && blockIdx.x == 0) features[(k0 + m) * NFEAT + j] = f;
            }
            xl[i] = f;
        }
        __syncthreads();
        const int m = m0 + r;
        if (m < rows) {
            const float* wr = wl + c * WS;
            const float* x = xl + r * NFEAT;
            float acc = 0.f;
            for (int k = 0; k < NFEAT; ++k) acc = fmaf(wr[k], x[k], acc);
            for (int k = 0; k < NFEAT; ++k) acc = fmaf(wr[NFEAT + k], f0l[k], acc);
            for (int k = 0; k < NFEAT; ++k) acc = fmaf(wr[2 * NFEAT + k], f0l[k], acc);
            emotion[(k0 + m) * NEMO + col0 + c] = acc + bc;
        }
    }
}

// ---- B clips of one length: rows g0 .. g0 + max_slots - 1 of the numbering g = c K + k, ec_plan_kernel's closed form with stream = c ----
__global__ __launch_bounds__(256) void ecb_plan_kernel(int64_t g0, int64_t G, int64_t K, int max_slots, int ring_len, int window_len,
                                                       int update_samples, int min_samples, EgmSlot* __restrict__ table) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= max_slots) return;
    const int64_t g = g0 + i;
    EgmSlot sl{-1, 0, 0, 0};
    if (g < G) {
        const int64_t c = g / K, k = g - c * K;
        const int64_t t = min_samples + k * update_samples;                      // <= L <= 2^30
        sl.stream = (int)c;
        if (t < ring_len) { sl.start = 0; sl.len = t < window_len ? (int)t : window_len; }
        else { sl.start = (int)(t - window_len); sl.len = window_len; }
        sl.nf = (sl.len - 960) / 160 + 1;
    }
    table[i] = sl;
}

// ---- the pass's rows g0 + m, as ec_epilogue_kernel: scrub, features[g], emotion[g] = W (f_g | f_0 | f_0) + b with f_0 = features of
// row 0 of the row's OWN clip c = g / K.  Row (c, 0) is slot c K - g0 of this pass when c K >= g0; otherwise an earlier pass wrote
// features[c K] (every workgroup reads it, none of this launch writes it).  The sum keeps that kernel's order: one fmaf chain over
// k = 0 .. 263 from zero, then + bias. ----
__global__ __launch_bounds__(256) void ecb_epilogue_kernel(const float* __restrict__ fout, int rows, int64_t g0, int64_t K,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ features, float* __restrict__ emotion) {
    using namespace ec;
    __shared__ float wl[TN * WS];
    __shared__ float xl[TM * NFEAT];
    __shared__ float f0l[TM * NFEAT];
    const int tid = threadIdx.x, c = tid % TN, r = tid / TN, col0 = blockIdx.x * TN;
    const float* wsrc = w + (int64_t)col0 * NCAT;
    for (int i = tid; i < TN * NCAT; i += 256) wl[(i / NCAT) * WS + i % NCAT] = wsrc[i];
    const float bc = bias[col0 + c];
    for (int m0 = 0; m0 < rows; m0 += TM) {
        __syncthreads();                                                         // the turn before is done with xl and f0l; wl is written
        for (int i = tid; i < TM * NFEAT; i += 256) {
            const int m = m0 + i / NFEAT, j = i % NFEAT;
            float f = 0.f, f0 = 0.f;
            if (m < rows) {
                f = ec_scrub(fout[(int64_t)m * NFEAT + j]);
                const int64_t r0 = (g0 + m) / K * K;                             // row 0 of this row's clip
                f0 = r0 >= g0 ? ec_scrub(fout[(r0 - g0) * NFEAT + j]) : features[r0 * NFEAT + j];
                if (blockIdx.x == 0) features[(g0 + m) * NFEAT + j] = f;
            }
            xl[i] = f;
            f0l[i] = f0;
        }
        __syncthreads();
        const int m = m0 + r;
        if (m < rows) {
            const float* wr = wl + c * WS;
            const float* x = xl + r * NFEAT;
            const float* x0 = f0l + r * NFEAT;
            float acc = 0.f;
            for (int k = 0; k < NFEAT; ++k) acc = fmaf(wr[k], x[k], acc);
            for (int k = 0; k < NFEAT; ++k) acc = fmaf(wr[NFEAT + k], x0[k], acc);
            for (int k = 0; k < NFEAT; ++k) acc = fmaf(wr[2 * NFEAT + k], x0[k], acc);
            emotion[(g0 + m) * NEMO + col0 + c] = acc + bc;
        }
    }
}

// ---- one window per workgroup: the row a live stream would hold when the window ends ----
__global__ __launch_bounds__(256) void ec_rows_kernel(const float* __restrict__ track, int64_t K, int64_t clip_len, const int32_t* __restrict__ starts,
                                                      int64_t hop, int64_t window_frames, int update_samples, int min_samples,
                                                      float* __restrict__ out, uint8_t* __restrict__ valid) {
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    float v = 0.f;
    if (K > 0) {
        int64_t e = ((int64_t)starts[b] + window_frames) * hop;
        if (e > clip_len) e = clip_len;
        int64_t k = e < min_samples ? 0 : (e - min_samples) / update_samples;
        if (k > K - 1) k = K - 1;
        v = track[k * ec::NEMO + tid];
    }
    out[b * ec::NEMO + tid] = v;
    if (valid && tid == 0) valid[b] = K > 0 ? 1 : 0;
}

// ---- the same mapping at width 9: window b = 16 blockIdx.x + tid / 16, column tid % 16 (columns 9 .. 15 idle); the row law is the
// only division ----
__global__ __launch_bounds__(256) void ec_rows9_kernel(const float* __restrict__ track, int64_t K, int64_t clip_len, const int32_t* __restrict__ starts,
                                                       int64_t B, int64_t hop, int64_t window_frames, int update_samples, int min_samples,
                                                       float* __restrict__ out, uint8_t* __restrict__ valid) {
    const int tid = threadIdx.x, c = tid % ec::RW;                               // RW is a power of two: a mask and a shift
    const int64_t b = (int64_t)blockIdx.x * ec::RW + tid / ec::RW;
    if (b >= B || c >= ec::NBASIC) return;
    float v = 0.f;
    if (K > 0) {
        int64_t e = ((int64_t)starts[b] + window_frames) * hop;
        if (e > clip_len) e = clip_len;
        int64_t k = e < min_samples ? 0 : (e - min_samples) / update_samples;
        if (k > K - 1) k = K - 1;
        v = track[k * ec::NBASIC + c];
    }
    out[b * ec::NBASIC + c] = v;
    if (valid && c == 0) valid[b] = K > 0 ? 1 : 0;
}

static int64_t ec_align16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

}  // namespace km

using namespace km;

extern "C" {

int km_emotion_clip_create(void** ec_out, double context_window_s, double update_interval_s, int64_t max_slots) {
    using namespace ec;
    if (!ec_out) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create: NULL argument");
    *ec_out = nullptr;
    if (!(context_window_s >= 1.0)) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create: Context window must be at least 1.0 seconds");
    if (!(update_interval_s >= 0.1)) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create: Update interval must be at least 0.1 seconds");
    if (update_interval_s > context_window_s) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create: Update interval cannot be larger than context window");
    if (max_slots < 1 || max_slots > 65535)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create: max_slots %lld, 1 .. 65535", (long long)max_slots);
    if (context_window_s > 3600.0) return fail(KM_ERR_UNSUPPORTED, "km_emotion_clip_create: context window of %g s", context_window_s);
    const int64_t R = (int64_t)((context_window_s + 2.0) * SR), Cw = (int64_t)(context_window_s * SR);
    const int64_t C = Cw < R ? Cw : R, U = (int64_t)(update_interval_s * SR), MIN = (int64_t)(0.5 * SR);
    const int64_t nf = km_egemaps_num_frames(C);
    if (nf > MAXF)
        return fail(KM_ERR_UNSUPPORTED, "km_emotion_clip_create: %lld frames per window, at most %d (20.5 s)", (long long)nf, MAXF);
    std::unique_ptr<EmotionClip> e(new (std::nothrow) EmotionClip());
    if (!e) return fail(KM_ERR_HIP, "km_emotion_clip_create: out of host memory");
    e->max_slots = max_slots;
    e->ring_len = (int)R; e->window_len = (int)C; e->update_samples = (int)U; e->min_samples = (int)MIN; e->max_nf = (int)nf;
    if (const int rc = km_egemaps_plan_create(&e->plan)) return rc;
    const int64_t ms = max_slots;
    // one allocation; `carve` hands out 16-byte aligned pieces, first with a null base to learn the size, then for real
    auto layout = [&](char* base) {
        int64_t at = 0;
        auto carve = [&](int64_t bytes) { char* p = base ? base + at : nullptr; at += ec_align16(bytes); return p; };
        e->table = reinterpret_cast<EgmSlot*>(carve(ms * (int64_t)sizeof(EgmSlot))); e->scale = reinterpret_cast<float*>(carve(ms * 4));
        e->rec = reinterpret_cast<float*>(carve(ms * nf * REC * 4)); e->fout = reinterpret_cast<float*>(carve(ms * NFEAT * 4));
        e->f0 = reinterpret_cast<float*>(carve(NFEAT * 4));
        e->w = reinterpret_cast<float*>(carve((int64_t)NEMO * NCAT * 4)); e->bias = reinterpret_cast<float*>(carve(NEMO * 4));
        return at;
    };
    const int64_t bytes = layout(nullptr);
    if (int rc = e->blob.alloc(bytes, "km_emotion_clip_create")) return rc;
    HIP_TRY(hipMemset(e->blob, 0, (size_t)bytes));
    layout(e->blob);
    *ec_out = e.release();
    return KM_OK;
}

int km_emotion_clip_create_basic(void** ec_out, double context_window_s, double update_interval_s, int64_t max_slots) {
    using namespace ec;
    if (!ec_out) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create_basic: NULL argument");
    *ec_out = nullptr;
    if (!(context_window_s >= 1.0)) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create_basic: Context window must be at least 1.0 seconds");
    if (!(update_interval_s >= 0.1)) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create_basic: Update interval must be at least 0.1 seconds");
    if (update_interval_s > context_window_s)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create_basic: Update interval cannot be larger than context window");
    if (max_slots < 1 || max_slots > 65535)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_create_basic: max_slots %lld, 1 .. 65535", (long long)max_slots);
    if (context_window_s > 3600.0) return fail(KM_ERR_UNSUPPORTED, "km_emotion_clip_create_basic: context window of %g s", context_window_s);
    const int64_t R = (int64_t)((context_window_s + 2.0) * SR), Cw = (int64_t)(context_window_s * SR);
    const int64_t C = Cw < R ? Cw : R, U = (int64_t)(update_interval_s * SR), MIN = (int64_t)(0.5 * SR);
    if (C > BASIC_MAX_WINDOW)
        return fail(KM_ERR_UNSUPPORTED, "km_emotion_clip_create_basic: a window of %lld samples, at most %d (65.5 s)", (long long)C, BASIC_MAX_WINDOW);
    const int64_t nf = 1 + C / BASIC_HOP;                                        // 32 ms frame records per window
    std::unique_ptr<EmotionClip> e(new (std::nothrow) EmotionClip());
    if (!e) return fail(KM_ERR_HIP, "km_emotion_clip_create_basic: out of host memory");
    e->max_slots = max_slots; e->basic = true;
    e->ring_len = (int)R; e->window_len = (int)C; e->update_samples = (int)U; e->min_samples = (int)MIN; e->max_nf = (int)nf;
    if (const int rc = km_prosody_plan_create(&e->prosody)) return rc;
    const int64_t table_bytes = ec_align16(max_slots * (int64_t)sizeof(EgmSlot));
    const int64_t bytes = table_bytes + ec_align16(max_slots * nf * BASIC_REC * 4);
    if (int rc = e->blob.alloc(bytes, "km_emotion_clip_create_basic")) return rc;
    HIP_TRY(hipMemset(e->blob, 0, (size_t)bytes));
    e->table = reinterpret_cast<EgmSlot*>((char*)e->blob);
    e->rec = reinterpret_cast<float*>((char*)e->blob + table_bytes);
    *ec_out = e.release();
    return KM_OK;
}

int km_emotion_clip_width(void* ec) {
    if (!ec) return 0;
    return static_cast<EmotionClip*>(ec)->basic ? ec::NBASIC : ec::NEMO;
}

int km_emotion_clip_destroy(void* ec) {
    if (!ec) return KM_OK;
    delete static_cast<EmotionClip*>(ec);
    return KM_OK;
}

int km_emotion_clip_set_compression(void* ec, const float* w_dev, const float* b_dev, void* stream) {
    if (!ec || !w_dev || !b_dev) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_set_compression: NULL argument");
    EmotionClip* e = static_cast<EmotionClip*>(ec);
    if (e->basic) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_set_compression: the basic back end has no compression layer");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(e->w, w_dev, (size_t)ec::NEMO * ec::NCAT * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->bias, b_dev, ec::NEMO * sizeof(float), hipMemcpyDeviceToDevice, st));
    e->has_compression = true;
    return KM_OK;
}

int64_t km_emotion_clip_num_rows(void* ec, int64_t clip_len) {
    if (!ec || clip_len < 0) return 0;
    return ec_num_rows(static_cast<EmotionClip*>(ec), clip_len);
}

int km_emotion_clip_build(void* ec, const float* clip_dev, int64_t clip_len, float* features_out, float* emotion_out, void* stream) {
    if (!ec) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build: NULL argument");
    EmotionClip* e = static_cast<EmotionClip*>(ec);
    if (clip_len < 0 || clip_len > ec::MAX_CLIP)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build: clip of %lld samples, 0 .. 2^30 (window starts are 32-bit)", (long long)clip_len);
    if (e->basic && features_out) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build: the basic back end has no functionals (features_out)");
    if (!e->basic && !e->has_compression) return fail(KM_ERR_NOT_READY, "km_emotion_clip_build: km_emotion_clip_set_compression first");
    const int64_t K = ec_num_rows(e, clip_len);
    if (K == 0) return KM_OK;                                                    // shorter than half a second: a track without rows
    if (!clip_dev || !emotion_out) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int ms = (int)e->max_slots;
    if (e->basic) {
        for (int64_t k0 = 0; k0 < K; k0 += ms) {                                 // slot i of the pass is row k0 + i; slots past K are empty
            hipLaunchKernelGGL(ec_plan_kernel, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, st, k0, K, ms, e->ring_len, e->window_len,
                               e->update_samples, e->min_samples, e->table);
            HIP_TRY(hipGetLastError());
            if (const int rc = prosody_ragged(e->prosody, clip_dev, clip_len, e->table, ms, e->max_nf, e->rec, emotion_out + k0 * ec::NBASIC, st))
                return rc;
        }
        return KM_OK;
    }
    for (int64_t k0 = 0; k0 < K; k0 += ms) {                                     // pass 0 first: it leaves features[0] in f0
        const int rows = (int)(K - k0 < ms ? K - k0 : ms);
        hipLaunchKernelGGL(ec_plan_kernel, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, st, k0, K, ms, e->ring_len, e->window_len,
                           e->update_samples, e->min_samples, e->table);
        HIP_TRY(hipGetLastError());
        if (const int rc = egm_ragged_functionals(e->plan, clip_dev, clip_len, e->table, ms, e->max_nf, e->scale, e->rec, e->fout, st)) return rc;
        hipLaunchKernelGGL(ec_epilogue_kernel, dim3(ec::NEMO / ec::TN), dim3(256), 0, st, (const float*)e->fout, rows, k0, e->f0,
                           (const float*)e->w, (const float*)e->bias, features_out, emotion_out);
        HIP_TRY(hipGetLastError());
    }
    return KM_OK;
}

int km_emotion_clip_build_batch(void* ec, const float* clips_dev, int64_t B, int64_t L, float* features_out, float* emotion_out, void* stream) {
    if (!ec) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build_batch: NULL argument");
    EmotionClip* e = static_cast<EmotionClip*>(ec);
    if (B < 0 || L < 0 || L > ec::MAX_CLIP)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build_batch: %lld clips of %lld samples, 0 .. 2^30 (window starts are 32-bit)",
                    (long long)B, (long long)L);
    if (e->basic && features_out)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build_batch: the basic back end has no functionals (features_out)");
    if (!e->basic && !e->has_compression) return fail(KM_ERR_NOT_READY, "km_emotion_clip_build_batch: km_emotion_clip_set_compression first");
    const int64_t K = ec_num_rows(e, L);
    if (K == 0 || B == 0) return KM_OK;
    if (B > 0x7fffffff / K)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build_batch: %lld clips x %lld rows, at most 2^31 - 1 rows", (long long)B, (long long)K);
    if (e->basic) {
        if (!clips_dev || !emotion_out) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build_batch: NULL argument");
        hipStream_t st = (hipStream_t)stream;
        const int ms = (int)e->max_slots;
        const int64_t G = B * K;
        for (int64_t g0 = 0; g0 < G; g0 += ms) {                                 // slot i of the pass is row g0 + i of (B, K, 9)
            hipLaunchKernelGGL(ecb_plan_kernel, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, st, g0, G, K, ms, e->ring_len, e->window_len,
                               e->update_samples, e->min_samples, e->table);
            HIP_TRY(hipGetLastError());
            if (const int rc = prosody_ragged(e->prosody, clips_dev, L, e->table, ms, e->max_nf, e->rec, emotion_out + g0 * ec::NBASIC, st))
                return rc;
        }
        return KM_OK;
    }
    // features_out is read back by the passes that follow a clip's row 0, so it is not optional here
    if (!clips_dev || !features_out || !emotion_out) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build_batch: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int ms = (int)e->max_slots;
    const int64_t G = B * K;
    for (int64_t g0 = 0; g0 < G; g0 += ms) {                                     // in order: a pass may read features[c, 0] of an earlier one
        const int rows = (int)(G - g0 < ms ? G - g0 : ms);
        hipLaunchKernelGGL(ecb_plan_kernel, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, st, g0, G, K, ms, e->ring_len, e->window_len,
                           e->update_samples, e->min_samples, e->table);
        HIP_TRY(hipGetLastError());
        if (const int rc = egm_ragged_functionals(e->plan, clips_dev, L, e->table, ms, e->max_nf, e->scale, e->rec, e->fout, st)) return rc;
        hipLaunchKernelGGL(ecb_epilogue_kernel, dim3(ec::NEMO / ec::TN), dim3(256), 0, st, (const float*)e->fout, rows, g0, K,
                           (const float*)e->w, (const float*)e->bias, features_out, emotion_out);
        HIP_TRY(hipGetLastError());
    }
    return KM_OK;
}

int km_emotion_clip_rows(void* ec, const float* emotion_track_dev, int64_t K, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                         int64_t hop, int64_t window_frames, float* emotion_out, uint8_t* valid_out, void* stream) {
    if (!ec) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_rows: NULL argument");
    EmotionClip* e = static_cast<EmotionClip*>(ec);
    if (clip_len < 0 || clip_len > ec::MAX_CLIP)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_rows: clip of %lld samples, 0 .. 2^30", (long long)clip_len);
    if (K != ec_num_rows(e, clip_len))
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_rows: a track of %lld rows, a clip of %lld samples has %lld", (long long)K,
                    (long long)clip_len, (long long)ec_num_rows(e, clip_len));
    if (B < 0 || B > 0x7fffffff || hop < 1 || hop > ec::MAX_CLIP || window_frames < 1 || window_frames > ec::MAX_CLIP)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_rows: B %lld, hop %lld, window_frames %lld", (long long)B, (long long)hop,
                    (long long)window_frames);
    if (B == 0) return KM_OK;
    if (!start_frames_dev || !emotion_out || (K > 0 && !emotion_track_dev)) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_rows: NULL argument");
    if (e->basic) {
        hipLaunchKernelGGL(ec_rows9_kernel, dim3((unsigned)((B + ec::RW - 1) / ec::RW)), dim3(ec::RW * ec::RW), 0, (hipStream_t)stream,
                           emotion_track_dev, K, clip_len, start_frames_dev, B, hop, window_frames, e->update_samples, e->min_samples, emotion_out,
                           valid_out);
    } else {
        hipLaunchKernelGGL(ec_rows_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, emotion_track_dev, K, clip_len, start_frames_dev, hop,
                           window_frames, e->update_samples, e->min_samples, emotion_out, valid_out);
    }
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // extern "C"
