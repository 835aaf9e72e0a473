// The emotion track of a resident clip: what one emotion stream (km_emotion_stream.hip) would hold after t samples of the clip,
// for every update time t_k = MIN + k U at once -- the offline producer of the model's 256-D emotion input.  A training window's
// emotion vector is the row of the update a live stream would last have made when the window ends, so a clip has ONE track and a
// step gathers rows from it by start frame.  B clips of one length (km_emotion_clip_build_batch) are the B "rings" of one build:
// rows numbered g = c K + k fill the passes across clip boundaries, and a single clip (km_emotion_clip_build) is B = 1.
//   ec_plan_kernel       the window of row (c, k) in closed form (AudioBuffer.get_window after t_k samples, src/features/
//                        opensmile_extractor.py:111-130) as an EgmSlot: clip c is the "ring", ring_len = clip length, no wrap
//   km_egemaps.hip       the five ragged eGeMAPS kernels, as the streams launch them (egm_ragged_functionals)
//   ec_epilogue_kernel   NaN / Inf -> 0 (:450-452), features[g], and W concat(features[g], features[c, 0], features[c, 0]) + b for all
//                        rows of the pass: the 300 / 600 ms slots are filled once per life (:478-490) and a clip is one life
//   ec_rows_kernel       window -> row: e = min(n, (s + T) h), k = clamp((e - MIN) / U, 0, K - 1), a copy of the row per window
// build and rows neither allocate, synchronise nor read back; rows' grid depends on the batch alone, so it captures into a hipGraph.
//
// The `basic` back end (km_emotion_clip_create_basic): the same slot law and the same row mapping, but a row is the nine raw prosodic
// values of its window as km_emotion_stream_create_basic's streams hold them.  ec_plan_kernel writes the table, prosody_ragged
// (km_prosody.hip) reads the windows in place from the clip and writes slot i to row i of the pointer it is handed -- which is track
// row g0 of the caller's output, since it skips empty slots: no staging copy, no epilogue.  ec_rows_kernel copies at width 9, sixteen
// windows per workgroup.
#include <hip/hip_runtime.h>

#include <new>

#include <memory>

#include "km_context.h"
#include "km_egemaps_window.h"
#include "km_egemaps_ragged.h"
#include "km_emotion_common.h"
#include "km_prosody_ragged.h"

namespace km {


namespace ec {
using namespace emo;
constexpr int TN = 16, TM = 16;          // the epilogue's tile: output columns per workgroup, rows per turn (TN * TM = 256 threads)
constexpr int ws(int nf) { return 3 * nf + 1; }    // LDS stride of a weight row: 265 (187 for the 62 of GeMAPS) is odd, so the 16 columns of a half wave hit 16 banks
static_assert(ws(NFEAT) % 2 == 1 && ws(62) % 2 == 1, "odd strides");
constexpr int64_t MAX_CLIP = (int64_t)1 << 30;     // egm_ragged_functionals' ring limit; EgmSlot.start is an int32
constexpr int RW = 16;                   // rows at width 9: the lanes a window takes, so 256 / 16 windows per workgroup
}  // namespace ec

struct EmotionClip : EmoTiming {
    int64_t max_slots = 0;
    void* plan = nullptr;
    DevBuf<char> blob;         // one allocation, carved below
    EgmSlot* table = nullptr;  // (max_slots)
    float* scale = nullptr;    // (max_slots)
    float* rec = nullptr;      // (max_slots, max_nf, 36)
    float* fout = nullptr;     // (max_slots, 88)
    float* f0 = nullptr;       // (88): features[0] of the clip being built, for a build without features_out
    float* w = nullptr;        // (256, 264) as nn.Linear stores it
    float* bias = nullptr;     // (256)
    bool has_compression = false;
    bool basic = false;        // the `basic` back end: rows of 9, rec is (max_slots, max_nf, 4), no scale / fout / f0 / w / bias
    int feature_set = 0;       // KM_FEATURE_SET_*; nfeat = 88 or 62: fout (max_slots, nfeat), f0 (nfeat), w (256, 3 nfeat)
    int nfeat = emo::NFEAT;
    bool long_windows = false; // km_emotion_clip_create_long with more than 2048 frames per window: the long tier of the per-window kernels (km_egemaps_window.hip)
    void* prosody = nullptr;
    ~EmotionClip() { (void)km_egemaps_plan_destroy(plan); (void)km_prosody_plan_destroy(prosody); }
};

static int64_t ec_num_rows(const EmotionClip* e, int64_t clip_len) {
    return clip_len < e->min_samples ? 0 : (clip_len - e->min_samples) / e->update_samples + 1;
}

// ---- rows g0 .. g0 + max_slots - 1 of the numbering g = c K + k as slots of clip c: [0, min(t, C)) while t < R (the OLDEST C
// samples, as get_window returns them before the ring has wrapped), [t - C, t) from t >= R on ----
__global__ __launch_bounds__(256) void ec_plan_kernel(int64_t g0, int64_t G, int64_t K, int max_slots, int ring_len, int window_len,
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
        sl.nf = emo_slot_frames(sl.len);
    }
    table[i] = sl;
}

// ---- the pass's rows g0 + m: scrub, features[g], emotion[g] = W (f_g | f_0 | f_0) + b with f_0 = features of row 0 of the row's OWN
// clip c = g / K.  Workgroup j owns output columns 16 j .. 16 j + 15: their 16 x 264 weights go to LDS once and serve every row of
// the pass, 16 rows per turn (thread = column x row).  Row (c, 0) is slot c K - g0 of this pass when c K >= g0; otherwise an earlier
// pass wrote features[c K] (every workgroup reads it, none of this launch writes it).  Without `features` (one clip, so c = 0) the
// object's f0 stands in for features[0]: block 0 of the pass that holds row 0 stores it, later passes read it.  A row's sum is one
// fmaf chain over k = 0 .. 263 from zero, then + bias: the order of es_epilogue_kernel, whatever the pass holds.  NF = 62 (GeMAPS): the
// same at 62 features a row and 186 weights a column. ----
template <int NF>
__global__ __launch_bounds__(256) void ec_epilogue_kernel(const float* __restrict__ fout, int rows, int64_t g0, int64_t K, float* __restrict__ f0,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ features, float* __restrict__ emotion) {
    using namespace ec;
    constexpr int NFEAT = NF, NCAT = 3 * NF, WS = ws(NF);
    __shared__ float wl[TN * WS];
    __shared__ float xl[TM * NFEAT];
    __shared__ float f0l[TM * NFEAT];
    const int tid = threadIdx.x, c = tid % TN, r = tid / TN, col0 = blockIdx.x * TN;
    const float* wsrc = w + (int64_t)col0 * NCAT;                                // rows col0 .. col0 + 15 of W: one contiguous piece
    for (int i = tid; i < TN * NCAT; i += 256) wl[(i / NCAT) * WS + i % NCAT] = wsrc[i];
    const float bc = bias[col0 + c];
    for (int m0 = 0; m0 < rows; m0 += TM) {
        __syncthreads();                                                         // the turn before is done with xl and f0l; wl is written
        for (int i = tid; i < TM * NFEAT; i += 256) {
            const int m = m0 + i / NFEAT, j = i % NFEAT;
            float f = 0.f, x0 = 0.f;
            if (m < rows) {
                f = emo_scrub(fout[(int64_t)m * NFEAT + j]);
                const int64_t r0 = (g0 + m) / K * K;                             // row 0 of this row's clip
                if (r0 >= g0) x0 = emo_scrub(fout[(r0 - g0) * NFEAT + j]);
                else x0 = features ? features[r0 * NFEAT + j] : f0[j];
                if (blockIdx.x == 0) {
                    if (features) features[(g0 + m) * NFEAT + j] = f;
                    else if (g0 + m == 0) f0[j] = f;
                }
            }
            xl[i] = f;
            f0l[i] = x0;
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

// ---- the row a live stream would hold when the window that starts at frame `start` ends (K > 0) ----
__device__ __forceinline__ int64_t ec_row_of(int64_t start, int64_t window_frames, int64_t hop, int64_t clip_len, int64_t K, int update_samples,
                                             int min_samples) {
    int64_t e = (start + window_frames) * hop;
    if (e > clip_len) e = clip_len;
    const int64_t k = e < min_samples ? 0 : (e - min_samples) / update_samples;
    return k > K - 1 ? K - 1 : k;
}

// ---- a copy of W floats per window, LANES lanes a window (a power of two: a mask and a shift): window b = (256 / LANES) blockIdx.x +
// tid / LANES, column tid % LANES, lanes W .. LANES - 1 idle.  <256, 256> is a window per workgroup, <9, 16> sixteen ----
template <int W, int LANES>
__global__ __launch_bounds__(256) void ec_rows_kernel(const float* __restrict__ track, int64_t K, int64_t clip_len, const int32_t* __restrict__ starts,
                                                      int64_t B, int64_t hop, int64_t window_frames, int update_samples, int min_samples,
                                                      float* __restrict__ out, uint8_t* __restrict__ valid) {
    const int tid = threadIdx.x, c = tid % LANES;
    const int64_t b = (int64_t)blockIdx.x * (256 / LANES) + tid / LANES;
    if (b >= B || c >= W) return;
    out[b * W + c] = K > 0 ? track[ec_row_of(starts[b], window_frames, hop, clip_len, K, update_samples, min_samples) * W + c] : 0.f;
    if (valid && c == 0) valid[b] = K > 0 ? 1 : 0;
}

static int ec_create(const char* fn, void** ec_out, double context_window_s, double update_interval_s, int64_t max_slots, bool basic,
                     bool long_windows = false, int feature_set = 0) {
    using namespace ec;
    if (!ec_out) return fail(KM_ERR_INVALID_ARG, "%s: NULL argument", fn);
    *ec_out = nullptr;
    if (!egm::set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "%s: feature set %d, 0 (eGeMAPS) or 1 (GeMAPS)", fn, feature_set);
    if (const int rc = emo_check_seconds(fn, context_window_s, update_interval_s)) return rc;
    if (max_slots < 1 || max_slots > 65535) return fail(KM_ERR_INVALID_ARG, "%s: max_slots %lld, 1 .. 65535", fn, (long long)max_slots);
    std::unique_ptr<EmotionClip> e(new (std::nothrow) EmotionClip());
    if (!e) return fail(KM_ERR_HIP, "%s: out of host memory", fn);
    if (const int rc = emo_timing(fn, context_window_s, update_interval_s, basic, e.get(), long_windows)) return rc;
    e->max_slots = max_slots; e->basic = basic;
    e->feature_set = feature_set; e->nfeat = egm::set_width(feature_set);
    e->long_windows = long_windows && e->max_nf > MAXF;                         // up to 2048 frames it is the plain object
    if (e->long_windows)
        if (const int rc = egm_window_prepare()) return rc;
    if (const int rc = basic ? km_prosody_plan_create(&e->prosody) : km_egemaps_plan_create(&e->plan)) return rc;
    const int64_t ms = max_slots, nf = e->max_nf, NF = e->nfeat;
    auto layout = [&](char* base) {
        EmoCarver c{base};
        e->table = c.take<EgmSlot>(ms); e->rec = c.take<float>(ms * nf * (basic ? BASIC_REC : REC));
        if (!basic) {
            e->scale = c.take<float>(ms); e->fout = c.take<float>(ms * NF); e->f0 = c.take<float>(NF);
            e->w = c.take<float>(NEMO * 3 * NF); e->bias = c.take<float>(NEMO);
        }
        return c.at;
    };
    const int64_t bytes = layout(nullptr);
    if (int rc = e->blob.alloc(bytes, fn)) return rc;
    HIP_TRY(hipMemset(e->blob, 0, (size_t)bytes));
    layout(e->blob);
    *ec_out = e.release();
    return KM_OK;
}

// ---- the passes of max_slots rows over the B K rows of B clips of L samples, in order: a pass may read features[c, 0] (or f0) of an
// earlier one.  Slot i of a pass is row g0 + i; slots past the last row are empty.  The back end decides which ragged extractor runs
// and whether an epilogue follows: prosody_ragged writes its nine values straight to row g0 + i of the track. ----
static int ec_build(EmotionClip* e, const float* clips_dev, int64_t B, int64_t L, int64_t K, float* features_out, float* emotion_out,
                    hipStream_t st) {
    const int ms = (int)e->max_slots;
    const int64_t G = B * K;
    for (int64_t g0 = 0; g0 < G; g0 += ms) {
        hipLaunchKernelGGL(ec_plan_kernel, dim3((unsigned)((ms + 255) / 256)), dim3(256), 0, st, g0, G, K, ms, e->ring_len, e->window_len,
                           e->update_samples, e->min_samples, e->table);
        HIP_TRY(hipGetLastError());
        if (e->basic) {
            if (const int rc = prosody_ragged(e->prosody, clips_dev, L, e->table, ms, e->max_nf, e->rec, emotion_out + g0 * ec::NBASIC, st)) return rc;
            continue;
        }
        if (const int rc = egm_ragged_functionals(e->plan, clips_dev, L, e->table, ms, e->max_nf, e->scale, e->rec, e->fout, st, e->long_windows,
                                                  e->feature_set))
            return rc;
        const auto epilogue = e->nfeat == egm::NFEAT_GEMAPS ? ec_epilogue_kernel<egm::NFEAT_GEMAPS> : ec_epilogue_kernel<ec::NFEAT>;
        hipLaunchKernelGGL(epilogue, dim3(ec::NEMO / ec::TN), dim3(256), 0, st, (const float*)e->fout, (int)(G - g0 < ms ? G - g0 : ms), g0, K,
                           e->f0, (const float*)e->w, (const float*)e->bias, features_out, emotion_out);
        HIP_TRY(hipGetLastError());
    }
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" {

int km_emotion_clip_create(void** ec_out, double context_window_s, double update_interval_s, int64_t max_slots) {
    return ec_create("km_emotion_clip_create", ec_out, context_window_s, update_interval_s, max_slots, false);
}

int km_emotion_clip_create_long(void** ec_out, double context_window_s, double update_interval_s, int64_t max_slots) {
    return ec_create("km_emotion_clip_create_long", ec_out, context_window_s, update_interval_s, max_slots, false, true);
}

int km_emotion_clip_create_basic(void** ec_out, double context_window_s, double update_interval_s, int64_t max_slots) {
    return ec_create("km_emotion_clip_create_basic", ec_out, context_window_s, update_interval_s, max_slots, true);
}

int km_emotion_clip_create_set(void** ec_out, double context_window_s, double update_interval_s, int64_t max_slots, int32_t feature_set,
                               int32_t long_windows) {
    return ec_create("km_emotion_clip_create_set", ec_out, context_window_s, update_interval_s, max_slots, false, long_windows != 0, feature_set);
}

int km_emotion_clip_feature_width(void* ec) {
    if (!ec) return 0;
    const EmotionClip* e = static_cast<EmotionClip*>(ec);
    return e->basic ? ec::NBASIC : e->nfeat;
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
    HIP_TRY(hipMemcpyAsync(e->w, w_dev, (size_t)ec::NEMO * 3 * e->nfeat * sizeof(float), hipMemcpyDeviceToDevice, st));
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
    return ec_build(e, clip_dev, 1, clip_len, K, features_out, emotion_out, (hipStream_t)stream);
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
    // features_out is read back by the passes that follow a clip's row 0, so it is not optional here
    if (!clips_dev || !emotion_out || (!e->basic && !features_out)) return fail(KM_ERR_INVALID_ARG, "km_emotion_clip_build_batch: NULL argument");
    return ec_build(e, clips_dev, B, L, K, features_out, emotion_out, (hipStream_t)stream);
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
    const auto kernel = e->basic ? ec_rows_kernel<ec::NBASIC, ec::RW> : ec_rows_kernel<ec::NEMO, ec::NEMO>;
    const int64_t per_group = e->basic ? 256 / ec::RW : 1;                      // windows per workgroup
    hipLaunchKernelGGL(kernel, dim3((unsigned)((B + per_group - 1) / per_group)), dim3(256), 0, (hipStream_t)stream, emotion_track_dev, K, clip_len,
                       start_frames_dev, B, hop, window_frames, e->update_samples, e->min_samples, emotion_out, valid_out);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // extern "C"
