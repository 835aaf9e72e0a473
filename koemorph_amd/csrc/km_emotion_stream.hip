// Emotion vectors of many speaker streams, resident on the device -- the real-time state machine of the reference's
// OpenSMILEeGeMAPSExtractor (src/features/opensmile_extractor.py) for all streams at once:
//   AudioBuffer.append / get_window          :29-154    es_append_kernel + es_advance_kernel, the window arithmetic of es_select_kernel
//   process_audio_frame / _extract_features  :287-425   es_select_kernel (who is due, who holds half a second), the ragged eGeMAPS
//                                                       kernels of km_egemaps.hip on the windows where they lie in the rings
//   _extract_features_from_audio             :450-452   es_epilogue_kernel: NaN / Inf -> 0
//   _update_window_features                  :460-502   es_epilogue_kernel: the 300 / 600 ms slots are filled once per life
//   get_concatenated_features                :559-608   es_epilogue_kernel: Linear(264, 256) of current | slot 300 | slot 600
//   reset                                    :640-659   es_reset_kernel, per stream
//
// A second back end on the same rings, push, selection, reset and capture contract (km_emotion_stream_create_basic): a selected
// stream's features are the nine raw values of EmotionExtractor._extract_basic on its window (km_prosody.hip over the same slot
// table), kept in the first 9 of the stream's 88 feature floats; no peak normalisation, no slots, no Linear(264, 256).
//
// A second feature set on the eGeMAPS back end (km_emotion_stream_create_set, KM_FEATURE_SET_GEMAPS): the 62 functionals of GeMAPS, the
// emotion input of the reference's `fast` variant.  The epilogue, the reset and the transpose are templates on the feature count NF, 88
// or 62: features (n, NF), slots (n, 2, NF), Linear(3 NF, 256) -- the same sequential chain over k with the removed columns' terms left out.
//
// Time is audio time: a stream is due when `update_samples` samples have arrived since its last update (the reference asks
// time.time()), so every result is a function of the call sequence.  Nothing here allocates, synchronises or reads back after
// creation and every grid is fixed by (n_streams, max_updates): push + update capture into a hipGraph as one linear chain.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include <memory>

#include "km_context.h"
#include "km_egemaps_window.h"
#include "km_egemaps_ragged.h"
#include "km_emotion_common.h"
#include "km_prosody_ragged.h"

namespace km {


namespace es {
using namespace emo;
constexpr int SEL_THREADS = 1024, MAX_STREAMS = 4096;   // the selection ranks all streams in one workgroup, waiting times in LDS
}  // namespace es

// per-stream counters (arrays of n_streams)
struct EsState {
    int32_t* write_pos;        // AudioBuffer.write_pos
    int32_t* is_full;          // AudioBuffer.is_full
    int64_t* total;            // samples since creation or reset
    int64_t* last_total;       // `total` at the last update, -1 = never
    int32_t* has_features;     // current_features is not None
    int32_t* slots_filled;     // window_features[0.3] / [0.6] are not None
};

struct EmotionStream : EmoTiming {
    int64_t n = 0, max_updates = 0;
    void* plan = nullptr;
    DevBuf<char> blob;         // one allocation, carved below
    float* ring = nullptr;     // (n, ring_len)
    EsState st{};
    float* features = nullptr; // (n, nfeat): (n, 88), or (n, 62) for GeMAPS; slots, fout and wt likewise
    float* slots = nullptr;    // (n, 2, 88)
    float* emotion = nullptr;  // (n, 256)
    uint8_t* updated = nullptr;// (n)
    EgmSlot* table = nullptr;  // (max_updates)
    float* scale = nullptr;    // (max_updates)
    float* rec = nullptr;      // (max_updates, max_nf, 36)
    float* fout = nullptr;     // (max_updates, 88)
    float* wt = nullptr;       // (264, 256): the compression weight transposed
    float* bias = nullptr;     // (256)
    bool has_compression = false;
    bool basic = false;        // the `basic` back end: features holds 9 values per stream (row stride 88), no slots, no emotion layer
    int feature_set = 0;       // KM_FEATURE_SET_*; nfeat = 88 or 62 (the basic back end keeps its 9 values at the stride of 88)
    int nfeat = emo::NFEAT;
    bool long_windows = false; // km_emotion_stream_create_long with more than 2048 frames per window: the long tier of the per-window kernels (km_egemaps_window.hip)
    void* prosody = nullptr;
    ~EmotionStream() { (void)km_egemaps_plan_destroy(plan); (void)km_prosody_plan_destroy(prosody); }
};

// ---- AudioBuffer.append (:63-96) ----
__global__ __launch_bounds__(256) void es_append_kernel(const float* __restrict__ samples, int m, const int32_t* __restrict__ counts,
                                                        float* __restrict__ ring, int ring_len, const int32_t* __restrict__ write_pos) {
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    int c = counts ? counts[s] : m;
    c = c < 0 ? 0 : (c > m ? m : c);
    if (i >= c) return;
    int j = write_pos[s] + i;                        // write_pos < ring_len, i < m <= ring_len
    if (j >= ring_len) j -= ring_len;
    ring[(int64_t)s * ring_len + j] = samples[(int64_t)s * m + i];
}

__global__ __launch_bounds__(256) void es_advance_kernel(int n, int m, const int32_t* __restrict__ counts, int ring_len, EsState st) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    int c = counts ? counts[s] : m;
    c = c < 0 ? 0 : (c > m ? m : c);
    if (c == 0) return;
    int wp = st.write_pos[s], full = st.is_full[s];
    const int room = ring_len - wp;
    if (c <= room) wp += c;
    else { wp = c - room; full = 1; }
    if (wp >= ring_len) { wp = 0; full = 1; }
    st.write_pos[s] = wp; st.is_full[s] = full; st.total[s] += c;
}

// ---- who updates on this call: eligibility, then the max_updates longest-waiting streams by counting ----
__global__ __launch_bounds__(es::SEL_THREADS) void es_select_kernel(int n, int max_updates, int ring_len, int window_len, int update_samples,
                                                                    int min_samples, EsState st, EgmSlot* __restrict__ table,
                                                                    uint8_t* __restrict__ updated) {
    __shared__ int64_t wait[es::MAX_STREAMS];
    const int tid = threadIdx.x;
    for (int k = tid; k < max_updates; k += es::SEL_THREADS) table[k] = EgmSlot{-1, 0, 0, 0};
    for (int s = tid; s < n; s += es::SEL_THREADS) {
        const int64_t total = st.total[s], last = st.last_total[s];
        const int len = st.is_full[s] ? window_len : (st.write_pos[s] < window_len ? st.write_pos[s] : window_len);
        const bool due = !st.has_features[s] || total - last >= update_samples;
        wait[s] = (total > 0 && due && len >= min_samples) ? total - last : -1;    // never updated: last = -1, waits longest of its age
        updated[s] = 0;
    }
    __syncthreads();
    for (int s = tid; s < n; s += es::SEL_THREADS) {
        const int64_t w = wait[s];
        if (w < 0) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) { const int64_t wj = wait[j]; rank += (wj > w || (wj == w && j < s)) ? 1 : 0; }
        if (rank >= max_updates) continue;
        const int wp = st.write_pos[s];
        EgmSlot sl;
        sl.stream = s;
        if (st.is_full[s]) { sl.len = window_len; sl.start = wp - window_len; if (sl.start < 0) sl.start += ring_len; }
        else { sl.len = wp < window_len ? wp : window_len; sl.start = 0; }
        sl.nf = emo_slot_frames(sl.len);
        table[rank] = sl;
        updated[s] = 1;
    }
}

// ---- per selected stream: scrub, slots, bookkeeping, Linear(3 NF, 256) ----
template <int NF>
__global__ __launch_bounds__(256) void es_epilogue_kernel(const EgmSlot* __restrict__ table, const float* __restrict__ fout, EsState st,
                                                          float* __restrict__ features, float* __restrict__ slots,
                                                          const float* __restrict__ wt, const float* __restrict__ bias, float* __restrict__ emotion) {
    using namespace es;
    constexpr int NFEAT = NF, NCAT = 3 * NF;
    __shared__ float x[NCAT];
    const int tid = threadIdx.x;
    const EgmSlot sl = table[blockIdx.x];
    if (sl.stream < 0) return;
    const int s = sl.stream;
    const bool filled = st.slots_filled[s] != 0;
    if (tid < NFEAT) {
        const float f = emo_scrub(fout[(int64_t)blockIdx.x * NFEAT + tid]);
        features[(int64_t)s * NFEAT + tid] = f;
        float* sp = slots + (int64_t)s * 2 * NFEAT;
        if (!filled) { sp[tid] = f; sp[NFEAT + tid] = f; }
        x[tid] = f; x[NFEAT + tid] = filled ? sp[tid] : f; x[2 * NFEAT + tid] = filled ? sp[NFEAT + tid] : f;
    }
    __syncthreads();                                   // also: every thread has read slots_filled before thread 0 sets it
    float acc = 0.f;
    for (int k = 0; k < NCAT; ++k) acc = fmaf(wt[k * NEMO + tid], x[k], acc);
    emotion[(int64_t)s * NEMO + tid] = acc + bias[tid];
    if (tid == 0) { st.last_total[s] = st.total[s]; st.has_features[s] = 1; st.slots_filled[s] = 1; }
}

// ---- rows of W floats, STRIDE apart in the object, to the caller's dense (n, W): <256, 256> the emotion rows, <9, 88> the nine
// values of the `basic` back end where they lie in `features` ----
template <int W, int STRIDE>
__global__ __launch_bounds__(256) void es_output_kernel(int n, const float* __restrict__ src, const int32_t* __restrict__ has_features,
                                                        const uint8_t* __restrict__ updated, float* __restrict__ emotion_out,
                                                        uint8_t* __restrict__ valid_out, uint8_t* __restrict__ updated_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (int64_t)n * W) emotion_out[i] = src[W == STRIDE ? i : (i / W) * STRIDE + i % W];
    if (i < n) {
        if (valid_out) valid_out[i] = has_features[i] ? 1 : 0;
        if (updated_out) updated_out[i] = updated[i];
    }
}

// ---- the `basic` back end: the nine values of a selected stream's window are its features as they are ----
__global__ __launch_bounds__(64) void es_basic_epilogue_kernel(const EgmSlot* __restrict__ table, const float* __restrict__ fout, EsState st,
                                                               float* __restrict__ features) {
    using namespace es;
    const EgmSlot sl = table[blockIdx.x];
    if (sl.stream < 0) return;
    const int s = sl.stream, tid = threadIdx.x;
    if (tid < NBASIC) features[(int64_t)s * NFEAT + tid] = fout[(int64_t)blockIdx.x * NBASIC + tid];
    if (tid == 0) { st.last_total[s] = st.total[s]; st.has_features[s] = 1; }
}

// ---- OpenSMILEeGeMAPSExtractor.reset, per stream ----
template <int NF>
__global__ __launch_bounds__(256) void es_reset_kernel(const uint8_t* __restrict__ mask, float* __restrict__ ring, int ring_len, EsState st,
                                                       float* __restrict__ features, float* __restrict__ slots, float* __restrict__ emotion,
                                                       uint8_t* __restrict__ updated) {
    using namespace es;
    constexpr int NFEAT = NF;
    const int s = blockIdx.y;
    if (mask && !mask[s]) return;
    float* r = ring + (int64_t)s * ring_len;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < ring_len; i += gridDim.x * 256) r[i] = 0.f;
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x;
    if (tid < NFEAT) { features[(int64_t)s * NFEAT + tid] = 0.f; slots[(int64_t)s * 2 * NFEAT + tid] = 0.f; slots[(int64_t)s * 2 * NFEAT + NFEAT + tid] = 0.f; }
    emotion[(int64_t)s * NEMO + tid] = 0.f;
    if (tid == 0) {
        st.write_pos[s] = 0; st.is_full[s] = 0; st.total[s] = 0; st.last_total[s] = -1; st.has_features[s] = 0; st.slots_filled[s] = 0;
        updated[s] = 0;
    }
}

template <int NF>
__global__ __launch_bounds__(256) void es_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt) {    // (256, 3 NF) -> (3 NF, 256)
    constexpr int NCAT = 3 * NF;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < es::NEMO * NCAT) { const int o = i / NCAT, k = i % NCAT; wt[k * es::NEMO + o] = w[i]; }
}

static int es_create(const char* fn, void** es_out, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates,
                     bool basic, bool long_windows = false, int feature_set = 0) {
    using namespace es;
    if (!es_out) return fail(KM_ERR_INVALID_ARG, "%s: NULL argument", fn);
    *es_out = nullptr;
    if (!egm::set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "%s: feature set %d, 0 (eGeMAPS) or 1 (GeMAPS)", fn, feature_set);
    if (n_streams < 1 || n_streams > MAX_STREAMS) return fail(KM_ERR_INVALID_ARG, "%s: n_streams %lld, 1 .. %d", fn, (long long)n_streams, MAX_STREAMS);
    if (const int rc = emo_check_seconds(fn, context_window_s, update_interval_s)) return rc;
    if (max_updates < 1 || max_updates > n_streams)
        return fail(KM_ERR_INVALID_ARG, "%s: max_updates %lld, 1 .. n_streams (%lld)", fn, (long long)max_updates, (long long)n_streams);
    std::unique_ptr<EmotionStream> e(new (std::nothrow) EmotionStream());
    if (!e) return fail(KM_ERR_HIP, "%s: out of host memory", fn);
    if (const int rc = emo_timing(fn, context_window_s, update_interval_s, basic, e.get(), long_windows)) return rc;
    e->n = n_streams; e->max_updates = max_updates; e->basic = basic;
    e->feature_set = feature_set; e->nfeat = egm::set_width(feature_set);
    e->long_windows = long_windows && e->max_nf > MAXF;                         // up to 2048 frames it is the plain object
    if (e->long_windows)
        if (const int rc = egm_window_prepare()) return rc;
    if (const int rc = basic ? km_prosody_plan_create(&e->prosody) : km_egemaps_plan_create(&e->plan)) return rc;
    const int64_t n = n_streams, mu = max_updates, R = e->ring_len, nf = e->max_nf, NF = e->nfeat;
    auto layout = [&](char* base) {
        EmoCarver c{base};
        e->ring = c.take<float>(n * R);
        e->st.write_pos = c.take<int32_t>(n); e->st.is_full = c.take<int32_t>(n);
        e->st.total = c.take<int64_t>(n); e->st.last_total = c.take<int64_t>(n);
        e->st.has_features = c.take<int32_t>(n); e->st.slots_filled = c.take<int32_t>(n);
        e->features = c.take<float>(n * NF); e->slots = c.take<float>(n * 2 * NF);
        e->emotion = c.take<float>(n * NEMO); e->updated = c.take<uint8_t>(n);
        e->table = c.take<EgmSlot>(mu); e->scale = c.take<float>(mu);
        e->rec = c.take<float>(mu * nf * (basic ? BASIC_REC : REC)); e->fout = c.take<float>(mu * (basic ? NBASIC : NF));
        e->wt = c.take<float>(3 * NF * NEMO); e->bias = c.take<float>(NEMO);
        return c.at;
    };
    const int64_t bytes = layout(nullptr);
    if (int rc = e->blob.alloc(bytes, fn)) return rc;
    HIP_TRY(hipMemset(e->blob, 0, (size_t)bytes));
    layout(e->blob);
    HIP_TRY(hipMemset(e->st.last_total, 0xff, (size_t)(n * 8)));       // last_total = -1
    *es_out = e.release();
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" {

int km_emotion_stream_create(void** es_out, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates) {
    return es_create("km_emotion_stream_create", es_out, n_streams, context_window_s, update_interval_s, max_updates, false);
}

int km_emotion_stream_create_long(void** es_out, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates) {
    return es_create("km_emotion_stream_create_long", es_out, n_streams, context_window_s, update_interval_s, max_updates, false, true);
}

int km_emotion_stream_create_basic(void** es_out, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates) {
    return es_create("km_emotion_stream_create", es_out, n_streams, context_window_s, update_interval_s, max_updates, true);   // the name both say
}

int km_emotion_stream_create_set(void** es_out, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates,
                                 int32_t feature_set, int32_t long_windows) {
    return es_create("km_emotion_stream_create_set", es_out, n_streams, context_window_s, update_interval_s, max_updates, false, long_windows != 0,
                     feature_set);
}

int km_emotion_stream_feature_width(void* es) {
    if (!es) return 0;
    const EmotionStream* e = static_cast<EmotionStream*>(es);
    return e->basic ? es::NBASIC : e->nfeat;
}

int km_emotion_stream_destroy(void* es) {
    if (!es) return KM_OK;
    delete static_cast<EmotionStream*>(es);
    return KM_OK;
}

int km_emotion_stream_set_compression(void* es, const float* w_dev, const float* b_dev, void* stream) {
    if (!es || !w_dev || !b_dev) return fail(KM_ERR_INVALID_ARG, "km_emotion_stream_set_compression: NULL argument");
    EmotionStream* e = static_cast<EmotionStream*>(es);
    if (e->basic) return fail(KM_ERR_INVALID_ARG, "km_emotion_stream_set_compression: the basic back end has no compression layer");
    hipStream_t st = (hipStream_t)stream;
    const auto transpose = e->nfeat == egm::NFEAT_GEMAPS ? es_transpose_kernel<egm::NFEAT_GEMAPS> : es_transpose_kernel<es::NFEAT>;
    hipLaunchKernelGGL(transpose, dim3((unsigned)((es::NEMO * 3 * e->nfeat + 255) / 256)), dim3(256), 0, st, w_dev, e->wt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(e->bias, b_dev, es::NEMO * sizeof(float), hipMemcpyDeviceToDevice, st));
    e->has_compression = true;
    return KM_OK;
}

int km_emotion_stream_push(void* es, const float* samples_dev, int64_t n_per_stream, const int32_t* counts_dev, void* stream) {
    if (!es || !samples_dev) return fail(KM_ERR_INVALID_ARG, "km_emotion_stream_push: NULL argument");
    EmotionStream* e = static_cast<EmotionStream*>(es);
    if (n_per_stream < 1 || n_per_stream > e->ring_len)
        return fail(KM_ERR_INVALID_ARG, "km_emotion_stream_push: %lld samples per stream, 1 .. %d (the ring)", (long long)n_per_stream, e->ring_len);
    hipStream_t st = (hipStream_t)stream;
    const int m = (int)n_per_stream;
    hipLaunchKernelGGL(es_append_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)e->n), dim3(256), 0, st, samples_dev, m, counts_dev, e->ring,
                       e->ring_len, (const int32_t*)e->st.write_pos);
    hipLaunchKernelGGL(es_advance_kernel, dim3((unsigned)((e->n + 255) / 256)), dim3(256), 0, st, (int)e->n, m, counts_dev, e->ring_len, e->st);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_emotion_stream_update(void* es, float* emotion_dev, uint8_t* valid_dev, uint8_t* updated_dev, void* stream) {
    if (!es || !emotion_dev) return fail(KM_ERR_INVALID_ARG, "km_emotion_stream_update: NULL argument");
    EmotionStream* e = static_cast<EmotionStream*>(es);
    if (!e->basic && !e->has_compression) return fail(KM_ERR_NOT_READY, "km_emotion_stream_update: km_emotion_stream_set_compression first");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(es_select_kernel, dim3(1), dim3(es::SEL_THREADS), 0, st, (int)e->n, (int)e->max_updates, e->ring_len, e->window_len,
                       e->update_samples, e->min_samples, e->st, e->table, e->updated);
    HIP_TRY(hipGetLastError());
    if (e->basic) {
        if (const int rc = prosody_ragged(e->prosody, e->ring, e->ring_len, e->table, (int)e->max_updates, e->max_nf, e->rec, e->fout, st)) return rc;
        hipLaunchKernelGGL(es_basic_epilogue_kernel, dim3((unsigned)e->max_updates), dim3(64), 0, st, (const EgmSlot*)e->table, (const float*)e->fout,
                           e->st, e->features);
        hipLaunchKernelGGL((es_output_kernel<es::NBASIC, es::NFEAT>), dim3((unsigned)((e->n * es::NBASIC + 255) / 256)), dim3(256), 0, st, (int)e->n,
                           (const float*)e->features, (const int32_t*)e->st.has_features, (const uint8_t*)e->updated, emotion_dev, valid_dev, updated_dev);
        HIP_TRY(hipGetLastError());
        return KM_OK;
    }
    if (const int rc = egm_ragged_functionals(e->plan, e->ring, e->ring_len, e->table, (int)e->max_updates, e->max_nf, e->scale, e->rec, e->fout, st,
                                              e->long_windows, e->feature_set))
        return rc;
    const auto epilogue = e->nfeat == egm::NFEAT_GEMAPS ? es_epilogue_kernel<egm::NFEAT_GEMAPS> : es_epilogue_kernel<es::NFEAT>;
    hipLaunchKernelGGL(epilogue, dim3((unsigned)e->max_updates), dim3(256), 0, st, (const EgmSlot*)e->table, (const float*)e->fout, e->st,
                       e->features, e->slots, (const float*)e->wt, (const float*)e->bias, e->emotion);
    hipLaunchKernelGGL((es_output_kernel<es::NEMO, es::NEMO>), dim3((unsigned)((e->n * es::NEMO + 255) / 256)), dim3(256), 0, st, (int)e->n, (const float*)e->emotion,
                       (const int32_t*)e->st.has_features, (const uint8_t*)e->updated, emotion_dev, valid_dev, updated_dev);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_emotion_stream_reset_streams(void* es, const uint8_t* mask_dev, void* stream) {
    if (!es) return fail(KM_ERR_INVALID_ARG, "km_emotion_stream_reset_streams: NULL argument");
    EmotionStream* e = static_cast<EmotionStream*>(es);
    const int bx = (e->ring_len + 256 * 8 - 1) / (256 * 8);
    const auto reset = e->nfeat == egm::NFEAT_GEMAPS ? es_reset_kernel<egm::NFEAT_GEMAPS> : es_reset_kernel<es::NFEAT>;
    hipLaunchKernelGGL(reset, dim3((unsigned)(bx < 256 ? bx : 256), (unsigned)e->n), dim3(256), 0, (hipStream_t)stream, mask_dev, e->ring,
                       e->ring_len, e->st, e->features, e->slots, e->emotion, e->updated);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_emotion_stream_features(void* es, float* features_dev, float* slots_dev, void* stream) {
    if (!es || !features_dev) return fail(KM_ERR_INVALID_ARG, "km_emotion_stream_features: NULL argument");
    EmotionStream* e = static_cast<EmotionStream*>(es);
    if (e->basic) {
        if (slots_dev) return fail(KM_ERR_INVALID_ARG, "km_emotion_stream_features: the basic back end has no window slots");
        hipLaunchKernelGGL((es_output_kernel<es::NBASIC, es::NFEAT>), dim3((unsigned)((e->n * es::NBASIC + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)e->n,
                           (const float*)e->features, (const int32_t*)e->st.has_features, (const uint8_t*)e->updated, features_dev,
                           (uint8_t*)nullptr, (uint8_t*)nullptr);
        HIP_TRY(hipGetLastError());
        return KM_OK;
    }
    HIP_TRY(hipMemcpyAsync(features_dev, e->features, (size_t)e->n * e->nfeat * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (slots_dev)
        HIP_TRY(hipMemcpyAsync(slots_dev, e->slots, (size_t)e->n * 2 * e->nfeat * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return KM_OK;
}

}  // extern "C"
