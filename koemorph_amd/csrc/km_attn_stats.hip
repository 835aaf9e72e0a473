// km_attn_stats.hip -- what the attention visualiser reduces the mel stream's attention maps to, accumulated on gfx950.
//
// Replaces the reductions under AttentionVisualizer (src/visualization/attention_viz.py: the mean map of :96-98 and the mass per
// frequency band of :329-331) for maps that never leave the GPU: (rows, Q, K) float32 maps -- a tile of km_sequence_forward_attn,
// 8 960 B per window at 28 x 80 -- are folded into a float64 / integer state in device memory by km_attn_stats_update, and
// km_attn_stats_compute turns the state into KM_ATTN_STATS_COUNT(Q, K) float64 values, also in device memory.  Nothing here
// allocates, synchronises or reads back outside create and destroy, so reset / update / compute can be captured in a graph.
//
// State and partial records, 8-byte slots, in the order of km_attn_stats_compute's output:
//   rows              maps seen (state only)
//   sum[q][k]         float64 sum of A over the maps                       -> mean map
//   ent[q]            float64 sum over maps of -sum_k A ln A, each term from the float32 entry in float64, 0 for A = 0
//   peak[q][k]        integer: maps whose largest entry of query q is key k, ties to the lowest k (np.argmax)
//
// REDUCTION ORDER (fixed; no atomics; the same rows in the same calls with the same max_rows_per_launch give the same bits):
//   attn_stats_partial_kernel   one workgroup per CHUNK_ROWS consecutive maps.  Every (q, k) sum is a column reduction over maps, so
//                               a lane owns ONE float4 of ONE query (K / 4 lanes per query, 64 / (K / 4) queries side by side in
//                               a wave: 20 lanes x 3 queries at K = 80, 4 lanes idle) and walks the chunk's maps with its four
//                               sums, its part of the entropy and its four peak counts in registers; a wave's loads of one map
//                               are one contiguous run (960 B).  Per map the query's argmax is a shuffle tree over its K / 4
//                               lanes -- the lower lane wins a tie, as the lower component does inside a float4 -- and the winner
//                               is shuffled back to the lane that counts it.  The entropy parts of a query's lanes are added by
//                               the same tree once, after the last map.  Every slot of the record has exactly one owner in the
//                               workgroup: no LDS, no barrier, plain stores.
//   attn_stats_fold_kernel      one thread per slot adds the launch's records to the state in workgroup order.
//   attn_stats_compute_kernel   one thread per output value.
// An update of more than max_rows_per_launch maps is cut into pieces (one partial + one fold launch each); the workspace holds the
// records of one piece.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_context.h"

namespace km {

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                                                                        \
            (void)hipGetLastError(); /* the runtime keeps a failed call as its last error: do not leave it to the next launch check */ \
            return fail(KM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));                                                           \
        }                                                                                                                              \
    } while (0)

namespace ast {
constexpr int CHUNK_ROWS = 16;                     // maps per workgroup: 1 380 windows (4 clips of 20 s) are 87 workgroups
constexpr int UNROLL = 4;                          // maps whose loads a lane keeps in flight
constexpr int MAX_WAVES = 16;                      // waves per workgroup: one per group of queries, the rest by a loop
constexpr int MAX_KEYS = 256;                      // K / 4 lanes of one wave hold a query's row
constexpr int64_t DEFAULT_ROWS_PER_LAUNCH = 4096;  // 256 records of 36 KB at 28 x 80
constexpr int64_t MAX_ROWS_PER_LAUNCH = (int64_t)1 << 20;
constexpr int FOLD_THREADS = 256, FOLD_BATCH = 8;
}  // namespace ast

union AstSlot { double d; long long i; };

struct AttnStatsAcc {
    AstSlot* state = nullptr;      // device: 1 + rec slots
    AstSlot* work = nullptr;       // device: max_records partial records
    int Q = 0, K = 0;
    int lanes_per_q = 0, q_per_wave = 0, q_groups = 0, waves = 0;
    int rec = 0;                   // slots per record: Q K + Q + Q K
    int64_t rows_per_launch = 0;
};

struct AstShape { int Q, K, lanes_per_q, q_per_wave, q_groups, rec; };

// -a ln a of a float32 entry, in float64; exactly 0 for a = 0 (and for anything that is not a positive number)
__device__ inline double ent_term(float a) { return a > 0.f ? -(double)a * log((double)a) : 0.0; }

__global__ void __launch_bounds__(ast::MAX_WAVES * 64)
attn_stats_partial_kernel(const float* __restrict__ attn, int64_t r0, int64_t r1, AstShape s, AstSlot* __restrict__ work) {
    using namespace ast;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int g = lane / s.lanes_per_q, l = lane - g * s.lanes_per_q;      // query of the wave's group, float4 slot of its row
    const int base = g * s.lanes_per_q;                                     // first lane of the query
    const int64_t c0 = r0 + (int64_t)blockIdx.x * CHUNK_ROWS;
    const int64_t c1 = c0 + CHUNK_ROWS < r1 ? c0 + CHUNK_ROWS : r1;
    const int64_t map_floats = (int64_t)s.Q * s.K;
    AstSlot* rec = work + (int64_t)blockIdx.x * s.rec;
    int steps = 0;                                                          // levels of the tree over lanes_per_q lanes
    while ((1 << steps) < s.lanes_per_q) ++steps;

    for (int t = wave; t < s.q_groups; t += n_waves) {                      // wave-uniform
        const int q = t * s.q_per_wave + g;
        const bool active = g < s.q_per_wave && q < s.Q;
        const float* col = attn + (active ? (int64_t)q * s.K + 4 * l : 0);
        double sum[4] = {0.0, 0.0, 0.0, 0.0}, ent = 0.0;
        unsigned cnt[4] = {0, 0, 0, 0};
        for (int64_t rb = c0; rb < c1; rb += UNROLL) {                      // wave-uniform
            float4 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (active && rb + u < c1) v[u] = *reinterpret_cast<const float4*>(col + (rb + u) * map_floats);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if (rb + u >= c1) break;                                    // wave-uniform
                const float4 a = v[u];
                sum[0] += (double)a.x; sum[1] += (double)a.y; sum[2] += (double)a.z; sum[3] += (double)a.w;
                ent += ((ent_term(a.x) + ent_term(a.y)) + ent_term(a.z)) + ent_term(a.w);
                // argmax of the query's row: first inside the float4, then over the query's lanes; strictly greater moves it
                float m = a.x; int mi = 4 * l;
                if (a.y > m) { m = a.y; mi = 4 * l + 1; }
                if (a.z > m) { m = a.z; mi = 4 * l + 2; }
                if (a.w > m) { m = a.w; mi = 4 * l + 3; }
                for (int st = 0; st < steps; ++st) {
                    const int off = 1 << st;
                    // lane l takes lane l + off of ITS query (lanes l = 0 mod 2 off hold the partial results; the others' are unused)
                    const int src = (l + off < s.lanes_per_q && active) ? lane + off : lane;
                    const float om = __shfl(m, src, 64);
                    const int oi = __shfl(mi, src, 64);
                    if (om > m) { m = om; mi = oi; }
                }
                const int win = __shfl(mi, active ? base : lane, 64);       // lane 0 of the query holds the row's argmax
                if (active && (win >> 2) == l) cnt[win & 3] += 1;
            }
        }
        // the entropy parts of the query's lanes, by the same tree
        for (int st = 0; st < steps; ++st) {
            const int off = 1 << st;
            const int src = (l + off < s.lanes_per_q && active) ? lane + off : lane;
            const double o = __shfl(ent, src, 64);
            if (src != lane) ent += o;
        }
        if (active) {
            const int e = q * s.K + 4 * l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                rec[e + j].d = sum[j];
                rec[s.Q * s.K + s.Q + e + j].i = (long long)cnt[j];
            }
            if (l == 0) rec[s.Q * s.K + q].d = ent;
        }
    }
}

// state[1 + e] += the launch's records, in workgroup order; slot 0 is the row count
__global__ void __launch_bounds__(ast::FOLD_THREADS)
attn_stats_fold_kernel(AstSlot* __restrict__ state, const AstSlot* __restrict__ work, int n_rec, int rec, int first_int, int64_t rows) {
    using namespace ast;
    const int e = blockIdx.x * FOLD_THREADS + threadIdx.x;
    if (e == 0) state[0].i += rows;
    if (e >= rec) return;
    AstSlot acc = state[1 + e];
    const bool is_int = e >= first_int;
    int b = 0;
    for (; b + FOLD_BATCH <= n_rec; b += FOLD_BATCH) {          // the loads are independent, only the additions are a chain
        AstSlot v[FOLD_BATCH];
#pragma unroll
        for (int j = 0; j < FOLD_BATCH; ++j) v[j] = work[(int64_t)(b + j) * rec + e];
#pragma unroll
        for (int j = 0; j < FOLD_BATCH; ++j) { if (is_int) acc.i += v[j].i; else acc.d += v[j].d; }
    }
    for (; b < n_rec; ++b) {
        const AstSlot v = work[(int64_t)b * rec + e];
        if (is_int) acc.i += v.i; else acc.d += v.d;
    }
    state[1 + e] = acc;
}

// The empty state is all zero bits.  A kernel rather than a memset node, as in km_metrics.hip.
__global__ void __launch_bounds__(256) attn_stats_reset_kernel(AstSlot* __restrict__ state, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) state[i].i = 0;
}

__global__ void __launch_bounds__(256) attn_stats_compute_kernel(const AstSlot* __restrict__ state, double* __restrict__ out, int n,
                                                                 int first_int) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long rows = state[0].i;
    double v = 0.0;
    if (rows > 0) {
        if (i == 0) v = (double)rows;
        else if (i - 1 >= first_int) v = (double)state[i].i;     // counts stay below 2^53
        else v = state[i].d / (double)rows;
    }
    out[i] = v;
}

}  // namespace km

using namespace km;

extern "C" {

int km_attn_stats_create(void** acc_out, int32_t n_queries, int32_t n_keys, int64_t max_rows_per_launch) {
    using namespace ast;
    if (!acc_out) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_create: NULL argument");
    if (n_queries < 1 || n_queries > 4096 || n_keys < 4 || n_keys % 4 != 0 || n_keys > MAX_KEYS)
        return fail(KM_ERR_INVALID_ARG, "km_attn_stats_create: %d queries x %d keys (keys: a multiple of 4 up to %d)", n_queries, n_keys, MAX_KEYS);
    if (max_rows_per_launch < 0 || max_rows_per_launch > MAX_ROWS_PER_LAUNCH)
        return fail(KM_ERR_INVALID_ARG, "km_attn_stats_create: max_rows_per_launch %lld (0 .. %lld)", (long long)max_rows_per_launch,
                    (long long)MAX_ROWS_PER_LAUNCH);
    AttnStatsAcc* a = new AttnStatsAcc();
    a->Q = n_queries; a->K = n_keys;
    a->lanes_per_q = n_keys / 4;
    a->q_per_wave = 64 / a->lanes_per_q;
    a->q_groups = (n_queries + a->q_per_wave - 1) / a->q_per_wave;
    a->waves = a->q_groups < MAX_WAVES ? a->q_groups : MAX_WAVES;
    a->rec = 2 * n_queries * n_keys + n_queries;
    a->rows_per_launch = max_rows_per_launch > 0 ? max_rows_per_launch : DEFAULT_ROWS_PER_LAUNCH;
    const int64_t max_rec = (a->rows_per_launch + CHUNK_ROWS - 1) / CHUNK_ROWS;
    const size_t state_bytes = (size_t)(1 + a->rec) * sizeof(AstSlot);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&a->state), state_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&a->work), (size_t)max_rec * a->rec * sizeof(AstSlot));
    if (e == hipSuccess) e = hipMemset(a->state, 0, state_bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // the cleared state is visible to whichever stream updates first
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (a->state) (void)hipFree(a->state);
        if (a->work) (void)hipFree(a->work);
        delete a;
        return fail(KM_ERR_HIP, "km_attn_stats_create: %s", hipGetErrorString(e));
    }
    *acc_out = a;
    return KM_OK;
}

int km_attn_stats_destroy(void* acc) {
    if (!acc) return KM_OK;
    AttnStatsAcc* a = static_cast<AttnStatsAcc*>(acc);
    if (a->state) (void)hipFree(a->state);
    if (a->work) (void)hipFree(a->work);
    delete a;
    return KM_OK;
}

int km_attn_stats_shape(void* acc, int32_t* n_queries, int32_t* n_keys) {
    if (!acc) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_shape: NULL accumulator");
    const AttnStatsAcc* a = static_cast<const AttnStatsAcc*>(acc);
    if (n_queries) *n_queries = a->Q;
    if (n_keys) *n_keys = a->K;
    return KM_OK;
}

int km_attn_stats_reset(void* acc, void* stream) {
    if (!acc) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_reset: NULL accumulator");
    AttnStatsAcc* a = static_cast<AttnStatsAcc*>(acc);
    const int n = 1 + a->rec;
    hipLaunchKernelGGL(attn_stats_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->state, n);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_attn_stats_update(void* acc, const float* attn_dev, int64_t rows, void* stream) {
    using namespace ast;
    if (!acc || rows < 0) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_update: bad argument");
    if (rows == 0) return KM_OK;
    if (!attn_dev) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_update: NULL maps");
    if ((uintptr_t)attn_dev & 15) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_update: maps must be 16-byte aligned");
    AttnStatsAcc* a = static_cast<AttnStatsAcc*>(acc);
    const AstShape s{a->Q, a->K, a->lanes_per_q, a->q_per_wave, a->q_groups, a->rec};
    const int first_int = a->Q * a->K + a->Q;
    hipStream_t st = (hipStream_t)stream;
    for (int64_t r0 = 0; r0 < rows; r0 += a->rows_per_launch) {
        const int64_t r1 = r0 + a->rows_per_launch < rows ? r0 + a->rows_per_launch : rows;
        const int n_rec = (int)((r1 - r0 + CHUNK_ROWS - 1) / CHUNK_ROWS);
        hipLaunchKernelGGL(attn_stats_partial_kernel, dim3((unsigned)n_rec), dim3((unsigned)(64 * a->waves)), 0, st, attn_dev, r0, r1, s, a->work);
        hipLaunchKernelGGL(attn_stats_fold_kernel, dim3((unsigned)((a->rec + FOLD_THREADS - 1) / FOLD_THREADS)), dim3(FOLD_THREADS), 0, st,
                           a->state, a->work, n_rec, a->rec, first_int, r1 - r0);
        HIP_TRY(hipGetLastError());
    }
    return KM_OK;
}

int km_attn_stats_compute(void* acc, double* out_dev, void* stream) {
    if (!acc || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_compute: NULL argument");
    AttnStatsAcc* a = static_cast<AttnStatsAcc*>(acc);
    const int n = 1 + a->rec;
    hipLaunchKernelGGL(attn_stats_compute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->state, out_dev, n,
                       a->Q * a->K + a->Q);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // extern "C"
