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
//
// MASKED UPDATE (km_attn_stats_update_masked): the rows with a non-zero mask byte, in index order, as if they had been compacted
// into a dense array first -- the state afterwards has the bits km_attn_stats_update leaves on that array.  How many rows are
// selected is known only on the device, so per piece p of max_rows_per_launch RANKS (the pieces the dense update would cut)
//   attn_stats_compact_kernel   one workgroup walks the mask with a running count (ballot + one LDS word per wave) and writes the row
//                               of every selected rank in [p R, (p + 1) R) into the index table, and the piece's row count
//   attn_stats_partial_kernel   the INDIRECT instantiation: chunk c of the piece reads its maps through the table; the grid is sized
//                               by the rows OFFERED, and a workgroup past the count writes an all-zero record
//   attn_stats_fold_kernel      adds the records and the device-side count.  state + (+0.0) == state for every state the fold can
//                               hold (it starts at +0.0 and never becomes -0.0), so the zero records change no bit.
//
// PER-STREAM STATE (km_attn_stats_streams_*): one independent state per stream and no reduction across rows at all: a workgroup
// per stream runs the partial kernel's body over that stream's ONE map and adds the result to the stream's state, which is what
// partial + fold do for rows = 1.
#include <hip/hip_runtime.h>

#include <cstdint>

#include <memory>

#include "km_context.h"

namespace km {


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
    DevBuf<AstSlot> state;         // 1 + rec slots
    DevBuf<AstSlot> work;          // max_records partial records
    int Q = 0, K = 0;
    int lanes_per_q = 0, q_per_wave = 0, q_groups = 0, waves = 0;
    int rec = 0;                   // slots per record: Q K + Q + Q K
    int64_t rows_per_launch = 0;
    DevBuf<int> table;             // 4 ints holding the piece's row count (a long long) + rows_per_launch row indices
};

struct AttnStatsStreams {          // km_attn_stats_streams_*: n_streams states of 1 + rec slots, nothing else
    DevBuf<AstSlot> state;
    int S = 0, Q = 0, K = 0;
    int lanes_per_q = 0, q_per_wave = 0, q_groups = 0, waves = 0, rec = 0;
};

struct AstShape { int Q, K, lanes_per_q, q_per_wave, q_groups, rec; };

// -a ln a of a float32 entry, in float64; exactly 0 for a = 0 (and for anything that is not a positive number)
__device__ inline double ent_term(float a) { return a > 0.f ? -(double)a * log((double)a) : 0.0; }

// The sums of one group of queries over maps c0 .. c1 - 1 (INDIRECT: over rows table[c0] .. table[c1 - 1]): what a lane of
// attn_stats_partial_kernel accumulates -- its four column sums, the query's entropy (in the query's lane 0 after the tree) and
// its four peak counts.  One body for every kernel of this file, so the addition order, the entropy tree and the tie rule are one code.
template <bool INDIRECT>
__device__ __forceinline__ void ast_group_sums(const float* __restrict__ col, const int* __restrict__ table, int64_t c0, int64_t c1,
                                               int64_t map_floats, const AstShape& s, bool active, int l, int lane, int base, int steps,
                                               double (&sum)[4], double& ent, unsigned (&cnt)[4]) {
    using namespace ast;
    for (int64_t rb = c0; rb < c1; rb += UNROLL) {                      // wave-uniform
        float4 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (active && rb + u < c1) {
                const int64_t row = INDIRECT ? (int64_t)table[rb + u] : rb + u;
                v[u] = *reinterpret_cast<const float4*>(col + row * map_floats);
            }
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
}

// INDIRECT: chunk blockIdx.x of the piece's selected rows, found through `table`; *count of them exist (r0 / r1 are unused)
template <bool INDIRECT>
__global__ void __launch_bounds__(ast::MAX_WAVES * 64)
attn_stats_partial_kernel(const float* __restrict__ attn, int64_t r0, int64_t r1, AstShape s, AstSlot* __restrict__ work,
                          const int* __restrict__ table, const long long* __restrict__ count) {
    using namespace ast;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int g = lane / s.lanes_per_q, l = lane - g * s.lanes_per_q;      // query of the wave's group, float4 slot of its row
    const int base = g * s.lanes_per_q;                                     // first lane of the query
    if constexpr (INDIRECT) { r0 = 0; r1 = *count; }
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
        ast_group_sums<INDIRECT>(col, table, c0, c1, map_floats, s, active, l, lane, base, steps, sum, ent, cnt);
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

// table[j] = the row of rank lo + j among the rows with a non-zero mask byte, for the ranks in [lo, hi); *count = how many of those
// ranks exist.  One workgroup: the ranks are a prefix sum over the mask, carried from round to round in `before` (the same in
// every thread); the walk ends once the piece is full.  table holds hi - lo entries; those past *count keep what they held.
constexpr int AST_COMPACT_THREADS = 1024;
__global__ void __launch_bounds__(AST_COMPACT_THREADS)
attn_stats_compact_kernel(const unsigned char* __restrict__ mask, int64_t rows, int64_t lo, int64_t hi, int* __restrict__ table,
                          long long* __restrict__ count) {
    constexpr int NWAVE = AST_COMPACT_THREADS / 64;
    __shared__ int wave_sel[NWAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t before = 0;
    for (int64_t r0 = 0; r0 < rows && before < hi; r0 += AST_COMPACT_THREADS) {        // workgroup-uniform
        const int64_t r = r0 + tid;
        const bool sel = r < rows && mask[r] != 0;
        const unsigned long long b = __ballot(sel);
        if (lane == 0) wave_sel[wave] = __popcll(b);
        __syncthreads();
        int in_waves_before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) {
            const int v = wave_sel[w];
            if (w < wave) in_waves_before += v;
            total += v;
        }
        const int64_t rank = before + in_waves_before + __popcll(b & ((1ull << lane) - 1ull));
        if (sel && rank >= lo && rank < hi) table[rank - lo] = (int)r;
        before += total;
        __syncthreads();                                                                // wave_sel is rewritten by the next round
    }
    if (tid == 0) {
        const int64_t n = (before < hi ? before : hi) - lo;
        *count = n > 0 ? n : 0;
    }
}

// state[1 + e] += the launch's records, in workgroup order; slot 0 is the row count (DEV_ROWS: the count the compaction left)
template <bool DEV_ROWS>
__global__ void __launch_bounds__(ast::FOLD_THREADS)
attn_stats_fold_kernel(AstSlot* __restrict__ state, const AstSlot* __restrict__ work, int n_rec, int rec, int first_int, int64_t rows,
                       const long long* __restrict__ rows_dev) {
    using namespace ast;
    const int e = blockIdx.x * FOLD_THREADS + threadIdx.x;
    if (e == 0) state[0].i += DEV_ROWS ? (int64_t)*rows_dev : rows;
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

// blockIdx.y: the stream of a per-stream accumulator (one state of n slots and one output vector of n values each)
// the states of the streams with mask[s] != 0 (NULL: all) become empty
__global__ void __launch_bounds__(256) attn_stats_streams_reset_kernel(AstSlot* __restrict__ state, int n, const unsigned char* __restrict__ mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && (!mask || mask[blockIdx.y])) state[(int64_t)blockIdx.y * n + i].i = 0;
}

// Stream blockIdx.x, if its mask byte is set: the partial kernel's body over the stream's one map, added to the stream's own state
// by the lane that owns the slot -- bit for bit what attn_stats_partial_kernel + attn_stats_fold_kernel do for rows = 1.
__global__ void __launch_bounds__(ast::MAX_WAVES * 64)
attn_stats_streams_update_kernel(const float* __restrict__ attn, const unsigned char* __restrict__ mask, AstShape s, AstSlot* __restrict__ state) {
    const int b = (int)blockIdx.x;
    if (!mask[b]) return;                                                   // workgroup-uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int g = lane / s.lanes_per_q, l = lane - g * s.lanes_per_q;
    const int base = g * s.lanes_per_q;
    const int64_t map_floats = (int64_t)s.Q * s.K;
    AstSlot* st = state + (int64_t)b * (1 + s.rec) + 1;
    int steps = 0;
    while ((1 << steps) < s.lanes_per_q) ++steps;
    for (int t = wave; t < s.q_groups; t += n_waves) {                      // wave-uniform
        const int q = t * s.q_per_wave + g;
        const bool active = g < s.q_per_wave && q < s.Q;
        const float* col = attn + (active ? (int64_t)q * s.K + 4 * l : 0);
        double sum[4] = {0.0, 0.0, 0.0, 0.0}, ent = 0.0;
        unsigned cnt[4] = {0, 0, 0, 0};
        ast_group_sums<false>(col, nullptr, b, (int64_t)b + 1, map_floats, s, active, l, lane, base, steps, sum, ent, cnt);
        if (active) {
            const int e = q * s.K + 4 * l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                st[e + j].d += sum[j];
                st[s.Q * s.K + s.Q + e + j].i += (long long)cnt[j];
            }
            if (l == 0) st[s.Q * s.K + q].d += ent;
        }
    }
    if (threadIdx.x == 0) st[-1].i += 1;
}

__global__ void __launch_bounds__(256) attn_stats_compute_kernel(const AstSlot* __restrict__ state, double* __restrict__ out, int n,
                                                                 int first_int) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    state += (int64_t)blockIdx.y * n;
    out += (int64_t)blockIdx.y * n;
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
    auto a = std::make_unique<AttnStatsAcc>();
    a->Q = n_queries; a->K = n_keys;
    a->lanes_per_q = n_keys / 4;
    a->q_per_wave = 64 / a->lanes_per_q;
    a->q_groups = (n_queries + a->q_per_wave - 1) / a->q_per_wave;
    a->waves = a->q_groups < MAX_WAVES ? a->q_groups : MAX_WAVES;
    a->rec = 2 * n_queries * n_keys + n_queries;
    a->rows_per_launch = max_rows_per_launch > 0 ? max_rows_per_launch : DEFAULT_ROWS_PER_LAUNCH;
    const int64_t max_rec = (a->rows_per_launch + CHUNK_ROWS - 1) / CHUNK_ROWS;
    if (int rc = a->state.alloc(1 + a->rec, "km_attn_stats_create")) return rc;
    if (int rc = a->work.alloc(max_rec * a->rec, "km_attn_stats_create")) return rc;
    if (int rc = a->table.alloc(4 + a->rows_per_launch, "km_attn_stats_create")) return rc;
    HIP_TRY(hipMemset(a->state, 0, (size_t)a->state.bytes()));
    HIP_TRY(hipMemset(a->table, 0, (size_t)a->table.bytes()));
    HIP_TRY(hipStreamSynchronize(nullptr));   // the cleared state is visible to whichever stream updates first
    *acc_out = a.release();
    return KM_OK;
}

int km_attn_stats_destroy(void* acc) {
    if (!acc) return KM_OK;
    delete static_cast<AttnStatsAcc*>(acc);
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
        hipLaunchKernelGGL(attn_stats_partial_kernel<false>, dim3((unsigned)n_rec), dim3((unsigned)(64 * a->waves)), 0, st, attn_dev, r0, r1, s,
                           a->work, (const int*)nullptr, (const long long*)nullptr);
        hipLaunchKernelGGL(attn_stats_fold_kernel<false>, dim3((unsigned)((a->rec + FOLD_THREADS - 1) / FOLD_THREADS)), dim3(FOLD_THREADS), 0, st,
                           a->state, a->work, n_rec, a->rec, first_int, r1 - r0, (const long long*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    return KM_OK;
}

int km_attn_stats_update_masked(void* acc, const float* attn_dev, const uint8_t* mask_dev, int64_t rows, void* stream) {
    using namespace ast;
    // the argument checks come before the accumulator is looked at
    if (!acc || rows < 0 || rows > INT32_MAX) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_update_masked: bad argument");
    if (rows == 0) return KM_OK;
    if (!attn_dev || !mask_dev) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_update_masked: NULL maps or mask");
    if ((uintptr_t)attn_dev & 15) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_update_masked: maps must be 16-byte aligned");
    AttnStatsAcc* a = static_cast<AttnStatsAcc*>(acc);
    const AstShape s{a->Q, a->K, a->lanes_per_q, a->q_per_wave, a->q_groups, a->rec};
    const int first_int = a->Q * a->K + a->Q;
    hipStream_t st = (hipStream_t)stream;
    const long long* count = reinterpret_cast<const long long*>(a->table.p);
    int* table = a->table + 4;
    // piece p holds the selected rows of rank [lo, hi): at most `rows` rows are selected, so these are all the pieces the dense
    // update could cut, and a piece whose ranks do not exist adds records of zeros and a count of 0
    for (int64_t lo = 0; lo < rows; lo += a->rows_per_launch) {
        const int64_t hi = lo + a->rows_per_launch < rows ? lo + a->rows_per_launch : rows;
        const int n_rec = (int)((hi - lo + CHUNK_ROWS - 1) / CHUNK_ROWS);
        hipLaunchKernelGGL(attn_stats_compact_kernel, dim3(1), dim3(AST_COMPACT_THREADS), 0, st, mask_dev, rows, lo, hi, table,
                           reinterpret_cast<long long*>(a->table.p));
        hipLaunchKernelGGL(attn_stats_partial_kernel<true>, dim3((unsigned)n_rec), dim3((unsigned)(64 * a->waves)), 0, st, attn_dev, (int64_t)0,
                           (int64_t)0, s, a->work, (const int*)table, count);
        hipLaunchKernelGGL(attn_stats_fold_kernel<true>, dim3((unsigned)((a->rec + FOLD_THREADS - 1) / FOLD_THREADS)), dim3(FOLD_THREADS), 0, st,
                           a->state, a->work, n_rec, a->rec, first_int, (int64_t)0, count);
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

// ---- one independent state per stream ----
int km_attn_stats_streams_create(void** acc_out, int64_t n_streams, int32_t n_queries, int32_t n_keys) {
    using namespace ast;
    if (!acc_out) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_streams_create: NULL argument");
    if (n_streams < 1 || n_streams > 65535) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_streams_create: %lld streams (1 .. 65535)", (long long)n_streams);
    if (n_queries < 1 || n_queries > 4096 || n_keys < 4 || n_keys % 4 != 0 || n_keys > MAX_KEYS)
        return fail(KM_ERR_INVALID_ARG, "km_attn_stats_streams_create: %d queries x %d keys (keys: a multiple of 4 up to %d)", n_queries, n_keys,
                    MAX_KEYS);
    auto a = std::make_unique<AttnStatsStreams>();
    a->S = (int)n_streams; a->Q = n_queries; a->K = n_keys;
    a->lanes_per_q = n_keys / 4;
    a->q_per_wave = 64 / a->lanes_per_q;
    a->q_groups = (n_queries + a->q_per_wave - 1) / a->q_per_wave;
    a->waves = a->q_groups < MAX_WAVES ? a->q_groups : MAX_WAVES;
    a->rec = 2 * n_queries * n_keys + n_queries;
    if (int rc = a->state.alloc(n_streams * (1 + a->rec), "km_attn_stats_streams_create")) return rc;
    HIP_TRY(hipMemset(a->state, 0, (size_t)a->state.bytes()));
    HIP_TRY(hipStreamSynchronize(nullptr));
    *acc_out = a.release();
    return KM_OK;
}

int km_attn_stats_streams_destroy(void* acc) {
    if (!acc) return KM_OK;
    delete static_cast<AttnStatsStreams*>(acc);
    return KM_OK;
}

int km_attn_stats_streams_update(void* acc, const float* attn_dev, const uint8_t* mask_dev, void* stream) {
    // the argument checks come before the accumulator is looked at
    if (!acc || !attn_dev || !mask_dev) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_streams_update: NULL argument");
    if ((uintptr_t)attn_dev & 15) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_streams_update: maps must be 16-byte aligned");
    AttnStatsStreams* a = static_cast<AttnStatsStreams*>(acc);
    const AstShape s{a->Q, a->K, a->lanes_per_q, a->q_per_wave, a->q_groups, a->rec};
    hipLaunchKernelGGL(attn_stats_streams_update_kernel, dim3((unsigned)a->S), dim3((unsigned)(64 * a->waves)), 0, (hipStream_t)stream, attn_dev,
                       mask_dev, s, a->state);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_attn_stats_streams_reset(void* acc, const uint8_t* mask_dev, void* stream) {
    if (!acc) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_streams_reset: NULL accumulator");
    AttnStatsStreams* a = static_cast<AttnStatsStreams*>(acc);
    const int n = 1 + a->rec;
    hipLaunchKernelGGL(attn_stats_streams_reset_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)a->S), dim3(256), 0, (hipStream_t)stream,
                       a->state, n, mask_dev);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_attn_stats_streams_compute(void* acc, double* out_dev, void* stream) {
    if (!acc || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_attn_stats_streams_compute: NULL argument");
    AttnStatsStreams* a = static_cast<AttnStatsStreams*>(acc);
    const int n = 1 + a->rec;
    hipLaunchKernelGGL(attn_stats_compute_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)a->S), dim3(256), 0, (hipStream_t)stream, a->state,
                       out_dev, n, a->Q * a->K + a->Q);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // extern "C"
