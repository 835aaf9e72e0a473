// km_metrics.hip -- streaming evaluation metrics on gfx950 (losses.py row; section 5, metrics).
//
// Replaces BlendshapeMetrics (src/model/losses.py:421-521) and compute_lip_sync_metrics (:524-583).  The reference moves
// every batch to the host, concatenates the epoch and reduces it with torch on the CPU; here the epoch never leaves the
// GPU.  An accumulator in device memory is folded forward by km_metrics_update, (N, 52) rows at a time, and
// km_metrics_compute turns it into KM_METRICS_COUNT float32 values, also in device memory.  Neither synchronises,
// allocates or reads back, so both can be captured in a graph.
//
// State (MetricsState), float64 or integer throughout, per column c of the 52:
//   n                         rows seen
//   shift_p, shift_t          the column's value in the FIRST row ever seen
//   S_P, S_T                  sum (p - shift_p), sum (t - shift_t)
//   S_PP, S_TT, S_PT          sum (p - shift_p)^2, sum (t - shift_t)^2, sum (p - shift_p)(t - shift_t)
//   S_ABS, S_SQ               sum |p - t|, sum (p - t)^2
//   S_DD, S_DP, S_DT          sum |dp - dt|, sum |dp|, sum |dt| over consecutive rows (dp = p[r] - p[r-1])
//   C_P, C_T, C_PT            rows with p > thr, t > thr, both; thr = 0.1f compared in float32 as torch compares
//   last_p, last_t            the last row of the previous update: torch.diff runs over the concatenation of all batches
//                             (losses.py:493-494), so the difference across a batch boundary counts
// and for three per-row scalars -- a_p, a_t = sum of columns 12..31 of pred / target (losses.py:543-553), e = the
// caller's audio energy -- the same shifted moments: Q_AP .. Q_APT over all rows, Q_E .. Q_AAE over the rows that came
// with an energy (Q_NE of them).  sum |p - t| over the mouth columns is S_ABS of columns 12..31.
//
// CENTRED SUMS, BY SHIFT: the reference gates each correlation on std() > 1e-6 (losses.py:479); a column at 0.7 +- 3e-6
// has mean^2 / var = 5e10, which leaves raw float64 moments five digits.  Every value is shifted by the column's first
// value before it is squared; the difference of two float32 values is exact in float64, a constant column sums to exactly
// zero, and all partial sums share one shift so merging them is plain addition (no Chan-style mean updates needed).
//
// REDUCTION ORDER (fixed; no floating-point atomics; two runs on the same data give the same bits):
//   metrics_partial_kernel   a wave reads 4 rows at a time as 52 contiguous float4 (lane = 13 * row + float4 slot, lanes
//                            52..63 idle), so a lane owns 4 columns across rows and keeps their sums in registers; rows are
//                            strided over the waves of the grid.  At the end the four row groups of a wave are added in
//                            group order (shuffles), the waves of a workgroup in wave order (LDS), and the workgroup
//                            writes ONE partial record to the workspace.
//   metrics_fold_kernel      a single workgroup adds the partial records to the running state in workgroup order, then
//                            stores the shifts (first update only), the carried last row and the row count.
//   metrics_compute_kernel   one wave: lane c finalises column c in float64, fixed xor-tree reductions across lanes, one
//                            rounding to float32 per result.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <memory>

#include "km_context.h"

namespace km {


namespace met {
constexpr int NC = 52, NQ = 13;                       // columns; float4 slots per row
constexpr int MOUTH_Q0 = 3, MOUTH_Q1 = 8;             // columns 12..31 are float4 slots 3..7 (losses.py:543)
enum Col { S_P = 0, S_T, S_PP, S_TT, S_PT, S_ABS, S_SQ, S_DD, S_DP, S_DT, NCF, C_P = NCF, C_T, C_PT, NCS };   // 10 float64 + 3 int64
enum Sca { Q_AP = 0, Q_AT, Q_APP, Q_ATT, Q_APT, Q_E, Q_EE, Q_AE, Q_A, Q_AA, NSF, Q_NE = NSF, NSS };            // 10 float64 + 1 int64
constexpr int REC_COLS = NC * NCS;                    // 676
constexpr int REC = REC_COLS + NSS;                   // 687 eight-byte slots per record
constexpr int WAVES = 8, THREADS = WAVES * 64, ROWS_PER_WAVE = 4;
constexpr int FOLD_THREADS = 704;                     // >= REC, 11 waves
constexpr int FOLD_BATCH = 32;                        // partial records the fold kernel keeps in flight per thread
constexpr int DEFAULT_WGS = 256, MAX_WGS = 4096;      // one 8-wave workgroup per CU: 196 VGPRs allow two waves per SIMD
constexpr int64_t MAX_ROWS_PER_LAUNCH = (int64_t)1 << 24;   // the per-lane counters are 32-bit
constexpr float THRESHOLD = 0.1f;                     // float32(0.1): `tensor_f32 > 0.1` in torch (losses.py:501-503)

__host__ __device__ inline bool slot_is_int(int e) { return e < REC_COLS ? (e % NCS) >= NCF : e == REC_COLS + Q_NE; }
}  // namespace met

union Slot { double d; long long i; };

struct MetricsState {
    Slot sums[met::REC];
    long long n;
    double shift_p[met::NC], shift_t[met::NC], shift_ap, shift_at, shift_e;
    alignas(16) float last_p[met::NC];                 // read back as float4: 16-byte aligned, 208 B each
    alignas(16) float last_t[met::NC];
};

struct MetricsAcc {
    DevBuf<MetricsState> state;
    DevBuf<Slot> work;                 // wgs partial records
    int wgs = met::DEFAULT_WGS;
};

// The sum of the four values of a float4 slot, then of the five mouth slots, always in this order: the shift of the
// mouth activity (its value in the first row) must cancel that row's own sum exactly.
__device__ inline double quad_sum(const float4 v) { return (((double)v.x + (double)v.y) + (double)v.z) + (double)v.w; }

__device__ inline double mouth_sum_row(const float* __restrict__ row) {
    double a = 0.0;
    for (int q = met::MOUTH_Q0; q < met::MOUTH_Q1; ++q) {
        const double s = quad_sum(*reinterpret_cast<const float4*>(row + 4 * q));
        a = q == met::MOUTH_Q0 ? s : a + s;
    }
    return a;
}

__device__ inline double shfl_d(double v, int src) { return __shfl(v, src, 64); }

__device__ inline void fold_elem(double (&a)[met::NCF], unsigned (&c)[3], float p, float t, float pp, float tp, double sp, double st,
                                 bool has_prev) {
    using namespace met;
    const double dp = (double)p - sp, dt = (double)t - st, d = (double)p - (double)t;
    a[S_P] += dp; a[S_T] += dt;
    a[S_PP] += dp * dp; a[S_TT] += dt * dt; a[S_PT] += dp * dt;
    a[S_ABS] += fabs(d); a[S_SQ] += d * d;
    if (has_prev) {
        const double vp = (double)p - (double)pp, vt = (double)t - (double)tp;
        a[S_DD] += fabs(vp - vt); a[S_DP] += fabs(vp); a[S_DT] += fabs(vt);
    }
    const bool ap = p > THRESHOLD, at = t > THRESHOLD;
    c[0] += ap; c[1] += at; c[2] += (ap && at);
}

// rows [r0, r1) of the call's arrays; row 0 of the call continues from the state's carried row.
__global__ void __launch_bounds__(met::THREADS)
metrics_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ energy, int64_t r0,
                       int64_t r1, const MetricsState* __restrict__ state, Slot* __restrict__ work) {
    using namespace met;
    __shared__ Slot lds[WAVES][REC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane / NQ, q = lane - NQ * g;              // row group 0..3 (4: idle lanes), float4 slot
    const bool active = lane < NC;
    const bool fresh = state->n == 0;                       // first rows ever: the shifts come from row 0 of this call
    const bool fresh_e = energy && state->sums[REC_COLS + Q_NE].i == 0;

    double sp[4], st[4];
    {
        float4 fp = make_float4(0.f, 0.f, 0.f, 0.f), ft = fp;
        if (fresh && active) {
            fp = *reinterpret_cast<const float4*>(pred + 4 * q);
            ft = *reinterpret_cast<const float4*>(target + 4 * q);
        }
        const float fpv[4] = {fp.x, fp.y, fp.z, fp.w}, ftv[4] = {ft.x, ft.y, ft.z, ft.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sp[j] = fresh ? (double)fpv[j] : state->shift_p[active ? 4 * q + j : 0];
            st[j] = fresh ? (double)ftv[j] : state->shift_t[active ? 4 * q + j : 0];
        }
    }
    const double s_ap = fresh ? mouth_sum_row(pred) : state->shift_ap;
    const double s_at = fresh ? mouth_sum_row(target) : state->shift_at;
    const double s_e = energy ? (fresh_e ? (double)energy[0] : state->shift_e) : 0.0;

    double acc[4][NCF];
    unsigned cnt[4][3];
    double sca[NSF];
    unsigned ne = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < NCF; ++k) acc[j][k] = 0.0;
        cnt[j][0] = cnt[j][1] = cnt[j][2] = 0;
    }
#pragma unroll
    for (int k = 0; k < NSF; ++k) sca[k] = 0.0;

    const int64_t stride = (int64_t)gridDim.x * WAVES * ROWS_PER_WAVE;
    for (int64_t base = r0 + ((int64_t)blockIdx.x * WAVES + wave) * ROWS_PER_WAVE; base < r1; base += stride) {   // wave-uniform
        const int64_t r = base + g;
        const bool valid = active && r < r1;
        const bool has_prev = valid && (r > 0 || !fresh);
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), t = p, pp = p, tp = p;
        if (valid) {
            p = *reinterpret_cast<const float4*>(pred + r * NC + 4 * q);
            t = *reinterpret_cast<const float4*>(target + r * NC + 4 * q);
        }
        if (has_prev) {
            if (r > 0) {
                pp = *reinterpret_cast<const float4*>(pred + (r - 1) * NC + 4 * q);
                tp = *reinterpret_cast<const float4*>(target + (r - 1) * NC + 4 * q);
            } else {
                pp = *reinterpret_cast<const float4*>(state->last_p + 4 * q);
                tp = *reinterpret_cast<const float4*>(state->last_t + 4 * q);
            }
        }
        if (valid) {
            fold_elem(acc[0], cnt[0], p.x, t.x, pp.x, tp.x, sp[0], st[0], has_prev);
            fold_elem(acc[1], cnt[1], p.y, t.y, pp.y, tp.y, sp[1], st[1], has_prev);
            fold_elem(acc[2], cnt[2], p.z, t.z, pp.z, tp.z, sp[2], st[2], has_prev);
            fold_elem(acc[3], cnt[3], p.w, t.w, pp.w, tp.w, sp[3], st[3], has_prev);
        }
        // mouth activity of the row: slots 3..7 of the row's 13 lanes, gathered on the row's first lane (no LDS)
        const double qp = quad_sum(p), qt = quad_sum(t);
        const int l0 = NQ * (g < ROWS_PER_WAVE ? g : 0);
        double ap = shfl_d(qp, l0 + MOUTH_Q0), at = shfl_d(qt, l0 + MOUTH_Q0);
#pragma unroll
        for (int m = MOUTH_Q0 + 1; m < MOUTH_Q1; ++m) {
            ap += shfl_d(qp, l0 + m);
            at += shfl_d(qt, l0 + m);
        }
        if (valid && q == 0) {
            const double xp = ap - s_ap, xt = at - s_at;
            sca[Q_AP] += xp; sca[Q_AT] += xt;
            sca[Q_APP] += xp * xp; sca[Q_ATT] += xt * xt; sca[Q_APT] += xp * xt;
            if (energy) {
                const double xe = (double)energy[r] - s_e;
                sca[Q_E] += xe; sca[Q_EE] += xe * xe; sca[Q_AE] += xp * xe;
                sca[Q_A] += xp; sca[Q_AA] += xp * xp;
                ++ne;
            }
        }
    }

    // the four row groups of the wave, in group order; lanes 0..12 then hold the wave's sums for their 4 columns
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < NCF; ++k) {
            double v = shfl_d(acc[j][k], q);
#pragma unroll
            for (int gg = 1; gg < ROWS_PER_WAVE; ++gg) v += shfl_d(acc[j][k], q + NQ * gg);
            if (lane < NQ) lds[wave][(4 * q + j) * NCS + k].d = v;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            long long v = (long long)__shfl(cnt[j][k], q, 64);
#pragma unroll
            for (int gg = 1; gg < ROWS_PER_WAVE; ++gg) v += (long long)__shfl(cnt[j][k], q + NQ * gg, 64);
            if (lane < NQ) lds[wave][(4 * q + j) * NCS + NCF + k].i = v;
        }
    }
#pragma unroll
    for (int k = 0; k < NSF; ++k) {
        double v = shfl_d(sca[k], 0);
#pragma unroll
        for (int gg = 1; gg < ROWS_PER_WAVE; ++gg) v += shfl_d(sca[k], NQ * gg);
        if (lane == 0) lds[wave][REC_COLS + k].d = v;
    }
    {
        long long v = (long long)__shfl(ne, 0, 64);
#pragma unroll
        for (int gg = 1; gg < ROWS_PER_WAVE; ++gg) v += (long long)__shfl(ne, NQ * gg, 64);
        if (lane == 0) lds[wave][REC_COLS + Q_NE].i = v;
    }
    __syncthreads();
    // the waves of the workgroup, in wave order
    Slot* out = work + (int64_t)blockIdx.x * REC;
    for (int e = tid; e < REC; e += THREADS) {
        Slot s = lds[0][e];
        if (slot_is_int(e)) { for (int w = 1; w < WAVES; ++w) s.i += lds[w][e].i; }
        else { for (int w = 1; w < WAVES; ++w) s.d += lds[w][e].d; }
        out[e] = s;
    }
}

// state += the `wgs` partial records, in workgroup order; then shifts (first rows only), carried row, row count.
__global__ void __launch_bounds__(met::FOLD_THREADS)
metrics_fold_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ energy, int64_t r0,
                    int64_t r1, MetricsState* __restrict__ state, const Slot* __restrict__ work, int wgs) {
    using namespace met;
    const int e = threadIdx.x;
    const bool fresh = state->n == 0;
    const bool fresh_e = energy && state->sums[REC_COLS + Q_NE].i == 0;
    const long long n_old = state->n;
    __syncthreads();                                           // every thread has read what thread 0 / thread Q_NE rewrite
    if (e < REC) {
        // workgroup order, FOLD_BATCH records in flight at a time: the loads are independent, only the additions are a chain
        // (one record per memory round trip made this kernel cost 0.23 us per partial record)
        Slot s = state->sums[e];
        const bool is_int = slot_is_int(e);
        int b = 0;
        for (; b + FOLD_BATCH <= wgs; b += FOLD_BATCH) {
            Slot v[FOLD_BATCH];
#pragma unroll
            for (int j = 0; j < FOLD_BATCH; ++j) v[j] = work[(int64_t)(b + j) * REC + e];
#pragma unroll
            for (int j = 0; j < FOLD_BATCH; ++j) { if (is_int) s.i += v[j].i; else s.d += v[j].d; }
        }
        for (; b < wgs; ++b) {
            const Slot v = work[(int64_t)b * REC + e];
            if (is_int) s.i += v.i; else s.d += v.d;
        }
        state->sums[e] = s;
    }
    if (e < NC) {
        if (fresh) { state->shift_p[e] = (double)pred[e]; state->shift_t[e] = (double)target[e]; }
        state->last_p[e] = pred[(r1 - 1) * NC + e];
        state->last_t[e] = target[(r1 - 1) * NC + e];
    }
    if (e == 64) {
        if (fresh) { state->shift_ap = mouth_sum_row(pred); state->shift_at = mouth_sum_row(target); }
        if (fresh_e) state->shift_e = (double)energy[0];
        state->n = n_old + (r1 - r0);
    }
}

// The empty state is all zero bits.  A kernel rather than a memset node, so a captured reset replays as the same kind of
// node as the update behind it.
__global__ void __launch_bounds__(256) metrics_reset_kernel(MetricsState* __restrict__ state) {
    static_assert(sizeof(MetricsState) % sizeof(long long) == 0, "the state is cleared in 8-byte words");
    long long* w = reinterpret_cast<long long*>(state);
    for (int i = threadIdx.x; i < (int)(sizeof(MetricsState) / sizeof(long long)); i += 256) w[i] = 0;
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ inline double wave_min(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ inline double wave_max(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

// Pearson correlation from shifted sums over n rows, gated as the reference gates it: both unbiased standard deviations
// above 1e-6 (losses.py:479, :555, :573), the result clipped to [-1, 1] as torch.corrcoef clips; NaN -> not valid.
__device__ inline bool corr_from_sums(double n, double sx, double sy, double sxx, double syy, double sxy, bool gate_x, bool gate_y,
                                      double* out) {
    *out = 0.0;
    if (n < 2.0) return false;
    const double vx = fmax(sxx - sx * sx / n, 0.0), vy = fmax(syy - sy * sy / n, 0.0);
    if (gate_x && !(sqrt(vx / (n - 1.0)) > 1e-6)) return false;
    if (gate_y && !(sqrt(vy / (n - 1.0)) > 1e-6)) return false;
    const double den = sqrt(vx) * sqrt(vy);
    if (!(den > 0.0)) return false;                            // 0 / 0: torch.corrcoef gives NaN, the reference then 0.0
    const double c = (sxy - sx * sy / n) / den;
    if (c != c) return false;
    *out = fmin(fmax(c, -1.0), 1.0);
    return true;
}

__global__ void __launch_bounds__(64) metrics_compute_kernel(const MetricsState* __restrict__ state, float* __restrict__ out) {
    using namespace met;
    const int c = threadIdx.x;
    const bool col = c < NC;
    const long long n = state->n;
    if (n == 0) {
        if (c < KM_METRICS_COUNT) out[c] = 0.f;
        return;
    }
    const double dn = (double)n;
    double s[NCF];
    long long k[3];
#pragma unroll
    for (int j = 0; j < NCF; ++j) s[j] = col ? state->sums[c * NCS + j].d : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) k[j] = col ? state->sums[c * NCS + NCF + j].i : 0;

    // accuracy (losses.py:463-471)
    const double sum_abs = wave_sum(s[S_ABS]), sum_sq = wave_sum(s[S_SQ]);
    const double mae_c = s[S_ABS] / dn;
    const double mae_max = wave_max(col ? mae_c : -INFINITY), mae_min = wave_min(col ? mae_c : INFINITY);
    const double mae_mean = wave_sum(col ? mae_c : 0.0) / NC;
    const double dev = col ? mae_c - mae_mean : 0.0;
    const double mae_std = sqrt(wave_sum(dev * dev) / (NC - 1));
    // per-column correlation (losses.py:474-489)
    double corr;
    const bool ok = col && corr_from_sums(dn, s[S_P], s[S_T], s[S_PP], s[S_TT], s[S_PT], true, true, &corr);
    const double n_ok = wave_sum(ok ? 1.0 : 0.0);
    const double corr_sum = wave_sum(ok ? corr : 0.0), corr_min = wave_min(ok ? corr : INFINITY);
    // temporal (losses.py:492-498)
    const double sum_dd = wave_sum(s[S_DD]), sum_dp = wave_sum(s[S_DP]), sum_dt = wave_sum(s[S_DT]);
    // activity (losses.py:501-519); counts stay below 2^53, so the float64 sums are exact
    const double cp = wave_sum((double)k[0]), ct = wave_sum((double)k[1]), cpt = wave_sum((double)k[2]);
    // lip sync (losses.py:543-581)
    const bool mouth = c >= 4 * MOUTH_Q0 && c < 4 * MOUTH_Q1;
    const double mouth_abs = wave_sum(mouth ? s[S_ABS] : 0.0);

    if (c != 0) return;
    const Slot* m = state->sums + REC_COLS;
    const double cells = dn * NC;
    out[0] = (float)(sum_abs / cells);
    out[1] = (float)(sum_sq / cells);
    out[2] = (float)sqrt(sum_sq / cells);
    out[3] = (float)mae_max;
    out[4] = (float)mae_min;
    out[5] = (float)mae_std;
    out[6] = (float)(n_ok > 0.0 ? corr_sum / n_ok : 0.0);
    out[7] = (float)(n_ok > 0.0 ? corr_min : 0.0);
    const double dcells = (dn - 1.0) * NC;
    out[8] = (float)(n > 1 ? sum_dd / dcells : 0.0);
    out[9] = (float)(n > 1 ? sum_dp / dcells : 0.0);
    out[10] = (float)(n > 1 ? sum_dt / dcells : 0.0);
    out[11] = (float)(cp / cells);
    out[12] = (float)(ct / cells);
    const double precision = cpt / (cpt + (cp - cpt) + 1e-8), recall = cpt / (cpt + (ct - cpt) + 1e-8);
    out[13] = (float)precision;
    out[14] = (float)recall;
    out[15] = (float)(2.0 * precision * recall / (precision + recall + 1e-8));
    out[16] = (float)(mouth_abs / (dn * (4 * (MOUTH_Q1 - MOUTH_Q0))));
    double mc, av = 0.0;
    corr_from_sums(dn, m[Q_AP].d, m[Q_AT].d, m[Q_APP].d, m[Q_ATT].d, m[Q_APT].d, true, true, &mc);
    out[17] = (float)mc;
    const long long ne = m[Q_NE].i;
    if (ne > 0) corr_from_sums((double)ne, m[Q_A].d, m[Q_E].d, m[Q_AA].d, m[Q_EE].d, m[Q_AE].d, false, true, &av);
    out[18] = (float)av;
    out[19] = (float)dn;
    out[20] = (float)n_ok;
    out[21] = ne > 0 ? 1.f : 0.f;
}

}  // namespace km

using namespace km;

extern "C" {

int km_metrics_create(void** acc_out) {
    if (!acc_out) return fail(KM_ERR_INVALID_ARG, "km_metrics_create: NULL argument");
    auto a = std::make_unique<MetricsAcc>();
    if (const char* env = std::getenv("KM_METRICS_WGS")) {     // read once, here; no launch path reads the environment
        const long v = std::strtol(env, nullptr, 10);
        if (v >= 1 && v <= met::MAX_WGS) a->wgs = (int)v;
    }
    if (int rc = a->state.alloc(1, "km_metrics_create")) return rc;
    if (int rc = a->work.alloc((int64_t)a->wgs * met::REC, "km_metrics_create")) return rc;
    HIP_TRY(hipMemset(a->state, 0, sizeof(MetricsState)));
    HIP_TRY(hipStreamSynchronize(nullptr));   // the cleared state is visible to whichever stream updates first
    *acc_out = a.release();
    return KM_OK;
}

int km_metrics_destroy(void* acc) {
    if (!acc) return KM_OK;
    delete static_cast<MetricsAcc*>(acc);
    return KM_OK;
}

int km_metrics_reset(void* acc, void* stream) {
    if (!acc) return fail(KM_ERR_INVALID_ARG, "km_metrics_reset: NULL accumulator");
    hipLaunchKernelGGL(metrics_reset_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<MetricsAcc*>(acc)->state);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_metrics_update(void* acc, const float* pred_dev, const float* target_dev, const float* audio_energy_dev, int64_t N,
                      void* stream) {
    using namespace met;
    if (!acc || N < 0) return fail(KM_ERR_INVALID_ARG, "km_metrics_update: bad argument");
    if (N == 0) return KM_OK;
    if (!pred_dev || !target_dev) return fail(KM_ERR_INVALID_ARG, "km_metrics_update: NULL rows");
    if (((uintptr_t)pred_dev | (uintptr_t)target_dev) & 15) return fail(KM_ERR_INVALID_ARG, "km_metrics_update: rows must be 16-byte aligned");
    MetricsAcc* a = static_cast<MetricsAcc*>(acc);
    hipStream_t st = (hipStream_t)stream;
    for (int64_t r0 = 0; r0 < N; r0 += MAX_ROWS_PER_LAUNCH) {
        const int64_t r1 = r0 + MAX_ROWS_PER_LAUNCH < N ? r0 + MAX_ROWS_PER_LAUNCH : N;
        const int64_t per_wg = WAVES * ROWS_PER_WAVE;
        const int64_t want = (r1 - r0 + per_wg - 1) / per_wg;
        const int wgs = (int)(want < a->wgs ? want : a->wgs);
        hipLaunchKernelGGL(metrics_partial_kernel, dim3((unsigned)wgs), dim3(THREADS), 0, st, pred_dev, target_dev, audio_energy_dev, r0,
                           r1, a->state, a->work);
        hipLaunchKernelGGL(metrics_fold_kernel, dim3(1), dim3(FOLD_THREADS), 0, st, pred_dev, target_dev, audio_energy_dev, r0, r1,
                           a->state, a->work, wgs);
        HIP_TRY(hipGetLastError());
    }
    return KM_OK;
}

int km_metrics_compute(void* acc, float* out_dev, void* stream) {
    if (!acc || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_metrics_compute: NULL argument");
    hipLaunchKernelGGL(metrics_compute_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<MetricsAcc*>(acc)->state, out_dev);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // extern "C"
