// km_loss_terms.hip -- the validation loss by component, accumulated in device memory (gfx950).
//
// Replaces the per-batch criterion call + .item() reads of the reference's validate() (src/train_sequential.py:257-283) and the
// `metrics` dict of KoeMorphLoss.forward (src/model/losses.py:111-183): the reference evaluates every term in float32 on the
// device and reads each one back per batch.  Here km_loss_terms_update evaluates, for one batch (N, 52), the eval-mode value of
// every term the training tail (km_train_tail.h) adds -- KoeMorphLoss's eight and DualStreamLoss's two -- plus their weighted
// total, in float64, and folds them into a small state in device memory; km_loss_terms_compute turns the state into means.
// Nothing synchronises, allocates or reads back, so both can be captured in a graph.
//
// Per batch (y = pred, t = target, e = y - t, all differences of float32 values taken in float64, where they are exact):
//   mse         sum e^2 / (52 N)                                              (losses.py:113-117)
//   l1          sum |e| / (52 N)                                              (:119-123)
//   perceptual  sum_g w_g sum_{i in g} e^2 / (|g| N), the four groups of :306-338; + 0.5 (1 - cos(m, a)) with m_b = mean of
//               columns 12..31 of row b and a = audio_energy_dev when that is given (:340-378; F.normalize's eps 1e-12,
//               cosine_similarity's 1e-8 on the product of the norms)
//   temporal    sum ((y - prev_pred) - (t - prev_target))^2 / (52 N)          (:185-200)   needs prev_pred_dev and prev_target_dev
//   velocity    sum |same difference| / (52 N)                                (:202-217)   needs both as well
//   sparsity    sum |y| / (52 N)                                              (:219-224)
//   smoothness  sum_{j < 51} |y[j + 1] - y[j]| / (51 N)                        (:226-234)
//   landmark    sum (e W^T)^2 / (136 N)                                       (:397-412)   needs landmark_w_dev
//   ds_velocity    sum ((y - p) - (t - p))^2 / (52 N), p = ds_prev_pred_dev   (src/train_dual_stream.py:489-495)   needs p
//   ds_separation  sum_b | mean(y[b, MOUTH]) - mean(y[b, EXPRESSION]) | / N   (:498-514)   on when ds_separation_weight > 0
//   total       mse_weight mse + l1_weight l1 + sum of cfg weight x term over the terms that were evaluated
// A term whose input is missing is skipped as km_loss_config documents it: it reports 0 and its update is not counted in
// its mean.  cfg = NULL evaluates mse and l1 only.  Independently of cfg every update adds its rows' smoothness
// mean_j |y[b, j + 1] - y[b, j]| to a per-ROW mean: what the reference's per-sequence statistics collect (:279-283).
//
// REDUCTION ORDER (fixed; no floating-point atomics; the same rows in the same calls give the same bits):
//   loss_terms_partial_kernel   row r belongs to wave (r mod 4 G) of a grid of G = min(ceil(N / 4), 256) four-wave workgroups;
//                               lane i < 52 owns column i and keeps its float64 sums over the wave's rows, in row order; the
//                               landmark products are lanes k, k + 64, k + 128 < 136.  At the end the 64 lanes are added by an
//                               xor butterfly, the waves of a workgroup in wave order (LDS), one record per workgroup.
//   loss_terms_fold_kernel      one wave: lane q adds quantity q of the G records in workgroup order; lane 0 turns the
//                               thirteen sums into the batch's terms, rounds each once to float32 for terms_dev, and adds
//                               the float64 values to the state.
//   loss_terms_compute_kernel   one thread per output: sum / count, rounded once.
#include <hip/hip_runtime.h>

#include <memory>

#include "km_context.h"

namespace km {


namespace lt {
constexpr int NC = 52, NL = 136;
constexpr int WAVES = 4, THREADS = WAVES * 64, MAX_WGS = 256;
enum Q { Q_SQ = 0, Q_ABS, Q_PERC, Q_TEMP, Q_VEL, Q_SPARS, Q_SMOOTH, Q_LM, Q_DSV, Q_SEP, Q_MM, Q_EE, Q_ME, NQ };
}  // namespace lt

struct LossTermsState {
    double sum[KM_LOSS_TERMS];          // per-batch float64 values added up, per term (KM_LOSS_TERM_TOTAL included)
    long long cnt[KM_LOSS_TERMS];       // updates in which the term was evaluated
    long long updates, rows;
    double row_smooth;                  // sum over rows of mean_j |y[j + 1] - y[j]|
};

struct LossTermsAcc {
    DevBuf<LossTermsState> state;
    DevBuf<double> work;                // MAX_WGS partial records
};

struct LossTermsArgs {
    const float *pred, *target, *prev_pred, *prev_target, *landmark_w, *energy, *ds_prev;
    int64_t N;
    int sep_on, has_cfg;
    float mse_w, l1_w, perceptual_w, temporal_w, sparsity_w, smoothness_w, landmark_w_w, velocity_w, ds_velocity_w, ds_separation_w;
};

__device__ inline double lt_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// MOUTH_INDICES = 14..40 and 51 (src/model/dual_stream_attention.py:14-45); the other 24 are the expression rows
__device__ inline bool lt_is_mouth(int i) { return (i >= 14 && i <= 40) || i == 51; }

__global__ void __launch_bounds__(lt::THREADS) loss_terms_partial_kernel(LossTermsArgs a, double* __restrict__ work) {
    using namespace lt;
    __shared__ double e_s[WAVES][64];
    __shared__ double red[WAVES][NQ];
    const int tid = threadIdx.x, i = tid & 63, w = tid >> 6;
    const bool col = i < NC;
    const bool have_prev = a.prev_pred && a.prev_target;
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    // perceptual groups (losses.py:306-330): weight / group size
    const double pg = !col ? 0.0 : (i < 12 ? 1.0 / 12.0 : (i < 32 ? 2.0 / 20.0 : (i < 44 ? 1.0 / 12.0 : 1.5 / 8.0)));
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    for (int64_t r = (int64_t)blockIdx.x * WAVES + w; r < a.N; r += stride) {       // wave-uniform
        double y = 0.0, t = 0.0;
        if (col) { y = (double)a.pred[r * NC + i]; t = (double)a.target[r * NC + i]; }
        const double e = y - t;
        acc[Q_SQ] += e * e;
        acc[Q_ABS] += fabs(e);
        acc[Q_PERC] += pg * (e * e);
        acc[Q_SPARS] += fabs(y);
        if (have_prev && col) {
            const double dd = (y - (double)a.prev_pred[r * NC + i]) - (t - (double)a.prev_target[r * NC + i]);
            acc[Q_TEMP] += dd * dd;
            acc[Q_VEL] += fabs(dd);
        }
        if (a.ds_prev && col) {
            const double p = (double)a.ds_prev[r * NC + i];
            const double dd = (y - p) - (t - p);
            acc[Q_DSV] += dd * dd;
        }
        const double y_right = __shfl_down(y, 1, 64);
        if (i < NC - 1) acc[Q_SMOOTH] += fabs(y_right - y);
        if (a.sep_on) {
            const double ms = lt_wave_sum(col && lt_is_mouth(i) ? y : 0.0), es = lt_wave_sum(col && !lt_is_mouth(i) ? y : 0.0);
            if (i == 0) acc[Q_SEP] += fabs(ms / 28.0 - es / 24.0);
        }
        if (a.energy) {
            const double m = lt_wave_sum(i >= 12 && i < 32 ? y : 0.0) / 20.0;
            if (i == 0) {
                const double ev = (double)a.energy[r];
                acc[Q_MM] += m * m; acc[Q_EE] += ev * ev; acc[Q_ME] += m * ev;
            }
        }
        if (a.landmark_w) {      // u = e W^T, W (136, 52); only this wave touches e_s[w]
            __builtin_amdgcn_wave_barrier();
            e_s[w][i] = e;
            __builtin_amdgcn_wave_barrier();
            for (int k = i; k < NL; k += 64) {
                double u = 0.0;
                for (int j = 0; j < NC; ++j) u += e_s[w][j] * (double)a.landmark_w[k * NC + j];
                acc[Q_LM] += u * u;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double v = lt_wave_sum(acc[q]);
        if (i == 0) red[w][q] = v;
    }
    __syncthreads();
    if (tid < NQ) {
        double v = red[0][tid];
        for (int ww = 1; ww < WAVES; ++ww) v += red[ww][tid];
        work[(int64_t)blockIdx.x * NQ + tid] = v;
    }
}

__global__ void __launch_bounds__(64) loss_terms_fold_kernel(LossTermsArgs a, const double* __restrict__ work, int wgs,
                                                              LossTermsState* __restrict__ state, float* __restrict__ terms_out) {
    using namespace lt;
    __shared__ double s[NQ];
    const int q = threadIdx.x;
    if (q < NQ) {
        double v = 0.0;
        for (int g = 0; g < wgs; ++g) v += work[(int64_t)g * NQ + q];
        s[q] = v;
    }
    __syncthreads();
    if (q != 0) return;
    const double n = (double)a.N, cells = n * NC;
    const bool have_prev = a.prev_pred && a.prev_target;
    double term[KM_LOSS_TERMS];
    bool on[KM_LOSS_TERMS];
    for (int k = 0; k < KM_LOSS_TERMS; ++k) { term[k] = 0.0; on[k] = false; }
    term[KM_LOSS_TERM_MSE] = s[Q_SQ] / cells; on[KM_LOSS_TERM_MSE] = true;
    term[KM_LOSS_TERM_L1] = s[Q_ABS] / cells; on[KM_LOSS_TERM_L1] = true;
    if (a.has_cfg) {
        double per = s[Q_PERC] / n;
        if (a.energy) {      // 0.5 (1 - cos) of the two normalised vectors (losses.py:340-378)
            const double nm = fmax(sqrt(s[Q_MM]), 1e-12), na = fmax(sqrt(s[Q_EE]), 1e-12);
            const double dot = s[Q_ME] / (nm * na), w1 = s[Q_MM] / (nm * nm), w2 = s[Q_EE] / (na * na);
            per += 0.5 * (1.0 - dot / sqrt(fmax(w1 * w2, 1e-16)));
        }
        term[KM_LOSS_TERM_PERCEPTUAL] = per; on[KM_LOSS_TERM_PERCEPTUAL] = true;
        if (have_prev) {
            term[KM_LOSS_TERM_TEMPORAL] = s[Q_TEMP] / cells; on[KM_LOSS_TERM_TEMPORAL] = true;
            term[KM_LOSS_TERM_VELOCITY] = s[Q_VEL] / cells; on[KM_LOSS_TERM_VELOCITY] = true;
        }
        term[KM_LOSS_TERM_SPARSITY] = s[Q_SPARS] / cells; on[KM_LOSS_TERM_SPARSITY] = true;
        term[KM_LOSS_TERM_SMOOTHNESS] = s[Q_SMOOTH] / (n * (NC - 1)); on[KM_LOSS_TERM_SMOOTHNESS] = true;
        if (a.landmark_w) { term[KM_LOSS_TERM_LANDMARK] = s[Q_LM] / (n * NL); on[KM_LOSS_TERM_LANDMARK] = true; }
        if (a.ds_prev) { term[KM_LOSS_TERM_DS_VELOCITY] = s[Q_DSV] / cells; on[KM_LOSS_TERM_DS_VELOCITY] = true; }
        if (a.sep_on) { term[KM_LOSS_TERM_DS_SEPARATION] = s[Q_SEP] / n; on[KM_LOSS_TERM_DS_SEPARATION] = true; }
    }
    const double wt[KM_LOSS_TERMS] = {a.mse_w, a.l1_w, a.perceptual_w, a.temporal_w, a.velocity_w, a.sparsity_w, a.smoothness_w,
                                      a.landmark_w_w, a.ds_velocity_w, a.ds_separation_w, 0.0};
    double total = 0.0;
    for (int k = 0; k < KM_LOSS_TERM_TOTAL; ++k)
        if (on[k]) total += wt[k] * term[k];
    term[KM_LOSS_TERM_TOTAL] = total; on[KM_LOSS_TERM_TOTAL] = true;
    for (int k = 0; k < KM_LOSS_TERMS; ++k) {
        if (terms_out) terms_out[k] = (float)term[k];
        if (on[k]) { state->sum[k] += term[k]; state->cnt[k] += 1; }
    }
    state->updates += 1;
    state->rows += a.N;
    state->row_smooth += s[Q_SMOOTH] / (NC - 1);
}

// The empty state is all zero bits.  A kernel rather than a memset node, as km_metrics_reset.
__global__ void __launch_bounds__(64) loss_terms_reset_kernel(LossTermsState* __restrict__ state) {
    static_assert(sizeof(LossTermsState) % sizeof(long long) == 0, "the state is cleared in 8-byte words");
    long long* w = reinterpret_cast<long long*>(state);
    for (int i = threadIdx.x; i < (int)(sizeof(LossTermsState) / sizeof(long long)); i += 64) w[i] = 0;
}

__global__ void __launch_bounds__(64) loss_terms_compute_kernel(const LossTermsState* __restrict__ state, float* __restrict__ out) {
    const int k = threadIdx.x;
    if (k < KM_LOSS_TERMS) out[k] = state->cnt[k] > 0 ? (float)(state->sum[k] / (double)state->cnt[k]) : 0.f;
    else if (k == KM_LOSS_TERMS) out[k] = (float)state->updates;
    else if (k == KM_LOSS_TERMS + 1) out[k] = state->rows > 0 ? (float)(state->row_smooth / (double)state->rows) : 0.f;
}

}  // namespace km

using namespace km;

extern "C" {

int km_loss_terms_create(void** acc_out) {
    if (!acc_out) return fail(KM_ERR_INVALID_ARG, "km_loss_terms_create: NULL argument");
    auto a = std::make_unique<LossTermsAcc>();
    if (int rc = a->state.alloc(1, "km_loss_terms_create")) return rc;
    if (int rc = a->work.alloc((int64_t)lt::MAX_WGS * lt::NQ, "km_loss_terms_create")) return rc;
    HIP_TRY(hipMemset(a->state, 0, sizeof(LossTermsState)));
    HIP_TRY(hipStreamSynchronize(nullptr));   // the cleared state is visible to whichever stream updates first
    *acc_out = a.release();
    return KM_OK;
}

int km_loss_terms_destroy(void* acc) {
    if (!acc) return KM_OK;
    delete static_cast<LossTermsAcc*>(acc);
    return KM_OK;
}

int km_loss_terms_reset(void* acc, void* stream) {
    if (!acc) return fail(KM_ERR_INVALID_ARG, "km_loss_terms_reset: NULL accumulator");
    hipLaunchKernelGGL(loss_terms_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<LossTermsAcc*>(acc)->state);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_loss_terms_update(void* acc, const km_loss_config* cfg, float mse_weight, float l1_weight, const float* pred_dev,
                         const float* target_dev, int64_t N, float* terms_dev, void* stream) {
    if (!acc || !pred_dev || !target_dev || N <= 0) return fail(KM_ERR_INVALID_ARG, "km_loss_terms_update: bad argument");
    // the struct holds device pointers the kernel dereferences: a caller built against another header is refused (km_train_set_loss)
    if (cfg && cfg->abi_version != KM_ABI_VERSION)
        return fail(KM_ERR_INVALID_ARG, "km_loss_config.abi_version %d != %d", cfg->abi_version, KM_ABI_VERSION);
    LossTermsAcc* a = static_cast<LossTermsAcc*>(acc);
    LossTermsArgs g{};
    g.pred = pred_dev; g.target = target_dev; g.N = N; g.mse_w = mse_weight; g.l1_w = l1_weight;
    if (cfg) {
        g.has_cfg = 1;
        g.prev_pred = cfg->prev_pred_dev; g.prev_target = cfg->prev_target_dev; g.landmark_w = cfg->landmark_w_dev;
        g.energy = cfg->audio_energy_dev; g.ds_prev = cfg->ds_prev_pred_dev; g.sep_on = cfg->ds_separation_weight > 0.f ? 1 : 0;
        g.perceptual_w = cfg->perceptual_weight; g.temporal_w = cfg->temporal_weight; g.sparsity_w = cfg->sparsity_weight;
        g.smoothness_w = cfg->smoothness_weight; g.landmark_w_w = cfg->landmark_weight; g.velocity_w = cfg->velocity_weight;
        g.ds_velocity_w = cfg->ds_velocity_weight; g.ds_separation_w = cfg->ds_separation_weight;
    }
    const int64_t want = (N + lt::WAVES - 1) / lt::WAVES;
    const int wgs = (int)(want < lt::MAX_WGS ? want : lt::MAX_WGS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_terms_partial_kernel, dim3((unsigned)wgs), dim3(lt::THREADS), 0, st, g, a->work);
    hipLaunchKernelGGL(loss_terms_fold_kernel, dim3(1), dim3(64), 0, st, g, a->work, wgs, a->state, terms_dev);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_loss_terms_compute(void* acc, float* out_dev, void* stream) {
    if (!acc || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_loss_terms_compute: NULL argument");
    hipLaunchKernelGGL(loss_terms_compute_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, static_cast<LossTermsAcc*>(acc)->state, out_dev);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // extern "C"
