// eGeMAPS low-level descriptors per frame: the 25 smoothed contours (18 for GeMAPS) that egm_functional_kernel reduces to the
// functionals, written out as rows -- at the native 100 Hz, or on a frame grid of `fps` rows per second (the model's frame rate).
//
//   egm_lld_kernel<SET>   grid (tiles of output rows, windows), 256 threads.  A tile stages the records of the frames its rows touch,
//                         two frames of halo a side (the smoothed F0 of a frame's neighbours enters its masked averages, and that
//                         needs THEIR neighbours' F0), smooths them in LDS and writes its rows -- contiguous in `out` -- with
//                         consecutive threads on consecutive floats.  Nothing is serial, nothing atomic; a window is as many
//                         workgroups as it has tiles.
// The smoothing restates the three `load` modes of egm_functional_kernel (km_egemaps_window.hip) statement by statement: the sum runs
// over the frames t-1, t, t+1 in that order and is divided by the count; the semitone is 12 log2f(f0s / 27.5f).  The contours are those
// behind the pinned functionals; that openSMILE's own LowLevelDescriptors level has these names in this order is UNPINNED, as for the
// whole back end.
//
// Frame grid: row k sits at the frame coordinate p = k * 100.0 / fps (float64, in that order), j = floor(p), w = p - j.  j >= nf - 1
// is the last frame, w == 0 frame j itself, otherwise fmaf((float)w, b - a, a) between frames j and j + 1 -- except that a column
// smoothed over non-zero values only (10-24) is never blended with a 0: where either side is 0 the row takes the nearer frame's
// value, the earlier one at w == 0.5.
#include <hip/hip_runtime.h>

#include <cmath>

#include "km_context.h"
#include "km_egemaps_dev.h"
#include "km_egemaps_lld.h"

namespace km {

namespace egm {
// (the tile sizes, lld_ecol and lld_field: km_egemaps_lld.h, shared with the stream rows of km_koemorph_audio.hip)
constexpr bool lld_gemaps_drops(int e) { return (e >= 5 && e <= 9) || e == 20 || e == 23; }
constexpr bool lld_columns_agree() {
    int n = 0;
    for (int e = 0; e < NLLD_EGEMAPS; ++e)
        if (!lld_gemaps_drops(e) && lld_ecol<SET_GEMAPS>(n++) != e) return false;
    return n == NLLD_GEMAPS;
}
static_assert(lld_columns_agree(), "GeMAPS: the 25 columns without flux, MFCC 1-4 and the bandwidths of F2 and F3, in their order");
static_assert(lld_field(0) == R_LOUD && lld_field(5) == R_FLUX && lld_field(9) == R_MFCC + 3 && lld_field(11) == R_JIT && lld_field(15) == R_H1A3 &&
              lld_field(16) == R_F && lld_field(17) == R_BW && lld_field(18) == R_FAMP && lld_field(23) == R_BW + 2 && lld_field(24) == R_FAMP + 2,
              "the record fields of the 25 columns");
static_assert(LLD_MAXF == 6548, "the long tier's frame count (km_egemaps_window.h)");
}  // namespace egm

template <int SET>
__global__ __launch_bounds__(256) void egm_lld_kernel(const float* __restrict__ recs, int nf, int rec_frames, int T_out, int rows, double fps,
                                                      float* __restrict__ out) {
    using namespace egm;
    constexpr int W = lld_width(SET);
    __shared__ float rec_s[LLD_STAGE * REC];      // records of frames s_lo .. s_hi
    __shared__ float f0s_s[LLD_STAGE];            // their smoothed F0 (the halo's outer frame is not needed and not written)
    __shared__ float lld_s[LLD_CORE * W];         // descriptors of frames f_lo .. f_hi
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * rows;
    const int nrow = T_out - k0 < rows ? T_out - k0 : rows;
    // frame j and weight w of row k: fps == 0 is the native grid
    auto coord = [&](int k, double& w) {
        w = 0.0;
        if (fps == 0.0) return k < nf - 1 ? k : nf - 1;
        const double p = (double)k * 100.0 / fps, fl = floor(p);
        if (fl >= (double)(nf - 1)) return nf - 1;
        w = p - fl;
        return (int)fl;
    };
    // the frames the rows touch: j of the first row up to j of the last, and j + 1 where the last row lies between two frames (rows
    // before it with the same j lie between them as well, rows with a smaller j end at j itself)
    double w_first, w_last;
    const int f_lo = coord(k0, w_first);
    const int j_last = coord(k0 + nrow - 1, w_last);
    const int f_hi = w_last != 0.0 ? j_last + 1 : j_last;                // w != 0 only for j < nf - 1
    if (nrow < 1 || f_hi - f_lo + 1 > LLD_CORE) return;                  // the host sizes `rows` so that this never happens; never index past LDS
    const int s_lo = f_lo - 2 > 0 ? f_lo - 2 : 0, s_hi = f_hi + 2 < nf ? f_hi + 2 : nf - 1;
    const float* rec = recs + ((int64_t)blockIdx.y * rec_frames + s_lo) * REC;
    for (int i = tid; i < (s_hi - s_lo + 1) * REC; i += 256) rec_s[i] = rec[i];
    __syncthreads();
    auto raw = [&](int t, int field) { return rec_s[(t - s_lo) * REC + field]; };
    // smoothed F0 (non-zero smoothing) of the frames f_lo - 1 .. f_hi + 1: it defines the voiced frames
    {
        const int a = f_lo - 1 > 0 ? f_lo - 1 : 0, b = f_hi + 1 < nf ? f_hi + 1 : nf - 1;
        for (int t = a + tid; t <= b; t += 256) {
            const float c = raw(t, R_F0);
            float acc = 0.f; int n = 0;
            if (c != 0.f)
                for (int q = (t > 0 ? t - 1 : 0); q <= (t + 1 < nf ? t + 1 : nf - 1); ++q) { const float x = raw(q, R_F0); if (x != 0.f) { acc += x; ++n; } }
            f0s_s[t - s_lo] = n ? acc / n : 0.f;
        }
    }
    __syncthreads();
    auto f0s = [&](int t) { return f0s_s[t - s_lo]; };
    for (int idx = tid; idx < (f_hi - f_lo + 1) * W; idx += 256) {
        const int t = f_lo + idx / W, e = lld_ecol<SET>(idx % W), field = lld_field(e);
        float r = 0.f;
        if (e == LLD_FIRST_NZ) r = f0s(t) > 0.f ? 12.0f * log2f(f0s(t) / 27.5f) : 0.f;
        else if (e < LLD_FIRST_NZ) {
            float acc = 0.f; int n = 0;
            for (int q = (t > 0 ? t - 1 : 0); q <= (t + 1 < nf ? t + 1 : nf - 1); ++q) { acc += raw(q, field); ++n; }
            r = acc / n;
        } else {
            const float c = f0s(t) > 0.f ? raw(t, field) : 0.f;
            if (c != 0.f) {
                float acc = 0.f; int n = 0;
                for (int q = (t > 0 ? t - 1 : 0); q <= (t + 1 < nf ? t + 1 : nf - 1); ++q) {
                    const float x = f0s(q) > 0.f ? raw(q, field) : 0.f;
                    if (x != 0.f) { acc += x; ++n; }
                }
                r = acc / n;
            }
        }
        lld_s[idx] = r;
    }
    __syncthreads();
    float* o = out + ((int64_t)blockIdx.y * T_out + k0) * W;
    for (int idx = tid; idx < nrow * W; idx += 256) {
        const int c = idx % W;
        double w;
        const int j = coord(k0 + idx / W, w);
        const float a = lld_s[(j - f_lo) * W + c];
        float r = a;
        if (w != 0.0) {                                                  // then j + 1 <= f_hi
            const float b = lld_s[(j + 1 - f_lo) * W + c];
            if (lld_ecol<SET>(c) < LLD_FIRST_NZ || (a != 0.f && b != 0.f)) r = fmaf((float)w, b - a, a);
            else r = w <= 0.5 ? a : b;
        }
        o[idx] = r;
    }
}

int64_t egm_lld_frames(int64_t L, double fps) {
    using namespace egm;
    if (fps == 0.0) return L < 960 ? 0 : (L - 960) / HOP + 1;            // km_egemaps_num_frames
    if (!std::isfinite(fps) || fps < LLD_FPS_MIN || fps > LLD_FPS_MAX || L < 0) return -1;
    return (int64_t)((double)L / 16000.0 * fps);
}

int egm_lld(const float* rec_dev, int nf, int rec_frames, int n, int64_t T_out, double fps, float* out_dev, hipStream_t st, int feature_set) {
    using namespace egm;
    if (!set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "egm_lld: feature set %d", feature_set);
    if (!rec_dev || !out_dev || n < 1 || n > 65535 || nf < 1 || nf > rec_frames || rec_frames > LLD_MAXF || T_out < 1 || T_out > (1 << 24) ||
        (fps == 0.0 ? T_out != nf : !(fps >= LLD_FPS_MIN && fps <= LLD_FPS_MAX)))
        return fail(KM_ERR_INVALID_ARG, "egm_lld: bad argument");
    // rows per tile: natively a row is a frame; otherwise the frames j(k0) .. j(k0 + rows - 1) + 1 of a tile are at most
    // (rows - 1) * 100 / fps + 3, and LLD_CORE fit
    int rows = LLD_CORE;
    if (fps != 0.0) {
        const double r = 1.0 + floor((LLD_CORE - 4) * fps / 100.0);
        rows = r < LLD_CORE ? (int)r : LLD_CORE;
    }
    const dim3 grid((unsigned)((T_out + rows - 1) / rows), (unsigned)n);
    if (feature_set == SET_GEMAPS)
        hipLaunchKernelGGL(egm_lld_kernel<SET_GEMAPS>, grid, dim3(256), 0, st, rec_dev, nf, rec_frames, (int)T_out, rows, fps, out_dev);
    else
        hipLaunchKernelGGL(egm_lld_kernel<SET_EGEMAPS>, grid, dim3(256), 0, st, rec_dev, nf, rec_frames, (int)T_out, rows, fps, out_dev);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" {

int km_egemaps_lld_width(int32_t feature_set) { return egm::lld_width(feature_set); }

int64_t km_egemaps_lld_frames(int64_t L, double fps) { return egm_lld_frames(L, fps); }

// the kernel alone on records the caller wrote (tests): any frame count up to 6548, there is no tier
int km_egemaps_llds_from_records(int32_t feature_set, const float* rec_dev, int64_t B, int64_t nf, int64_t L_for_grid, double fps, float* out_dev,
                                 void* stream) {
    const char* who = "km_egemaps_llds_from_records";
    if (!egm::set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "%s: feature set %d, 0 (eGeMAPS) or 1 (GeMAPS)", who, (int)feature_set);
    if (!rec_dev || !out_dev || B <= 0) return fail(KM_ERR_INVALID_ARG, "%s: bad argument", who);
    if (nf < 1) return fail(KM_ERR_INVALID_ARG, "%s: %lld frames per window, at least 1", who, (long long)nf);
    if (nf > egm::LLD_MAXF) return fail(KM_ERR_UNSUPPORTED, "%s: %lld frames per window, at most %d (65.5 s)", who, (long long)nf, egm::LLD_MAXF);
    if (B > 65535) return fail(KM_ERR_UNSUPPORTED, "%s: at most 65535 windows per call", who);
    int64_t T_out = nf;
    if (fps != 0.0) {
        T_out = egm_lld_frames(L_for_grid, fps);
        if (T_out < 0) return fail(KM_ERR_INVALID_ARG, "%s: fps %g, finite and within 1 .. 400 (0: the native 100 Hz)", who, fps);
        if (L_for_grid > egm::MAX_LLD_GRID) return fail(KM_ERR_UNSUPPORTED, "%s: a grid for %lld samples, at most %lld (65.5 s)", who, (long long)L_for_grid, (long long)egm::MAX_LLD_GRID);
    }
    if (T_out == 0) return KM_OK;                                        // an empty grid: nothing to launch
    return egm_lld(rec_dev, (int)nf, (int)nf, (int)B, T_out, fps, out_dev, (hipStream_t)stream, feature_set);
}

}  // extern "C"
