// eGeMAPS windows beyond 2048 frames (20.5 s): the two per-window kernels of km_egemaps.hip -- pitch track and functionals -- for up
// to 6548 frames, a window of 2^20 samples (65.5 s), the limit of the `basic` back end.  The long_context variant of the reference
// (configs/model/dual_stream.yaml: 30 s context, 0.2 s updates) has 2995 frames per window.
//
// The other three kernels (peak, frame, voiced) work per frame and take any frame count; only these two hold a window in LDS.  Here
// the window lives in DYNAMIC LDS (gfx950: 160 KB per workgroup):
//   egm_long_viterbi_kernel     the recursion of egm_viterbi_kernel statement for statement.  The seven inputs of a step for 6548
//                               frames would be 183 KB, so they are staged in chunks of 4096 frames (112 KB): all threads gather a
//                               chunk, thread 0 walks it out of LDS, repeat; costs and the previous frame's log-frequencies stay in
//                               thread 0's registers across chunks.  The back pointers of the WHOLE window stay in LDS, a byte per
//                               frame, for the backtrack.  118 KB.
//   egm_long_functional_kernel  egm_functional_kernel's arithmetic in its fixed orders (256-stride partial sums through block_sum,
//                               serial compaction and slope scan, segment scan) on three contours of 6548 floats, the sort padded
//                               to 8192.  83 KB.  One statement differs beyond 2048 frames: the position of a percentile is an exact
//                               quotient there, not a float32 product (see pct).
// At any frame count up to 2048 both give, on the same records, the bits of the kernels they restate (tests/test_gpu_egemaps_long.py);
// a translation unit of their own keeps the register allocation of the five existing kernels where it is.
#include <hip/hip_runtime.h>

#include "km_context.h"
#include "km_egemaps_long.h"

namespace km {

namespace egml {
constexpr int SR = 16000, HOP = 160;
enum Rec { R_LOUD = 0, R_ALPHA, R_HAMM, R_SL0, R_SL1, R_FLUX, R_MFCC, R_RMS = 10, R_CF = 11, R_CS = 14, R_VOI = 17, R_F = 18, R_BW = 21,
           R_F0 = 24, R_JIT, R_SHIM, R_HNR, R_H1H2, R_H1A3, R_FAMP = 30 };                 // egm::Rec (km_egemaps.hip)
constexpr float VOICING_CUTOFF = 0.55f, RMS_FLOOR = 0.001f;
constexpr int BP_BYTES = (MAXF + 15) / 16 * 16;
constexpr int TRACK_LDS = 7 * CHUNK * (int)sizeof(float) + BP_BYTES;
constexpr int FUNC_LDS = (2 * MAXF + SORT_MAX) * (int)sizeof(float);
static_assert(TRACK_LDS <= 160 * 1024 && FUNC_LDS <= 160 * 1024, "gfx950: 160 KB of LDS per workgroup");
static_assert(MAXF <= SORT_MAX && MAXF == 6548, "the sort buffer holds every frame of the longest window");
}  // namespace egml

// block_sum of km_egemaps.hip: an xor butterfly inside each wave, then the four wave results in wave order
__device__ __forceinline__ float egml_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float egml_block_sum(float v, float* red) {
    v = egml_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ void egml_bitonic_sort(float* s, int n2) {      // ascending, n2 a power of two, padding = +inf
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool up = (i & k) == 0;
                    const float x = s[i], y = s[ixj];
                    if ((x > y) == up) { s[i] = y; s[ixj] = x; }
                }
            }
            __syncthreads();
        }
}

// pitch track over the candidates: states 0..2 = candidate, 3 = unvoiced (egm_viterbi_kernel)
template <bool RAGGED>
__global__ __launch_bounds__(256) void egm_long_viterbi_kernel(float* __restrict__ recs, int nf, int rec_frames, const EgmSlot* __restrict__ slots) {
    using namespace egml;
    extern __shared__ float dyn[];
    float* in = dyn;                                                     // [7][CHUNK]: [0] voiced-ok, [1..3] log2 f (or -1), [4..6] strength
    unsigned char* bp = reinterpret_cast<unsigned char*>(dyn + 7 * CHUNK);   // [MAXF] back pointers (two bits per state), then the chosen state
    if constexpr (RAGGED) {
        const EgmSlot sl = slots[blockIdx.x];
        if (sl.stream < 0) return;
        nf = sl.nf;
    }
    if (nf > MAXF) return;                                               // refused on the host; never index past the LDS arrays
    float* rec = recs + (int64_t)blockIdx.x * rec_frames * REC;
    const float w_local = 2.0f, w_vv = 10.0f, w_vuv = 10.0f / 8.0f, w_thr = 4.0f, INF = 1e30f;
    float cost[4], lf_prev[3] = {0.f, 0.f, 0.f};                         // thread 0's, carried from chunk to chunk
    for (int t0 = 0; t0 < nf; t0 += CHUNK) {
        const int n = nf - t0 < CHUNK ? nf - t0 : CHUNK;
        for (int i = threadIdx.x; i < n; i += 256) {
            const float* r = rec + (int64_t)(t0 + i) * REC;
            in[i] = (r[R_VOI] >= VOICING_CUTOFF && r[R_RMS] >= RMS_FLOOR) ? 1.f : 0.f;
            for (int c = 0; c < 3; ++c) {
                const float f = r[R_CF + c];
                in[(1 + c) * CHUNK + i] = f > 0.f ? log2f(f) : -1.f;     // candidates are >= 25 Hz: log2 > 0
                in[(4 + c) * CHUNK + i] = r[R_CS + c];
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 0; i < n; ++i) {
                const int t = t0 + i;
                const bool vok = in[i] != 0.f;
                float loc[4], lf[3];
                for (int c = 0; c < 3; ++c) {
                    const float l2 = in[(1 + c) * CHUNK + i];
                    const bool has = l2 >= 0.f;
                    lf[c] = has ? l2 : 0.f;
                    loc[c] = has ? w_local * (1.0f - in[(4 + c) * CHUNK + i]) + (vok ? 0.f : w_thr) : INF;
                }
                loc[3] = vok ? w_thr : 0.f;
                float nc[4];
                int packed = 0;                                   // back pointers: two bits per state
                for (int s = 0; s < 4; ++s) {
                    if (t == 0) { nc[s] = loc[s]; continue; }
                    if (loc[s] >= INF) { nc[s] = INF; continue; }
                    float best = INF; int arg = 0;
                    for (int p = 0; p < 4; ++p) {
                        if (cost[p] >= INF) continue;
                        const float tr = (s < 3 && p < 3) ? w_vv * fabsf(lf[s] - lf_prev[p]) : ((s == 3 && p == 3) ? 0.f : w_vuv);
                        const float v = cost[p] + tr;
                        if (v < best) { best = v; arg = p; }
                    }
                    nc[s] = best + loc[s];
                    packed |= arg << (2 * s);
                }
                bp[t] = (unsigned char)packed;
                for (int s = 0; s < 4; ++s) cost[s] = nc[s];
                for (int c = 0; c < 3; ++c) lf_prev[c] = lf[c];
            }
        }
        __syncthreads();                                          // the walk is done with the chunk before the next gather overwrites it
    }
    if (threadIdx.x == 0) {
        int s = 0;
        for (int q = 1; q < 4; ++q) if (cost[q] < cost[s]) s = q;
        for (int t = nf - 1; t >= 0; --t) {
            const int packed = bp[t];
            bp[t] = (unsigned char)s;                             // the state chosen for frame t
            s = (packed >> (2 * s)) & 3;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nf; t += 256) {
        float* r = rec + (int64_t)t * REC;
        const int st = bp[t];
        r[R_F0] = st < 3 ? r[R_CF + st] : 0.f;
    }
}

// functionals: one workgroup per window (egm_functional_kernel)
template <bool RAGGED>
__global__ __launch_bounds__(256) void egm_long_functional_kernel(const float* __restrict__ recs, int nf, int rec_frames,
                                                                  const EgmSlot* __restrict__ slots, float* __restrict__ out) {
    using namespace egml;
    extern __shared__ float dyn[];
    float* v = dyn;                       // [MAXF] contour (smoothed)
    float* f0s = dyn + MAXF;              // [MAXF] smoothed F0
    float* s = dyn + 2 * MAXF;            // [SORT_MAX] sort buffer
    __shared__ float red[256], res[16];
    __shared__ int cnt_s[4];
    const int tid = threadIdx.x;
    if constexpr (RAGGED) {
        const EgmSlot sl = slots[blockIdx.x];
        if (sl.stream < 0) return;
        nf = sl.nf;
    }
    if (nf > MAXF) return;                                               // refused on the host; never index past the LDS arrays
    const float* rec = recs + (int64_t)blockIdx.x * rec_frames * REC;
    float* o = out + (int64_t)blockIdx.x * 88;
    auto raw = [&](int t, int field) { return rec[(int64_t)t * REC + field]; };
    // smoothed F0 (non-zero smoothing) defines the voiced frames
    for (int t = tid; t < nf; t += 256) {
        const float c = raw(t, R_F0);
        float acc = 0.f; int n = 0;
        if (c != 0.f)
            for (int q = (t > 0 ? t - 1 : 0); q <= (t + 1 < nf ? t + 1 : nf - 1); ++q) { const float x = raw(q, R_F0); if (x != 0.f) { acc += x; ++n; } }
        f0s[t] = n ? acc / n : 0.f;
    }
    __syncthreads();
    // load a contour: mode 0 plain 3-frame average, 1 non-zero average of the values masked to voiced frames, 2 semitone of f0s
    auto load = [&](int field, int mode) {
        for (int t = tid; t < nf; t += 256) {
            float r = 0.f;
            if (mode == 2) r = f0s[t] > 0.f ? 12.0f * log2f(f0s[t] / 27.5f) : 0.f;
            else if (mode == 0) {
                float acc = 0.f; int n = 0;
                for (int q = (t > 0 ? t - 1 : 0); q <= (t + 1 < nf ? t + 1 : nf - 1); ++q) { acc += raw(q, field); ++n; }
                r = acc / n;
            } else {
                const float c = f0s[t] > 0.f ? raw(t, field) : 0.f;
                if (c != 0.f) {
                    float acc = 0.f; int n = 0;
                    for (int q = (t > 0 ? t - 1 : 0); q <= (t + 1 < nf ? t + 1 : nf - 1); ++q) {
                        const float x = f0s[q] > 0.f ? raw(q, field) : 0.f;
                        if (x != 0.f) { acc += x; ++n; }
                    }
                    r = acc / n;
                }
            }
            v[t] = r;
        }
        __syncthreads();
    };
    // mean and normalised standard deviation over frames selected by sel: 0 all, 1 voiced, 2 unvoiced
    auto mean_sn = [&](int sel, float& m, float& sn) {
        float a0 = 0.f; int n0 = 0;
        for (int t = tid; t < nf; t += 256) { const bool vo = f0s[t] > 0.f; if (sel == 0 || (sel == 1) == vo) { a0 += v[t]; ++n0; } }
        const float sum = egml_block_sum(a0, red);
        const int n = (int)egml_block_sum((float)n0, red);
        m = n ? sum / n : 0.f;
        float a1 = 0.f;
        for (int t = tid; t < nf; t += 256) { const bool vo = f0s[t] > 0.f; if (sel == 0 || (sel == 1) == vo) { const float dd = v[t] - m; a1 += dd * dd; } }
        const float var = egml_block_sum(a1, red);
        sn = (n && m != 0.f) ? sqrtf(var / n) / fabsf(m) : 0.f;
    };
    // the ten functionals of a contour over the selected frames -> o[base .. base + 9]
    auto ten = [&](int sel, int base) {
        float m, sn;
        mean_sn(sel, m, sn);
        // compact the selected values (order preserved) into s by thread 0 -- also the scan for slopes
        if (tid == 0) {
            int n = 0;
            for (int t = 0; t < nf; ++t) { const bool vo = f0s[t] > 0.f; if (sel == 0 || (sel == 1) == vo) s[n++] = v[t]; }
            cnt_s[0] = n;
            // slopes of the rising / falling parts (cut at local extrema), their spread as a running mean and a running sum of
            // squared deviations (Welford), as egm_functional_kernel says why
            float rs = 0.f, rm = 0.f, rq = 0.f, fs = 0.f, fm = 0.f, fq = 0.f; int rn = 0, fn = 0;
            if (n >= 2) {
                int start = 0;
                for (int t = 1; t < n; ++t) {
                    const bool last = t == n - 1;
                    const bool turn = !last && ((s[t] - s[t - 1]) * (s[t + 1] - s[t]) < 0.f);
                    if (turn || last) {
                        const float dv = s[t] - s[start];
                        const float sl = dv / ((t - start) * (float)HOP / SR);
                        if (dv > 0.f) { rs += sl; ++rn; const float d = sl - rm; rm += d / rn; rq += d * (sl - rm); }
                        else if (dv < 0.f) { fs += sl; ++fn; const float d = sl - fm; fm += d / fn; fq += d * (sl - fm); }
                        start = t;
                    }
                }
            }
            res[0] = rn ? rs / rn : 0.f; res[1] = rn ? sqrtf(fmaxf(rq / rn, 0.f)) : 0.f;
            res[2] = fn ? fs / fn : 0.f; res[3] = fn ? sqrtf(fmaxf(fq / fn, 0.f)) : 0.f;
        }
        __syncthreads();
        const int n = cnt_s[0];
        int n2 = 1;
        while (n2 < n) n2 <<= 1;
        for (int i = n + tid; i < n2; i += 256) s[i] = INFINITY;
        __syncthreads();
        if (n2 > 1) egml_bitonic_sort(s, n2);
        if (tid == 0) {
            // percentile p = pn / pd at position p (n - 1).  Up to 2048 frames the position is egm_functional_kernel's float32 product
            // (equal bits).  Beyond, float32 numbers near the position are 2.4e-4 to 4.9e-4 apart, and that times the gap between two
            // sorted neighbours -- 7 loudness units between the clusters of a speech-like window of 30 s -- was 4.7 times the tolerance
            // of the class: there the position is the exact quotient, integer part and remainder
            auto pct = [&](float p) {                               // egm_functional_kernel's
                if (n == 0) return 0.f;
                const float pos = p * (n - 1);
                const int i = (int)floorf(pos); const float fr = pos - i;
                return i + 1 >= n ? s[i] : s[i] * (1.f - fr) + s[i + 1] * fr;
            };
            auto pct_exact = [&](int pn, int pd) {
                if (n == 0) return 0.f;
                const int q = pn * (n - 1), i = q / pd;
                const float fr = (float)(q - i * pd) / pd;
                return i + 1 >= n ? s[i] : s[i] * (1.f - fr) + s[i + 1] * fr;
            };
            float p20, p50, p80;
            if (nf > MAXF_SHORT) { p20 = pct_exact(1, 5); p50 = pct_exact(1, 2); p80 = pct_exact(4, 5); }
            else { p20 = pct(0.2f); p50 = pct(0.5f); p80 = pct(0.8f); }
            o[base] = m; o[base + 1] = sn; o[base + 2] = p20; o[base + 3] = p50; o[base + 4] = p80; o[base + 5] = p80 - p20;
            o[base + 6] = res[0]; o[base + 7] = res[1]; o[base + 8] = res[2]; o[base + 9] = res[3];
        }
        __syncthreads();
    };
    float m, sn;
    load(R_F0, 2); ten(1, 0);
    load(R_LOUD, 0); ten(0, 10);
    // loudness peaks (local maxima of the smoothed contour)
    {
        float pk = 0.f;
        for (int t = 1 + tid; t + 1 < nf; t += 256) if (v[t] > v[t - 1] && v[t] >= v[t + 1]) pk += 1.f;
        const float npk = egml_block_sum(pk, red);
        if (tid == 0) o[81] = npk / (nf * (float)HOP / SR);
    }
    load(R_FLUX, 0);
    mean_sn(0, m, sn); if (tid == 0) { o[20] = m; o[21] = sn; }
    mean_sn(1, m, sn); if (tid == 0) { o[66] = m; o[67] = sn; }
    mean_sn(2, m, sn); if (tid == 0) o[80] = m;
    for (int i = 0; i < 4; ++i) {
        load(R_MFCC + i, 0);
        mean_sn(0, m, sn); if (tid == 0) { o[22 + 2 * i] = m; o[23 + 2 * i] = sn; }
        mean_sn(1, m, sn); if (tid == 0) { o[68 + 2 * i] = m; o[69 + 2 * i] = sn; }
    }
    {
        const int fields[14] = {R_JIT, R_SHIM, R_HNR, R_H1H2, R_H1A3, R_F, R_BW, R_FAMP, R_F + 1, R_BW + 1, R_FAMP + 1, R_F + 2, R_BW + 2, R_FAMP + 2};
        for (int i = 0; i < 14; ++i) {
            load(fields[i], 1);
            mean_sn(1, m, sn); if (tid == 0) { o[30 + 2 * i] = m; o[31 + 2 * i] = sn; }
        }
        const int spec[4] = {R_ALPHA, R_HAMM, R_SL0, R_SL1};
        for (int i = 0; i < 4; ++i) {
            load(spec[i], 0);
            mean_sn(1, m, sn); if (tid == 0) { o[58 + 2 * i] = m; o[59 + 2 * i] = sn; }
            mean_sn(2, m, sn); if (tid == 0) o[76 + i] = m;
        }
    }
    // voiced / unvoiced segments and the equivalent sound level
    {
        float e2 = 0.f;
        for (int t = tid; t < nf; t += 256) { const float r = raw(t, R_RMS); e2 += r * r; }
        const float es = egml_block_sum(e2, red);
        if (tid == 0) {
            float vs = 0.f, vq = 0.f, us = 0.f, uq = 0.f; int vn = 0, un = 0, run = 0; bool cur = false;
            for (int t = 0; t <= nf; ++t) {
                const bool vo = t < nf && f0s[t] > 0.f;
                if (t == nf || (run && vo != cur)) {
                    if (run) { const float len = (float)run; if (cur) { vs += len; vq += len * len; ++vn; } else { us += len; uq += len * len; ++un; } }
                    run = 0;
                }
                if (t < nf) { cur = vo; ++run; }
            }
            const float dur = nf * (float)HOP / SR, fr = (float)HOP / SR;
            o[82] = vn / dur;
            o[83] = vn ? vs / vn * fr : 0.f;
            o[84] = vn ? sqrtf(fmaxf(vq / vn - (vs / vn) * (vs / vn), 0.f)) * fr : 0.f;
            o[85] = un ? us / un * fr : 0.f;
            o[86] = un ? sqrtf(fmaxf(uq / un - (us / un) * (us / un), 0.f)) * fr : 0.f;
            o[87] = 10.0f * log10f(fmaxf(es / nf, 1e-12f));
        }
    }
}

int egm_long_prepare() {
    using namespace egml;
    static PerDeviceOnce once;
    int device = -1;
    HIP_TRY(hipGetDevice(&device));
    if (!once.first(device)) return KM_OK;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_long_viterbi_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, TRACK_LDS));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_long_viterbi_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, TRACK_LDS));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_long_functional_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, FUNC_LDS));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_long_functional_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, FUNC_LDS));
    return KM_OK;
}

static int egm_long_check(const char* who, const void* rec, const void* out, int nf, int rec_frames, const EgmSlot* slots, int n) {
    using namespace egml;
    if (!rec || !out || n < 1 || n > 65535 || rec_frames < 1 || rec_frames > MAXF || (!slots && (nf < 1 || nf > rec_frames)))
        return fail(KM_ERR_INVALID_ARG, "%s: bad argument", who);
    return egm_long_prepare();
}

int egm_long_track(float* rec_dev, int nf, int rec_frames, const EgmSlot* slots_dev, int n, hipStream_t st) {
    if (const int rc = egm_long_check("egm_long_track", rec_dev, rec_dev, nf, rec_frames, slots_dev, n)) return rc;
    if (slots_dev) hipLaunchKernelGGL(egm_long_viterbi_kernel<true>, dim3((unsigned)n), dim3(256), egml::TRACK_LDS, st, rec_dev, 0, rec_frames, slots_dev);
    else hipLaunchKernelGGL(egm_long_viterbi_kernel<false>, dim3((unsigned)n), dim3(256), egml::TRACK_LDS, st, rec_dev, nf, rec_frames, (const EgmSlot*)nullptr);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int egm_long_functional(const float* rec_dev, int nf, int rec_frames, const EgmSlot* slots_dev, int n, float* out_dev, hipStream_t st) {
    if (const int rc = egm_long_check("egm_long_functional", rec_dev, out_dev, nf, rec_frames, slots_dev, n)) return rc;
    if (slots_dev)
        hipLaunchKernelGGL(egm_long_functional_kernel<true>, dim3((unsigned)n), dim3(256), egml::FUNC_LDS, st, rec_dev, 0, rec_frames, slots_dev, out_dev);
    else
        hipLaunchKernelGGL(egm_long_functional_kernel<false>, dim3((unsigned)n), dim3(256), egml::FUNC_LDS, st, rec_dev, nf, rec_frames,
                           (const EgmSlot*)nullptr, out_dev);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" {

// The test hooks of km_egemaps_track_from_records / km_egemaps_functionals_from_records: ALWAYS the kernels of this file, at 1 to 6548
// frames, so that their bits can be held against the existing kernels' up to 2048.
static int check_records_long(const char* who, const void* rec, const void* out, int64_t B, int64_t nf) {
    if (!rec || !out || B <= 0) return fail(KM_ERR_INVALID_ARG, "%s: bad argument", who);
    if (nf < 1) return fail(KM_ERR_INVALID_ARG, "%s: %lld frames per window, at least 1", who, (long long)nf);
    if (nf > egml::MAXF) return fail(KM_ERR_UNSUPPORTED, "%s: %lld frames per window, at most %d (65.5 s)", who, (long long)nf, egml::MAXF);
    if (B > 65535) return fail(KM_ERR_UNSUPPORTED, "%s: at most 65535 windows per call", who);
    return KM_OK;
}

int km_egemaps_track_from_records_long(float* rec_dev, int64_t B, int64_t nf, void* stream) {
    if (const int rc = check_records_long("km_egemaps_track_from_records_long", rec_dev, rec_dev, B, nf)) return rc;
    return egm_long_track(rec_dev, (int)nf, (int)nf, nullptr, (int)B, (hipStream_t)stream);
}

int km_egemaps_functionals_from_records_long(const float* rec_dev, int64_t B, int64_t nf, float* out_dev, void* stream) {
    if (const int rc = check_records_long("km_egemaps_functionals_from_records_long", rec_dev, out_dev, B, nf)) return rc;
    return egm_long_functional(rec_dev, (int)nf, (int)nf, nullptr, (int)B, out_dev, (hipStream_t)stream);
}

}  // extern "C"
