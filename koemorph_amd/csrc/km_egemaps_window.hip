// The two eGeMAPS kernels that hold a whole window in LDS -- pitch track and functionals -- written once and compiled for two capacity
// tiers (km_egemaps_window.h).  The other three kernels (peak, frame, voiced: km_egemaps.hip) work per frame and take any frame count.
//
//   ShortTier   2048 frames (20.5 s): every plain entry point and object.  59 KB (track) and 24 KB (functionals) of LDS.
//   LongTier    6548 frames, a window of 2^20 samples (65.5 s), the limit of the `basic` back end: the `_long` entry points and objects.
//               The long_context variant of the reference (configs/model/dual_stream.yaml: 30 s context, 0.2 s updates) has 2995
//               frames per window.  118 KB and 83 KB (gfx950: 160 KB per workgroup).
// The window lives in DYNAMIC LDS carved at constexpr offsets; only the long tier is beyond 64 KB and needs the function attribute.
//
//   egm_viterbi_kernel     per window: pitch track over the candidates (sequential dynamic programme, 4 states).  The seven inputs of
//                          a step are staged in chunks of Tier::CHUNK frames -- for 6548 frames they would be 183 KB, a chunk of 4096
//                          is 112 KB; the short tier's chunk is its whole window, a single pass.  The back pointers of the WHOLE
//                          window stay in LDS, a byte per frame, for the backtrack.
//   egm_functional_kernel  per window: 3-frame smoothing, means / normalised deviations / percentiles (bitonic sort in LDS) / slopes of
//                          rising and falling parts over voiced, unvoiced or all frames, in fixed orders: 256-stride partial sums
//                          through block_sum, serial compaction and slope scan, segment scan.  Three arrays of Tier::MAXF floats, the
//                          sort buffer padded to Tier::SORT_MAX.
// The order of the float32 operations is the contract (the tests pin bits).  Nothing in the arithmetic depends on the tier: at any frame
// count up to 2048 the long tier gives, on the same records, the short tier's bits (tests/test_gpu_egemaps_long.py) -- chunking and the
// sort's capacity are where they differ.
#include <hip/hip_runtime.h>

#include "km_context.h"
#include "km_egemaps_dev.h"
#include "km_egemaps_window.h"

namespace km {

__device__ __forceinline__ void bitonic_sort(float* s, int n2) {      // ascending, n2 a power of two, padding = +inf
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

// pitch track over the candidates: states 0..2 = candidate, 3 = unvoiced.  One thread per window walks the frames; the back pointers
// live in the bp LDS array (two bits per state), which the backtrack then overwrites with the chosen state.
template <bool RAGGED, class Tier>
__global__ __launch_bounds__(256) void egm_viterbi_kernel(float* __restrict__ recs, int nf, int rec_frames, const EgmSlot* __restrict__ slots) {
    using namespace egm;
    constexpr int MAXF = Tier::MAXF, CHUNK = Tier::CHUNK;
    static_assert(track_lds<Tier>() <= 160 * 1024, "gfx950: 160 KB of LDS per workgroup");
    // The recursion itself is sequential (thread 0), but its inputs are not: all threads first gather the seven numbers a step needs --
    // voicing flag, log2 of the three candidate frequencies, their strengths -- into LDS, so that the walk reads LDS instead of paying
    // a global round trip per frame (2.7 ms -> 0.2 ms per call), and write the chosen F0 back together at the end.  Beyond CHUNK frames:
    // all threads gather a chunk, thread 0 walks it out of LDS, repeat; costs and the previous frame's log-frequencies stay in thread
    // 0's registers across chunks.
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

// functionals: one workgroup per window.  SET (km_egemaps_dev.h): the GeMAPS instantiations skip the seven contours none of their 62
// values reads (flux, MFCC 1-4, the bandwidths of F2 and F3) and the RMS sum of the sound level, and write the values they keep at
// stride 62, at the place out_col gives; each value is computed by the statements that compute it among the 88.
template <bool RAGGED, class Tier, int SET>
__global__ __launch_bounds__(256) void egm_functional_kernel(const float* __restrict__ recs, int nf, int rec_frames, const EgmSlot* __restrict__ slots,
                                                             float* __restrict__ out) {
    using namespace egm;
    constexpr int MAXF = Tier::MAXF, SORT_MAX = Tier::SORT_MAX;
    constexpr bool FULL = SET == SET_EGEMAPS;
    static_assert(func_lds<Tier>() <= 160 * 1024, "gfx950: 160 KB of LDS per workgroup");
    static_assert(MAXF <= SORT_MAX && (SORT_MAX & (SORT_MAX - 1)) == 0, "the sort buffer holds every frame of the longest window");
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
    float* o = out + (int64_t)blockIdx.x * set_width(SET);
    auto col = [](int c) { return FULL ? c : gemaps_pos(c); };           // where eGeMAPS column c is written
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
        const float sum = block_sum(a0, red);
        const int n = (int)block_sum((float)n0, red);
        m = n ? sum / n : 0.f;
        float a1 = 0.f;
        for (int t = tid; t < nf; t += 256) { const bool vo = f0s[t] > 0.f; if (sel == 0 || (sel == 1) == vo) { const float dd = v[t] - m; a1 += dd * dd; } }
        const float var = block_sum(a1, red);
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
            // slopes of the rising / falling parts (cut at local extrema).  Their spread is accumulated as a running mean and
            // a running sum of squared deviations (Welford): E[x^2] - E[x]^2 in float32 leaves the rounding of x^2 behind, and
            // its square root is 2e-4 of the slope where the true deviation is zero (a single part, equal parts)
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
        if (n2 > 1) bitonic_sort(s, n2);
        if (tid == 0) {
            // percentile p = pn / pd at position p (n - 1).  Up to 2048 frames the position is the float32 product.  Beyond, float32
            // numbers near the position are 2.4e-4 to 4.9e-4 apart, and that times the gap between two sorted neighbours -- 7 loudness
            // units between the clusters of a speech-like window of 30 s -- was 4.7 times the tolerance of the class: there the
            // position is the exact quotient, integer part and remainder.  A condition on the window, not on the tier: the long tier
            // at 2048 frames or fewer keeps giving the short tier's bits
            auto pct = [&](float p) {
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
            if (nf > ShortTier::MAXF) { p20 = pct_exact(1, 5); p50 = pct_exact(1, 2); p80 = pct_exact(4, 5); }
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
        const float npk = block_sum(pk, red);
        if (tid == 0) o[col(81)] = npk / (nf * (float)HOP / SR);
    }
    if constexpr (FULL) {
        load(R_FLUX, 0);
        mean_sn(0, m, sn); if (tid == 0) { o[20] = m; o[21] = sn; }
        mean_sn(1, m, sn); if (tid == 0) { o[66] = m; o[67] = sn; }
        mean_sn(2, m, sn); if (tid == 0) o[80] = m;
        for (int i = 0; i < 4; ++i) {
            load(R_MFCC + i, 0);
            mean_sn(0, m, sn); if (tid == 0) { o[22 + 2 * i] = m; o[23 + 2 * i] = sn; }
            mean_sn(1, m, sn); if (tid == 0) { o[68 + 2 * i] = m; o[69 + 2 * i] = sn; }
        }
    }
    {
        const int fields[14] = {R_JIT, R_SHIM, R_HNR, R_H1H2, R_H1A3, R_F, R_BW, R_FAMP, R_F + 1, R_BW + 1, R_FAMP + 1, R_F + 2, R_BW + 2, R_FAMP + 2};
        for (int i = 0; i < 14; ++i) {
            if (!FULL && (fields[i] == R_BW + 1 || fields[i] == R_BW + 2)) continue;
            load(fields[i], 1);
            mean_sn(1, m, sn); if (tid == 0) { o[col(30 + 2 * i)] = m; o[col(31 + 2 * i)] = sn; }
        }
        const int spec[4] = {R_ALPHA, R_HAMM, R_SL0, R_SL1};
        for (int i = 0; i < 4; ++i) {
            load(spec[i], 0);
            mean_sn(1, m, sn); if (tid == 0) { o[col(58 + 2 * i)] = m; o[col(59 + 2 * i)] = sn; }
            mean_sn(2, m, sn); if (tid == 0) o[col(76 + i)] = m;
        }
    }
    // voiced / unvoiced segments and the equivalent sound level
    {
        float es = 0.f;
        if constexpr (FULL) {
            float e2 = 0.f;
            for (int t = tid; t < nf; t += 256) { const float r = raw(t, R_RMS); e2 += r * r; }
            es = block_sum(e2, red);
        }
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
            o[col(82)] = vn / dur;
            o[col(83)] = vn ? vs / vn * fr : 0.f;
            o[col(84)] = vn ? sqrtf(fmaxf(vq / vn - (vs / vn) * (vs / vn), 0.f)) * fr : 0.f;
            o[col(85)] = un ? us / un * fr : 0.f;
            o[col(86)] = un ? sqrtf(fmaxf(uq / un - (us / un) * (us / un), 0.f)) * fr : 0.f;
            if constexpr (FULL) o[87] = 10.0f * log10f(fmaxf(es / nf, 1e-12f));
        }
    }
}

int egm_window_prepare() {
    using namespace egm;
    static PerDeviceOnce once;
    int device = -1;
    HIP_TRY(hipGetDevice(&device));
    if (!once.first(device)) return KM_OK;
    constexpr hipFuncAttribute attr = hipFuncAttributeMaxDynamicSharedMemorySize;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_viterbi_kernel<false, LongTier>), attr, track_lds<LongTier>()));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_viterbi_kernel<true, LongTier>), attr, track_lds<LongTier>()));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_functional_kernel<false, LongTier, SET_EGEMAPS>), attr, func_lds<LongTier>()));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_functional_kernel<true, LongTier, SET_EGEMAPS>), attr, func_lds<LongTier>()));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_functional_kernel<false, LongTier, SET_GEMAPS>), attr, func_lds<LongTier>()));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&egm_functional_kernel<true, LongTier, SET_GEMAPS>), attr, func_lds<LongTier>()));
    return KM_OK;
}

static int window_check(const char* who, const void* rec, const void* out, int nf, int rec_frames, const EgmSlot* slots, int n, bool long_tier) {
    using namespace egm;
    if (!rec || !out || n < 1 || n > 65535 || rec_frames < 1 || rec_frames > (long_tier ? LongTier::MAXF : ShortTier::MAXF) ||
        (!slots && (nf < 1 || nf > rec_frames)))
        return fail(KM_ERR_INVALID_ARG, "%s: bad argument", who);
    return long_tier ? egm_window_prepare() : KM_OK;
}

template <class Tier>
static void launch_track(float* rec, int nf, int rec_frames, const EgmSlot* slots, int n, hipStream_t st) {
    constexpr int lds = egm::track_lds<Tier>();
    if (slots) hipLaunchKernelGGL((egm_viterbi_kernel<true, Tier>), dim3((unsigned)n), dim3(256), lds, st, rec, 0, rec_frames, slots);
    else hipLaunchKernelGGL((egm_viterbi_kernel<false, Tier>), dim3((unsigned)n), dim3(256), lds, st, rec, nf, rec_frames, (const EgmSlot*)nullptr);
}

template <class Tier, int SET>
static void launch_functional(const float* rec, int nf, int rec_frames, const EgmSlot* slots, int n, float* out, hipStream_t st) {
    constexpr int lds = egm::func_lds<Tier>();
    if (slots) hipLaunchKernelGGL((egm_functional_kernel<true, Tier, SET>), dim3((unsigned)n), dim3(256), lds, st, rec, 0, rec_frames, slots, out);
    else hipLaunchKernelGGL((egm_functional_kernel<false, Tier, SET>), dim3((unsigned)n), dim3(256), lds, st, rec, nf, rec_frames, (const EgmSlot*)nullptr, out);
}

int egm_track(float* rec_dev, int nf, int rec_frames, const EgmSlot* slots_dev, int n, bool long_tier, hipStream_t st) {
    if (const int rc = window_check("egm_track", rec_dev, rec_dev, nf, rec_frames, slots_dev, n, long_tier)) return rc;
    if (long_tier) launch_track<egm::LongTier>(rec_dev, nf, rec_frames, slots_dev, n, st);
    else launch_track<egm::ShortTier>(rec_dev, nf, rec_frames, slots_dev, n, st);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int egm_functional(const float* rec_dev, int nf, int rec_frames, const EgmSlot* slots_dev, int n, float* out_dev, bool long_tier, hipStream_t st,
                   int feature_set) {
    using namespace egm;
    if (!set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "egm_functional: feature set %d", feature_set);
    if (const int rc = window_check("egm_functional", rec_dev, out_dev, nf, rec_frames, slots_dev, n, long_tier)) return rc;
    if (feature_set == SET_GEMAPS) {
        if (long_tier) launch_functional<LongTier, SET_GEMAPS>(rec_dev, nf, rec_frames, slots_dev, n, out_dev, st);
        else launch_functional<ShortTier, SET_GEMAPS>(rec_dev, nf, rec_frames, slots_dev, n, out_dev, st);
    } else if (long_tier) launch_functional<LongTier, SET_EGEMAPS>(rec_dev, nf, rec_frames, slots_dev, n, out_dev, st);
    else launch_functional<ShortTier, SET_EGEMAPS>(rec_dev, nf, rec_frames, slots_dev, n, out_dev, st);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" {

// The two kernels that are pure functions of the record array, on records the caller wrote (tests): the same kernels, the same launch
// shape as in km_egemaps_functionals, no copy.  The plain hooks run the short tier; the `_long` hooks ALWAYS the long tier, at 1 to
// 6548 frames, so that its bits can be held against the short tier's up to 2048.
static int check_records(const char* who, const void* rec, const void* out, int64_t B, int64_t nf, int cap, const char* seconds_text) {
    if (!rec || !out || B <= 0) return fail(KM_ERR_INVALID_ARG, "%s: bad argument", who);
    if (nf < 1) return fail(KM_ERR_INVALID_ARG, "%s: %lld frames per window, at least 1", who, (long long)nf);
    if (nf > cap) return fail(KM_ERR_UNSUPPORTED, "%s: %lld frames per window, at most %d (%s)", who, (long long)nf, cap, seconds_text);
    if (B > 65535) return fail(KM_ERR_UNSUPPORTED, "%s: at most 65535 windows per call", who);
    return KM_OK;
}

int km_egemaps_track_from_records(float* rec_dev, int64_t B, int64_t nf, void* stream) {
    if (const int rc = check_records("km_egemaps_track_from_records", rec_dev, rec_dev, B, nf, egm::ShortTier::MAXF, "20.5 s")) return rc;
    return egm_track(rec_dev, (int)nf, (int)nf, nullptr, (int)B, false, (hipStream_t)stream);
}

int km_egemaps_functionals_from_records(const float* rec_dev, int64_t B, int64_t nf, float* out_dev, void* stream) {
    if (const int rc = check_records("km_egemaps_functionals_from_records", rec_dev, out_dev, B, nf, egm::ShortTier::MAXF, "20.5 s")) return rc;
    return egm_functional(rec_dev, (int)nf, (int)nf, nullptr, (int)B, out_dev, false, (hipStream_t)stream);
}

int km_egemaps_track_from_records_long(float* rec_dev, int64_t B, int64_t nf, void* stream) {
    if (const int rc = check_records("km_egemaps_track_from_records_long", rec_dev, rec_dev, B, nf, egm::LongTier::MAXF, "65.5 s")) return rc;
    return egm_track(rec_dev, (int)nf, (int)nf, nullptr, (int)B, true, (hipStream_t)stream);
}

int km_egemaps_functionals_from_records_long(const float* rec_dev, int64_t B, int64_t nf, float* out_dev, void* stream) {
    if (const int rc = check_records("km_egemaps_functionals_from_records_long", rec_dev, out_dev, B, nf, egm::LongTier::MAXF, "65.5 s")) return rc;
    return egm_functional(rec_dev, (int)nf, (int)nf, nullptr, (int)B, out_dev, true, (hipStream_t)stream);
}

int km_feature_set_width(int32_t feature_set) { return egm::set_width(feature_set); }

// either hook above for either feature set: out_dev is (B, km_feature_set_width); long_windows != 0 ALWAYS runs the long tier
int km_egemaps_functionals_from_records_set(int32_t feature_set, int32_t long_windows, const float* rec_dev, int64_t B, int64_t nf, float* out_dev,
                                            void* stream) {
    const char* who = "km_egemaps_functionals_from_records_set";
    if (!egm::set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "%s: feature set %d, 0 (eGeMAPS) or 1 (GeMAPS)", who, (int)feature_set);
    if (const int rc = long_windows ? check_records(who, rec_dev, out_dev, B, nf, egm::LongTier::MAXF, "65.5 s")
                                    : check_records(who, rec_dev, out_dev, B, nf, egm::ShortTier::MAXF, "20.5 s"))
        return rc;
    return egm_functional(rec_dev, (int)nf, (int)nf, nullptr, (int)B, out_dev, long_windows != 0, (hipStream_t)stream, feature_set);
}

}  // extern "C"
