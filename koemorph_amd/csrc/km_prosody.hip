// The `basic` prosodic emotion features on the device: the reference's EmotionExtractor._extract_basic
// (src/features/emotion_extractor.py:503-545), called once per batch row on the whole audio handed to forward (:280-300):
//   [energy, zcr, spectral_centroid, f0_mean, f0_std, mean, std, max, min], raw, no normalisation.
//
// PARITY UNPINNED.  The reference pins only librosa>=0.10.0 and the package is not part of this repository's environment: the
// arithmetic restates what librosa.feature.zero_crossing_rate, librosa.feature.spectral_centroid and librosa.yin(fmin=50,
// fmax=400) do at their 0.10 defaults (frame_length 2048, hop 512, centred; edge padding for the crossings, zero padding for the
// STFT and for yin) and has not been checked against the package by anyone.  What is tested is this file == the float64
// restatement in tests/prosody_cases.py, plus known answers.  One deliberate deviation: librosa obtains the difference function
// from an FFT autocorrelation and zeroes terms below 1e-6; here it is the direct sum of squared differences, which is well
// conditioned, equals librosa's wherever a frame's energy is far above 1e-6 and is exactly 0 on digital silence (f0 = 400
// there, as librosa gives).  Inputs are assumed finite.
//
// With y one window of L >= 1 samples at 16 kHz, F = 1 + L / 512 frames, frame f position n in [0, 2048) reading source index
// s = 512 f + n - 1024, z_f[n] = y[s] inside [0, L) and 0 outside, e_f[n] = y[clamp(s, 0, L - 1)]:
//   Z_f   = #{n in 1..2047 : neg(e_f[n]) != neg(e_f[n-1])} / 2048, neg(v) = v < -1e-10
//   C_f   = sum_k 7.8125 k |X_f[k]| / S_f, X_f = rfft(z_f * periodic Hann), S_f = sum_k |X_f[k]| (1 when below FLT_MIN)
//   d_f[t] = sum_{j=1..1024} (z_f[j] - z_f[j+t])^2 for t = 1..320; c_f[i] = d_f[40+i] / (sum_{t=1..40+i} d_f[t] / (40+i) + FLT_MIN),
//   i = 0..280; i* = the first trough of c below 0.1, else the first index of its minimum; parabolic shift where 0 < i* < 280 and
//   |b| < |a|; f0_f = 16000 / (40 + i* + shift)
//
//   pr_frame_kernel    one workgroup per (row, frame): the frame in LDS, the crossings, the 2048-point real FFT as one 1024-point
//                      complex FFT of the even / odd samples plus the split step, the 320 lags five to a lane (the z[j] read is a
//                      broadcast, the z[j + t] reads of a wave are 5 dwords apart: no two lanes of a 32-lane group on one bank),
//                      then c, the trough search and the interpolation; writes the record (Z_f, C_f, f0_f, i*).  The samples, the
//                      window, the FFT and |X| are float32; the lag sums, c, the interpolation and the centroid's two sums are double
//   pr_window_kernel   one workgroup per row: means of Z_f, C_f, f0_f, the two-pass deviation of f0_f, and energy, mean, two-pass
//                      deviation, max and min of the samples (float32 values summed in double)
// Every sum has a fixed order that depends on L and F only (strided per-thread partial sums, shuffle trees, a fixed tree over the
// waves); there are no atomics.  Rows come from one descriptor {offset, start, length, ring} -- dense rows, windows of a resident
// clip by a device table of start samples, or the slot table of km_emotion_stream's plan kernel -- and sample i is
// base[offset + (start + i) mod ring] (ring = 0: linear), so the three sources run the same arithmetic in the same order.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "km_context.h"
#include "km_prosody_ragged.h"

namespace km {

namespace pr {
constexpr int SR = 16000, NFFT = 2048, HOP = 512, NH = NFFT / 2, NB = NH + 1, NREC = 4, NOUT = 9;
constexpr int TMIN = 40, TMAX = 320, NC = TMAX - TMIN + 1;       // periods of fmax = 400 Hz and fmin = 50 Hz; 281 entries of c
constexpr int O_TW = NFFT;                                       // tables: window (2048) | W_2048^k, k < 1024, as (cos, -sin)
constexpr int TAB_FLOATS = NFFT + 2 * NH;
constexpr int64_t MAX_L = 1 << 20;
constexpr int WIN_THREADS = 512;
}  // namespace pr

struct PrPlan {
    DevBuf<float> tab;
};

// where the rows lie
struct PrSource {
    const float* base;
    int32_t mode;                // 0 dense rows, 1 windows of a clip, 2 ring slots
    int32_t L;                   // dense, windows: the nominal length
    int64_t row_stride;          // dense
    int64_t clip_len;            // windows
    const int32_t* starts;       // windows
    const EgmSlot* slots;        // slots
    int32_t ring_len;            // slots
};

struct PrDesc {
    int64_t offset;
    int32_t start, length, ring;                                 // length < 0: no row at all, nothing is written
};

__device__ __forceinline__ PrDesc pr_describe(const PrSource& s, int row) {
    PrDesc d{0, 0, -1, 0};
    if (s.mode == 0) {
        d.offset = (int64_t)row * s.row_stride; d.length = s.L;
    } else if (s.mode == 1) {
        const int64_t st = s.starts[row];
        if (st < 0 || st >= s.clip_len) { d.length = 0; return d; }
        const int64_t room = s.clip_len - st;
        d.offset = st; d.length = (int32_t)(room < s.L ? room : s.L);
    } else {
        const EgmSlot sl = s.slots[row];
        if (sl.stream < 0) return d;
        d.offset = (int64_t)sl.stream * s.ring_len; d.start = sl.start; d.length = sl.len; d.ring = s.ring_len;
    }
    return d;
}

__device__ __forceinline__ float pr_sample(const float* __restrict__ base, const PrDesc& d, int i) {     // 0 <= i < d.length
    int k = d.start + i;
    if (d.ring && k >= d.ring) k -= d.ring;
    return base[d.offset + k];
}

// ---- reductions in a fixed order: butterfly over the lanes, then a fixed tree over the waves ----
template <class T, class Op>
__device__ __forceinline__ T pr_wave(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
template <int WAVES, class T, class Op>
__device__ __forceinline__ T pr_block(T v, T* red, Op op) {
    v = pr_wave(v, op);
    __syncthreads();                                             // red may still be read from the reduction before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t[WAVES];
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t[w] = red[w];
#pragma unroll
    for (int n = WAVES; n > 1; n >>= 1)
#pragma unroll
        for (int w = 0; w < n / 2; ++w) t[w] = op(t[2 * w], t[2 * w + 1]);
    return t[0];
}
struct PrAdd { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct PrMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct PrMin { __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); } };

__device__ __forceinline__ int pr_bitrev10(int v) { return (int)(__brev((unsigned)v) >> 22); }

// in-place 1024-point complex FFT in LDS, radix-2 DIT on bit-reversed input; tw holds W_2048^k, so W_1024^j = tw[2 j]
__device__ __forceinline__ void pr_fft1024(float2* buf, const float2* tw) {
    const int tid = threadIdx.x;
    for (int s = 0; s < 10; ++s) {
        const int half = 1 << s;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = tid + 256 * r;
            const int j = i & (half - 1);
            const int base = ((i >> s) << (s + 1)) + j;
            const float2 w = tw[j << (10 - s)];
            const float2 a = buf[base], b = buf[base + half];
            const float2 bw = make_float2(b.x * w.x - b.y * w.y, b.x * w.y + b.y * w.x);
            buf[base] = make_float2(a.x + bw.x, a.y + bw.y);
            buf[base + half] = make_float2(a.x - bw.x, a.y - bw.y);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ bool pr_neg(float v) { return v < -1e-10f; }

__global__ __launch_bounds__(256) void pr_frame_kernel(PrSource src, const float* __restrict__ tab, float* __restrict__ rec, int max_frames) {
    using namespace pr;
    __shared__ __align__(16) float smem[3 * NFFT];
    float* z = smem;                                             // the zero-padded frame; with zb's head the lag sums of the four waves
    float2* zb = reinterpret_cast<float2*>(smem + NFFT);         // the edge-padded frame, then the FFT buffer
    float2* tw = reinterpret_cast<float2*>(smem + 2 * NFFT);     // the twiddles, then d, its running sum and c
    __shared__ float red[4];
    __shared__ double redd[4];
    const int tid = threadIdx.x, row = blockIdx.y, f = blockIdx.x;
    const PrDesc d = pr_describe(src, row);
    if (d.length <= 0 || f >= 1 + d.length / HOP) return;
    const float* __restrict__ base = src.base;
    const int L = d.length;

    // the frame, zero padded (z) and edge padded (e)
    float* e = reinterpret_cast<float*>(zb);
#pragma unroll
    for (int r = 0; r < NFFT / 256; ++r) {
        const int n = tid + 256 * r, s = HOP * f + n - NH;
        const float v = pr_sample(base, d, s < 0 ? 0 : (s >= L ? L - 1 : s));
        e[n] = v;
        z[n] = (s >= 0 && s < L) ? v : 0.f;
    }
    for (int k = tid; k < NH; k += 256) tw[k] = reinterpret_cast<const float2*>(tab + O_TW)[k];
    __syncthreads();

    // crossings: position 0 never counts
    float cnt = 0.f;
#pragma unroll
    for (int r = 0; r < NFFT / 256; ++r) {
        const int n = tid + 256 * r;
        if (n > 0 && pr_neg(e[n]) != pr_neg(e[n - 1])) cnt += 1.f;
    }
    const float Zf = pr_block<4>(cnt, red, PrAdd()) * (1.f / NFFT);                // a count <= 2047 over 2048: exact
    __syncthreads();                                                             // e is dead

    // rfft(z * w): Y[m] = z[2m] w[2m] + i z[2m+1] w[2m+1], then X[k] = E[k] + W_2048^k O[k]
    for (int m = tid; m < NH; m += 256)
        zb[pr_bitrev10(m)] = make_float2(z[2 * m] * tab[2 * m], z[2 * m + 1] * tab[2 * m + 1]);
    __syncthreads();
    pr_fft1024(zb, tw);
    double sm = 0.0, sw = 0.0;                                                   // float32 magnitudes, summed in double
    for (int k = tid; k < NB; k += 256) {
        const float2 y = zb[k & (NH - 1)], yc = zb[(NH - k) & (NH - 1)];
        const float2 w = k < NH ? tw[k] : make_float2(-1.f, 0.f);
        const float ar = 0.5f * (y.x + yc.x), ai = 0.5f * (y.y - yc.y);              // E = (Y[k] + conj Y[N-k]) / 2
        const float br = 0.5f * (y.y + yc.y), bi = -0.5f * (y.x - yc.x);             // O = (Y[k] - conj Y[N-k]) / (2i)
        const float xr = ar + (w.x * br - w.y * bi), xi = ai + (w.x * bi + w.y * br);
        const float mag = sqrtf(xr * xr + xi * xi);
        sm += (double)mag;
        sw += (double)((float)k * ((float)SR / NFFT)) * (double)mag;            // 7.8125 k is exact
    }
    double S = pr_block<4>(sm, redd, PrAdd());
    const double Wsum = pr_block<4>(sw, redd, PrAdd());
    if (S < (double)FLT_MIN) S = 1.0;
    const float Cf = (float)(Wsum / S);
    __syncthreads();                                                             // zb and tw are dead

    // d[t], t = 1..320: wave p sums j = 1 + 256 p .. 256 p + 256 in that order, lane l the lags 1 + 5 l .. 5 + 5 l.  The differences
    // and their squares are taken in double: a difference of two floats is exact there, and where c is flat around its minimum the
    // interpolated period moves by 1e4 times the relative error of d, which float32 sums (1e-7) would bring to 1e-5 of a sample.
    double* part = reinterpret_cast<double*>(smem);                              // (4, 320): 10240 bytes over z and the head of zb
    double* dl = reinterpret_cast<double*>(tw);                                  // dl[t - 1] = d[t]
    double* cum = dl + TMAX;                                                     // cum[t - 1] = d[1] + .. + d[t]
    double* c = cum + TMAX;                                                      // (281); 7368 of tw's 8192 bytes
    {
        const int p = tid >> 6, l = tid & 63, t0 = 1 + 5 * l;
        double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        const int jb = 1 + 256 * p;
#pragma unroll 2
        for (int u0 = 0; u0 < 256; u0 += 4) {
            const int j = jb + u0;
            double a[4], b[8];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = (double)z[j + u];
#pragma unroll
            for (int v = 0; v < 8; ++v) b[v] = (double)z[j + t0 + v];            // j + t0 + v <= 1021 + 316 + 7 < 2048
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < 5; ++k) { const double df = a[u] - b[u + k]; acc[k] = fma(df, df, acc[k]); }
        }
        __syncthreads();                                                         // every wave is done with z
#pragma unroll
        for (int k = 0; k < 5; ++k) part[p * TMAX + 5 * l + k] = acc[k];
    }
    __syncthreads();
    for (int t = tid; t < TMAX; t += 256)
        dl[t] = (part[t] + part[TMAX + t]) + (part[2 * TMAX + t] + part[3 * TMAX + t]);
    __syncthreads();
    if (tid < 64) {                                                              // running sum: five per lane, then a scan over the lanes
        double s[5];
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < 5; ++k) { run += dl[5 * tid + k]; s[k] = run; }
        double incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const double up = __shfl_up(incl, o, 64); if (tid >= o) incl += up; }
        const double before = __shfl_up(incl, 1, 64);
#pragma unroll
        for (int k = 0; k < 5; ++k) cum[5 * tid + k] = tid == 0 ? s[k] : before + s[k];
    }
    __syncthreads();
    for (int i = tid; i < NC; i += 256) {
        const int t = TMIN + i;
        c[i] = dl[t - 1] / (cum[t - 1] / (double)t + (double)FLT_MIN);
    }
    __syncthreads();
    if (tid < 64) {
        int first = NC, arg = NC;                                                // first trough below 0.1; first index of the minimum
        double best = INFINITY;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int i = 5 * tid + k;
            if (i < NC) {
                const double v = c[i];
                const bool trough = i == 0 ? v < c[1] : (i == NC - 1 ? v < c[NC - 2] : (v < c[i - 1] && v <= c[i + 1]));
                if (trough && v < 0.1 && first == NC) first = i;
                if (v < best) { best = v; arg = i; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int f2 = __shfl_xor(first, o, 64), a2 = __shfl_xor(arg, o, 64);
            const double b2 = __shfl_xor(best, o, 64);
            first = f2 < first ? f2 : first;
            if (b2 < best || (b2 == best && a2 < arg)) { best = b2; arg = a2; }
        }
        if (tid == 0) {
            const int is = first < NC ? first : arg;
            double shift = 0.0;
            if (is > 0 && is < NC - 1) {
                const double a = c[is + 1] + c[is - 1] - 2.0 * c[is], b = (c[is + 1] - c[is - 1]) * 0.5;
                if (fabs(b) < fabs(a)) shift = -b / a;
            }
            float* r = rec + ((int64_t)row * max_frames + f) * NREC;
            r[0] = Zf; r[1] = Cf; r[2] = (float)((double)SR / ((double)(TMIN + is) + shift)); r[3] = (float)is;
        }
    }
}

__global__ __launch_bounds__(pr::WIN_THREADS) void pr_window_kernel(PrSource src, const float* __restrict__ rec, int max_frames,
                                                                  float* __restrict__ out) {
    using namespace pr;
    constexpr int WV = WIN_THREADS / 64;
    __shared__ float red[WV];
    __shared__ double redd[WV];
    const int tid = threadIdx.x, row = blockIdx.x;
    const PrDesc d = pr_describe(src, row);
    if (d.length < 0) return;
    float* o = out + (int64_t)row * NOUT;
    if (d.length == 0) { if (tid < NOUT) o[tid] = 0.f; return; }
    const float* __restrict__ base = src.base;
    const int L = d.length, F = 1 + L / HOP;
    const float* r = rec + (int64_t)row * max_frames * NREC;

    // float32 values, summed in double: the results are the correctly rounded means of what the frame kernel wrote and of y
    double sz = 0.0, sc = 0.0, sf = 0.0;
    for (int f = tid; f < F; f += WIN_THREADS) { sz += (double)r[f * NREC]; sc += (double)r[f * NREC + 1]; sf += (double)r[f * NREC + 2]; }
    const float zcr = (float)(pr_block<WV>(sz, redd, PrAdd()) / (double)F);
    const float cen = (float)(pr_block<WV>(sc, redd, PrAdd()) / (double)F);
    const double f0md = pr_block<WV>(sf, redd, PrAdd()) / (double)F;
    const float f0m = (float)f0md;
    double qf = 0.0;
    for (int f = tid; f < F; f += WIN_THREADS) { const double df = (double)r[f * NREC + 2] - f0md; qf += df * df; }
    const float f0s = (float)sqrt(pr_block<WV>(qf, redd, PrAdd()) / (double)F);

    double s1 = 0.0, s2 = 0.0;
    float mx = -INFINITY, mn = INFINITY;
    for (int i = tid; i < L; i += WIN_THREADS) {
        const float v = pr_sample(base, d, i);
        s1 += (double)v; s2 += (double)v * (double)v; mx = fmaxf(mx, v); mn = fminf(mn, v);
    }
    const double meand = pr_block<WV>(s1, redd, PrAdd()) / (double)L;
    const float mean = (float)meand;
    const float energy = (float)(pr_block<WV>(s2, redd, PrAdd()) / (double)L);
    mx = pr_block<WV>(mx, red, PrMax());
    mn = pr_block<WV>(mn, red, PrMin());
    double q = 0.0;
    for (int i = tid; i < L; i += WIN_THREADS) { const double dv = (double)pr_sample(base, d, i) - meand; q += dv * dv; }
    const float sd = (float)sqrt(pr_block<WV>(q, redd, PrAdd()) / (double)L);
    if (tid == 0) {
        o[0] = energy; o[1] = zcr; o[2] = cen; o[3] = f0m; o[4] = f0s; o[5] = mean; o[6] = sd; o[7] = mx; o[8] = mn;
    }
}

static int pr_launch(PrPlan* p, const PrSource& src, int rows, int max_frames, float* rec, float* out, hipStream_t st) {
    hipLaunchKernelGGL(pr_frame_kernel, dim3((unsigned)max_frames, (unsigned)rows), dim3(256), 0, st, src, (const float*)p->tab, rec, max_frames);
    hipLaunchKernelGGL(pr_window_kernel, dim3((unsigned)rows), dim3(pr::WIN_THREADS), 0, st, src, (const float*)rec, max_frames, out);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int prosody_ragged(void* plan, const float* rings_dev, int64_t ring_len, const EgmSlot* slots_dev, int n_slots, int max_frames,
                   float* rec_dev, float* out_dev, hipStream_t st) {
    PrSource src{};
    src.base = rings_dev; src.mode = 2; src.slots = slots_dev; src.ring_len = (int32_t)ring_len;
    return pr_launch(static_cast<PrPlan*>(plan), src, n_slots, max_frames, rec_dev, out_dev, st);
}

}  // namespace km

using namespace km;

extern "C" {

int km_prosody_plan_create(void** plan_out) {
    using namespace pr;
    if (!plan_out) return fail(KM_ERR_INVALID_ARG, "km_prosody_plan_create: NULL argument");
    *plan_out = nullptr;
    std::unique_ptr<PrPlan> p(new (std::nothrow) PrPlan());
    if (!p) return fail(KM_ERR_HIP, "km_prosody_plan_create: out of host memory");
    const double PI = 3.14159265358979323846;
    std::vector<float> h(TAB_FLOATS);
    for (int n = 0; n < NFFT; ++n) h[n] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * n / NFFT));
    for (int k = 0; k < NH; ++k) { h[O_TW + 2 * k] = (float)std::cos(-2.0 * PI * k / NFFT); h[O_TW + 2 * k + 1] = (float)std::sin(-2.0 * PI * k / NFFT); }
    if (int rc = p->tab.alloc(TAB_FLOATS, "km_prosody_plan_create")) return rc;
    HIP_TRY(hipMemcpy(p->tab, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    *plan_out = p.release();
    return KM_OK;
}

int km_prosody_plan_destroy(void* plan) {
    if (!plan) return KM_OK;
    delete static_cast<PrPlan*>(plan);
    return KM_OK;
}

int64_t km_prosody_num_frames(int64_t L) { return L < 1 ? 0 : 1 + L / pr::HOP; }

int64_t km_prosody_workspace_floats(int64_t B, int64_t L) {
    if (B <= 0 || L <= 0) return -1;
    return B * km_prosody_num_frames(L) * pr::NREC;
}

static int pr_check(const char* who, int64_t rows, int64_t L) {
    if (rows < 1 || L < 1) return fail(KM_ERR_INVALID_ARG, "%s: %lld rows of %lld samples, at least 1 of each", who, (long long)rows, (long long)L);
    if (L > pr::MAX_L) return fail(KM_ERR_UNSUPPORTED, "%s: %lld samples per window, at most %lld (65.5 s)", who, (long long)L, (long long)pr::MAX_L);
    if (rows > 65535) return fail(KM_ERR_UNSUPPORTED, "%s: at most 65535 windows per call", who);
    return KM_OK;
}

int km_prosody_features(void* plan, const float* audio_dev, int64_t B, int64_t L, int64_t row_stride, float* work_dev, int64_t work_floats,
                        float* out_dev, float* frames_dev, void* stream) {
    if (!plan || !audio_dev || !out_dev || (!work_dev && !frames_dev)) return fail(KM_ERR_INVALID_ARG, "km_prosody_features: NULL argument");
    if (const int rc = pr_check("km_prosody_features", B, L)) return rc;
    if (row_stride < L) return fail(KM_ERR_INVALID_ARG, "km_prosody_features: row stride %lld below the row length %lld", (long long)row_stride, (long long)L);
    if (!frames_dev && work_floats < km_prosody_workspace_floats(B, L)) return fail(KM_ERR_WORKSPACE, "km_prosody_features: workspace too small");
    PrSource src{};
    src.base = audio_dev; src.mode = 0; src.L = (int32_t)L; src.row_stride = row_stride;
    return pr_launch(static_cast<PrPlan*>(plan), src, (int)B, (int)km_prosody_num_frames(L), frames_dev ? frames_dev : work_dev, out_dev,
                     (hipStream_t)stream);
}

int km_prosody_windows(void* plan, const float* clip_dev, int64_t clip_len, const int32_t* start_samples_dev, int64_t W, int64_t L,
                       float* work_dev, int64_t work_floats, float* out_dev, void* stream) {
    if (!plan || !clip_dev || !start_samples_dev || !work_dev || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_prosody_windows: NULL argument");
    if (const int rc = pr_check("km_prosody_windows", W, L)) return rc;
    if (clip_len < 1 || clip_len > INT32_MAX) return fail(KM_ERR_INVALID_ARG, "km_prosody_windows: a clip of %lld samples, 1 .. 2^31 - 1", (long long)clip_len);
    if (work_floats < km_prosody_workspace_floats(W, L)) return fail(KM_ERR_WORKSPACE, "km_prosody_windows: workspace too small");
    PrSource src{};
    src.base = clip_dev; src.mode = 1; src.L = (int32_t)L; src.clip_len = clip_len; src.starts = start_samples_dev;
    return pr_launch(static_cast<PrPlan*>(plan), src, (int)W, (int)km_prosody_num_frames(L), work_dev, out_dev, (hipStream_t)stream);
}

}  // extern "C"
