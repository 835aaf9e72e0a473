// eGeMAPSv02 functionals (88 values per audio window) on gfx950 -- SURVEY.md section 8 row f-4, second half.
//
// Replaces the openSMILE call of the reference's long-context emotion stream, OpenSMILEeGeMAPSExtractor._extract_features_from_audio
// (src/features/opensmile_extractor.py:427-439: peak normalisation, `self.smile.process_signal`, 88 functionals) for many
// 20 s windows at once.  At BASELINE's streaming configuration (1 024 speaker streams, one update per 0.3 s) that is 3 400
// windows of 320 000 samples per second -- hundreds of CPU cores of openSMILE.
//
// PARITY UNPINNED: openSMILE is a third-party package the reference neither vendors nor pins and that is not installed
// here.  The arithmetic below is the restatement in oracle/egemaps.py (the published GeMAPS / eGeMAPS parameter definitions,
// Eyben et al. 2016, with openSMILE 3.0's documented processing chain); the tests compare this file with that oracle and
// with known answers on synthetic signals.  Every constant is defined once, in EgmPlan (host, double) == oracle/egemaps.py.
//
//   egm_peak_kernel        per window: 1 / max |x|                                   (opensmile_extractor.py:431-433)
//   egm_frame_kernel       per 10 ms frame: 60 ms Gaussian + 20 ms Hamming frames as ONE 1024-point complex FFT in LDS,
//                          spectral descriptors, loudness, MFCC 1-4, sub-harmonic-summation pitch candidates, LPC formants
//   egm_viterbi_kernel     per window: pitch track over the candidates (sequential dynamic programme, 4 states); km_egemaps_window.hip
//   egm_voiced_kernel      per voiced frame: HNR (autocorrelation), jitter / shimmer (pitch periods marked in the
//                          waveform), harmonic differences and formant amplitudes
//   egm_functional_kernel  per window: 3-frame smoothing, means / normalised deviations / percentiles (bitonic sort in
//                          LDS) / slopes of rising and falling parts over voiced, unvoiced or all frames; km_egemaps_window.hip
// The frame and functional kernels also take the feature set (km_egemaps_dev.h): eGeMAPS, or the 62 functionals of GeMAPS, which leave
// out the work only the other 26 need.
// Each kernel has two instantiations: over a dense (B, L) array of windows (km_egemaps_*), and over ragged windows that are read
// in place from stream rings through a slot table written on the device (egm_ragged_functionals, for km_emotion_stream.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include <memory>

#include "km_context.h"
#include "km_egemaps_dev.h"
#include "km_egemaps_ragged.h"
#include "km_egemaps_lld.h"
#include "km_egemaps_window.h"

namespace km {


namespace egm {                         // SR, HOP, the record layout and the voicing thresholds: km_egemaps_dev.h
constexpr int N60 = 960, N20 = 320, NFFT = 1024, NB = NFFT / 2 + 1, OFF20 = (N60 - N20) / 2;
constexpr int NBANDS = 26, LPC = 11, NCAND = 3, PPO = 48, NHARM = 15;
}  // namespace egm

struct EgmPlan {
    // host tables (double precision arithmetic, stored as float), mirrored on the device
    std::vector<float> h;
    DevBuf<float> d;
    // offsets into the table blob
    int o_g60, o_ham, o_tw, o_fb_w, o_fb_start, o_fb_count, o_fb_off, o_eql, o_dct, o_logi, o_logf, o_hshift, o_hweight, o_pre, o_cos,
        o_sl0, o_sl1, o_gg;
    int n_log, j0, j1, nb_lpc, b_alpha[4], b_hamm[3], b_sl0[2], b_sl1[2], fb_nnz;
};

static int push(std::vector<float>& h, const std::vector<double>& v) {
    const int o = (int)h.size();
    for (double x : v) h.push_back((float)x);
    while (h.size() % 4) h.push_back(0.f);
    return o;
}
static int pushi(std::vector<float>& h, const std::vector<int>& v) {
    const int o = (int)h.size();
    for (int x : v) { float f; std::memcpy(&f, &x, 4); h.push_back(f); }
    while (h.size() % 4) h.push_back(0.f);
    return o;
}

static EgmPlan* build_egm_plan() {
    using namespace egm;
    EgmPlan* p = new EgmPlan();
    const double PI = 3.14159265358979323846;
    std::vector<double> g60(N60), ham(N20), tw(NFFT);
    for (int n = 0; n < N60; ++n) { const double k = n - (N60 - 1) / 2.0; g60[n] = std::exp(-0.5 * std::pow(k / (0.4 * (N60 - 1) / 2.0), 2)); }
    for (int n = 0; n < N20; ++n) ham[n] = 0.54 - 0.46 * std::cos(2.0 * PI * n / (N20 - 1));
    for (int k = 0; k < NFFT / 2; ++k) { tw[2 * k] = std::cos(-2.0 * PI * k / NFFT); tw[2 * k + 1] = std::sin(-2.0 * PI * k / NFFT); }
    p->o_g60 = push(p->h, g60); p->o_ham = push(p->h, ham); p->o_tw = push(p->h, tw);
    // window autocorrelation for the HNR's window compensation: gg[lag] = sum_n g[n] g[n + lag]
    std::vector<double> gg(N60);
    for (int lag = 0; lag < N60; ++lag) { double s = 0; for (int n = 0; n + lag < N60; ++n) s += g60[n] * g60[n + lag]; gg[lag] = s; }
    p->o_gg = push(p->h, gg);
    // 26 triangular HTK-mel filters, 20 .. 8000 Hz, over the 513 bins (sparse)
    auto mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
    auto imel = [](double m) { return 700.0 * (std::exp(m / 1127.0) - 1.0); };
    std::vector<double> edges(NBANDS + 2), w, eql(NBANDS);
    std::vector<int> start(NBANDS), count(NBANDS), off(NBANDS);
    for (int j = 0; j < NBANDS + 2; ++j) edges[j] = imel(mel(20.0) + (mel(8000.0) - mel(20.0)) * j / (NBANDS + 1));
    for (int j = 0; j < NBANDS; ++j) {
        const double l = edges[j], c = edges[j + 1], r = edges[j + 2];
        int s = -1, n = 0;
        off[j] = (int)w.size();
        for (int k = 0; k < NB; ++k) {
            const double f = k * (double)SR / NFFT;
            const double v = std::fmax(0.0, std::fmin((f - l) / (c - l), (r - f) / (r - c)));
            if (v > 0) { if (s < 0) s = k; n = k - s + 1; }
        }
        start[j] = s < 0 ? 0 : s; count[j] = n;
        for (int k = start[j]; k < start[j] + n; ++k) {
            const double f = k * (double)SR / NFFT;
            w.push_back(std::fmax(0.0, std::fmin((f - l) / (c - l), (r - f) / (r - c))));
        }
        const double w2 = std::pow(2.0 * PI * c, 2);
        eql[j] = ((w2 + 56.8e6) * w2 * w2) / (std::pow(w2 + 6.3e6, 2) * (w2 + 0.38e9));
    }
    p->fb_nnz = (int)w.size();
    p->o_fb_w = push(p->h, w); p->o_fb_start = pushi(p->h, start); p->o_fb_count = pushi(p->h, count); p->o_fb_off = pushi(p->h, off);
    p->o_eql = push(p->h, eql);
    std::vector<double> dct(4 * NBANDS);
    for (int i = 1; i <= 4; ++i)
        for (int j = 0; j < NBANDS; ++j)
            dct[(i - 1) * NBANDS + j] = std::sqrt(2.0 / NBANDS) * std::cos(PI * i * (j + 0.5) / NBANDS) * (1.0 + 11.0 * std::sin(PI * i / 22.0));
    p->o_dct = push(p->h, dct);
    // log2-frequency axis: PPO points per octave from 25 Hz to Nyquist, linear interpolation from the FFT bins
    p->n_log = (int)std::floor(std::log2((SR / 2.0) / 25.0) * PPO) + 1;
    p->j0 = (int)std::ceil(std::log2(55.0 / 25.0) * PPO);
    p->j1 = (int)std::floor(std::log2(1000.0 / 25.0) * PPO) + 1;
    std::vector<int> logi(p->n_log); std::vector<double> logf(p->n_log);
    for (int j = 0; j < p->n_log; ++j) {
        const double f = 25.0 * std::pow(2.0, (double)j / PPO), pos = f / ((double)SR / NFFT);
        int i0 = (int)std::floor(pos);
        if (i0 >= NB - 1) i0 = NB - 2;
        logi[j] = i0; logf[j] = pos - i0;
    }
    p->o_logi = pushi(p->h, logi); p->o_logf = push(p->h, logf);
    std::vector<int> hs(NHARM); std::vector<double> hw(NHARM);
    for (int h = 0; h < NHARM; ++h) { hs[h] = (int)std::lround(PPO * std::log2((double)(h + 1))); hw[h] = std::pow(0.85, h); }
    p->o_hshift = pushi(p->h, hs); p->o_hweight = push(p->h, hw);
    // LPC on the spectrum below 5.5 kHz: pre-emphasis and trapezoid weights folded together, cosine table for 12 lags
    p->nb_lpc = (int)(5500.0 / ((double)SR / NFFT)) + 1;
    std::vector<double> pre(p->nb_lpc), cs((size_t)p->nb_lpc * (LPC + 1));
    for (int k = 0; k < p->nb_lpc; ++k) {
        const double wv = PI * k / (p->nb_lpc - 1);
        pre[k] = (1.0 + 0.97 * 0.97 - 2.0 * 0.97 * std::cos(wv)) * ((k == 0 || k == p->nb_lpc - 1) ? 0.5 : 1.0);
        for (int l = 0; l <= LPC; ++l) cs[(size_t)l * p->nb_lpc + k] = std::cos(wv * l);
    }
    p->o_pre = push(p->h, pre); p->o_cos = push(p->h, cs);
    // band edges as bin ranges [lo, hi): f >= lo_hz && f < hi_hz
    auto bin_ge = [](double hz) { return (int)std::ceil(hz / ((double)SR / NFFT) - 1e-9); };
    p->b_alpha[0] = bin_ge(50); p->b_alpha[1] = bin_ge(1000); p->b_alpha[2] = bin_ge(1000); p->b_alpha[3] = bin_ge(5000);
    p->b_hamm[0] = 0; p->b_hamm[1] = bin_ge(2000); p->b_hamm[2] = bin_ge(5000);
    auto regress = [&](double lo, double hi, int (&b)[2]) {
        b[0] = bin_ge(lo); b[1] = bin_ge(hi);
        std::vector<double> fx(b[1] - b[0]);
        double m = 0, ss = 0;
        for (int k = b[0]; k < b[1]; ++k) m += k * (double)SR / NFFT;
        m /= (b[1] - b[0]);
        for (int k = b[0]; k < b[1]; ++k) { fx[k - b[0]] = k * (double)SR / NFFT - m; ss += fx[k - b[0]] * fx[k - b[0]]; }
        for (auto& v : fx) v /= ss;
        return fx;
    };
    p->o_sl0 = push(p->h, regress(0, 500, p->b_sl0));
    p->o_sl1 = push(p->h, regress(500, 1500, p->b_sl1));
    return p;
}

struct EgmArgs {
    const float* audio; int64_t L; int nf;
    const float* scale;      // (B) peak normalisation factors, or null
    const float* tab;        // EgmPlan table blob
    float* rec;              // (B, rec_frames, REC)
    int rec_frames;          // frames between two windows' records: nf, or the longest window's count when windows are ragged
    const EgmSlot* slots;    // ragged windows only: per window {stream, ring start, length, frames} (km_egemaps_ragged.h)
    int ring_len;            // ragged windows only: samples per stream ring; audio is then (n_streams, ring_len)
    int o_g60, o_ham, o_tw, o_fb_w, o_fb_start, o_fb_count, o_fb_off, o_eql, o_dct, o_logi, o_logf, o_hshift, o_hweight, o_pre, o_cos,
        o_sl0, o_sl1, o_gg;
    int n_log, j0, j1, nb_lpc, b_alpha[4], b_hamm[3], b_sl0[2], b_sl1[2];
};

// Where a window's samples are.  The kernels below are written once against `xw[i]`, sample i of the window: LinearWin is
// window b of a dense (B, L) array (km_egemaps_functionals, RAGGED = false), RingWin a window of its own length that starts
// anywhere in a stream's ring and may wrap (the emotion streams, RAGGED = true: a device-written EgmSlot per window, a block
// whose slot is empty or whose frame lies beyond the slot's frames leaves before it touches LDS or a barrier).  Only the
// address differs; the arithmetic on the samples is the same code.
struct LinearWin {
    const float* p;
    __device__ __forceinline__ float operator[](int64_t i) const { return p[i]; }
};
struct RingWin {
    const float* p; int start, n;
    __device__ __forceinline__ float operator[](int i) const { const int j = start + i; return p[j >= n ? j - n : j]; }   // start < n, i <= n
};
template <bool RAGGED> struct EgmWin;
template <> struct EgmWin<false> {
    using Src = LinearWin;
    static __device__ __forceinline__ bool open(const float* audio, int64_t L, const EgmSlot*, int, int b, Src& x, int& len, int& nf) {
        x.p = audio + (int64_t)b * L; len = (int)L;
        return true;
    }
};
template <> struct EgmWin<true> {
    using Src = RingWin;
    static __device__ __forceinline__ bool open(const float* audio, int64_t, const EgmSlot* slots, int ring_len, int b, Src& x, int& len, int& nf) {
        const EgmSlot s = slots[b];
        if (s.stream < 0) return false;
        x.p = audio + (int64_t)s.stream * ring_len; x.start = s.start; x.n = ring_len; len = s.len; nf = s.nf;
        return true;
    }
};

template <bool RAGGED>
__global__ __launch_bounds__(256) void egm_peak_kernel(const float* __restrict__ x, int64_t L, const EgmSlot* __restrict__ slots, int ring_len,
                                                       float* __restrict__ scale) {
    __shared__ float red[256];
    typename EgmWin<RAGGED>::Src p; int len = 0, nf = 0;
    if (!EgmWin<RAGGED>::open(x, L, slots, ring_len, blockIdx.x, p, len, nf)) return;
    float m = 0.f;
    if constexpr (RAGGED) { for (int i = threadIdx.x; i < len; i += 256) m = fmaxf(m, fabsf(p[i])); }
    else { for (int64_t i = threadIdx.x; i < L; i += 256) m = fmaxf(m, fabsf(p[i])); }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) scale[blockIdx.x] = red[0] > 0.f ? 1.0f / red[0] : 1.0f;
}

// block-wide maximum, as block_sum (km_egemaps_dev.h): a butterfly inside each wave, then the four wave results in wave order
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// in-place 1024-point complex FFT of buf (interleaved re, im) in LDS: bit-reversed load order is the caller's; radix-2 DIT
__device__ __forceinline__ void fft1024(float2* buf, const float2* tw) {
    const int tid = threadIdx.x;
    for (int s = 0; s < 10; ++s) {
        const int half = 1 << s;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = tid + 256 * r;
            const int j = i & (half - 1);
            const int base = ((i >> s) << (s + 1)) + j;
            const float2 w = tw[j << (9 - s)];
            const float2 a = buf[base], b = buf[base + half];
            const float2 bw = make_float2(b.x * w.x - b.y * w.y, b.x * w.y + b.y * w.x);
            buf[base] = make_float2(a.x + bw.x, a.y + bw.y);
            buf[base + half] = make_float2(a.x - bw.x, a.y - bw.y);
        }
        __syncthreads();
    }
}
__device__ __forceinline__ int bitrev10(int v) { return (int)(__brev((unsigned)v) >> 22); }

// window-compensated autocorrelation of the Gaussian-windowed frame sw[960] at lags lag0 .. lag0 + nl - 1 (nl <= 128), one lag
// per thread, into r[]: r = sum_n sw[n] sw[n + lag] / gg[lag] * gg[0]
__device__ __forceinline__ void acf_lags(const float* sw, const float* gg, int lag0, int nl, float* r) {
    using namespace egm;
    const int i = threadIdx.x;
    if (i < nl) {
        const int lag = lag0 + i;
        float acc = 0.f;
        for (int n = 0; n + lag < N60; ++n) acc = fmaf(sw[n], sw[n + lag], acc);
        r[i] = acc / fmaxf(gg[lag], 1e-12f) * gg[0];
    }
    __syncthreads();
}

// 60 ms Gaussian frame (real part) and, optionally, a 20 ms Hamming frame (imaginary part) -> 1024-point spectra.
// zb is loaded in bit-reversed order; after the FFT M60[k] = |(Z[k] + conj Z[N-k]) / 2|, M20[k] = |(Z[k] - conj Z[N-k]) / 2i|.
template <class Src>
__device__ __forceinline__ void frame_spectra(const EgmArgs& a, const Src& xw, float sc, int start60, int start20, bool with20,
                                              float2* zb, const float2* tw, float* M60, float* M20) {
    using namespace egm;
    const float* g60 = a.tab + a.o_g60; const float* ham = a.tab + a.o_ham;
    for (int n = threadIdx.x; n < NFFT; n += 256) {
        float re = 0.f, im = 0.f;
        if (n < N60) re = g60[n] * xw[start60 + n] * sc;
        if (with20 && n < N20) im = ham[n] * xw[start20 + n] * sc;
        zb[bitrev10(n)] = make_float2(re, im);
    }
    __syncthreads();
    fft1024(zb, tw);
    for (int k = threadIdx.x; k < NB; k += 256) {
        const float2 z = zb[k], zc = zb[(NFFT - k) & (NFFT - 1)];
        const float ar = 0.5f * (z.x + zc.x), ai = 0.5f * (z.y - zc.y);          // (Z[k] + conj Z[N-k]) / 2
        const float br = 0.5f * (z.y + zc.y), bi = -0.5f * (z.x - zc.x);         // (Z[k] - conj Z[N-k]) / (2i)
        M60[k] = sqrtf(ar * ar + ai * ai);
        if (M20) M20[k] = sqrtf(br * br + bi * bi);
    }
    __syncthreads();
}

// SET (km_egemaps_window.h): the GeMAPS instantiations leave out what only the spectral flux and the MFCCs need -- the previous
// frame's transform and Mp, the flux sum, the four DCT sums -- and write 0 to those five fields.  Every other statement is the same,
// in the same order: every other field of a record has the eGeMAPS instantiation's bits.
template <bool RAGGED, int SET>
__global__ __launch_bounds__(256, 6) void egm_frame_kernel(EgmArgs a) {
    using namespace egm;
    constexpr bool FULL = SET == SET_EGEMAPS;
    __shared__ float2 zb[NFFT];
    __shared__ float2 tw[NFFT / 2];
    __shared__ float M60[NB + 3], M20[NB + 3], Mp[NB + 3], red[256], E[32], slog[512], shs[256], misc[64], sw[N60], rl[128];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    typename EgmWin<RAGGED>::Src xw; int len = 0, nf = a.nf;
    if (!EgmWin<RAGGED>::open(a.audio, a.L, a.slots, a.ring_len, b, xw, len, nf) || t >= nf) return;
    const float sc = a.scale ? a.scale[b] : 1.0f;
    float* rec = a.rec + ((int64_t)b * a.rec_frames + t) * REC;
    for (int k = tid; k < NFFT / 2; k += 256) tw[k] = reinterpret_cast<const float2*>(a.tab + a.o_tw)[k];
    __syncthreads();
    // previous frame's 20 ms spectrum (for the spectral flux): the imaginary slot of a transform whose real slot is unused
    if (FULL && t > 0) {
        const float* ham = a.tab + a.o_ham;
        for (int n = tid; n < NFFT; n += 256) zb[bitrev10(n)] = make_float2(n < N20 ? ham[n] * xw[HOP * (t - 1) + OFF20 + n] * sc : 0.f, 0.f);
        __syncthreads();
        fft1024(zb, tw);
        for (int k = tid; k < NB; k += 256) Mp[k] = sqrtf(zb[k].x * zb[k].x + zb[k].y * zb[k].y);
        __syncthreads();
    }
    frame_spectra(a, xw, sc, HOP * t, HOP * t + OFF20, true, zb, tw, M60, M20);

    // ---- frame energy; the windowed frame stays in LDS for the voicing measure ----
    float e2 = 0.f;
    for (int n = tid; n < N60; n += 256) { const float v = xw[HOP * t + n] * sc; e2 += v * v; sw[n] = v * a.tab[a.o_g60 + n]; }
    const float rms = sqrtf(block_sum(e2, red) / N60);

    // ---- band powers -> loudness, MFCC 1-4 ----
    if (tid < NBANDS) {
        const int s0 = __float_as_int(a.tab[a.o_fb_start + tid]), cnt = __float_as_int(a.tab[a.o_fb_count + tid]);
        const float* w = a.tab + a.o_fb_w + __float_as_int(a.tab[a.o_fb_off + tid]);
        float acc = 0.f;
        for (int k = 0; k < cnt; ++k) acc = fmaf(M20[s0 + k] * M20[s0 + k], w[k], acc);
        E[tid] = acc;
    }
    __syncthreads();
    if (tid < 64) {          // wave 0, lane j = band j: the 26 powers / logarithms in parallel, sums by butterfly
        const bool on = tid < NBANDS;
        const float ej = on ? E[tid] : 0.f;
        const float loud = wave_sum(on ? powf(ej * a.tab[a.o_eql + tid], 0.33f) : 0.f);
        const float le = on ? logf(fmaxf(ej, 1e-8f)) : 0.f;
        float c[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (FULL) {
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = wave_sum(on ? le * a.tab[a.o_dct + i * NBANDS + tid] : 0.f);
        }
        if (tid == 0) {
            rec[R_LOUD] = loud;
#pragma unroll
            for (int i = 0; i < 4; ++i) rec[R_MFCC + i] = c[i];
            rec[R_RMS] = rms;
        }
    }
    // ---- alpha ratio, Hammarberg index, slopes, flux ----
    {
        float lo = 0.f, hi = 0.f, pl = 0.f, ph = 0.f, s0 = 0.f, s1 = 0.f, fl = 0.f;
        for (int k = tid; k < NB; k += 256) {
            const float pw = M20[k] * M20[k];
            if (k >= a.b_alpha[0] && k < a.b_alpha[1]) lo += pw;
            if (k >= a.b_alpha[2] && k < a.b_alpha[3]) hi += pw;
            if (k >= a.b_hamm[0] && k < a.b_hamm[1]) pl = fmaxf(pl, pw);
            if (k >= a.b_hamm[1] && k < a.b_hamm[2]) ph = fmaxf(ph, pw);
            const float ldb = 10.0f * log10f(pw + 1e-12f);
            if (k >= a.b_sl0[0] && k < a.b_sl0[1]) s0 = fmaf(ldb, a.tab[a.o_sl0 + k - a.b_sl0[0]], s0);
            if (k >= a.b_sl1[0] && k < a.b_sl1[1]) s1 = fmaf(ldb, a.tab[a.o_sl1 + k - a.b_sl1[0]], s1);
            if (FULL && t > 0) { const float dm = M20[k] - Mp[k]; fl += dm * dm; }
        }
        const float LO = block_sum(lo, red), HI = block_sum(hi, red), PL = block_max(pl, red), PH = block_max(ph, red);
        const float S0 = block_sum(s0, red), S1 = block_sum(s1, red), FL = FULL ? block_sum(fl, red) : 0.f;
        if (tid == 0) {
            rec[R_ALPHA] = 10.0f * log10f((LO + 1e-12f) / (HI + 1e-12f));
            rec[R_HAMM] = 10.0f * log10f((PL + 1e-12f) / (PH + 1e-12f));
            rec[R_SL0] = S0; rec[R_SL1] = S1;
            rec[R_FLUX] = FULL && t > 0 ? sqrtf(FL / NB) : 0.f;
        }
    }
    // ---- sub-harmonic summation on the log2-frequency axis ----
    for (int j = tid; j < a.n_log; j += 256) {
        const int i0 = __float_as_int(a.tab[a.o_logi + j]); const float fr = a.tab[a.o_logf + j];
        slog[j] = M60[i0] * (1.0f - fr) + M60[i0 + 1] * fr;
    }
    __syncthreads();
    float sm[2] = {0.f, 0.f};
    for (int r = 0; r < 2; ++r) {
        const int j = tid + 256 * r;
        if (j < a.n_log) sm[r] = (j == 0 || j == a.n_log - 1) ? slog[j] : 0.25f * slog[j - 1] + 0.5f * slog[j] + 0.25f * slog[j + 1];
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r) { const int j = tid + 256 * r; if (j < a.n_log) slog[j] = sm[r]; }
    __syncthreads();
    const int nshs = a.j1 - a.j0;
    float sv = 0.f;
    if (tid < nshs) {
        for (int h = 0; h < NHARM; ++h) {
            const int idx = a.j0 + tid + __float_as_int(a.tab[a.o_hshift + h]);
            if (idx < a.n_log) sv = fmaf(a.tab[a.o_hweight + h], slog[idx], sv);
        }
        shs[tid] = sv;
    }
    const float peak = block_max(tid < nshs ? sv : 0.f, red);
    const float mean = block_sum(tid < nshs ? sv : 0.f, red) / nshs;
    (void)mean;
    // greedy candidates: highest point (first index on ties), then blank +- 1/6 octave around it -- one block arg-max per
    // candidate (the value first, then the lowest index that reaches it) instead of thread 0 scanning the curve NCAND times
    {
        int kprev[NCAND];
#pragma unroll
        for (int c = 0; c < NCAND; ++c) {
            bool blanked = tid >= nshs;
#pragma unroll
            for (int q = 0; q < c; ++q) if (kprev[q] >= 0 && tid >= kprev[q] - PPO / 6 && tid <= kprev[q] + PPO / 6) blanked = true;
            const float v = blanked ? 0.f : sv;
            const float best = block_max(v, red);
            const float ki = block_max((best > 0.f && !blanked && v == best) ? (float)(nshs - tid) : 0.f, red);   // first index wins
            const int k = best > 0.f ? nshs - (int)ki : -1;
            kprev[c] = k;
            if (tid == 0) {
                if (k < 0) { rec[R_CF + c] = 0.f; rec[R_CS + c] = 0.f; misc[c] = -1000.f; }
                else {
                    misc[c] = (float)k;
                    float dlt = 0.f;
                    if (k > 0 && k < nshs - 1) {
                        const float y0 = shs[k - 1], y1 = shs[k], y2 = shs[k + 1], den = y0 - 2.f * y1 + y2;
                        dlt = den == 0.f ? 0.f : fminf(fmaxf(0.5f * (y0 - y2) / den, -0.5f), 0.5f);
                    }
                    rec[R_CF + c] = 25.0f * exp2f((a.j0 + k + dlt) / (float)PPO);
                    rec[R_CS + c] = shs[k] / peak;
                    if (c == 0) misc[4] = rec[R_CF];
                }
            }
        }
        if (tid == 0 && kprev[0] < 0) misc[4] = 0.f;
    }
    __syncthreads();
    // ---- voicing: normalised autocorrelation at the strongest candidate's lag (+- 10 %), only if it is a local maximum ----
    {
        const float cf0 = misc[4];
        float vo = 0.f;
        if (cf0 > 0.f) {                                   // uniform
            const float T0 = (float)SR / cf0;
            int lo = (int)floorf(0.9f * T0), hi = (int)ceilf(1.1f * T0);
            lo = lo < 1 ? 1 : lo; hi = hi > N60 - 2 ? N60 - 2 : hi;
            const int nl = hi - lo + 3;                    // lags lo - 1 .. hi + 1
            acf_lags(sw, a.tab + a.o_gg, lo - 1, nl < 128 ? nl : 128, rl);
            float r0p = 0.f;
            for (int n = tid; n < N60; n += 256) r0p += sw[n] * sw[n];
            const float r0 = block_sum(r0p, red);
            if (tid == 0 && r0 > 0.f) {
                const int ne = nl < 128 ? nl : 128;
                int k = 1;
                for (int q = 2; q < ne - 1; ++q) if (rl[q] > rl[k]) k = q;
                if (rl[k] >= rl[k - 1] && rl[k] >= rl[k + 1]) vo = fminf(fmaxf(rl[k] / r0, 0.f), 1.f);
            }
        }
        if (tid == 0) rec[R_VOI] = vo;
    }
    // ---- LPC formants from the 20 ms power spectrum below 5.5 kHz ----
    {
        float* R = misc + 8;       // [12]
        for (int l = 0; l <= LPC; ++l) {
            float acc = 0.f;
            for (int k = tid; k < a.nb_lpc; k += 256) acc = fmaf(M20[k] * M20[k] * a.tab[a.o_pre + k], a.tab[a.o_cos + l * a.nb_lpc + k], acc);
            const float v = block_sum(acc, red);
            if (tid == 0) R[l] = v;
        }
        __syncthreads();
        if (tid < 64) {     // wave 0: Levinson-Durbin redundantly in every lane (uniform), then ONE ROOT PER LANE
            float F[3] = {0.f, 0.f, 0.f}, BW[3] = {0.f, 0.f, 0.f};
            float* fsel = misc + 24;   // [LPC] candidate frequencies, [LPC] bandwidths behind them
            float* bsel = fsel + LPC;
            if (R[0] > 0.f) {           // uniform
                float ac[LPC + 1], tmp[LPC + 1];
                ac[0] = 1.f;
#pragma unroll
                for (int i = 1; i <= LPC; ++i) ac[i] = 0.f;
                float err = R[0];
                bool ok = true;
#pragma unroll
                for (int i = 1; i <= LPC; ++i) {                            // Levinson-Durbin
                    if (!ok) continue;
                    float acc = R[i];
#pragma unroll
                    for (int j = 1; j < i; ++j) acc = fmaf(ac[j], R[i - j], acc);
                    const float kk = -acc / err;
#pragma unroll
                    for (int j = 1; j < i; ++j) tmp[j] = ac[j] + kk * ac[i - j];
#pragma unroll
                    for (int j = 1; j < i; ++j) ac[j] = tmp[j];
                    ac[i] = kk;
                    err *= 1.0f - kk * kk;
                    if (err <= 0.f) ok = false;
                }
                // roots of z^11 + ac[1] z^10 + ... + ac[11] by Durand-Kerner (Weierstrass) iteration, lane i = root i, all
                // roots updated together from the previous iterate (the serial version updated them one after another on
                // thread 0 and was 85 % of this kernel's time); the partners' values come by shuffle
                const int li = tid < LPC ? tid : 0;
                const float ang = 2.0f * 3.14159265f * (li + 0.35f) / LPC;
                float zr = 0.9f * cosf(ang), zi = 0.9f * sinf(ang);
                for (int it = 0; it < 60; ++it) {
                    float pr = 1.f, pi = 0.f;                               // Horner: p(z_i)
#pragma unroll
                    for (int j = 1; j <= LPC; ++j) { const float nr = pr * zr - pi * zi + ac[j], ni = pr * zi + pi * zr; pr = nr; pi = ni; }
                    float qr = 1.f, qi = 0.f;                               // prod_{j != i} (z_i - z_j)
#pragma unroll
                    for (int j = 0; j < LPC; ++j) {
                        const float zjr = __shfl(zr, j), zji = __shfl(zi, j);
                        const float dr = zr - zjr, di = zi - zji;
                        const float nr = qr * dr - qi * di, ni = qr * di + qi * dr;
                        if (j != li) { qr = nr; qi = ni; }
                    }
                    const float den = qr * qr + qi * qi + 1e-30f;
                    const float cr = (pr * qr + pi * qi) / den, ci = (pi * qr - pr * qi) / den;
                    zr -= cr; zi -= ci;
                    const float change = wave_max(tid < LPC ? fabsf(cr) + fabsf(ci) : 0.f);
                    if (change < 1e-7f) break;                              // uniform
                }
                const float fs2 = 11000.0f;
                float fr = -1.f, bw = 0.f;
                if (tid < LPC && zi > 1e-6f) {
                    const float f = atan2f(zi, zr) * fs2 / (2.0f * 3.14159265f);
                    const float bq = -logf(fmaxf(sqrtf(zr * zr + zi * zi), 1e-12f)) * fs2 / 3.14159265f;
                    if (f > 90.f && f < 5400.f && bq < 1000.f) { fr = f; bw = bq; }
                }
                if (tid < LPC) { fsel[tid] = fr; bsel[tid] = bw; }
                __builtin_amdgcn_wave_barrier();
                if (tid == 0) {
                    for (int c = 0; c < 3; ++c) {                           // three lowest
                        int best = -1;
                        for (int i = 0; i < LPC; ++i) if (fsel[i] > 0.f && (best < 0 || fsel[i] < fsel[best])) best = i;
                        if (best < 0) break;
                        F[c] = fsel[best]; BW[c] = bsel[best]; fsel[best] = -1.f;
                    }
                }
            }
            if (tid == 0)
                for (int c = 0; c < 3; ++c) { rec[R_F + c] = F[c]; rec[R_BW + c] = BW[c]; }
        }
    }
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void egm_voiced_kernel(EgmArgs a) {
    using namespace egm;
    __shared__ float2 zb[NFFT];
    __shared__ float2 tw[NFFT / 2];
    __shared__ float M60[NB + 3], seg[N60], red[256], cc[128];
    __shared__ int redi[256], marks[64];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    typename EgmWin<RAGGED>::Src xw; int len = 0, nf = a.nf;
    if (!EgmWin<RAGGED>::open(a.audio, a.L, a.slots, a.ring_len, b, xw, len, nf) || t >= nf) return;
    const float sc = a.scale ? a.scale[b] : 1.0f;
    float* rec = a.rec + ((int64_t)b * a.rec_frames + t) * REC;
    const float f0 = rec[R_F0];
    __syncthreads();                                     // everyone has read the record before thread 0 rewrites parts of it
    if (f0 <= 0.f) {
        if (tid == 0) {
            rec[R_JIT] = rec[R_SHIM] = rec[R_HNR] = rec[R_H1H2] = rec[R_H1A3] = 0.f;
            for (int c = 0; c < 3; ++c) { rec[R_FAMP + c] = 0.f; rec[R_F + c] = 0.f; rec[R_BW + c] = 0.f; }   // formants: voiced frames only
        }
        return;
    }
    for (int k = tid; k < NFFT / 2; k += 256) tw[k] = reinterpret_cast<const float2*>(a.tab + a.o_tw)[k];
    for (int n = tid; n < N60; n += 256) seg[n] = xw[HOP * t + n] * sc;
    __syncthreads();
    frame_spectra(a, xw, sc, HOP * t, 0, false, zb, tw, M60, nullptr);
    const float T0 = (float)SR / f0;
    int lo = (int)floorf(0.9f * T0), hi = (int)ceilf(1.1f * T0);
    if (hi > N60 - 2) hi = N60 - 2;
    const float* g60 = a.tab + a.o_g60; const float* gg = a.tab + a.o_gg;
    // ---- HNR from the window-compensated autocorrelation at the pitch lag ----
    float r0p = 0.f;
    for (int n = tid; n < N60; n += 256) { const float v = seg[n] * g60[n]; r0p += v * v; }
    const float r0 = block_sum(r0p, red);
    float best = 0.f;
    {
        float* swv = reinterpret_cast<float*>(zb);        // the FFT buffer is idle from here on (occupancy: LDS per workgroup)
        for (int n = tid; n < N60; n += 256) swv[n] = seg[n] * g60[n];
        __syncthreads();
        const int lag0 = lo > 1 ? lo : 1;
        const int nl = hi - lag0 + 1 < 128 ? hi - lag0 + 1 : 128;
        acf_lags(swv, gg, lag0, nl, cc);
        for (int q = 0; q < nl; ++q) best = fmaxf(best, cc[q]);
        __syncthreads();
    }
    // ---- pitch periods: one candidate lag per thread ----
    {
        float mv = -INFINITY; int mi = 0;
        for (int n = tid; n < N60; n += 256) if (seg[n] > mv) { mv = seg[n]; mi = n; }
        red[tid] = mv; redi[tid] = mi;
        __syncthreads();
        if (tid == 0) {
            float bv = red[0]; int bi = redi[0];
            for (int k = 1; k < 256; ++k) if (red[k] > bv || (red[k] == bv && redi[k] < bi)) { bv = red[k]; bi = redi[k]; }
            const int T = (int)roundf(T0);
            marks[0] = bi >= T ? bi % T : bi;
            marks[63] = 1;                                // number of marks
        }
        __syncthreads();
        const int lagA = lo > 2 ? lo : 2;
        for (int step = 0; step < 60; ++step) {
            const int pos = marks[marks[63] - 1];
            const int lag = lagA + tid;
            float c = -INFINITY;
            if (lag <= hi && pos + 2 * lag <= N60) {
                float ab = 0.f, aa = 0.f, bb = 0.f;
                for (int n = 0; n < lag; ++n) { const float u = seg[pos + n], v = seg[pos + lag + n]; ab = fmaf(u, v, ab); aa = fmaf(u, u, aa); bb = fmaf(v, v, bb); }
                c = ab / sqrtf(fmaxf(aa * bb, 1e-20f));
            }
            // strongest lag, first one on ties: block arg-max (value, then the lowest index reaching it) instead of a scan
            const int nl = hi - lagA + 1 < 128 ? hi - lagA + 1 : 128;
            const bool in = tid < nl;
            const float bc = block_max(in ? c : -INFINITY, red);
            const float kf = block_max((in && c == bc && bc > -INFINITY) ? (float)(128 - tid) : 0.f, red);
            if (tid == 0) {
                const int bl = kf > 0.f ? lagA + (128 - (int)kf) : 0;
                if (bl == 0 || bc < 0.5f || marks[63] >= 62) marks[62] = 0;          // stop
                else { marks[marks[63]] = pos + bl; marks[63] += 1; marks[62] = 1; }
            }
            __syncthreads();
            if (marks[62] == 0) break;
        }
    }
    if (tid == 0) {
        const float rr = fminf(fmaxf(best / fmaxf(r0, 1e-20f), 1e-6f), 1.0f - 1e-6f);
        rec[R_HNR] = 10.0f * log10f(rr / (1.0f - rr));
        const int nm = marks[63];
        float jit = 0.f, shim = 0.f;
        if (nm >= 3) {
            float psum = 0.f, dsum = 0.f, prev_amp = 0.f, ssum = 0.f;
            for (int i = 0; i + 1 < nm; ++i) {
                const float per = (float)(marks[i + 1] - marks[i]);
                psum += per;
                if (i > 0) dsum += fabsf(per - (float)(marks[i] - marks[i - 1]));
                float mx = -INFINITY, mn = INFINITY;
                for (int n = marks[i]; n < marks[i + 1]; ++n) { mx = fmaxf(mx, seg[n]); mn = fminf(mn, seg[n]); }
                const float amp = fmaxf(mx - mn, 1e-9f);
                if (i > 0) ssum += fabsf(20.0f * log10f(amp / prev_amp));
                prev_amp = amp;
            }
            jit = (dsum / (nm - 2)) / (psum / (nm - 1));
            shim = ssum / (nm - 2);
        }
        rec[R_JIT] = jit; rec[R_SHIM] = shim;
        // harmonic amplitudes: strongest bin within +- 20 % of f0 around the target frequency, in dB
        const float binw = (float)SR / NFFT;
        auto harm_db = [&](float freq) {
            int l = (int)floorf((freq - 0.2f * f0) / binw), h = (int)ceilf((freq + 0.2f * f0) / binw);
            l = l < 0 ? 0 : l; h = h > NB - 1 ? NB - 1 : h;
            float m = 0.f;
            for (int k = l; k <= h; ++k) m = fmaxf(m, M60[k]);
            return 20.0f * log10f(fmaxf(m, 1e-12f));
        };
        const float h1 = harm_db(f0), h2 = harm_db(2.0f * f0);
        rec[R_H1H2] = h1 - h2;
        float h1a3 = 0.f;
        for (int c = 0; c < 3; ++c) {
            const float F = rec[R_F + c];
            float amp = 0.f;
            if (F > 0.f) {
                const float av = harm_db(fmaxf(f0, rintf(F / f0) * f0));
                amp = av - h1;
                if (c == 2) h1a3 = h1 - av;
            }
            rec[R_FAMP + c] = amp;
        }
        rec[R_H1A3] = h1a3;
    }
}

static EgmArgs egm_args(const EgmPlan* p, const float* audio, int64_t L, int nf, const float* scale, float* rec) {
    EgmArgs a{};
    a.audio = audio; a.L = L; a.nf = nf; a.scale = scale; a.tab = p->d; a.rec = rec; a.rec_frames = nf; a.slots = nullptr; a.ring_len = 0;
    a.o_g60 = p->o_g60; a.o_ham = p->o_ham; a.o_tw = p->o_tw; a.o_fb_w = p->o_fb_w; a.o_fb_start = p->o_fb_start; a.o_fb_count = p->o_fb_count;
    a.o_fb_off = p->o_fb_off; a.o_eql = p->o_eql; a.o_dct = p->o_dct; a.o_logi = p->o_logi; a.o_logf = p->o_logf; a.o_hshift = p->o_hshift;
    a.o_hweight = p->o_hweight; a.o_pre = p->o_pre; a.o_cos = p->o_cos; a.o_sl0 = p->o_sl0; a.o_sl1 = p->o_sl1; a.o_gg = p->o_gg;
    a.n_log = p->n_log; a.j0 = p->j0; a.j1 = p->j1; a.nb_lpc = p->nb_lpc;
    for (int i = 0; i < 4; ++i) a.b_alpha[i] = p->b_alpha[i];
    for (int i = 0; i < 3; ++i) a.b_hamm[i] = p->b_hamm[i];
    for (int i = 0; i < 2; ++i) { a.b_sl0[i] = p->b_sl0[i]; a.b_sl1[i] = p->b_sl1[i]; }
    return a;
}

// The five kernels over ragged windows that live in stream rings (km_emotion_stream.hip): fixed grids of max_nf frames x
// n_slots windows, everything else from the slot table on the device.  long_windows: the object was made for windows beyond 2048
// frames (km_emotion_*_create_long): max_nf up to 6548, and the two per-window kernels run at their long tier for every slot.
// The first four of them -- peak, frame, pitch track, voiced -- under the caller's name: the frame records of every slot's window
static int ragged_records(const char* who, void* plan, const float* rings_dev, int64_t ring_len, const EgmSlot* slots_dev, int n_slots, int max_nf,
                          float* scale_dev, float* rec_dev, hipStream_t st, bool long_windows, int feature_set) {
    using namespace egm;
    if (!set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "%s: feature set %d", who, feature_set);
    if (!plan || !rings_dev || !slots_dev || !scale_dev || !rec_dev || n_slots < 1 || n_slots > 65535 || max_nf < 1 ||
        max_nf > (long_windows ? LongTier::MAXF : ShortTier::MAXF) || ring_len < 1 || ring_len > (1 << 30))
        return fail(KM_ERR_INVALID_ARG, "%s: bad argument", who);
    EgmArgs a = egm_args(static_cast<EgmPlan*>(plan), rings_dev, 0, 0, scale_dev, rec_dev);
    a.rec_frames = max_nf; a.slots = slots_dev; a.ring_len = (int)ring_len;
    hipLaunchKernelGGL(egm_peak_kernel<true>, dim3((unsigned)n_slots), dim3(256), 0, st, rings_dev, (int64_t)0, slots_dev, (int)ring_len, scale_dev);
    const auto frame_kernel = feature_set == SET_GEMAPS ? egm_frame_kernel<true, SET_GEMAPS> : egm_frame_kernel<true, SET_EGEMAPS>;
    hipLaunchKernelGGL(frame_kernel, dim3((unsigned)max_nf, (unsigned)n_slots), dim3(256), 0, st, a);
    if (const int rc = egm_track(rec_dev, 0, max_nf, slots_dev, n_slots, long_windows, st)) return rc;
    hipLaunchKernelGGL(egm_voiced_kernel<true>, dim3((unsigned)max_nf, (unsigned)n_slots), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int egm_ragged_records(void* plan, const float* rings_dev, int64_t ring_len, const EgmSlot* slots_dev, int n_slots, int max_nf, float* scale_dev,
                       float* rec_dev, hipStream_t st, bool long_windows, int feature_set) {
    return ragged_records("egm_ragged_records", plan, rings_dev, ring_len, slots_dev, n_slots, max_nf, scale_dev, rec_dev, st, long_windows, feature_set);
}

int egm_ragged_functionals(void* plan, const float* rings_dev, int64_t ring_len, const EgmSlot* slots_dev, int n_slots, int max_nf,
                           float* scale_dev, float* rec_dev, float* out_dev, hipStream_t st, bool long_windows, int feature_set) {
    if (!out_dev) return fail(KM_ERR_INVALID_ARG, "egm_ragged_functionals: bad argument");
    if (const int rc = ragged_records("egm_ragged_functionals", plan, rings_dev, ring_len, slots_dev, n_slots, max_nf, scale_dev, rec_dev, st,
                                      long_windows, feature_set))
        return rc;
    return egm_functional(rec_dev, 0, max_nf, slots_dev, n_slots, out_dev, long_windows, st, feature_set);
}

}  // namespace km

using namespace km;

extern "C" {

int km_egemaps_plan_create(void** plan_out) {
    if (!plan_out) return fail(KM_ERR_INVALID_ARG, "km_egemaps_plan_create: NULL argument");
    std::unique_ptr<EgmPlan> p(build_egm_plan());
    if (int rc = p->d.alloc((int64_t)p->h.size(), "km_egemaps_plan_create")) return rc;
    HIP_TRY(hipMemcpy(p->d, p->h.data(), p->h.size() * sizeof(float), hipMemcpyHostToDevice));
    *plan_out = p.release();
    return KM_OK;
}

int km_egemaps_plan_destroy(void* plan) {
    if (!plan) return KM_OK;
    delete static_cast<EgmPlan*>(plan);
    return KM_OK;
}

int64_t km_egemaps_num_frames(int64_t L) { return L < egm::N60 ? 0 : (L - egm::N60) / egm::HOP + 1; }

int64_t km_egemaps_workspace_floats(int64_t B, int64_t L) {
    if (B <= 0 || L <= 0) return -1;
    return B * (km_egemaps_num_frames(L) * egm::REC + 4);
}

// km_egemaps_functionals and km_egemaps_functionals_long (`who` is the name the texts carry).  The latter takes windows of up to 2^20
// samples: beyond 2048 frames the two per-window kernels run at their long tier between the same per-frame kernels; up to 2048
// frames it launches what the former launches
// Its checks and its launches up to the frame records (peak, frame, track, voiced) are egm_window_records, which km_egemaps_llds shares:
// *rec_out is where the records of the B windows lie in the workspace, *nf_out their frame count, *long_tier_out the per-window tier
static int egm_window_records(const char* who, int feature_set, bool long_windows, void* plan, const float* audio_dev, int64_t B, int64_t L,
                              int32_t normalize, float* work_dev, int64_t work_floats, const float* out_dev, void* stream, float** rec_out,
                              int64_t* nf_out, bool* long_tier_out, bool launch = true) {
    using namespace egm;
    if (!plan || !audio_dev || !work_dev || !out_dev || B <= 0 || L <= 0) return fail(KM_ERR_INVALID_ARG, "%s: bad argument", who);
    const int64_t nf = km_egemaps_num_frames(L);
    if (nf < 1) return fail(KM_ERR_INVALID_ARG, "%s: the window is shorter than one 60 ms frame (%lld samples)", who, (long long)L);
    if (long_windows && L > MAX_WINDOW)
        return fail(KM_ERR_UNSUPPORTED, "%s: a window of %lld samples, at most %lld (65.5 s)", who, (long long)L, (long long)MAX_WINDOW);
    if (!long_windows && nf > ShortTier::MAXF)
        return fail(KM_ERR_UNSUPPORTED, "%s: %lld frames per window, at most %d (20.5 s)", who, (long long)nf, ShortTier::MAXF);
    if (work_floats < km_egemaps_workspace_floats(B, L)) return fail(KM_ERR_WORKSPACE, "%s: workspace too small", who);
    if (B > 65535) return fail(KM_ERR_UNSUPPORTED, "%s: at most 65535 windows per call", who);
    if (!launch) return KM_OK;                     // km_egemaps_llds with an empty frame grid: the checks alone
    const bool long_tier = nf > ShortTier::MAXF;
    EgmPlan* p = static_cast<EgmPlan*>(plan);
    hipStream_t st = (hipStream_t)stream;
    float* scale = work_dev;                       // (B), padded to 4 B floats
    float* rec = work_dev + 4 * B;
    if (normalize) {
        hipLaunchKernelGGL(egm_peak_kernel<false>, dim3((unsigned)B), dim3(256), 0, st, audio_dev, L, (const EgmSlot*)nullptr, 0, scale);
        HIP_TRY(hipGetLastError());
    }
    const EgmArgs a = egm_args(p, audio_dev, L, (int)nf, normalize ? scale : nullptr, rec);
    const auto frame_kernel = feature_set == SET_GEMAPS ? egm_frame_kernel<false, SET_GEMAPS> : egm_frame_kernel<false, SET_EGEMAPS>;
    hipLaunchKernelGGL(frame_kernel, dim3((unsigned)nf, (unsigned)B), dim3(256), 0, st, a);
    if (const int rc = egm_track(rec, (int)nf, (int)nf, nullptr, (int)B, long_tier, st)) return rc;
    hipLaunchKernelGGL(egm_voiced_kernel<false>, dim3((unsigned)nf, (unsigned)B), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    *rec_out = rec; *nf_out = nf; *long_tier_out = long_tier;
    return KM_OK;
}

static int egm_functionals(const char* who, int feature_set, bool long_windows, void* plan, const float* audio_dev, int64_t B, int64_t L, int32_t normalize,
                           float* work_dev, int64_t work_floats, float* out_dev, void* stream) {
    float* rec = nullptr; int64_t nf = 0; bool long_tier = false;
    if (const int rc = egm_window_records(who, feature_set, long_windows, plan, audio_dev, B, L, normalize, work_dev, work_floats, out_dev, stream, &rec,
                                          &nf, &long_tier))
        return rc;
    return egm_functional(rec, (int)nf, (int)nf, nullptr, (int)B, out_dev, long_tier, (hipStream_t)stream, feature_set);
}

int km_egemaps_functionals(void* plan, const float* audio_dev, int64_t B, int64_t L, int32_t normalize, float* work_dev,
                           int64_t work_floats, float* out_dev, void* stream) {
    return egm_functionals("km_egemaps_functionals", egm::SET_EGEMAPS, false, plan, audio_dev, B, L, normalize, work_dev, work_floats, out_dev, stream);
}

int km_egemaps_functionals_long(void* plan, const float* audio_dev, int64_t B, int64_t L, int32_t normalize, float* work_dev,
                                int64_t work_floats, float* out_dev, void* stream) {
    return egm_functionals("km_egemaps_functionals_long", egm::SET_EGEMAPS, true, plan, audio_dev, B, L, normalize, work_dev, work_floats, out_dev, stream);
}

// either call above for either feature set: out_dev is (B, km_feature_set_width(feature_set)).  With set 0 the launches are theirs
int km_egemaps_functionals_set(void* plan, int32_t feature_set, int32_t long_windows, const float* audio_dev, int64_t B, int64_t L, int32_t normalize,
                               float* work_dev, int64_t work_floats, float* out_dev, void* stream) {
    if (!egm::set_known(feature_set))
        return fail(KM_ERR_INVALID_ARG, "km_egemaps_functionals_set: feature set %d, 0 (eGeMAPS) or 1 (GeMAPS)", (int)feature_set);
    return egm_functionals("km_egemaps_functionals_set", feature_set, long_windows != 0, plan, audio_dev, B, L, normalize, work_dev, work_floats, out_dev,
                           stream);
}

// The low-level descriptors per frame, out_dev (B, km_egemaps_lld_frames(L, fps), km_egemaps_lld_width(feature_set)): the checks and
// the launches of km_egemaps_functionals_set up to the records, then egm_lld_kernel where that has the functionals (km_egemaps_lld.hip)
int km_egemaps_llds(void* plan, int32_t feature_set, int32_t long_windows, const float* audio_dev, int64_t B, int64_t L, int32_t normalize,
                    float* work_dev, int64_t work_floats, double fps, float* out_dev, void* stream) {
    const char* who = "km_egemaps_llds";
    if (!egm::set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "%s: feature set %d, 0 (eGeMAPS) or 1 (GeMAPS)", who, (int)feature_set);
    if (fps != 0.0 && egm_lld_frames(0, fps) < 0)
        return fail(KM_ERR_INVALID_ARG, "%s: fps %g, finite and within 1 .. 400 (0: the native 100 Hz)", who, fps);
    const int64_t T_out = egm_lld_frames(L, fps);
    float* rec = nullptr; int64_t nf = 0; bool long_tier = false;
    if (const int rc = egm_window_records(who, feature_set, long_windows != 0, plan, audio_dev, B, L, normalize, work_dev, work_floats, out_dev, stream,
                                          &rec, &nf, &long_tier, T_out != 0))
        return rc;
    if (T_out == 0) return KM_OK;                  // less than one row of the grid: nothing was launched
    return egm_lld(rec, (int)nf, (int)nf, (int)B, T_out, fps, out_dev, (hipStream_t)stream, feature_set);
}

// per-frame records of the most recent call on this workspace, for the tests: (B, nf, 36) floats
int km_egemaps_records(const float* work_dev, int64_t B, int64_t L, float* rec_host, void* stream) {
    if (!work_dev || !rec_host || B <= 0) return fail(KM_ERR_INVALID_ARG, "km_egemaps_records: bad argument");
    const int64_t nf = km_egemaps_num_frames(L);
    HIP_TRY(hipMemcpyAsync(rec_host, work_dev + 4 * B, (size_t)B * nf * egm::REC * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return KM_OK;
}

}  // extern "C"
