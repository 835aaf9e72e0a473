// Audio front of the KoeMorphModel stream engine (km_koemorph_audio_*, include/koemorph.h): audio is pushed per stream, and the mel and
// emotion rows km_koemorph_stream_step takes come out, with their per-stream counts -- samples, rows and counters on the device.
//
// The law.  hop = int(16000 / fps).  Stream s has received n_s samples since creation or its last reset; frame k is due as soon as
// n_s >= (k + 1) * hop, so after a push the stream has K = n_s / hop frames and the push renders frames c_s .. K - 1 (c_s: the count
// before it).  Integer arithmetic: the two tracks never drift apart or behind the audio.
//   mel row k      the row of the 512-point STFT frame centred on sample k * hop of the stream (periodic Hann, "window" normalisation,
//                  HTK filters 80 .. 8000 Hz, log(mel + 1e-8)), reflected at the stream's first sample only: with hop >= 257 every frame
//                  has its samples when it is due.  A function of the stream's samples alone.
//   emotion row k  a push that leaves new frames sets the window: a0 = the smallest multiple of 160 >= n_s - W (0 while n_s <= W),
//                  len = n_s - a0, m = a0 / 160, nf = (len - 960) / 160 + 1 (0 below 960).  Its descriptors are those of km_egemaps_llds
//                  on the window's samples (normalised, native rate).  Row k sits at p = (double)(k * hop) / 160.0, j = floor(p) - m,
//                  w = p - floor(p): frame 0 for j < 0, the last frame for j >= nf - 1, frame j for w == 0, otherwise
//                  fmaf((float)w, b - a, a) between frames j and j + 1 with egm_lld_kernel's exception for the columns smoothed over
//                  non-zero values.  Written emotion_dim wide, zeros to the right; a window without a frame gives a row of zeros.
//
// Sample i of a life sits at (origin + i) mod ring_len: a reset leaves the ring's write position where it stands and makes it the next
// life's origin, so nothing of the ring needs clearing (a frame never reaches behind its life's sample 0: it is mirrored there).
//
// A push is SEVEN launches whatever the streams' phases are: kma_advance_kernel (samples into the rings, counters, the push's table and
// the eGeMAPS slots), kma_mel_rows_kernel, the four record kernels of the ragged eGeMAPS chain on the windows where they lie in the
// rings (egm_ragged_records), kma_lld_rows_kernel.  Nothing allocates, synchronises or reads back outside create.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>

#include "km_api_internal.h"
#include "km_context.h"
#include "km_device.h"
#include "km_egemaps_lld.h"
#include "km_egemaps_ragged.h"
#include "km_egemaps_window.h"
#include "km_koemorph_audio.h"

namespace km {

void EgmPlanDelete::operator()(void* p) const { (void)km_egemaps_plan_destroy(p); }

namespace kma {
constexpr int NFFT = 512, NBIN = NFFT / 2 + 1;
constexpr int MAX_MELS = 256, MAX_NNZ = 1024;      // what kma_mel_rows_kernel holds in LDS
constexpr int MIN_HOP = NFFT / 2 + 1;              // frame 0 needs samples up to index 256
constexpr double MIN_FPS = 10.0;
}  // namespace kma

// ---- samples into the rings, counters, the push's table ----
struct KmaAdvArgs {
    const float* samples; const int* counts; int M;         // (N, M) samples; counts (N) or null = M for every stream
    float* ring; int ring_len;
    long long* total; int* origin; KmaEntry* table; EgmSlot* slots; int* row_counts;
    int hop, W;
};

__global__ __launch_bounds__(256) void kma_advance_kernel(KmaAdvArgs a) {
    const int s = blockIdx.x, tid = threadIdx.x;
    int n = a.counts ? a.counts[s] : a.M;
    n = n < 0 ? 0 : (n > a.M ? a.M : n);
    const long long n0 = a.total[s];
    const int origin = a.origin[s];
    const int p0 = (int)((origin + n0) % a.ring_len);
    const float* src = a.samples + (int64_t)s * a.M;
    float* dst = a.ring + (int64_t)s * a.ring_len;
    for (int i = tid; i < n; i += 256) {
        int p = p0 + i;                                       // i < M <= max_samples < ring_len
        p = p >= a.ring_len ? p - a.ring_len : p;
        dst[p] = src[i];
    }
    __syncthreads();                                          // every thread has read the counter
    if (tid == 0) {
        EgmSlot sl;
        const KmaEntry e = kma_schedule(n0, n, a.hop, a.W, a.ring_len, origin, s, &sl);
        a.table[s] = e;
        a.slots[s] = sl;
        a.total[s] = e.total;
        a.row_counts[s] = e.rows;
    }
}

// the masked streams (mask null: all) start again at sample 0, where their ring's write position stands
__global__ __launch_bounds__(256) void kma_reset_kernel(const unsigned char* __restrict__ mask, long long* total, int* origin, int ring_len, int n) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n || (mask && !mask[s])) return;
    origin[s] = (int)((origin[s] + total[s]) % ring_len);
    total[s] = 0;
}

// ---- one mel row per workgroup: Hann window, 512-point transform, power, HTK filters, log(mel + eps) ----
struct KmaMelArgs {
    const float* ring; int ring_len;
    const KmaEntry* table;
    int hop, n_mels, max_rows;
    const float* window; const float2* twiddle;              // MelPlan: n_fft window values, W_512^q
    const int* fb_start; const int* fb_count; const int* fb_offset; const float* fb_weight; int fb_nnz;
    LogParams lp;
    float* out;                                               // (N, max_rows, n_mels)
};

__global__ __launch_bounds__(256) void kma_mel_rows_kernel(KmaMelArgs a) {
    using namespace kma;
    __shared__ float2 buf[NFFT];
    __shared__ float pw[NBIN + 3];
    __shared__ int fbs[MAX_MELS], fbc[MAX_MELS], fbo[MAX_MELS];
    __shared__ float fbw[MAX_NNZ];
    const int s = blockIdx.y, r = blockIdx.x, tid = threadIdx.x;
    const KmaEntry e = a.table[s];
    if (r >= e.rows) return;
    for (int i = tid; i < a.n_mels; i += 256) { fbs[i] = a.fb_start[i]; fbc[i] = a.fb_count[i]; fbo[i] = a.fb_offset[i]; }
    for (int i = tid; i < a.fb_nnz; i += 256) fbw[i] = a.fb_weight[i];
    // the frame centred on sample k * hop, reflected at the stream's first sample; bit-reversed for the decimation in time below
    const long long base = (e.first + r) * (long long)a.hop - NFFT / 2;
    const float* x = a.ring + (int64_t)s * a.ring_len;
    for (int n = tid; n < NFFT; n += 256) {
        long long q = base + n;
        q = q < 0 ? -q : q;
        buf[__brev((unsigned)n) >> 23] = make_float2(x[(int)((e.origin + q) % a.ring_len)] * a.window[n], 0.f);
    }
    __syncthreads();
    // nine radix-2 stages, one butterfly per thread and stage: a row is one transform of its own 512 samples
#pragma unroll 1
    for (int st = 1; st <= 9; ++st) {
        const int half = 1 << (st - 1);
        const int j = tid & (half - 1), i0 = ((tid >> (st - 1)) << st) + j, i1 = i0 + half;
        const float2 tw = a.twiddle[j << (9 - st)];
        const float2 u = buf[i0], v = buf[i1];
        const float2 t = make_float2(v.x * tw.x - v.y * tw.y, v.x * tw.y + v.y * tw.x);
        buf[i0] = make_float2(u.x + t.x, u.y + t.y);
        buf[i1] = make_float2(u.x - t.x, u.y - t.y);
        __syncthreads();
    }
    for (int k = tid; k < NBIN; k += 256) { const float2 z = buf[k]; pw[k] = z.x * z.x + z.y * z.y; }
    __syncthreads();
    float* o = a.out + ((int64_t)s * a.max_rows + r) * a.n_mels;
    for (int m = tid; m < a.n_mels; m += 256) {
        const int cnt = fbc[m];
        const float* pr = pw + fbs[m];
        const float* wt = fbw + fbo[m];
        float acc = 0.f;
        for (int i = 0; i < cnt; ++i) acc = fmaf(pr[i], wt[i], acc);
        o[m] = log_one_t<KM_LOG_LN_EPS>(a.lp, acc, 0.f, 0.f);
    }
}

// ---- the descriptor rows of a push: egm_lld_kernel's staging and smoothing on the frames the stream's new rows touch, the rows on
// the shifted grid p = k * hop / 160 - m ----
struct KmaLldArgs {
    const float* recs; int rec_frames;                       // (N, rec_frames, 36) records of the streams' windows
    const KmaEntry* table;
    int hop, rows_tile, max_rows, emotion_dim;
    float* out;                                               // (N, max_rows, emotion_dim)
};

template <int SET>
__global__ __launch_bounds__(256) void kma_lld_rows_kernel(KmaLldArgs a) {
    using namespace egm;
    constexpr int W = lld_width(SET);
    __shared__ float rec_s[LLD_STAGE * REC];
    __shared__ float f0s_s[LLD_STAGE];
    __shared__ float lld_s[LLD_CORE * W];
    const int tid = threadIdx.x, s = blockIdx.y;
    const KmaEntry e = a.table[s];
    const int k0 = blockIdx.x * a.rows_tile;
    const int nrow = e.rows - k0 < a.rows_tile ? e.rows - k0 : a.rows_tile;
    if (nrow < 1) return;
    float* o = a.out + ((int64_t)s * a.max_rows + k0) * a.emotion_dim;
    const int nf = e.nf;
    if (nf == 0) {                                            // a window without a frame: rows of zeros
        for (int idx = tid; idx < nrow * a.emotion_dim; idx += 256) o[idx] = 0.f;
        return;
    }
    // frame j and weight w of the push's row r
    auto coord = [&](int r, double& w) {
        w = 0.0;
        const double p = (double)((e.first + r) * (long long)a.hop) / 160.0, fl = floor(p);
        const long long j = (long long)fl - e.m;
        if (j < 0) return 0;                                  // creation rules this out
        if (j >= (long long)(nf - 1)) return nf - 1;
        w = p - fl;
        return (int)j;
    };
    double w_first, w_last;
    const int f_lo = coord(k0, w_first);
    const int j_last = coord(k0 + nrow - 1, w_last);
    const int f_hi = w_last != 0.0 ? j_last + 1 : j_last;                // w != 0 only for j < nf - 1
    if (f_hi - f_lo + 1 > LLD_CORE) return;                              // the host sizes rows_tile so that this never happens; never index past LDS
    const int s_lo = f_lo - 2 > 0 ? f_lo - 2 : 0, s_hi = f_hi + 2 < nf ? f_hi + 2 : nf - 1;
    const float* rec = a.recs + ((int64_t)s * a.rec_frames + s_lo) * REC;
    for (int i = tid; i < (s_hi - s_lo + 1) * REC; i += 256) rec_s[i] = rec[i];
    __syncthreads();
    auto raw = [&](int t, int field) { return rec_s[(t - s_lo) * REC + field]; };
    {
        const int fa = f_lo - 1 > 0 ? f_lo - 1 : 0, fb = f_hi + 1 < nf ? f_hi + 1 : nf - 1;
        for (int t = fa + tid; t <= fb; t += 256) {
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
        const int t = f_lo + idx / W, ec = lld_ecol<SET>(idx % W), field = lld_field(ec);
        float r = 0.f;
        if (ec == LLD_FIRST_NZ) r = f0s(t) > 0.f ? 12.0f * log2f(f0s(t) / 27.5f) : 0.f;
        else if (ec < LLD_FIRST_NZ) {
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
    for (int idx = tid; idx < nrow * a.emotion_dim; idx += 256) {
        const int row = idx / a.emotion_dim, c = idx - row * a.emotion_dim;
        float r = 0.f;                                                   // zeros to the right of the descriptors
        if (c < W) {
            double w;
            const int j = coord(k0 + row, w);
            const float va = lld_s[(j - f_lo) * W + c];
            r = va;
            if (w != 0.0) {                                              // then j + 1 <= f_hi
                const float vb = lld_s[(j + 1 - f_lo) * W + c];
                if (lld_ecol<SET>(c) < LLD_FIRST_NZ || (va != 0.f && vb != 0.f)) r = fmaf((float)w, vb - va, va);
                else r = w <= 0.5 ? va : vb;
            }
        }
        o[idx] = r;
    }
}

// ---- host ----
struct KmaPlan { int hop = 0, rows_tile = 0; int64_t max_rows = 0, ring_len = 0, W = 0, max_nf = 0, launches = 0, device_bytes = 0; };

static int kma_guard(km_handle h, const char* who, bool created) {
    if (!h) return fail(KM_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (h->kind != 2) return fail(KM_ERR_INVALID_ARG, "%s: not a KoeMorphModel handle (km_koemorph_create), kind %d", who, h->kind);
    if (created && h->ka.streams == 0) return fail(KM_ERR_INVALID_ARG, "%s: no audio engine: call km_koemorph_audio_create", who);
    return KM_OK;
}

// The one function behind km_koemorph_audio_plan and km_koemorph_audio_create: KM_OK and the plan, or the refusal
static int kma_plan(Context* c, const char* who, int64_t N, double fps, double window_s, int64_t max_samples, int feature_set, KmaPlan* out) {
    using namespace kma;
    if (N < 1) return fail(KM_ERR_INVALID_ARG, "%s: n_streams %lld < 1", who, (long long)N);
    if (N > 65535) return fail(KM_ERR_INVALID_ARG, "%s: n_streams %lld, at most 65535", who, (long long)N);
    if (!egm::set_known(feature_set)) return fail(KM_ERR_INVALID_ARG, "%s: feature set %d, 0 (eGeMAPS) or 1 (GeMAPS)", who, feature_set);
    if (!std::isfinite(fps) || fps <= 0.0) return fail(KM_ERR_INVALID_ARG, "%s: fps %g is not a positive finite number", who, fps);
    if (!std::isfinite(window_s) || window_s <= 0.0 || window_s > 4096.0)
        return fail(KM_ERR_INVALID_ARG, "%s: emotion window of %g s, a positive number of seconds", who, window_s);
    if (max_samples < 1 || max_samples > ((int64_t)1 << 20))
        return fail(KM_ERR_INVALID_ARG, "%s: max_samples %lld, 1 .. 2^20", who, (long long)max_samples);
    if (fps < MIN_FPS) return fail(KM_ERR_UNSUPPORTED, "%s: fps %g, at least %g", who, fps, MIN_FPS);
    KmaPlan p;
    p.hop = (int)(16000.0 / fps);
    if (p.hop < MIN_HOP) return fail(KM_ERR_UNSUPPORTED, "%s: hop %d (fps %g), at least %d: a frame must hold its samples when it is due", who, p.hop, fps, MIN_HOP);
    p.W = (int64_t)(window_s * 16000.0);
    const int64_t need = max_samples + p.hop + 1120;
    if (p.W < need)
        return fail(KM_ERR_INVALID_ARG, "%s: emotion window of %lld samples, at least max_samples + hop + 1120 = %lld", who, (long long)p.W, (long long)need);
    p.max_nf = (p.W - 960) / 160 + 1;
    if (p.max_nf > egm::ShortTier::MAXF)
        return fail(KM_ERR_UNSUPPORTED, "%s: an emotion window of %lld frames, at most %d (20.5 s)", who, (long long)p.max_nf, egm::ShortTier::MAXF);
    p.max_rows = max_samples / p.hop + 1;
    if (p.max_rows > 1024) return fail(KM_ERR_UNSUPPORTED, "%s: %lld rows per push, at most 1024", who, (long long)p.max_rows);
    const km_koemorph_config& k = c->kmm;
    if (k.mel_dim < 1 || k.mel_dim > MAX_MELS) return fail(KM_ERR_UNSUPPORTED, "%s: mel_dim %d, 1 .. %d", who, k.mel_dim, MAX_MELS);
    if (k.emotion_dim < egm::lld_width(feature_set))
        return fail(KM_ERR_UNSUPPORTED, "%s: emotion_dim %d is narrower than the %d descriptors of the feature set", who, k.emotion_dim, egm::lld_width(feature_set));
    p.ring_len = p.W + max_samples;
    // rows per tile of kma_lld_rows_kernel: the frames j(k0) .. j(k0 + rows - 1) + 1 are at most (rows - 1) * hop / 160 + 3, and LLD_CORE fit
    const double r = 1.0 + std::floor((egm::LLD_CORE - 4) * 160.0 / p.hop);
    p.rows_tile = r < egm::LLD_CORE ? (int)r : egm::LLD_CORE;
    p.launches = 7;
    p.device_bytes = N * (4 * p.ring_len + 8 + 4 + (int64_t)sizeof(KmaEntry) + (int64_t)sizeof(EgmSlot) + 4 + 4 * p.max_nf * egm::REC);
    *out = p;
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" {

int km_koemorph_audio_plan(km_handle h, int64_t n_streams, double fps, double emotion_window_s, int64_t max_samples, int32_t feature_set,
                           int64_t out[8]) {
    const char* who = "km_koemorph_audio_plan";
    if (int rc = kma_guard(h, who, false)) return rc;
    if (!out) return fail(KM_ERR_INVALID_ARG, "%s: out is NULL", who);
    for (int i = 0; i < 8; ++i) out[i] = 0;
    KmaPlan p;
    const int rc = kma_plan(h, who, n_streams, fps, emotion_window_s, max_samples, feature_set, &p);
    if (rc == KM_ERR_UNSUPPORTED) return KM_OK;                          // out[0] = 0; km_last_error holds the reason
    if (rc != KM_OK) return rc;
    out[0] = 1; out[1] = p.hop; out[2] = p.max_rows; out[3] = p.ring_len; out[4] = p.W; out[5] = p.max_nf; out[6] = p.launches; out[7] = p.device_bytes;
    return KM_OK;
}

int km_koemorph_audio_schedule(int64_t samples_before, int64_t pushed, int32_t hop, int64_t window_samples, int64_t ring_len, int64_t origin,
                               int32_t stream, int64_t out[10]) {
    const char* who = "km_koemorph_audio_schedule";
    if (!out) return fail(KM_ERR_INVALID_ARG, "%s: out is NULL", who);
    if (samples_before < 0 || pushed < 0 || pushed > ((int64_t)1 << 20)) return fail(KM_ERR_INVALID_ARG, "%s: %lld samples before, %lld pushed", who, (long long)samples_before, (long long)pushed);
    if (origin < 0 || origin >= ring_len) return fail(KM_ERR_INVALID_ARG, "%s: origin %lld outside the ring of %lld", who, (long long)origin, (long long)ring_len);
    if (hop < 1 || window_samples < 1 || window_samples > ((int64_t)1 << 30) || ring_len < window_samples || ring_len > ((int64_t)1 << 30))
        return fail(KM_ERR_INVALID_ARG, "%s: hop %d, window %lld, ring %lld", who, (int)hop, (long long)window_samples, (long long)ring_len);
    EgmSlot sl;
    const KmaEntry e = kma_schedule(samples_before, (int)pushed, hop, (int)window_samples, (int)ring_len, (int)origin, stream, &sl);
    out[0] = e.first; out[1] = e.rows; out[2] = e.a0; out[3] = e.len; out[4] = e.nf; out[5] = e.m; out[6] = e.total;
    out[7] = sl.stream; out[8] = sl.start; out[9] = sl.nf;
    return KM_OK;
}

int km_koemorph_audio_create(km_handle h, int64_t n_streams, double fps, double emotion_window_s, int64_t max_samples, int32_t feature_set) {
    const char* who = "km_koemorph_audio_create";
    if (int rc = kma_guard(h, who, false)) return rc;
    Context* c = h;
    KmaPlan p;
    if (int rc = kma_plan(c, who, n_streams, fps, emotion_window_s, max_samples, feature_set, &p)) return rc;
    if (!c->host_finalized) return fail(KM_ERR_NOT_FINALIZED, "%s: call km_finalize first", who);
    if (int rc = need_ready(c)) return rc;
    const int64_t N = n_streams;
    HIP_TRY(hipDeviceSynchronize());                // a second create replaces the first: nothing of it may be in flight
    c->ka = KoeMorphAudio{};
    KoeMorphAudio ka;
    km_mel_config mc{};                             // MelConfig.torchaudio(16000, fps, 512, mel_dim, 80, 8000, normalized, "reflect", 1e-8)
    mc.sample_rate = 16000; mc.n_fft = kma::NFFT; mc.hop_length = p.hop; mc.n_mels = c->kmm.mel_dim; mc.f_min = 80.0f; mc.f_max = 8000.0f;
    mc.mel_scale = KM_MEL_HTK; mc.slaney_norm = 0; mc.pad_mode = KM_PAD_REFLECT; mc.window_norm = 1; mc.log_mode = KM_LOG_LN_EPS;
    mc.amin = 1e-10f; mc.top_db = 80.0f; mc.db_add = 0.0f; mc.db_scale = 1.0f; mc.log_eps = 1e-8f;
    ka.mel.reset(build_mel_plan(mc));
    if ((int64_t)ka.mel->fb_weight.size() > kma::MAX_NNZ)
        return fail(KM_ERR_UNSUPPORTED, "%s: %lld filter taps at mel_dim %d, at most %d", who, (long long)ka.mel->fb_weight.size(), mc.n_mels, kma::MAX_NNZ);
    for (int i = 0; i < mc.n_mels; ++i)
        if (ka.mel->fb_start[i] + ka.mel->fb_count[i] > kma::NBIN) return fail(KM_ERR_UNSUPPORTED, "%s: filter %d reaches past bin %d", who, i, kma::NBIN - 1);
    if (int rc = upload_mel_plan(ka.mel.get())) return rc;
    void* eplan = nullptr;
    if (int rc = km_egemaps_plan_create(&eplan)) return rc;
    ka.egm.reset(eplan);
    if (int rc = ka.ring.alloc(N * p.ring_len, who)) return rc;
    if (int rc = ka.total.alloc(N, who)) return rc;
    if (int rc = ka.origin.alloc(N, who)) return rc;
    if (int rc = ka.table.alloc(N * (int64_t)sizeof(KmaEntry), who)) return rc;
    if (int rc = ka.slots.alloc(N * (int64_t)sizeof(EgmSlot), who)) return rc;
    if (int rc = ka.scale.alloc(N, who)) return rc;
    if (int rc = ka.rec.alloc(N * p.max_nf * egm::REC, who)) return rc;
    HIP_TRY(hipMemset(ka.ring, 0, (size_t)ka.ring.bytes()));
    HIP_TRY(hipMemset(ka.total, 0, (size_t)ka.total.bytes()));
    HIP_TRY(hipMemset(ka.origin, 0, (size_t)ka.origin.bytes()));
    HIP_TRY(hipMemset(ka.table, 0, (size_t)ka.table.bytes()));
    HIP_TRY(hipMemset(ka.slots, 0xff, (size_t)ka.slots.bytes()));        // stream -1: empty
    HIP_TRY(hipMemset(ka.scale, 0, (size_t)ka.scale.bytes()));
    HIP_TRY(hipMemset(ka.rec, 0, (size_t)ka.rec.bytes()));
    HIP_TRY(hipDeviceSynchronize());
    ka.hop = p.hop; ka.rows_tile = p.rows_tile; ka.feature_set = feature_set; ka.max_samples = max_samples; ka.ring_len = p.ring_len;
    ka.W = p.W; ka.max_nf = p.max_nf; ka.max_rows = p.max_rows;
    ka.streams = N;
    c->ka = std::move(ka);
    return KM_OK;
}

int km_koemorph_audio_rows(km_handle h, const float* samples_dev, int64_t M, const int32_t* counts_dev, float* mel_rows_dev,
                           float* emotion_rows_dev, int32_t* row_counts_dev, void* stream) {
    const char* who = "km_koemorph_audio_rows";
    if (int rc = kma_guard(h, who, true)) return rc;
    Context* c = h;
    KoeMorphAudio& ka = c->ka;
    if (!samples_dev) return fail(KM_ERR_INVALID_ARG, "%s: samples_dev is NULL", who);
    if (!mel_rows_dev) return fail(KM_ERR_INVALID_ARG, "%s: mel_rows_dev is NULL", who);
    if (!emotion_rows_dev) return fail(KM_ERR_INVALID_ARG, "%s: emotion_rows_dev is NULL", who);
    if (!row_counts_dev) return fail(KM_ERR_INVALID_ARG, "%s: row_counts_dev is NULL", who);
    if (M < 1 || M > ka.max_samples) return fail(KM_ERR_INVALID_ARG, "%s: %lld samples per stream, 1 .. %lld (max_samples)", who, (long long)M, (long long)ka.max_samples);
    hipStream_t st = (hipStream_t)stream;
    const unsigned N = (unsigned)ka.streams;
    KmaEntry* table = reinterpret_cast<KmaEntry*>(ka.table.p);
    EgmSlot* slots = reinterpret_cast<EgmSlot*>(ka.slots.p);
    KmaAdvArgs a{};
    a.samples = samples_dev; a.counts = counts_dev; a.M = (int)M; a.ring = ka.ring; a.ring_len = (int)ka.ring_len; a.total = ka.total; a.origin = ka.origin;
    a.table = table; a.slots = slots; a.row_counts = row_counts_dev; a.hop = ka.hop; a.W = (int)ka.W;
    hipLaunchKernelGGL(kma_advance_kernel, dim3(N), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    MelPlan* mp = ka.mel.get();
    KmaMelArgs m{};
    m.ring = ka.ring; m.ring_len = (int)ka.ring_len; m.table = table; m.hop = ka.hop; m.n_mels = mp->cfg.n_mels; m.max_rows = (int)ka.max_rows;
    m.window = mp->d_window; m.twiddle = reinterpret_cast<const float2*>(mp->d_twiddle.p);
    m.fb_start = mp->d_fb_start; m.fb_count = mp->d_fb_count; m.fb_offset = mp->d_fb_offset; m.fb_weight = mp->d_fb_weight;
    m.fb_nnz = (int)mp->fb_weight.size(); m.lp = plan_log_params(mp); m.out = mel_rows_dev;
    hipLaunchKernelGGL(kma_mel_rows_kernel, dim3((unsigned)ka.max_rows, N), dim3(256), 0, st, m);
    HIP_TRY(hipGetLastError());
    if (int rc = egm_ragged_records(ka.egm.get(), ka.ring, ka.ring_len, slots, (int)N, (int)ka.max_nf, ka.scale, ka.rec, st, false, ka.feature_set))
        return rc;
    KmaLldArgs l{};
    l.recs = ka.rec; l.rec_frames = (int)ka.max_nf; l.table = table; l.hop = ka.hop; l.rows_tile = ka.rows_tile; l.max_rows = (int)ka.max_rows;
    l.emotion_dim = c->kmm.emotion_dim; l.out = emotion_rows_dev;
    const dim3 grid((unsigned)((ka.max_rows + ka.rows_tile - 1) / ka.rows_tile), N);
    if (ka.feature_set == egm::SET_GEMAPS) hipLaunchKernelGGL(kma_lld_rows_kernel<egm::SET_GEMAPS>, grid, dim3(256), 0, st, l);
    else hipLaunchKernelGGL(kma_lld_rows_kernel<egm::SET_EGEMAPS>, grid, dim3(256), 0, st, l);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_koemorph_audio_reset(km_handle h, const uint8_t* mask_dev, void* stream) {
    const char* who = "km_koemorph_audio_reset";
    if (int rc = kma_guard(h, who, true)) return rc;
    KoeMorphAudio& ka = h->ka;
    hipLaunchKernelGGL(kma_reset_kernel, dim3((unsigned)((ka.streams + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask_dev, ka.total.p, ka.origin.p,
                       (int)ka.ring_len, (int)ka.streams);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_koemorph_audio_samples(km_handle h, int64_t* totals_dev, void* stream) {
    const char* who = "km_koemorph_audio_samples";
    if (int rc = kma_guard(h, who, true)) return rc;
    if (!totals_dev) return fail(KM_ERR_INVALID_ARG, "%s: totals_dev is NULL", who);
    HIP_TRY(hipMemcpyAsync(totals_dev, h->ka.total.p, (size_t)h->ka.streams * sizeof(int64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return KM_OK;
}

int km_koemorph_audio_destroy(km_handle h) {
    if (int rc = kma_guard(h, "km_koemorph_audio_destroy", false)) return rc;
    if (h->ka.streams == 0) return KM_OK;
    HIP_TRY(hipDeviceSynchronize());
    h->ka = KoeMorphAudio{};
    return KM_OK;
}

}  // extern "C"
