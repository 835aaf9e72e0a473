// Rational sample-rate conversion on the device: whole clips and many stateful streams (km_resampler_* / km_resample_clip).
//
// The output law.  With up / down the reduced ratio, h the caller's 2 half + 1 taps and x[0..N) the input,
//     y[m] = sum_j x[j] h[m down - j up + half],      n_out(N) = ceil(N up / down),
// over the j whose tap index lies in [0, 2 half]; samples before 0 and from N on are zeros.  Write c = m down + half, q = c / up,
// p = c % up: the taps output m touches are h[p + k up] for k = 0 .. K - 1 (K = 2 half / up + 1) on the samples x[q - k], so the
// filter is stored as a polyphase table tab[p][k] = float(h[p + k up]) (0 where p + k up > 2 half) and
//     y[m] = fmaf chain over k = K - 1 .. 0 (ascending j) of x[q - k] * tab[p][k],   starting from +0.
// THE BIT RULE: every path below evaluates exactly this chain for output m -- all K terms, in this order, a sample outside the
// signal entering as 0.0f -- so an output has the same bits from the clip kernel, from push under any chunking and from flush.
//
// The stream state.  A stream that has consumed N samples has emitted E = max(0, ceil((N up - half) / down)) outputs, the ones
// whose samples have all arrived.  It keeps the last T = ceil(2 half / up) samples (the tail, T >= K - 1) and one integer
//     d = E down + half - N up          in [0, max(half, down - 1)],
// the tap position c of its next output counted from its next sample.  A push of n samples emits ceil((n up - d) / down) outputs
// (none while n up <= d) with c = d + i down in the frame whose sample 0 is the chunk's first and whose samples -T .. -1 are the
// tail; a flush emits the ceil((half - d) / down) outputs still owed up to n_out(N) against zeros.  Nothing counts samples.
//
// Layout.  One 256-thread workgroup computes tiles of RS_TILE outputs.  In LDS: the table (row stride K | 1: 32 consecutive
// outputs sit on phases p0 + l down mod up, so with an odd stride, an odd `down` and up a multiple of 32 -- the 160 and 640 phase
// tables -- their rows start on 32 different banks; tables of 1 or 2 phases are broadcast reads), the tile's input span (16-byte
// quads, vector loads where the source is aligned and inside the signal) and the tile's outputs, which leave as 16-byte stores.
// The clip kernel gives every tile a workgroup.  The stream kernel gives every STREAM a workgroup, which loops over the stream's
// tiles and rewrites the tail after a barrier: the tail is read by every output of a push and rewritten by the same push.
// Neither allocates, synchronises nor reads back; the grids depend on (n_streams) and (n_out) alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <vector>

#include <memory>

#include "km_context.h"

namespace km {


namespace rs {
constexpr int THREADS = 256, TILE = 1024;
constexpr int64_t LDS_BUDGET = 64 * 1024;              // table + span + tile outputs; what a launch gets without opting in to more
constexpr int64_t MAX_STREAMS = 65535, MAX_PUSH = 1 << 20;
}  // namespace rs

struct RsGeom {
    int up, down, half, K, stride, T;      // K taps per phase, table row stride, tail length
    int tab_floats, span_cap;              // LDS carve: table (multiple of 4), span (multiple of 4), then TILE outputs
};

struct Resampler {
    int64_t n = 0;
    RsGeom g{};
    size_t lds_bytes = 0;
    DevBuf<char> blob;          // one allocation: the three views below
    float* table = nullptr;     // (up, stride), padded to tab_floats
    float* tail = nullptr;      // (n, T)
    int32_t* d = nullptr;       // (n)
};

__device__ __forceinline__ bool rs_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One tile: `count` (1 .. TILE) outputs whose first has tap position c0 >= 0 in the frame of x.  The signal is x[0..n) with
// hist[0..T) in front of it (hist may be NULL: zeros) and zeros everywhere else.  Ends with a barrier: LDS may be reused at once.
__device__ void rs_tile(const RsGeom& g, const float* __restrict__ hist, const float* __restrict__ x, int64_t n, int64_t c0, int count,
                        float* __restrict__ out, const float* lds_tab, float* lds_span, float* lds_out) {
    const int tid = threadIdx.x;
    const int64_t q0 = c0 / g.up;
    const int r0 = (int)(c0 - q0 * g.up);
    const int64_t js = (q0 - (g.K - 1)) & ~(int64_t)3;                       // first staged sample, rounded down to a quad
    const int lead = (int)(q0 - js);                                         // span index of sample q0
    const int len = lead + (int)(((int64_t)r0 + (int64_t)(count - 1) * g.down) / g.up) + 1;      // <= span_cap (km_resampler_create)
    const bool vec = x && rs_aligned16(x);
    for (int v = tid; v * 4 < len; v += rs::THREADS) {
        const int64_t j = js + (int64_t)v * 4;
        float4 w;
        if (vec && j >= 0 && j + 3 < n) {
            w = *reinterpret_cast<const float4*>(x + j);
        } else {
            float e[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t ji = j + i;
                float val = 0.0f;
                if (ji >= 0) { if (ji < n) val = x[ji]; }
                else if (hist && ji >= -(int64_t)g.T) val = hist[g.T + ji];
                e[i] = val;
            }
            w = make_float4(e[0], e[1], e[2], e[3]);
        }
        *reinterpret_cast<float4*>(lds_span + v * 4) = w;
    }
    __syncthreads();
    for (int i = tid; i < count; i += rs::THREADS) {
        const int cc = r0 + i * g.down;
        const int jr = cc / g.up, p = cc - jr * g.up;
        const float* xs = lds_span + lead + jr;
        const float* tp = lds_tab + p * g.stride;
        float acc = 0.0f;
        for (int k = g.K - 1; k >= 0; --k) acc = fmaf(xs[-k], tp[k], acc);
        lds_out[i] = acc;
    }
    __syncthreads();
    if (rs_aligned16(out)) {
        const int quads = count >> 2;
        for (int v = tid; v < quads; v += rs::THREADS) *reinterpret_cast<float4*>(out + v * 4) = *reinterpret_cast<const float4*>(lds_out + v * 4);
        for (int i = quads * 4 + tid; i < count; i += rs::THREADS) out[i] = lds_out[i];
    } else {
        for (int i = tid; i < count; i += rs::THREADS) out[i] = lds_out[i];
    }
    __syncthreads();
}

__device__ __forceinline__ void rs_load_table(const RsGeom& g, const float* __restrict__ table, float* lds_tab) {
    for (int v = threadIdx.x; v * 4 < g.tab_floats; v += rs::THREADS)
        *reinterpret_cast<float4*>(lds_tab + v * 4) = *reinterpret_cast<const float4*>(table + v * 4);
    __syncthreads();
}

__global__ __launch_bounds__(rs::THREADS) void rs_clip_kernel(RsGeom g, const float* __restrict__ table, const float* __restrict__ clip, int64_t n_in,
                                                              float* __restrict__ out, int64_t n_out) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* lds_tab = rs_lds;
    float* lds_span = lds_tab + g.tab_floats;
    float* lds_out = lds_span + g.span_cap;
    rs_load_table(g, table, lds_tab);
    const int64_t m0 = (int64_t)blockIdx.x * rs::TILE;
    const int64_t left = n_out - m0;
    const int count = left < rs::TILE ? (int)left : rs::TILE;
    if (count <= 0) return;
    rs_tile(g, nullptr, clip, n_in, m0 * g.down + g.half, count, out + m0, lds_tab, lds_span, lds_out);
}

// flush = 0: stream s consumes counts[s] (all n_per when counts is NULL) samples of its row.  flush = 1: the streams of the mask
// (all when it is NULL) emit what they still owe against zeros and are left reset.
__global__ __launch_bounds__(rs::THREADS) void rs_stream_kernel(RsGeom g, const float* __restrict__ table, int flush, const float* __restrict__ samples,
                                                                int n_per, const int32_t* __restrict__ counts, const uint8_t* __restrict__ mask,
                                                                float* __restrict__ out, int64_t out_stride, int32_t* __restrict__ out_counts,
                                                                float* __restrict__ tails, int32_t* __restrict__ dstate) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* lds_tab = rs_lds;
    float* lds_span = lds_tab + g.tab_floats;
    float* lds_out = lds_span + g.span_cap;
    const int s = blockIdx.x, tid = threadIdx.x;
    int c = 0;
    if (flush) {
        if (mask && !mask[s]) { if (tid == 0) out_counts[s] = 0; return; }
    } else {
        c = counts ? counts[s] : n_per;
        c = c < 0 ? 0 : (c > n_per ? n_per : c);
        if (c == 0) { if (tid == 0) out_counts[s] = 0; return; }
    }
    const int64_t d = dstate[s];
    rs_load_table(g, table, lds_tab);                  // its barrier also orders every thread's read of d before the write below
    const int64_t reach = flush ? (int64_t)g.half : (int64_t)c * g.up;           // outputs with c < reach are emitted
    int64_t cnt = reach > d ? (reach - d + g.down - 1) / g.down : 0;
    if (cnt > out_stride) cnt = out_stride;            // never past the row (the host checked that it cannot happen)
    float* tail = tails + (int64_t)s * g.T;
    const float* x = flush ? nullptr : samples + (int64_t)s * n_per;
    for (int64_t t0 = 0; t0 < cnt; t0 += rs::TILE) {
        const int count = cnt - t0 < rs::TILE ? (int)(cnt - t0) : rs::TILE;
        rs_tile(g, tail, x, c, d + t0 * g.down, count, out + (int64_t)s * out_stride + t0, lds_tab, lds_span, lds_out);
    }
    // every read of the tail lies before a barrier of rs_tile (or there was none); now the tail moves on
    if (flush) {
        for (int i = tid; i < g.T; i += rs::THREADS) tail[i] = 0.0f;
    } else if (c >= g.T) {
        for (int i = tid; i < g.T; i += rs::THREADS) tail[i] = x[c - g.T + i];
    } else {
        // shift left by c in passes of one element per thread: pass p reads tail[i + c] for its own i, which this pass writes only
        // after the barrier and earlier passes (lower i) never wrote
        const int keep = g.T - c;
        for (int base = 0; base < g.T; base += rs::THREADS) {
            const int i = base + tid;
            float val = 0.0f;
            if (i < g.T) val = i < keep ? tail[i + c] : x[i - keep];
            __syncthreads();
            if (i < g.T) tail[i] = val;
            __syncthreads();
        }
    }
    if (tid == 0) {
        dstate[s] = flush ? g.half : (int32_t)(d + cnt * g.down - reach);
        out_counts[s] = (int32_t)cnt;
    }
}

__global__ __launch_bounds__(rs::THREADS) void rs_reset_kernel(int T, int half, const uint8_t* __restrict__ mask, float* __restrict__ tails,
                                                               int32_t* __restrict__ dstate) {
    const int s = blockIdx.x;
    if (mask && !mask[s]) return;
    for (int i = threadIdx.x; i < T; i += rs::THREADS) tails[(int64_t)s * T + i] = 0.0f;
    if (threadIdx.x == 0) dstate[s] = half;
}

static int64_t rs_align16(int64_t bytes) { return (bytes + 15) / 16 * 16; }
static int64_t rs_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace km

using namespace km;

extern "C" {

int km_resampler_create(void** rs_out, int64_t n_streams, int32_t up, int32_t down, const double* taps_host, int64_t n_taps) {
    if (!rs_out || !taps_host) return fail(KM_ERR_INVALID_ARG, "km_resampler_create: NULL argument");
    *rs_out = nullptr;
    if (n_streams < 1 || n_streams > rs::MAX_STREAMS)
        return fail(KM_ERR_INVALID_ARG, "km_resampler_create: n_streams %lld, 1 .. %lld", (long long)n_streams, (long long)rs::MAX_STREAMS);
    if (up < 1 || down < 1) return fail(KM_ERR_INVALID_ARG, "km_resampler_create: up %d, down %d must be positive", up, down);
    if (up == down) return fail(KM_ERR_INVALID_ARG, "km_resampler_create: up == down (%d): nothing to resample", up);
    if (n_taps < 1 || n_taps % 2 == 0)
        return fail(KM_ERR_INVALID_ARG, "km_resampler_create: %lld taps, an odd number (2 half_len + 1) is expected", (long long)n_taps);
    const int64_t half = (n_taps - 1) / 2;
    const int64_t K = (2 * half) / up + 1, stride = K | 1, T = rs_ceil_div(2 * half, up);
    const int64_t tab_floats = (up * stride + 3) / 4 * 4;
    const int64_t span_cap = (rs_ceil_div((int64_t)(rs::TILE - 1) * down, up) + K + 3 + 3) / 4 * 4;
    const int64_t lds_bytes = (tab_floats + span_cap + rs::TILE) * 4;
    if (lds_bytes > rs::LDS_BUDGET || n_taps > (1 << 24))
        return fail(KM_ERR_UNSUPPORTED, "km_resampler_create: %d/%d with %lld taps needs %lld bytes of LDS (table %lld, input span %lld), at most %lld",
                    up, down, (long long)n_taps, (long long)lds_bytes, (long long)(tab_floats * 4), (long long)(span_cap * 4), (long long)rs::LDS_BUDGET);
    std::unique_ptr<Resampler> r(new (std::nothrow) Resampler());
    if (!r) return fail(KM_ERR_HIP, "km_resampler_create: out of host memory");
    r->n = n_streams;
    r->g = RsGeom{up, down, (int)half, (int)K, (int)stride, (int)T, (int)tab_floats, (int)span_cap};
    r->lds_bytes = (size_t)lds_bytes;
    std::vector<float> tab((size_t)tab_floats, 0.0f);                        // the one rounding of the taps to fp32
    for (int64_t p = 0; p < up; ++p)
        for (int64_t k = 0; k < K && p + k * up <= 2 * half; ++k) tab[(size_t)(p * stride + k)] = (float)taps_host[p + k * up];
    const int64_t tab_bytes = rs_align16(tab_floats * 4), tail_bytes = rs_align16(n_streams * T * 4 + 16), d_bytes = rs_align16(n_streams * 4);
    const int64_t bytes = tab_bytes + tail_bytes + d_bytes;
    if (int rc = r->blob.alloc(bytes, "km_resampler_create")) return rc;
    HIP_TRY(hipMemset(r->blob, 0, (size_t)bytes));
    r->table = reinterpret_cast<float*>(r->blob.p);
    r->tail = reinterpret_cast<float*>(r->blob + tab_bytes);
    r->d = reinterpret_cast<int32_t*>(r->blob + tab_bytes + tail_bytes);
    HIP_TRY(hipMemcpy(r->table, tab.data(), (size_t)tab_floats * 4, hipMemcpyHostToDevice));
    const std::vector<int32_t> d0((size_t)n_streams, (int32_t)half);
    HIP_TRY(hipMemcpy(r->d, d0.data(), (size_t)n_streams * 4, hipMemcpyHostToDevice));
    *rs_out = r.release();
    return KM_OK;
}

int km_resampler_destroy(void* rs) {
    if (!rs) return KM_OK;
    delete static_cast<Resampler*>(rs);
    return KM_OK;
}

int km_resampler_out_max(void* rs, int64_t n_in_max, int64_t* n_out_max) {
    if (!rs || !n_out_max) return fail(KM_ERR_INVALID_ARG, "km_resampler_out_max: NULL argument");
    Resampler* r = static_cast<Resampler*>(rs);
    if (n_in_max < 0 || n_in_max > rs::MAX_PUSH)
        return fail(KM_ERR_INVALID_ARG, "km_resampler_out_max: %lld samples, 0 .. %lld", (long long)n_in_max, (long long)rs::MAX_PUSH);
    *n_out_max = rs_ceil_div(n_in_max * r->g.up, r->g.down) + 1;
    return KM_OK;
}

int km_resampler_push(void* rs, const float* samples_dev, int64_t n_per_stream, const int32_t* counts_dev, float* out_dev, int64_t out_stride,
                      int32_t* out_counts_dev, void* stream) {
    if (!rs || !samples_dev || !out_dev || !out_counts_dev) return fail(KM_ERR_INVALID_ARG, "km_resampler_push: NULL argument");
    Resampler* r = static_cast<Resampler*>(rs);
    if (n_per_stream < 1 || n_per_stream > rs::MAX_PUSH)
        return fail(KM_ERR_INVALID_ARG, "km_resampler_push: %lld samples per stream, 1 .. %lld", (long long)n_per_stream, (long long)rs::MAX_PUSH);
    const int64_t need = rs_ceil_div(n_per_stream * r->g.up, r->g.down);
    if (out_stride < need)
        return fail(KM_ERR_INVALID_ARG, "km_resampler_push: out_stride %lld, %lld samples per stream can emit %lld", (long long)out_stride,
                    (long long)n_per_stream, (long long)need);
    hipLaunchKernelGGL(rs_stream_kernel, dim3((unsigned)r->n), dim3(rs::THREADS), r->lds_bytes, (hipStream_t)stream, r->g, (const float*)r->table, 0,
                       samples_dev, (int)n_per_stream, counts_dev, (const uint8_t*)nullptr, out_dev, out_stride, out_counts_dev, r->tail, r->d);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_resampler_flush(void* rs, const uint8_t* mask_dev, float* out_dev, int64_t out_stride, int32_t* out_counts_dev, void* stream) {
    if (!rs || !out_dev || !out_counts_dev) return fail(KM_ERR_INVALID_ARG, "km_resampler_flush: NULL argument");
    Resampler* r = static_cast<Resampler*>(rs);
    const int64_t need = rs_ceil_div(r->g.half, r->g.down);
    if (out_stride < need)
        return fail(KM_ERR_INVALID_ARG, "km_resampler_flush: out_stride %lld, a flush can emit %lld", (long long)out_stride, (long long)need);
    hipLaunchKernelGGL(rs_stream_kernel, dim3((unsigned)r->n), dim3(rs::THREADS), r->lds_bytes, (hipStream_t)stream, r->g, (const float*)r->table, 1,
                       (const float*)nullptr, 0, (const int32_t*)nullptr, mask_dev, out_dev, out_stride, out_counts_dev, r->tail, r->d);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_resampler_reset_streams(void* rs, const uint8_t* mask_dev, void* stream) {
    if (!rs) return fail(KM_ERR_INVALID_ARG, "km_resampler_reset_streams: NULL argument");
    Resampler* r = static_cast<Resampler*>(rs);
    hipLaunchKernelGGL(rs_reset_kernel, dim3((unsigned)r->n), dim3(rs::THREADS), 0, (hipStream_t)stream, r->g.T, r->g.half, mask_dev, r->tail, r->d);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int km_resample_clip(void* rs, const float* clip_dev, int64_t n_in, float* out_dev, int64_t n_out, void* stream) {
    if (!rs || !clip_dev || !out_dev) return fail(KM_ERR_INVALID_ARG, "km_resample_clip: NULL argument");
    Resampler* r = static_cast<Resampler*>(rs);
    if (n_in < 1 || n_in > ((int64_t)1 << 40)) return fail(KM_ERR_INVALID_ARG, "km_resample_clip: %lld samples, 1 .. 2^40", (long long)n_in);
    const int64_t want = rs_ceil_div(n_in * r->g.up, r->g.down);
    if (n_out != want)
        return fail(KM_ERR_INVALID_ARG, "km_resample_clip: n_out %lld, %lld samples at %d/%d give %lld", (long long)n_out, (long long)n_in, r->g.up,
                    r->g.down, (long long)want);
    const int64_t tiles = rs_ceil_div(n_out, rs::TILE);
    if (tiles > 0x7fffffff) return fail(KM_ERR_UNSUPPORTED, "km_resample_clip: %lld output tiles", (long long)tiles);
    hipLaunchKernelGGL(rs_clip_kernel, dim3((unsigned)tiles), dim3(rs::THREADS), r->lds_bytes, (hipStream_t)stream, r->g, (const float*)r->table, clip_dev,
                       n_in, out_dev, n_out);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // extern "C"
