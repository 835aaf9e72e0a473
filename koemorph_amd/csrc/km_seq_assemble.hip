// Sequence mode, assembled route (option seq_assemble): a tile of windows written into the front end's own workspace layout
// (ws.melpow (windows, T + 1, NK) + ws.melmax) from the images the clip-level front-end launches left, so that every core that
// reads the power-mel workspace behind km_forward_audio runs behind sequence mode unchanged.  A translation unit of its own: the
// kernels of every other unit are compiled exactly as before.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_api_internal.h"
#include "km_context.h"

namespace km {

// ---------------------------------------------------------------------------------------------------------
// seq_assemble_kernel.  Window w of the tile is global window g = win0 + w: clip g / n_per_clip, position i = g % n_per_clip.
// Row f = 0 .. T of its workspace image is
//   f < E        row f of the window's left-edge image  (frames 0 .. E - 1: they reach into the zero padding before the window)
//   f > T - E    row 1 of right-edge image j = T - f    (frames T - E + 1 .. T: ... behind it; row 0 of those images is frame 0 again
//                                                        and is not read)
//   otherwise    row i stride + f of the clip's image   (the frame lies inside the window: it IS that clip frame)
// The rows of a window are consecutive in f, so the interior is ONE run of (T + 1 - 2 E) NK floats of the clip's image and the
// left edge one run of E NK floats: a thread moves float4 k of the window's image with one 16-byte load and one 16-byte store, and
// only the E rows of the right edge cost an index division.  blockIdx.x is the window, blockIdx.y a slab of slab4 float4 (a multiple
// of NT * UNROLL, so a wave's 64 lanes always touch 1 KB of consecutive addresses); UNROLL loads are in flight per thread before the
// first store.  The workgroup of slab 0 also stores the window maximum: the maximum of the T + 1 rows' own maxima, which the front end
// left as float bits of non-negative numbers (unsigned max == float max; exact, whatever the order).  A plain store: the slot needs
// no zeroing, and the core that consumes it hands it back zeroed as it does behind the front end.  No atomics; 16 bytes of LDS.
// ---------------------------------------------------------------------------------------------------------
namespace seqasm {
constexpr int NT = 256, UNROLL = 4;
constexpr int kTargetGroups = 2048;      // eight workgroups of four waves per CU of a 256-CU device
}

struct SeqAsmArgs {
    const float4* pow; const unsigned* fmax;        // (clips, nfc, nk4) / (clips, nfc)
    const float4* left; const unsigned* lmax;       // (total, E, nk4) / (total, E)
    const float4* right; const unsigned* rmax;      // (E, total, 2, nk4) / (E, total, 2)
    float4* melpow; unsigned* melmax;               // (tile, T + 1, nk4) / (tile)
    int64_t win0, total;
    int nfc, stride, n_per_clip, E, T, nk4, slab4;
};

__global__ __launch_bounds__(seqasm::NT) void seq_assemble_kernel(SeqAsmArgs a) {
    using namespace seqasm;
    __shared__ unsigned red[NT / 64];
    const int tid = (int)threadIdx.x, w = (int)blockIdx.x;
    const int64_t g = a.win0 + w, clip = g / a.n_per_clip;
    const int64_t row0 = clip * a.nfc + (g - clip * a.n_per_clip) * a.stride;      // the clip-image row of the window's frame 0
    const int n4 = (a.T + 1) * a.nk4, lo4 = a.E * a.nk4, hi4 = (a.T + 1 - a.E) * a.nk4;
    const float4* __restrict__ src_in = a.pow + row0 * a.nk4;
    const float4* __restrict__ src_l = a.left + g * lo4;
    float4* __restrict__ dst = a.melpow + (int64_t)w * n4;
    const int beg = (int)blockIdx.y * a.slab4;
    const int end = beg + a.slab4 < n4 ? beg + a.slab4 : n4;
    const int end_in = end < hi4 ? end : hi4;                                       // left edge and interior: two runs, no division
    int i0 = beg + tid;
    for (; i0 + (UNROLL - 1) * NT < end_in; i0 += NT * UNROLL) {                    // whole steps: UNROLL loads, then UNROLL stores
        const float4 v0 = (i0 < lo4 ? src_l : src_in)[i0];                          // (named values, not an array: an array with a
        const float4 v1 = (i0 + NT < lo4 ? src_l : src_in)[i0 + NT];                // loop over it is given a home in LDS)
        const float4 v2 = (i0 + 2 * NT < lo4 ? src_l : src_in)[i0 + 2 * NT];
        const float4 v3 = (i0 + 3 * NT < lo4 ? src_l : src_in)[i0 + 3 * NT];
        dst[i0] = v0; dst[i0 + NT] = v1; dst[i0 + 2 * NT] = v2; dst[i0 + 3 * NT] = v3;
    }
    static_assert(UNROLL == 4, "the loop above is written out for four loads");
#pragma unroll 1
    for (; i0 < end_in; i0 += NT) dst[i0] = (i0 < lo4 ? src_l : src_in)[i0];         // the rest of the run
#pragma unroll 1
    for (int i = (beg > hi4 ? beg : hi4) + tid; i < end; i += NT) {                  // the E rows of the right edge (last slab only)
        const int f = i / a.nk4, j = a.T - f;
        dst[i] = a.right[(((int64_t)j * a.total + g) * 2 + 1) * a.nk4 + (i - f * a.nk4)];
    }
    if (blockIdx.y != 0) return;                                                    // workgroup-uniform
    unsigned m = 0;
#pragma unroll 1
    for (int f = tid; f <= a.T; f += NT) {
        unsigned v;
        if (f < a.E) v = a.lmax[g * a.E + f];
        else if (f > a.T - a.E) v = a.rmax[((int64_t)(a.T - f) * a.total + g) * 2 + 1];
        else v = a.fmax[row0 + f];
        m = max(m, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        unsigned mx = red[0];
#pragma unroll
        for (int k = 1; k < NT / 64; ++k) mx = max(mx, red[k]);
        a.melmax[w] = mx;
    }
}

// The per-row maxima the front end raises with atomicMax start from zero: both arrays cleared by ONE small launch.  A kernel, not
// two hipMemsetAsync calls: in a replayed capture of the call, memset nodes ahead of the front-end launches were seen to take
// effect out of order with them (rows of maxima lost or kept from the replay before), kernel nodes follow one another.
__global__ __launch_bounds__(256) void seq_zero_maxima_kernel(unsigned* __restrict__ a, int64_t na, unsigned* __restrict__ b, int64_t nb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < na) a[i] = 0u;
    else if (i < na + nb) b[i - na] = 0u;
}

int launch_seq_zero_maxima(unsigned* fmax, int64_t n_fmax, unsigned* emax, int64_t n_emax, void* stream) {
    if (!fmax || !emax || n_fmax <= 0 || n_emax <= 0 || n_fmax + n_emax >= ((int64_t)1 << 38))
        return fail(KM_ERR_INVALID_ARG, "sequence maxima: bad argument");
    hipLaunchKernelGGL(seq_zero_maxima_kernel, dim3((unsigned)((n_fmax + n_emax + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fmax, n_fmax,
                       emax, n_emax);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int launch_seq_assemble(Context* c, const SeqAssemble& s, int64_t nw, int64_t win0, void* stream) {
    using namespace seqasm;
    const int NK = c->NK, T = s.T, E = s.E;
    if (nw <= 0 || win0 < 0 || win0 + nw > s.total || NK % 4 != 0 || E < 1 || T + 1 < 2 * E || s.nfc < T + 1 || s.stride < 1 || s.n_per_clip < 1 ||
        s.total % s.n_per_clip != 0 || (int64_t)(s.n_per_clip - 1) * s.stride + T + 1 > s.nfc)
        return fail(KM_ERR_INVALID_ARG, "sequence assemble: bad argument");
    if (nw > c->ws.windows || T + 1 > c->ws.frames || NK > c->ws.mels)
        return fail(KM_ERR_WORKSPACE, "workspace holds %lld windows x %lld frames, need %lld x %d: call km_reserve", (long long)c->ws.windows,
                    (long long)c->ws.frames, (long long)nw, T + 1);
    if (!aligned16(s.pow) || !aligned16(s.left) || !aligned16(s.right) || !aligned16(c->ws.melpow.p))
        return fail(KM_ERR_INVALID_ARG, "sequence assemble: the images must be 16-byte aligned");
    // 32-bit float4 indices inside a window; 64-bit ones into the images, whose element counts the caller keeps below 2^31
    const int nk4 = NK / 4;
    const int64_t n4 = (int64_t)(T + 1) * nk4;
    if (n4 >= (1 << 28) || nw > 0x7fffffff) return fail(KM_ERR_INVALID_ARG, "sequence assemble: window or tile too large");
    const int unit = NT * UNROLL;
    const int64_t max_slabs = (n4 + unit - 1) / unit;
    int64_t slabs = (kTargetGroups + nw - 1) / nw;
    if (slabs > max_slabs) slabs = max_slabs;
    const int slab4 = (int)(((n4 + slabs - 1) / slabs + unit - 1) / unit * unit);
    slabs = (n4 + slab4 - 1) / slab4;
    const SeqAsmArgs a{reinterpret_cast<const float4*>(s.pow), s.fmax, reinterpret_cast<const float4*>(s.left), s.lmax,
                       reinterpret_cast<const float4*>(s.right), s.rmax, reinterpret_cast<float4*>(c->ws.melpow.p), c->ws.melmax,
                       win0, s.total, s.nfc, s.stride, s.n_per_clip, E, T, nk4, slab4};
    hipLaunchKernelGGL(seq_assemble_kernel, dim3((unsigned)nw, (unsigned)slabs), dim3(NT), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    // melmax_dirty stays as it is: slots 0 .. nw - 1 were just stored and are re-zeroed by the core launch that follows, the
    // slots beyond are as clean or as dirty as they were
    return KM_OK;
}

}  // namespace km
