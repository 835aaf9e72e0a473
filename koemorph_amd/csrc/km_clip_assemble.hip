// Training and validation from a resident clip at every shape and hop (option clip_assemble; km_clip_plan route 2).  The windows of a
// batch start at start[b] hop inside ONE clip.  E = ceil((n_fft / 2) / hop) frames at either end of a window see its zero padding and
// belong to it alone; every other frame IS a frame of the clip.  So a call computes
//   the span image   clip frames min_start .. max_start + T, each once: one front-end launch over the clip as one long window
//   the edge image   per window two snippets of Ls = (2 E - 1) hop samples (its first and its last Ls samples) as 2 B dense rows of
//                    2 E frames: window frame f < E is row f of the left snippet, window frame T - j (j < E) row 2 E - 1 - j of the
//                    right one (rows E .. 2 E - 1: a run)
// with the front end as it is (a frame has the same bits whatever row of whatever launch computes it), and then either writes the
// packed training input (clip_pack_edges_kernel) or the front end's own workspace layout (clip_assemble_kernel), so that the
// training program and every core behind km_forward_audio's power path run unchanged.  A translation unit of its own: the kernels of
// every other unit are compiled exactly as before.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_api_internal.h"
#include "km_context.h"
#include "km_device.h"

namespace km {

// ---------------------------------------------------------------------------------------------------------
// The plan (km_clip_plan names it; km_train_step_clip / km_forward_clip run it).  Host arithmetic on the handle's shape, its
// front-end plan and its switches alone, so the query and the call cannot disagree.
// ---------------------------------------------------------------------------------------------------------
static bool clip_rp_planned(Context* c, MelPlan* p) { return p->cfg.n_fft == 1024 && !c->opt.mel_two_frame && !p->fbg_gid.empty(); }

// clip_frames_shared, mel_packs and train_fe_packs as the host knows them before the plan is uploaded
static bool clip_shared_planned(Context* c, MelPlan* p) {
    const km_mel_config& m = p->cfg;
    return m.pad_mode == KM_PAD_CONSTANT && 2 * m.hop_length >= m.n_fft && m.n_mels == c->NK && c->NK % 4 == 0;
}
static bool clip_packs_planned(Context* c, MelPlan* p) {
    const km_mel_config& m = p->cfg;
    const int64_t n_frames = (int64_t)c->T + 1;
    return !c->opt.train_no_fe_pack && !c->opt.train_no_dma && clip_rp_planned(c, p) && m.log_mode == KM_LOG_DB_MAX && m.top_db == m.db_add &&
           m.db_scale > 0.f && n_frames >= 3 && m.n_mels == c->NK;
}

ClipPlan clip_plan(Context* c, int64_t B, int64_t min_start, int64_t max_start, int mode) {
    MelPlan* plan = c->mel_plans[0];
    const km_mel_config& m = plan->cfg;
    const int64_t hop = m.hop_length, T = c->T, lim = (int64_t)1 << 31;
    ClipPlan p{};
    p.E = (int)((m.n_fft / 2 + hop - 1) / hop);
    p.n_span = (max_start - min_start) + T + 1;
    const bool training = mode == 1, with_attention = mode == 2;
    const bool rp = clip_rp_planned(c, plan), shared = clip_shared_planned(c, plan);
    bool today, base;
    if (training) {
        today = shared && clip_packs_planned(c, plan);
        base = clip_packs_planned(c, plan) && T >= 2 && m.n_mels <= 128;
    } else {
        today = c->fused_ok && c->opt.core_split != 3 && c->opt.core_split != 6 && rp && shared;
        // the power path of km_forward_audio (the split-bf16 variants of the fused core apart)
        base = c->fused_ok ? (c->opt.core_split != 3 && c->opt.core_split != 6) : core_takes_power(c, with_attention);
    }
    const int64_t Ls = (2 * (int64_t)p.E - 1) * hop;
    const bool sizes_ok = B <= 32767 && p.n_span < lim / c->NK && B * 4 * p.E < lim / c->NK && B * 2 * (Ls + 3) < lim;
    if (today) {
        p.route = 1;
        p.stft_frames = p.n_span + 2 * B;
    } else if (c->opt.clip_assemble && base && rp && m.pad_mode == KM_PAD_CONSTANT && m.n_mels == c->NK && c->NK % 4 == 0 && T + 1 >= 2 * p.E &&
               sizes_ok) {
        p.route = 2;
        p.stft_frames = p.n_span + B * 4 * p.E;              // per window two snippets of 2 E frames
    } else {
        p.route = 0;
        p.stft_frames = B * (T + 1);
    }
    return p;
}

// ---------------------------------------------------------------------------------------------------------
// clip_edge_snippets_kernel.  Row 2 b of snip (2 B, LsPad) is the first Ls samples of window b, row 2 b + 1 its last Ls samples
// (the window is clip samples [s hop, (s + T) hop), s = max(start[b], 0)); samples beyond clip_len read as zeros, as
// km_gather_windows fills them.  LsPad = Ls rounded up to four floats: a thread stores one aligned float4 (the columns beyond Ls are
// zeros nobody reads).  The loads are scalar: a window starts at any sample.  No atomics, no LDS.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clip_edge_snippets_kernel(const float* __restrict__ clip, int64_t clip_len, const int* __restrict__ start,
                                                                 int hop, int T, int Ls, int ls4, float4* __restrict__ snip) {
    const int c4 = (int)(blockIdx.x * 256 + threadIdx.x), row = (int)blockIdx.y;
    if (c4 >= ls4) return;
    int s = start[row >> 1];
    s = s < 0 ? 0 : s;
    const int64_t base = (int64_t)s * hop + ((row & 1) ? (int64_t)T * hop - Ls : 0);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int col = c4 * 4 + k;
        const int64_t q = base + col;
        v[k] = (col < Ls && q < clip_len) ? clip[q] : 0.f;
    }
    snip[(int64_t)row * ls4 + c4] = make_float4(v[0], v[1], v[2], v[3]);
}

// The images of one call.  Every buffer is grow-only (DevBuf::grow refuses inside a stream capture, before any launch); the
// per-row maxima the front end raises with atomicMax are zeroed by launch_seq_zero_maxima, a kernel: memset nodes ahead of the
// front-end launches were seen to take effect out of order with them in a replayed capture.
int launch_clip_images(Context* c, MelPlan* plan, const float* clip, int64_t clip_len, const int* start_frames, int64_t B, int min_start,
                       int64_t n_span, int E, void* stream) {
    const km_mel_config& m = plan->cfg;
    const int NK = c->NK, T = c->T, hop = m.hop_length;
    const int64_t Ls = (2 * (int64_t)E - 1) * hop, ls4 = (Ls + 3) / 4;
    if (!clip || !start_frames || B <= 0 || clip_len <= 0 || min_start < 0 || n_span < T + 1 || E < 1 || T + 1 < 2 * E || B > 32767 ||
        Ls > (int64_t)T * hop || !mel_rp_ok(c, plan) || m.pad_mode != KM_PAD_CONSTANT || m.n_mels != NK || NK % 4 != 0)
        return fail(KM_ERR_INVALID_ARG, "clip images: bad argument");
    ClipAsmBufs& im = c->clipasm;
    const char* what = "resident clip (option clip_assemble): elements of the span / edge images";
    if (int rc = im.span.grow(n_span * NK, stream, what)) return rc;
    if (int rc = im.smax.grow(n_span, stream, what)) return rc;
    if (int rc = im.snip.grow(2 * B * ls4 * 4, stream, what)) return rc;
    if (int rc = im.edge.grow(B * 4 * E * NK, stream, what)) return rc;
    if (int rc = im.emax.grow(B * 4 * E, stream, what)) return rc;
    if (int rc = ensure_chunk_counters(c, 2 * B, stream)) return rc;
    if (int rc = launch_seq_zero_maxima(im.smax, n_span, im.emax, B * 4 * E, stream)) return rc;
    // (1) the span: the clip from sample min_start hop on as ONE long window of n_span frames, zero beyond the clip's end (a span
    // that begins beyond it reads as zeros and keeps its pointer inside the clip).  Its first and last E rows see the padding of
    // that long window; they are rows no window reads.
    const int64_t off = (int64_t)min_start * hop;
    const SeqFrames span_img{im.span, im.smax, n_span, 1};
    const MelSrc span_src = off < clip_len ? mel_clip_windows(clip + off, clip_len - off, 1, (n_span - 1) * hop, 0, 0, 1)
                                           : mel_clip_windows(clip, 0, 1, (n_span - 1) * hop, 0, 0, 1);
    if (int rc = launch_mel_power(c, plan, span_src, stream, mel_to_frames(&span_img))) return rc;
    // (2) the snippets, then their 2 E frames each as 2 B dense rows
    hipLaunchKernelGGL(clip_edge_snippets_kernel, dim3((unsigned)((ls4 + 255) / 256), (unsigned)(2 * B)), dim3(256), 0, (hipStream_t)stream, clip,
                       clip_len, start_frames, hop, T, (int)Ls, (int)ls4, reinterpret_cast<float4*>(im.snip.p));
    HIP_TRY(hipGetLastError());
    const SeqFrames edge_img{im.edge, im.emax, 2 * E, 1};
    return launch_mel_power(c, plan, mel_clip_windows(im.snip, ls4 * 4, 2 * B, Ls, 0, 0, 1), stream, mel_to_frames(&edge_img));
}

// ---------------------------------------------------------------------------------------------------------
// clip_assemble_kernel: seq_assemble_kernel with the window's clip row taken from the start table and the edge rows from the edge
// image above.  Row f = 0 .. T of window w's workspace image is
//   f < E        row f of its left snippet                       (edge rows (2 w) 2 E + f)
//   f > T - E    row f - (T + 1 - 2 E) of its right snippet      (edge rows (2 w + 1) 2 E + E ..: a run as well)
//   otherwise    row start[w] - min_start + f of the span image
// Three runs of float4: no index division anywhere.  blockIdx.x is the window, blockIdx.y a slab of slab4 float4; the workgroup of
// slab 0 also stores the window maximum, the maximum of the T + 1 rows' own maxima (float bits of non-negative numbers: unsigned
// max == float max).  A plain store; no atomics; 16 bytes of LDS.
// ---------------------------------------------------------------------------------------------------------
namespace clipasm {
constexpr int NT = 256, UNROLL = 4;
constexpr int kTargetGroups = 2048;
}

struct ClipAsmArgs {
    const float4* span; const unsigned* smax;       // (n_span, nk4) / (n_span)
    const float4* edge; const unsigned* emax;       // (2 B, 2 E, nk4) / (2 B, 2 E)
    const int* start;                               // (B)
    float4* melpow; unsigned* melmax;               // (B, T + 1, nk4) / (B)
    int min_start, n_span, E, T, nk4, slab4;
};

__global__ __launch_bounds__(clipasm::NT) void clip_assemble_kernel(ClipAsmArgs a) {
    using namespace clipasm;
    __shared__ unsigned red[NT / 64];
    const int tid = (int)threadIdx.x, w = (int)blockIdx.x;
    int s = a.start[w];
    s = s < 0 ? 0 : s;
    int row0 = s - a.min_start;                      // inside the span whenever min_start / n_span are the batch's extremes
    row0 = row0 < 0 ? 0 : (row0 > a.n_span - (a.T + 1) ? a.n_span - (a.T + 1) : row0);
    const int n4 = (a.T + 1) * a.nk4, lo4 = a.E * a.nk4, hi4 = (a.T + 1 - a.E) * a.nk4;
    const float4* __restrict__ src_in = a.span + (int64_t)row0 * a.nk4;
    const float4* __restrict__ src_l = a.edge + (int64_t)(2 * w) * 2 * a.E * a.nk4;
    const float4* __restrict__ src_r = a.edge + ((int64_t)(2 * w + 1) * 2 * a.E + a.E) * a.nk4 - hi4;      // indexed by i >= hi4
    float4* __restrict__ dst = a.melpow + (int64_t)w * n4;
    const int beg = (int)blockIdx.y * a.slab4;
    const int end = beg + a.slab4 < n4 ? beg + a.slab4 : n4;
    auto src = [=](int i) {                          // (captured by value: a closure of references is given a home in scratch)
        const float4* p = src_in;
        if (i < lo4) p = src_l;
        if (i >= hi4) p = src_r;
        return p[i];
    };
    int i0 = beg + tid;
    for (; i0 + (UNROLL - 1) * NT < end; i0 += NT * UNROLL) {                       // whole steps: UNROLL loads, then UNROLL stores
        const float4 v0 = src(i0), v1 = src(i0 + NT), v2 = src(i0 + 2 * NT), v3 = src(i0 + 3 * NT);
        dst[i0] = v0; dst[i0 + NT] = v1; dst[i0 + 2 * NT] = v2; dst[i0 + 3 * NT] = v3;
    }
    static_assert(UNROLL == 4, "the loop above is written out for four loads");
#pragma unroll 1
    for (; i0 < end; i0 += NT) dst[i0] = src(i0);
    if (blockIdx.y != 0) return;                                                    // workgroup-uniform
    unsigned m = 0;
    const unsigned* __restrict__ lmax = a.emax + (int64_t)(2 * w) * 2 * a.E;
    const unsigned* __restrict__ rmax = a.emax + (int64_t)(2 * w + 1) * 2 * a.E + a.E - (a.T + 1 - a.E);   // indexed by f > T - E
#pragma unroll 1
    for (int f = tid; f <= a.T; f += NT) {
        const unsigned v = f < a.E ? lmax[f] : (f > a.T - a.E ? rmax[f] : a.smax[row0 + f]);
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

int launch_clip_assemble(Context* c, const int* start_frames, int64_t B, int min_start, int64_t n_span, int E, void* stream) {
    using namespace clipasm;
    const int NK = c->NK, T = c->T;
    const ClipAsmBufs& im = c->clipasm;
    if (!start_frames || B <= 0 || NK % 4 != 0 || E < 1 || T + 1 < 2 * E || n_span < T + 1 || n_span * NK > im.span.n || n_span > im.smax.n ||
        B * 4 * E * NK > im.edge.n || B * 4 * E > im.emax.n || n_span >= (1ll << 31))
        return fail(KM_ERR_INVALID_ARG, "clip assemble: bad argument");
    if (B > c->ws.windows || T + 1 > c->ws.frames || NK > c->ws.mels)
        return fail(KM_ERR_WORKSPACE, "workspace holds %lld windows x %lld frames, need %lld x %d: call km_reserve", (long long)c->ws.windows,
                    (long long)c->ws.frames, (long long)B, T + 1);
    if (!aligned16(im.span.p) || !aligned16(im.edge.p) || !aligned16(c->ws.melpow.p))
        return fail(KM_ERR_INVALID_ARG, "clip assemble: the images must be 16-byte aligned");
    const int nk4 = NK / 4;
    const int64_t n4 = (int64_t)(T + 1) * nk4;
    if (n4 >= (1 << 28) || B > 65535) return fail(KM_ERR_INVALID_ARG, "clip assemble: window or batch too large");
    const int unit = NT * UNROLL;
    const int64_t max_slabs = (n4 + unit - 1) / unit;
    int64_t slabs = (kTargetGroups + B - 1) / B;
    if (slabs > max_slabs) slabs = max_slabs;
    const int slab4 = (int)(((n4 + slabs - 1) / slabs + unit - 1) / unit * unit);
    slabs = (n4 + slab4 - 1) / slab4;
    const ClipAsmArgs a{reinterpret_cast<const float4*>(im.span.p), im.smax, reinterpret_cast<const float4*>(im.edge.p), im.emax, start_frames,
                        reinterpret_cast<float4*>(c->ws.melpow.p), c->ws.melmax, min_start, (int)n_span, E, T, nk4, slab4};
    hipLaunchKernelGGL(clip_assemble_kernel, dim3((unsigned)B, (unsigned)slabs), dim3(NT), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    // melmax_dirty stays as it is: slots 0 .. B - 1 were just stored and are re-zeroed by the core launch that follows
    return KM_OK;
}

// ---------------------------------------------------------------------------------------------------------
// clip_pack_edges_kernel: train_clip_pack_kernel with E edge rows at either end.  One 1024-thread workgroup per window.  Column
// j < T of the window's packed rows is window frame j, columns T .. T + 2 are frames T - 2 .. T (the last three computed frames, as
// the PACK store of the front end places them: edge rows when E >= 3, span rows otherwise), the rest up to KP is zero.  A tile of
// columns is read frame-major with every load in flight before the first is used, and written mel-major, transposed through LDS;
// the same db10 of the same powers: bit-identical to the packing front end.  The workgroup sees all T + 1 frames, so the window
// maximum is a plain store: no atomics, no zeroed slots needed.
// ---------------------------------------------------------------------------------------------------------
namespace clipedges {
constexpr int NT = 1024, MAXI = 24, LDS_FLOATS = 24 * 1024;      // a thread holds up to MAXI powers of a tile; 96 KB of LDS
// LDS row stride of the [column][mel] tile: 18 (mod 64) dwords, so that the transposed read of a wave meets 64 different banks
inline int row_stride(int n_mels) { return (n_mels + 45) / 64 * 64 + 18; }
// columns per tile: a multiple of 32 within the register and LDS budgets
inline int tile_cols(int n_mels, int KP) {
    int c = NT * MAXI / n_mels;
    const int l = LDS_FLOATS / row_stride(n_mels);
    c = (c < l ? c : l) / 32 * 32;
    return c < KP ? c : KP;
}
}  // namespace clipedges

struct ClipPackEdgesArgs {
    const float* span;      // (n_span, n_mels): row r = clip frame min_start + r
    const float* edge;      // (2 B, 2 E, n_mels)
    const int* start;       // (B) start frames
    int min_start, n_span, E, T, KP, n_mels, row_stride, tile_cols;
    float amin;
    float* xt;              // (B, n_mels, KP)
    unsigned* melmax;       // (B) float bits
};

__global__ __launch_bounds__(clipedges::NT) void clip_pack_edges_kernel(ClipPackEdgesArgs a) {
    using namespace clipedges;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float redmax[NT / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    int s = a.start[b];
    s = s < 0 ? 0 : s;
    int row0 = s - a.min_start;
    row0 = row0 < 0 ? 0 : (row0 > a.n_span - (a.T + 1) ? a.n_span - (a.T + 1) : row0);
    const float* __restrict__ src_in = a.span + (int64_t)row0 * a.n_mels;                                         // indexed by f n_mels
    const float* __restrict__ src_l = a.edge + (int64_t)(2 * b) * 2 * a.E * a.n_mels;
    const float* __restrict__ src_r = a.edge + ((int64_t)(2 * b + 1) * 2 * a.E + a.E - (a.T + 1 - a.E)) * a.n_mels;  // by f > T - E
    const int dq = NT / a.n_mels, dr = NT % a.n_mels;
    const int cl0 = tid / a.n_mels, m0 = tid - cl0 * a.n_mels;
    float vmax = 0.f;
    for (int c0 = 0; c0 < a.KP; c0 += a.tile_cols) {
        const int ncol = a.KP - c0 < a.tile_cols ? a.KP - c0 : a.tile_cols;
        const int total = ncol * a.n_mels;
        float pwv[MAXI];
        int cl = cl0, m = m0;
#pragma unroll
        for (int k = 0; k < MAXI; ++k) {
            const int col = c0 + cl;
            const int f = col < a.T ? col : col - 2;
            pwv[k] = -1.f;                                     // no frame behind this column (powers are >= 0)
            if (tid + k * NT < total && col < a.T + 3)
                pwv[k] = (f < a.E ? src_l : (f > a.T - a.E ? src_r : src_in))[f * a.n_mels + m];
            cl += dq; m += dr;
            if (m >= a.n_mels) { m -= a.n_mels; ++cl; }
        }
        if (c0 > 0) __syncthreads();                           // the previous tile has been written out
        cl = cl0; m = m0;
#pragma unroll
        for (int k = 0; k < MAXI; ++k) {
            if (tid + k * NT < total) {
                const float pw = pwv[k];
                vmax = fmaxf(vmax, pw);
                smem[cl * a.row_stride + m] = pw >= 0.f ? db10(pw, a.amin) : 0.f;
            }
            cl += dq; m += dr;
            if (m >= a.n_mels) { m -= a.n_mels; ++cl; }
        }
        __syncthreads();
        // half-wave h of the workgroup owns mel rows h, h + 32, ...; its 32 lanes walk the tile's columns 32 at a time
        const int lane32 = tid & 31;
        for (int m2 = tid >> 5; m2 < a.n_mels; m2 += NT / 32) {
            float* dst = a.xt + ((int64_t)b * a.n_mels + m2) * a.KP + c0;
            for (int c = lane32; c < ncol; c += 32) dst[c] = smem[c * a.row_stride + m2];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
    if ((tid & 63) == 0) redmax[tid >> 6] = vmax;
    __syncthreads();
    if (tid == 0) {
        float mx = redmax[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) mx = fmaxf(mx, redmax[w]);
        a.melmax[b] = __float_as_uint(mx);                     // the maximum over all T + 1 frames of the window
    }
}

int launch_clip_pack_edges(Context* c, MelPlan* p, const int* start_frames, int64_t B, int min_start, int64_t n_span, int E, int KP, float* xt,
                           void* stream) {
    const km_mel_config& m = p->cfg;
    const int T = c->T;
    const ClipAsmBufs& im = c->clipasm;
    if (!start_frames || !xt || B <= 0 || B > 65535 || T < 2 || KP < T + 3 || E < 1 || T + 1 < 2 * E || n_span < T + 1 || m.n_mels > 128 ||
        m.n_mels < 1 || n_span * m.n_mels > im.span.n || B * 4 * E * m.n_mels > im.edge.n || n_span * m.n_mels >= (1ll << 31) || B > c->ws.windows)
        return fail(KM_ERR_INVALID_ARG, "clip pack: bad argument");
    ClipPackEdgesArgs a;
    a.span = im.span; a.edge = im.edge; a.start = start_frames; a.min_start = min_start; a.n_span = (int)n_span; a.E = E; a.T = T; a.KP = KP;
    a.n_mels = m.n_mels; a.row_stride = clipedges::row_stride(m.n_mels); a.tile_cols = clipedges::tile_cols(m.n_mels, KP);
    a.amin = m.amin; a.xt = xt; a.melmax = c->ws.melmax;
    const size_t lds = (size_t)a.tile_cols * a.row_stride * sizeof(float);
    static PerDeviceOnce once;
    if (once.first(c->device))
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&clip_pack_edges_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(clipedges::LDS_FLOATS * sizeof(float))));
    hipLaunchKernelGGL(clip_pack_edges_kernel, dim3((unsigned)B), dim3(clipedges::NT), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" int km_clip_plan(km_handle h, int64_t B, int32_t min_start_frame, int32_t max_start_frame, int32_t training, int64_t out[4]) {
    if (!h || !out || B <= 0 || min_start_frame < 0 || max_start_frame < min_start_frame || training < 0 || training > 2)
        return fail(KM_ERR_INVALID_ARG, "km_clip_plan: bad argument");
    if (h->kind != 0) return fail(KM_ERR_INVALID_ARG, "km_clip_plan needs a dual-stream handle (km_create)");
    if (!h->host_finalized) return fail(KM_ERR_NOT_FINALIZED, "km_clip_plan: call km_finalize_host or km_finalize first");
    const ClipPlan p = clip_plan(h, B, min_start_frame, max_start_frame, training);
    out[0] = p.route; out[1] = p.n_span; out[2] = p.stft_frames; out[3] = p.E;
    return KM_OK;
}
