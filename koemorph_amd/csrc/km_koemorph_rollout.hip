// Autoregressive rollout of the legacy KoeMorphModel (km_koemorph_rollout*, include/koemorph.h): B clips of F per-frame feature
// rows -> the blendshape track of frames first_frame .. F - 1, every frame conditioned on the one before it.
//
// The law: frame i runs km_koemorph_forward on the DENSE window of rows i - T_i + 1 .. i, T_i = min(i + 1, T) (a clip's first
// frames see shorter windows, not padded ones: a left-padded window would leave the causal mask's query 0 without a key), no
// audio mask, prev = frame i - 1's out (prev0 for the first rendered frame), the caller's smoother state updated frame by frame.
//
// Route 1 (the fused width, T <= 32): frames with a short window run as they would alone (window gather, kmmf_encoder_kernel,
// kmmf_decode_kernel, row scatter).  The others go in chunks of the reserved chunk_frames: ONE gather of the chunk's B x frames
// overlapping windows into a dense staging buffer (the encoder kernel and its addresses are untouched), ONE kmmf_encoder_kernel
// launch over all of them, ONE kmmf_rollout_kernel launch (km_kmmf.hip) that walks each clip's serial chain in a workgroup.
// Route 0 (everything else): per frame, gather + launch_koemorph + scatter.  Nothing but launches on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_api_internal.h"
#include "km_context.h"
#include "km_kmmf.h"

namespace km {

#include "km_kmm_tail.h"

// km_kmmf.hip
int launch_kmmf_encoder(Context* c, const float* mel, const float* emo, int64_t B, int64_t T, const unsigned char* kvalid, float* xm,
                        float* xe, void* stream);
int launch_kmmf_rollout(Context* c, const float* xm, const float* xe, int64_t clips, int64_t frames, int64_t T, const float* prev,
                        const KmmTail& tail, int64_t out_stride, float* prev_io, void* stream);
// km_koemorph.hip
KmmTail koemorph_tail(Context* c, const float* prev, float* state, int apply_constraints, float* out, float* raw);

constexpr int64_t kRolloutChunkDefault = 256;     // README "KoeMorphModel rollout": the measured table this default is read from

// dst[s] (W, Tw, dim[s]) <- window w = (clip w / nf, frame k = w % nf): rows start0 + k .. + Tw - 1 of the clip's F rows of src[s].
// blockIdx.y = stream.  vec[s]: 16-byte moves (dim % 4 == 0 and an aligned source)
struct GatherArgs {
    const float* src[2]; float* dst[2]; int dim[2]; int vec[2];
    int64_t F, start0, W; int nf, Tw;
};

__global__ __launch_bounds__(256) void kmm_rollout_gather_kernel(GatherArgs a) {
    const int s = blockIdx.y;
    const int w = a.vec[s] ? 4 : 1, dq = a.dim[s] / w;
    const int64_t total = a.W * a.Tw * dq;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cq = (int)(i % dq);
        const int64_t row = i / dq;
        const int t = (int)(row % a.Tw);
        const int64_t win = row / a.Tw, clip = win / a.nf, k = win % a.nf;
        const int64_t srow = clip * a.F + a.start0 + k + t;
        if (w == 4) reinterpret_cast<float4*>(a.dst[s])[i] = reinterpret_cast<const float4*>(a.src[s])[srow * dq + cq];
        else a.dst[s][i] = a.src[s][srow * dq + cq];
    }
}

// one frame's dense (B, NB) rows -> row `r` of (B, rows, NB)
__global__ __launch_bounds__(256) void kmm_rollout_scatter_kernel(const float* __restrict__ o, const float* __restrict__ w, float* __restrict__ out,
                                                                  float* __restrict__ raw, int64_t B, int NB, int64_t rows, int64_t r) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * NB) return;
    const int64_t b = i / NB, q = i % NB;
    out[(b * rows + r) * NB + q] = o[i];
    if (raw) raw[(b * rows + r) * NB + q] = w[i];
}

static int64_t up4(int64_t n) { return (n + 3) & ~(int64_t)3; }

static bool rollout_fused(Context* c, int64_t T) { return c->kmm_fused && !c->opt.kmm_no_fuse && T >= 1 && T <= kmmf::TMAX; }

// launches of one launch_koemorph at T frames (km_koemorph.hip, no maps)
static int64_t forward_launches(Context* c, int64_t T, bool prev) {
    if (rollout_fused(c, T)) return 2;
    const km_koemorph_config& k = c->kmm;
    return 2 * (2 + 9 * (int64_t)k.num_encoder_layers) + 1 + (prev ? 2 : 0) + 1 + (k.num_attention_layers > 0 ? 1 : 0) +
           6 * (int64_t)k.num_attention_layers + 1 + 3 * (int64_t)k.decoder_layers + 1;
}

// workspace floats of the two layouts for B clips, windows of T frames and chunks of `cw` frames
static int64_t ws_route0(Context* c, int64_t B, int64_t T) {
    return up4(B * T * c->kmm.mel_dim) + up4(B * T * c->kmm.emotion_dim) + 3 * up4(B * c->NB);
}
static int64_t ws_route1(Context* c, int64_t B, int64_t T, int64_t cw) {
    const int64_t W = B * (cw > 1 ? cw : 1);
    return up4(W * T * c->kmm.mel_dim) + up4(W * T * c->kmm.emotion_dim) + 2 * W * T * kmmf::D + 3 * up4(B * c->NB);
}

struct RolloutPlan {
    int route;                 // 0 per-frame launches, 1 rollout kernel
    int64_t chunks, short_frames, launches, ws_floats;
    int64_t full0;             // first frame with a window of T frames that the call renders (F if none)
};

// The one function behind km_koemorph_rollout_plan and km_koemorph_rollout.  aligned: both row pointers are 16-byte aligned
// (the query has no pointers and assumes so)
static RolloutPlan rollout_plan(Context* c, int64_t B, int64_t F, int64_t T, int64_t first, int64_t chunk, bool aligned) {
    RolloutPlan p{};
    p.route = (rollout_fused(c, T) && aligned) ? 1 : 0;
    const int64_t short_end = (T - 1 < F ? T - 1 : F);          // frames 0 .. T - 2 have short windows
    p.short_frames = short_end > first ? short_end - first : 0;
    p.full0 = first + p.short_frames;
    const int64_t n_full = F - p.full0;
    if (p.route == 1) {
        p.chunks = (n_full + chunk - 1) / chunk;
        p.launches = 4 * p.short_frames + 3 * p.chunks;         // gather, encoder, decode, scatter | gather, encoder, rollout
        p.ws_floats = ws_route1(c, B, T, n_full < chunk ? n_full : chunk);
    } else {
        for (int64_t i = first; i < F; ++i) p.launches += 2 + forward_launches(c, i + 1 < T ? i + 1 : T, true);
        // (the conditioning net's two products of the chain are absent from a first frame without prev0: the query cannot know)
        p.ws_floats = ws_route0(c, B, T < F ? T : F);
    }
    return p;
}

static int gather(Context* c, const float* mel, const float* emo, float* smel, float* semo, int64_t F, int64_t start0, int64_t W,
                  int64_t nf, int64_t Tw, bool aligned, hipStream_t st) {
    GatherArgs g{};
    g.src[0] = mel; g.src[1] = emo; g.dst[0] = smel; g.dst[1] = semo; g.dim[0] = c->kmm.mel_dim; g.dim[1] = c->kmm.emotion_dim;
    g.vec[0] = aligned && g.dim[0] % 4 == 0; g.vec[1] = aligned && g.dim[1] % 4 == 0;
    g.F = F; g.start0 = start0; g.W = W; g.nf = (int)nf; g.Tw = (int)Tw;
    const int64_t dmax = g.dim[0] > g.dim[1] ? g.dim[0] : g.dim[1];
    int64_t blocks = (W * Tw * dmax / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
    hipLaunchKernelGGL(kmm_rollout_gather_kernel, dim3((unsigned)blocks, 2), dim3(256), 0, st, g);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

static int rollout(Context* c, const float* mel, const float* emo, int64_t B, int64_t F, int64_t T, int64_t first, const float* prev0,
                   float* state, int apply_constraints, float* out, float* raw, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const bool aligned = aligned16(mel) && aligned16(emo);
    const RolloutPlan p = rollout_plan(c, B, F, T, first, c->ro.chunk, aligned);
    if (p.ws_floats > c->ro.ws.n)
        return fail(KM_ERR_WORKSPACE, "km_koemorph_rollout: %lld workspace floats, %lld reserved: call km_koemorph_rollout_reserve",
                    (long long)p.ws_floats, (long long)c->ro.ws.n);
    const int NB = c->NB;
    const int64_t rows = F - first;
    // carve: the three (B, NB) frame buffers, then the staged windows, then (route 1) the chunk's encodings
    float* pb[2] = {c->ro.ws, c->ro.ws + up4(B * NB)};
    float* rawb = pb[1] + up4(B * NB);
    float* smel = rawb + up4(B * NB);
    const int64_t W1 = p.route == 1 ? B * (F - p.full0 < c->ro.chunk ? (F - p.full0 > 1 ? F - p.full0 : 1) : c->ro.chunk) : B;
    const int64_t Tws = p.route == 1 ? T : (T < F ? T : F);
    float* semo = smel + up4(W1 * Tws * c->kmm.mel_dim);
    float* xm = semo + up4(W1 * Tws * c->kmm.emotion_dim);
    float* xe = xm + W1 * T * kmmf::D;
    const float* prev = prev0;
    const int64_t per_frame_end = p.route == 1 ? p.full0 : F;
    int j = 0;
    for (int64_t i = first; i < per_frame_end; ++i, ++j) {
        const int64_t Ti = i + 1 < T ? i + 1 : T;
        if (int rc = gather(c, mel, emo, smel, semo, F, i - Ti + 1, B, 1, Ti, aligned, st)) return rc;
        float* o = pb[j & 1];
        if (int rc = launch_koemorph(c, smel, semo, B, Ti, nullptr, prev, state, apply_constraints, o, raw ? rawb : nullptr, nullptr, stream))
            return rc;
        hipLaunchKernelGGL(kmm_rollout_scatter_kernel, dim3((unsigned)((B * NB + 255) / 256)), dim3(256), 0, st, o, rawb, out, raw, B, NB, rows,
                           i - first);
        HIP_TRY(hipGetLastError());
        prev = o;
    }
    if (p.route != 1) return KM_OK;
    for (int64_t fs = p.full0; fs < F; fs += c->ro.chunk) {
        const int64_t cw = F - fs < c->ro.chunk ? F - fs : c->ro.chunk;
        if (int rc = gather(c, mel, emo, smel, semo, F, fs - T + 1, B * cw, cw, T, aligned, st)) return rc;
        if (int rc = launch_kmmf_encoder(c, smel, semo, B * cw, T, nullptr, xm, xe, stream)) return rc;
        const KmmTail ta = koemorph_tail(c, prev, state, apply_constraints, out + (fs - first) * NB, raw ? raw + (fs - first) * NB : nullptr);
        if (int rc = launch_kmmf_rollout(c, xm, xe, B, cw, T, prev, ta, rows * NB, pb[0], stream)) return rc;
        prev = pb[0];
    }
    return KM_OK;
}

}  // namespace km

using namespace km;

extern "C" {

int km_koemorph_rollout_reserve(km_handle h, int64_t max_clips, int64_t max_context, int64_t chunk_frames) {
    if (!h) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_reserve: NULL handle");
    Context* c = h;
    if (c->kind != 2) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_reserve: not a KoeMorphModel handle (km_koemorph_create)");
    if (max_clips < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_reserve: max_clips %lld < 1", (long long)max_clips);
    if (max_context < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_reserve: max_context %lld < 1", (long long)max_context);
    if (chunk_frames < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_reserve: chunk_frames %lld < 1", (long long)chunk_frames);
    if (int rc = need_ready(h)) return rc;
    // the per-frame launches (route 0, short windows) carve km_koemorph_forward's workspace
    if (int rc = reserve_koemorph(c, max_clips, max_context)) return rc;
    if (max_clips <= c->ro.clips && max_context <= c->ro.context && chunk_frames == c->ro.chunk) return KM_OK;
    const int64_t Bm = max_clips > c->ro.clips ? max_clips : c->ro.clips, Tm = max_context > c->ro.context ? max_context : c->ro.context;
    int64_t need = ws_route0(c, Bm, Tm);
    if (c->kmm_fused) {
        const int64_t n1 = ws_route1(c, Bm, Tm < kmmf::TMAX ? Tm : kmmf::TMAX, chunk_frames);
        if (n1 > need) need = n1;
    }
    c->ro.clips = c->ro.context = c->ro.chunk = 0;
    if (need > c->ro.ws.n)
        if (int rc = c->ro.ws.grow(need, nullptr, "km_koemorph_rollout_reserve")) return rc;
    c->ro.clips = Bm; c->ro.context = Tm; c->ro.chunk = chunk_frames;
    return KM_OK;
}

int km_koemorph_rollout_plan(km_handle h, int64_t B, int64_t F, int64_t T, int64_t first_frame, int64_t out[5]) {
    if (!h || !out) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_plan: NULL argument");
    Context* c = h;
    if (c->kind != 2) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_plan: not a KoeMorphModel handle (km_koemorph_create)");
    if (!c->host_finalized) return fail(KM_ERR_NOT_FINALIZED, "km_koemorph_rollout_plan: call km_finalize_host or km_finalize first");
    if (B < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_plan: B %lld < 1", (long long)B);
    if (F < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_plan: F %lld < 1", (long long)F);
    if (T < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_plan: T %lld < 1", (long long)T);
    if (first_frame < 0 || first_frame >= F)
        return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout_plan: first_frame %lld outside 0 .. %lld", (long long)first_frame, (long long)(F - 1));
    const RolloutPlan p = rollout_plan(c, B, F, T, first_frame, c->ro.chunk > 0 ? c->ro.chunk : kRolloutChunkDefault, true);
    out[0] = p.route; out[1] = p.chunks; out[2] = p.short_frames; out[3] = p.launches; out[4] = p.ws_floats;
    return KM_OK;
}

int km_koemorph_rollout(km_handle h, const float* mel_dev, const float* emotion_dev, int64_t B, int64_t F, int64_t T, int64_t first_frame,
                        const float* prev0_dev, float* smoother_state_dev, int32_t apply_constraints, float* out_dev, float* raw_dev,
                        void* stream) {
    if (!h) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: NULL handle");
    Context* c = h;
    if (c->kind != 2) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: not a KoeMorphModel handle (km_koemorph_create)");
    if (!mel_dev) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: mel_dev is NULL");
    if (!emotion_dev) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: emotion_dev is NULL");
    if (!out_dev) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: out_dev is NULL");
    if (B < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: B %lld < 1", (long long)B);
    if (F < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: F %lld < 1", (long long)F);
    if (T < 1) return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: T %lld < 1", (long long)T);
    if (first_frame < 0 || first_frame >= F)
        return fail(KM_ERR_INVALID_ARG, "km_koemorph_rollout: first_frame %lld outside 0 .. %lld", (long long)first_frame, (long long)(F - 1));
    if (int rc = need_ready(h)) return rc;
    if (c->ro.clips == 0 || !c->ro.ws)
        return fail(KM_ERR_WORKSPACE, "km_koemorph_rollout: no workspace: call km_koemorph_rollout_reserve");
    if (B > c->ro.clips || T > c->ro.context)
        return fail(KM_ERR_WORKSPACE, "km_koemorph_rollout: %lld clips x %lld context frames, reserved %lld x %lld: call km_koemorph_rollout_reserve",
                    (long long)B, (long long)T, (long long)c->ro.clips, (long long)c->ro.context);
    return rollout(c, mel_dev, emotion_dev, B, F, T, first_frame, prev0_dev, smoother_state_dev, apply_constraints, out_dev, raw_dev, stream);
}

}  // extern "C"
