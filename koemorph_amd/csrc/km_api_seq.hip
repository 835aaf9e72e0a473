// C-ABI entry points of sequence mode: km_sequence_* (declared in include/koemorph.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "km_api_internal.h"
#include "km_context.h"
#include "km_device.h"
#include "km_gemm.h"

using namespace km;

extern "C" {

int64_t km_sequence_num_outputs(km_handle h, int64_t L, int32_t stride_frames) {
    if (!h || L < 0 || stride_frames <= 0) return -1;
    const int64_t num_frames = L / h->cfg.mel.hop_length;                       // sequential_dual_stream_model.py:84
    const int64_t n = (num_frames - h->T) / stride_frames + 1;                   // :96 (floor division)
    const int64_t nn = (num_frames - h->T) >= 0 ? n : ((num_frames - h->T - (stride_frames - 1)) / stride_frames + 1);
    return nn > 1 ? nn : 1;
}

}  // extern "C"

// The schedule of a sequence call (km_sequence_plan names it; sequence_forward runs it).  Host arithmetic on the handle's shape,
// its front-end plan and its switches alone, so the query and the call cannot disagree.
//   route 0  per window: every window's T + 1 STFT frames
//   route 1  the clip's STFT once + frames 0 and T of every window, both images read by the fused core (which takes frames 0 and
//            T alone from the edge image: right only where no other frame sees the window's padding, clip_frames_shared)
//   route 2  option seq_assemble: the clip's STFT once + the E frames at either end of every window that see its padding
//            (E = ceil((n_fft / 2) / hop), koemorph_amd/clip_span.py::edge_frames), assembled per tile into the workspace the core
//            behind km_forward_audio's power path reads (km_seq_assemble.hip)
struct SeqPlan { int route, E; int64_t N, nfc, stft_frames; };

// mel_rp_ok as the host knows it before the plan is uploaded (upload_mel_plan mirrors the grouped filter image whenever it exists)
static bool mel_rp_planned(Context* c, MelPlan* p) { return p->cfg.n_fft == 1024 && !c->opt.mel_two_frame && !p->fbg_gid.empty(); }

static SeqPlan seq_plan(km_handle h, int64_t B, int64_t L, int32_t stride_frames, bool with_attention) {
    Context* c = h;
    MelPlan* plan = c->mel_plans[0];
    const km_mel_config& m = plan->cfg;
    const int64_t hop = m.hop_length, n_frames = (int64_t)c->T + 1, lim = (int64_t)1 << 31;
    SeqPlan p{};
    p.N = km_sequence_num_outputs(h, L, stride_frames);
    p.E = (int)((m.n_fft / 2 + hop - 1) / hop);
    p.nfc = (p.N - 1) * stride_frames + n_frames;                                // clip frames any window touches
    const bool rp = mel_rp_planned(c, plan), dedup = !c->opt.seq_per_window;     // seq_per_window: tests compare the schedules
    const bool sizes_ok = B < lim && p.N < lim && p.nfc < lim;                   // (the products below then fit 64 bits)
    const int64_t total = sizes_ok ? B * p.N : 0;
    if (c->opt.seq_assemble && dedup && core_takes_power(c, with_attention) && rp && m.pad_mode == KM_PAD_CONSTANT && c->NK % 4 == 0 && n_frames >= 2 * p.E &&
        L >= (int64_t)c->T * hop && sizes_ok && B * p.nfc < lim / c->NK && total * 3 * p.E < lim / c->NK) {
        p.route = 2;
        p.stft_frames = B * p.nfc + total * 3 * p.E;         // per window E left-edge rows and E launches of 2 rows (row 0 discarded)
    } else if (c->fused_ok && dedup && rp && clip_frames_shared(c, plan) && p.N < (1 << 24)) {
        p.route = 1;
        p.stft_frames = B * (p.nfc + 2 * p.N);
    } else {
        p.route = 0;
        p.stft_frames = B * p.N * n_frames;
    }
    return p;
}

extern "C" {

int km_sequence_plan(km_handle h, int64_t B, int64_t L, int32_t stride_frames, int32_t with_attention, int64_t out[4]) {
    if (!h || !out || B <= 0 || L <= 0 || stride_frames <= 0) return fail(KM_ERR_INVALID_ARG, "km_sequence_plan: bad argument");
    if (h->kind != 0) return fail(KM_ERR_INVALID_ARG, "km_sequence_plan needs a dual-stream handle (km_create)");
    if (!h->host_finalized) return fail(KM_ERR_NOT_FINALIZED, "km_sequence_plan: call km_finalize_host or km_finalize first");
    const SeqPlan p = seq_plan(h, B, L, stride_frames, with_attention != 0);
    if (p.N > 0x7fffffff) return fail(KM_ERR_INVALID_ARG, "too many output frames");
    out[0] = p.route; out[1] = p.N; out[2] = p.stft_frames; out[3] = p.E;
    return KM_OK;
}

// Where a window's emotion logit comes from in km_sequence_forward_track: the rows of every clip's track and the closed-form
// window -> row map (SeqTrackMap).  Null: one vector per clip (km_sequence_forward).
struct SeqTrack { const float* track; int64_t K, first, interval, sample_offset, clip_len; };

// What km_sequence_forward_attn adds to a sequence call: the pre-weight sigmoid values (B, N, 52) and the head-averaged maps
// (B, N, 28, NK) of every window, indexed like out_dev, and / or an accumulator (km_attn_stats_*) that takes every tile's maps.
// With an accumulator and no caller's map the maps of a tile live in seq.attn and are overwritten by the next tile.
struct SeqOutputs { float* raw; float* attn; void* stats; };

static int sequence_forward(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev, const SeqTrack* trk,
                            int32_t stride_frames, int32_t smooth, float* out_dev, void* stream, const SeqOutputs& xo = SeqOutputs{nullptr, nullptr, nullptr}) {
    Context* c = h;
    if (!c->fused_ok && !c->ws.generic)
        return fail(KM_ERR_WORKSPACE, "generic workspace missing: call km_reserve after km_finalize");
    const int hop = c->cfg.mel.hop_length;
    const int64_t N = km_sequence_num_outputs(h, L, stride_frames);
    const int64_t W = (int64_t)c->T * hop;                 // window_samples (sequential_dual_stream_model.py:54)
    const int64_t step = (int64_t)stride_frames * hop;     // stride_samples (:55)
    const int64_t n_frames = 1 + W / hop;
    if (c->ws.windows < B || c->ws.windows < 1 || n_frames > c->ws.frames)
        return fail(KM_ERR_WORKSPACE, "workspace too small for %lld clips / %lld-frame windows: call km_reserve",
                    (long long)B, (long long)n_frames);
    if (N > 0x7fffffff) return fail(KM_ERR_INVALID_ARG, "too many output frames");
    const int64_t total = B * N, tile = c->ws.windows;
    // Shared-frame path.  Windows start at multiples of the hop (:101-117), so frame f of window i IS clip frame
    // i*stride + f for f = 1 .. T-1; only frame 0 and frame T see the zero padding at the window boundary.  The STFT
    // of the clip is computed once (N-1)*stride + T + 1 frames instead of N * (T+1)), the two edge frames per window
    // separately, and the core reads its rows from both images.  Results are bit-identical to the per-window path.
    // That holds for hop >= n_fft / 2 (clip_frames_shared); below it frames 1 and T - 1 reach into the padding too, and the
    // schedule is the per-window one unless option seq_assemble asks for the assembled route, which knows every edge frame.
    MelPlan* plan = c->mel_plans[0];
    const SeqPlan sp = seq_plan(h, B, L, stride_frames, xo.attn != nullptr || xo.stats != nullptr);
    const bool shared = sp.route == 1, assembled = sp.route == 2;
    const int64_t nfc = sp.nfc;                                                 // clip frames any window touches
    const int64_t edge_rows = assembled ? 3 * sp.E : 2;                         // rows per window of the edge image(s)
    if (shared || assembled) {     // grow-only images and their per-row maxima; allocates, so refused inside a stream capture, before any launch
        const char* what = "km_sequence_forward: elements of the clip / window images";
        if (int rc = c->seq.pow.grow(B * nfc * c->NK, stream, what)) return rc;
        if (int rc = c->seq.fmax.grow(B * nfc, stream, what)) return rc;
        if (int rc = c->seq.edge.grow(total * edge_rows * c->NK, stream, what)) return rc;
        if (int rc = c->seq.emax.grow(total * edge_rows, stream, what)) return rc;
        if (assembled)
            if (int rc = ensure_chunk_counters(c, total, stream)) return rc;    // the edge launches run over all windows at once
    }
    const int64_t map_floats = (int64_t)28 * c->NK;
    const bool tile_maps = xo.stats && !xo.attn;     // the maps of one tile at a time, for the accumulator alone
    if (tile_maps)
        if (int rc = c->seq.attn.grow(tile * map_floats, stream, "km_sequence_forward_attn: floats of the maps of one tile")) return rc;
    // rows of tile w0: the caller's arrays at w0, or the tile buffer
    auto raw_at = [&](int64_t w0) { return xo.raw ? xo.raw + w0 * c->NB : nullptr; };
    auto attn_at = [&](int64_t w0) { return xo.attn ? xo.attn + w0 * map_floats : (tile_maps ? c->seq.attn : nullptr); };
    auto stats_take = [&](int64_t w0, int64_t nw) { return xo.stats ? km_attn_stats_update(xo.stats, attn_at(w0), nw, stream) : KM_OK; };
    const float* zemo = c->ws.zemo;
    if (trk) {
        // a logit per track ROW (about nine windows share one), then one per window by the closed-form map: the core launches
        // below read zwin[win0 + b]
        const char* what = "km_sequence_forward_track: track rows / windows";
        if (int rc = c->seq.ztrack.grow(B * trk->K, stream, what)) return rc;
        if (int rc = c->seq.zwin.grow(total, stream, what)) return rc;
        if (int rc = launch_emotion(c, trk->track, B * trk->K, c->seq.ztrack, stream)) return rc;
        const SeqTrackMap map{trk->K, trk->first, trk->interval, trk->sample_offset, trk->clip_len, step, W};
        if (int rc = launch_seq_track_logits(c, c->seq.ztrack, c->seq.zwin, total, (int)N, map, stream)) return rc;
        zemo = c->seq.zwin;
    } else {
        // emotion features ONCE for the entire audio (:88): one logit per clip
        if (int rc = launch_emotion(c, emotion_dev, B, c->ws.zemo, stream)) return rc;
    }
    SeqAssemble sa{};
    SeqCore sc{};
    if (assembled) {
        const int E = sp.E, T = c->T;
        if (int rc = launch_seq_zero_maxima(c->seq.fmax, B * nfc, c->seq.emax, total * edge_rows, stream)) return rc;
        // (1) every clip as one long "window" of nfc frames
        const SeqFrames clip_img{c->seq.pow, c->seq.fmax, nfc, 1};
        if (int rc = launch_mel_power(c, plan, mel_clip_windows(audio_dev, L, B, (nfc - 1) * hop, 0, 0, 1), stream, mel_to_frames(&clip_img))) return rc;
        // (2) the edge frames of every window with the front end as it is: frames 0 .. E - 1 in one launch, then frame T - j as row
        // 1 of a two-row launch with frame_mul = T - j (its row 0, frame 0 again, is not read), j = 0 .. E - 1
        const MelSrc wins = mel_clip_windows(audio_dev, L, total, W, step, 0, (int)N);
        const SeqFrames left_img{c->seq.edge, c->seq.emax, E, 1};
        if (int rc = launch_mel_power(c, plan, wins, stream, mel_to_frames(&left_img))) return rc;
        float* right = c->seq.edge + total * E * c->NK;
        unsigned* rmax = c->seq.emax + total * E;
        for (int j = 0; j < E; ++j) {
            const SeqFrames right_img{right + (int64_t)j * total * 2 * c->NK, rmax + (int64_t)j * total * 2, 2, T - j};
            if (int rc = launch_mel_power(c, plan, wins, stream, mel_to_frames(&right_img))) return rc;
        }
        // (3) per tile: the windows' rows and maxima into the workspace, then the core km_forward_audio runs on its power path
        // (the assemble kernel stores the maxima it needs; the slots of a fresh workspace beyond a short tile are cleared once, as
        // launch_mel_power clears them, because the core launches below declare the maxima clean)
        if (int rc = clear_stale_maxima(c, stream)) return rc;
        sa = SeqAssemble{c->seq.pow, c->seq.fmax, c->seq.edge, c->seq.emax, right, rmax, total, (int)nfc, (int)stride_frames, (int)N, E, T};
    } else if (shared) {
        hipStream_t st = (hipStream_t)stream;
        HIP_TRY(hipMemsetAsync(c->seq.fmax, 0, (size_t)B * nfc * sizeof(unsigned), st));
        HIP_TRY(hipMemsetAsync(c->seq.emax, 0, (size_t)total * 2 * sizeof(unsigned), st));
        // (1) every clip as one long "window" of nfc frames, zero beyond the clip end
        const SeqFrames clip_img{c->seq.pow, c->seq.fmax, nfc, 1};
        if (int rc = launch_mel_power(c, plan, mel_clip_windows(audio_dev, L, B, (nfc - 1) * hop, 0, 0, 1), stream, mel_to_frames(&clip_img))) return rc;
        // (2) the first and last frame of every window (rows 0 and 1 = frames 0 and T of the window)
        const SeqFrames edge_img{c->seq.edge, c->seq.emax, 2, (int)(n_frames - 1)};
        if (int rc = launch_mel_power(c, plan, mel_clip_windows(audio_dev, L, total, W, step, 0, (int)N), stream, mel_to_frames(&edge_img))) return rc;
        // (3) per tile: window maxima, then the fused core reading rows from both images
        sc = SeqCore{c->seq.pow, c->seq.edge, (int)nfc, (int)stride_frames, (int)N};
    }
    // The tiles.  Ahead of the core, route 2 assembles the tile's rows into the workspace, route 1 takes its window maxima from the
    // images, route 0 runs the front end per window (which also clears stale maxima); the core reads a logit per window of the
    // sequence (track) or per clip.  A generic shape on route 0 keeps the staged log-mel and the chain behind it, as
    // km_core_forward runs it: the one tile that is not the core behind the power-mel.
    const bool staged = sp.route == 0 && !c->fused_ok;
    for (int64_t w0 = 0; w0 < total; w0 += tile) {
        const int64_t nw = (total - w0) < tile ? (total - w0) : tile;
        float* out = out_dev + w0 * c->NB;
        CoreSrc cs = trk ? core_workspace_seq_win(w0) : core_workspace_seq(w0, (int)N);
        if (assembled) {
            if (int rc = launch_seq_assemble(c, sa, nw, w0, stream)) return rc;
        } else if (shared) {
            if (int rc = launch_seq_window_max(c, c->seq.fmax, c->seq.emax, nw, w0, (int)nfc, (int)stride_frames, (int)N, (int)n_frames, stream)) return rc;
            cs = trk ? core_strided_win(&sc, w0) : core_strided(&sc, w0);
        } else {
            const MelSrc src = mel_clip_windows(audio_dev, L, nw, W, step, w0, (int)N);
            if (int rc = staged ? launch_mel(c, plan, src, 0, c->ws.mel, c->ws.mel_short, stream) : launch_mel_power(c, plan, src, stream)) return rc;
        }
        if (staged) {     // per-window logits gathered from the per-clip ones, GEMM-chain core
            if (!trk)
                if (int rc = launch_gather_clip_logits(c, c->ws.zemo, c->ws.zemo_win, nw, w0, (int)N, stream)) return rc;
            if (int rc = launch_core_generic(c, c->ws.mel, nw, n_frames, c->ws.mel_short, trk ? zemo + w0 : c->ws.zemo_win, out, raw_at(w0),
                                             attn_at(w0), stream)) return rc;
        } else {
            if (int rc = launch_core_power(c, plan, nw, n_frames, zemo, out, stream, with_outputs(cs, raw_at(w0), attn_at(w0)))) return rc;
        }
        if (int rc = stats_take(w0, nw)) return rc;
    }
    if (smooth) return launch_ema_scan(c, out_dev, B, N, stream);
    return KM_OK;
}

int km_sequence_forward(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                        int32_t stride_frames, int32_t smooth, float* out_dev, void* stream) {
    if (int rc = need_dual(h)) return rc;
    if (!audio_dev || !emotion_dev || !out_dev || B <= 0 || L <= 0 || stride_frames <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward: bad argument");
    return sequence_forward(h, audio_dev, B, L, emotion_dev, nullptr, stride_frames, smooth, out_dev, stream);
}

int km_sequence_forward_track(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* track_dev, int64_t K,
                              int64_t first_samples, int64_t interval_samples, int64_t sample_offset, int64_t clip_len,
                              int32_t stride_frames, int32_t smooth, float* out_dev, void* stream) {
    // the argument checks need no handle state and come first: they hold on a handle that is not finalized yet
    if (!h || !audio_dev || !track_dev || !out_dev || B <= 0 || L <= 0 || stride_frames <= 0)
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_track: bad argument");
    const int64_t lim = (int64_t)1 << 62;                  // keeps sample_offset + (window index) * step + window inside int64
    if (K < 1 || interval_samples < 1 || first_samples < 0 || sample_offset < 0 || clip_len > lim || clip_len < L ||
        clip_len - L < sample_offset)
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_track: K %lld, first %lld, interval %lld, offset %lld, clip_len %lld for a chunk of %lld",
                    (long long)K, (long long)first_samples, (long long)interval_samples, (long long)sample_offset, (long long)clip_len,
                    (long long)L);
    if (K > 0x7fffffff / B) return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_track: %lld x %lld track rows, at most 2^31 - 1", (long long)B, (long long)K);
    if (int rc = need_dual(h)) return rc;
    const SeqTrack trk{track_dev, K, first_samples, interval_samples, sample_offset, clip_len};
    return sequence_forward(h, audio_dev, B, L, nullptr, &trk, stride_frames, smooth, out_dev, stream);
}

int km_sequence_forward_attn(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                             const float* track_dev, int64_t K, int64_t first_samples, int64_t interval_samples,
                             int64_t sample_offset, int64_t clip_len, int32_t stride_frames, int32_t smooth,
                             float* out_dev, float* raw_dev, float* attn_dev, void* stats, void* stream) {
    // as in km_sequence_forward_track, the argument checks need no handle state and come first
    if (!h || !audio_dev || !out_dev || B <= 0 || L <= 0 || stride_frames <= 0 || (emotion_dev != nullptr) == (track_dev != nullptr))
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: bad argument (exactly one of emotion_dev and track_dev)");
    if (track_dev) {
        const int64_t lim = (int64_t)1 << 62;
        if (K < 1 || interval_samples < 1 || first_samples < 0 || sample_offset < 0 || clip_len > lim || clip_len < L ||
            clip_len - L < sample_offset)
            return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: K %lld, first %lld, interval %lld, offset %lld, clip_len %lld for a chunk of %lld",
                        (long long)K, (long long)first_samples, (long long)interval_samples, (long long)sample_offset, (long long)clip_len,
                        (long long)L);
        if (K > 0x7fffffff / B) return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: %lld x %lld track rows, at most 2^31 - 1", (long long)B, (long long)K);
    }
    if (stats && attn_dev && !aligned16(attn_dev))
        return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: with an accumulator attn_dev must be 16-byte aligned");
    if (int rc = need_dual(h)) return rc;
    if (stats) {
        int32_t q = 0, k = 0;
        if (int rc = km_attn_stats_shape(stats, &q, &k)) return rc;
        if (q != 28 || k != h->NK)
            return fail(KM_ERR_INVALID_ARG, "km_sequence_forward_attn: the accumulator holds %d x %d maps, the model's are 28 x %d", q, k, h->NK);
    }
    if (attn_dev || stats)
        if (int rc = attn_refused(h, "km_sequence_forward_attn")) return rc;
    const SeqOutputs xo{raw_dev, attn_dev, stats};
    if (track_dev) {
        const SeqTrack trk{track_dev, K, first_samples, interval_samples, sample_offset, clip_len};
        return sequence_forward(h, audio_dev, B, L, nullptr, &trk, stride_frames, smooth, out_dev, stream, xo);
    }
    return sequence_forward(h, audio_dev, B, L, emotion_dev, nullptr, stride_frames, smooth, out_dev, stream, xo);
}

}  // extern "C"
