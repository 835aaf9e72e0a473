/*
 * koemorph.h -- C-ABI of libkoemorph_hip.so, the MI355X (gfx950) implementation of the
 * KoeMorph hot path.
 *
 * The reference (atsuki-ichikawa/KoeMorph) is 100 % Python and has no FFI / plugin
 * interface; its boundary for this path is a set of torch.nn.Module.forward methods
 * (SURVEY.md section 8b).  This header is what a maintainer would bind from those methods
 * (ctypes stub in INTEGRATION.md).  Every entry point cites the reference interface it
 * replaces as path:line relative to the reference repository root.
 *
 * Conventions
 *   - plain C: pointers, sizes, int status codes.  No torch / C++ types.
 *   - every function returns KM_OK (0) or a negative km_status; km_last_error() gives a
 *     thread-local message for the last failure on the calling thread.
 *   - all `const float*` / `float*` arguments named *_dev are DEVICE pointers owned by the
 *     caller (e.g. torch tensor.data_ptr()), fp32, contiguous, 16-byte aligned.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Launch functions
 *     (everything taking a stream except km_finalize / km_reserve) neither allocate nor
 *     synchronise, so they can be captured into a hipGraph.
 *   - the library owns a packed copy of the weights and a workspace; km_reserve sizes the
 *     workspace up front, launch functions fail with KM_ERR_WORKSPACE if it is too small.
 *   - not re-entrant per handle (the reference modules are not either: stateful EMA,
 *     src/model/simplified_dual_stream_model.py:164); use one handle per thread/stream.
 */
#ifndef KOEMORPH_H
#define KOEMORPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: km_koemorph_config grew (output_activation, smoothing_method, smoothing_window); km_loss_config grew (ds_*) and now
 * starts with its own abi_version -- a caller built against the version-1 header is refused instead of being read past. */
#define KM_ABI_VERSION 2

typedef enum km_status {
    KM_OK = 0,
    KM_ERR_INVALID_ARG = -1,   /* bad shape / NULL / misaligned pointer (reference: ValueError, src/features/stft.py:115-116) */
    KM_ERR_UNSUPPORTED = -2,   /* configuration has no kernel */
    KM_ERR_NOT_FINALIZED = -3, /* forward before km_finalize, or a parameter is missing */
    KM_ERR_WORKSPACE = -4,     /* km_reserve was not called with a large enough batch */
    KM_ERR_HIP = -5,           /* HIP runtime error; message in km_last_error() */
    KM_ERR_NOT_READY = -6      /* streaming: ring not full yet (reference returns None, src/features/mel_sliding_window.py:126-127) */
} km_status;

typedef struct km_context* km_handle;

/* Mel front-end variants (the reference has three inconsistent ones). */
typedef enum km_mel_scale { KM_MEL_SLANEY = 0, KM_MEL_HTK = 1 } km_mel_scale;
typedef enum km_pad_mode { KM_PAD_CONSTANT = 0, KM_PAD_REFLECT = 1 } km_pad_mode;
typedef enum km_log_mode {
    KM_LOG_DB_MAX = 0, /* librosa.power_to_db(ref=np.max, amin, top_db) then (x + db_add) * db_scale */
    KM_LOG_LN_EPS = 1  /* log(mel + log_eps)  (src/features/stft.py:123) */
} km_log_mode;

typedef struct km_mel_config {
    int32_t sample_rate;   /* 16000 */
    int32_t n_fft;         /* 512 or 1024 */
    int32_t hop_length;    /* int(sample_rate / target_fps): 533 @30 fps, 266 @60 fps */
    int32_t n_mels;        /* 80 */
    float f_min;           /* 80 */
    float f_max;           /* 8000 */
    int32_t mel_scale;     /* km_mel_scale */
    int32_t slaney_norm;   /* 1: area-normalised triangles (librosa norm='slaney') */
    int32_t pad_mode;      /* km_pad_mode; frames are always centred (center=True) */
    int32_t window_norm;   /* 1: divide the STFT by sqrt(sum(w^2)) (torchaudio normalized=True) */
    int32_t log_mode;      /* km_log_mode */
    float amin;            /* 1e-10 */
    float top_db;          /* 80 */
    float db_add;          /* 80  -> (x + 80) / 80, simplified_dual_stream_model.py:200; 0 for none */
    float db_scale;        /* 1/80;  1 for none */
    float log_eps;         /* 1e-8 */
} km_mel_config;

/* Mirrors DualStreamCrossAttention.__init__ (src/model/dual_stream_attention.py:57-70)
 * plus the front end and smoothing of SimplifiedDualStreamModel
 * (src/model/simplified_dual_stream_model.py:28-55,163). */
typedef struct km_config {
    int32_t abi_version;          /* KM_ABI_VERSION */
    int32_t d_model;              /* 256 */
    int32_t num_heads;            /* 8 */
    int32_t num_mel_channels;     /* 80 */
    int32_t mel_sequence_length;  /* 256 */
    int32_t mel_temporal_frames;  /* 3 */
    int32_t emotion_dim;          /* 256 */
    int32_t num_blendshapes;      /* 52 */
    float temperature;            /* 1.0 */
    km_mel_config mel;            /* batch front end of the model */
} km_config;

/* ---- lifecycle ---------------------------------------------------------------------- */
int km_abi_version(void);
const char* km_last_error(void);

/* Construct for the current HIP device.  Replaces DualStreamCrossAttention.__init__ /
 * SimplifiedDualStreamModel.__init__.  Works without a GPU (host-side state only) so that
 * parameter folding can be exercised on the CPU; device memory is touched from km_finalize on. */
int km_create(const km_config* cfg, km_handle* out);
int km_destroy(km_handle h);
/* Bytes of device memory this library holds in the whole process: every allocation of every handle (km_create, the accumulators,
 * the emotion / resampler / eGeMAPS handles) counts from the moment it exists until it is freed.  0 after load; back at its earlier
 * value once everything created since has been destroyed.  A leak check that does not depend on what else uses the device. */
int64_t km_live_device_bytes(void);

/* Replaces nn.Module.load_state_dict for one tensor.  `key` is the reference state-dict key
 * relative to DualStreamCrossAttention (e.g. "mel_attention.in_proj_weight"; the full-model
 * prefix "dual_stream_attention." is accepted and stripped) or "smoothing_alpha"
 * (simplified_dual_stream_model.py:163).  `data` is a HOST pointer to fp32. */
int km_load_param(km_handle h, const char* key, const float* data, const int64_t* shape, int32_t ndim);
/* Copy a parameter back to the host (state_dict()); n = number of floats in `out`. */
int km_get_param(km_handle h, const char* key, float* out, int64_t n);
/* Number of parameters the configuration expects / has received so far. */
int km_param_count(km_handle h, int32_t* expected, int32_t* loaded);

/* Fold + pack the weights for the kernels (host, double precision) and upload them.
 * Must follow the last km_load_param and precede any forward.  Allocates and synchronises. */
int km_finalize(km_handle h, void* stream);
/* Host half of km_finalize only (no GPU needed): used by the CPU tests. */
int km_finalize_host(km_handle h);
/* Size the workspace for batches up to max_windows windows of up to max_samples audio samples
 * (0 = core only).  Allocates; call outside any graph capture. */
int km_reserve(km_handle h, int64_t max_windows, int64_t max_samples);

/* ---- forward path ---------------------------------------------------------------------- */

/* Batch log-mel front end.  Replaces SimplifiedDualStreamModel.extract_mel_features
 * (src/model/simplified_dual_stream_model.py:166-229) with the handle's km_config.mel:
 * audio_dev (B, L) -> mel_long_dev (B, n_frames, n_mels), mel_short_dev (B, 3, n_mels) = the
 * last three frames, n_frames = 1 + L / hop.  mel_short_dev may be NULL. */
int km_mel_batch(km_handle h, const float* audio_dev, int64_t B, int64_t L,
                 float* mel_long_dev, float* mel_short_dev, void* stream);
int64_t km_mel_num_frames(km_handle h, int64_t L);

/* Stand-alone front end with an explicit configuration and output frame policy.  Replaces
 * MelSpectrogramExtractor.forward (src/features/stft.py:101-142) and
 * MelSlidingWindowExtractor.process_audio_batch / the per-tick extraction
 * (src/features/mel_sliding_window.py:280-307,326-365).  out_frames > 0 truncates, or pads by
 * repeating the last frame, to exactly out_frames rows (stft.py:130-140). */
int km_mel_extract(km_handle h, const km_mel_config* cfg, const float* audio_dev, int64_t B, int64_t L,
                   int64_t out_frames, float* mel_dev, void* stream);

/* Attention core.  Replaces DualStreamCrossAttention.forward
 * (src/model/dual_stream_attention.py:162-280), eval mode:
 *   mel_dev (B, T_in, 80)  zero-padded / truncated to mel_sequence_length (:193-202)
 *   mel_short_dev (B, 3, 80), emotion_dev (B, emotion_dim)
 *   out_dev (B, 52)                      'blendshapes'
 *   raw_dev (B, 52) or NULL              sigmoid outputs before the stream weights; the host
 *                                        derives 'mel_blendshapes' / 'emotion_blendshapes' (:257-262)
 *   attn_mel_dev (B, 28, 80) or NULL     'mel_attention_weights' (head-averaged)
 * ('emotion_attention_weights' is identically 1: softmax over a single key, :234-239.) */
int km_core_forward(km_handle h, const float* mel_dev, int64_t B, int64_t T_in,
                    const float* mel_short_dev, const float* emotion_dev,
                    float* out_dev, float* raw_dev, float* attn_mel_dev, void* stream);

/* The two halves of km_core_forward as separate launches (same arithmetic; bench.py times the
 * dominant kernel alone through km_core_forward_z):
 *   km_emotion_logit   emotion stream, z_dev (B) = the decoder logit shared by the 24 expression rows
 *                      (src/model/dual_stream_attention.py:216-218, :234-240, :248)
 *   km_core_forward_z  mel stream + decoder + stream weights with the logits supplied by the caller. */
int km_emotion_logit(km_handle h, const float* emotion_dev, int64_t B, float* z_dev, void* stream);
int km_core_forward_z(km_handle h, const float* mel_dev, int64_t B, int64_t T_in,
                      const float* mel_short_dev, const float* z_dev,
                      float* out_dev, float* raw_dev, float* attn_mel_dev, void* stream);

/* Temporal smoothing.  Replaces SimplifiedDualStreamModel.apply_temporal_smoothing
 * (src/model/simplified_dual_stream_model.py:341-368): alpha = sigmoid(smoothing_alpha);
 * first != 0 stores x into state and leaves x unchanged, otherwise x = alpha*x + (1-alpha)*state
 * and state = x.  x_dev, state_dev: (B, 52). */
int km_smooth(km_handle h, float* x_dev, float* state_dev, int64_t B, int32_t first, void* stream);

/* Whole-model forward.  Replaces SimplifiedDualStreamModel.forward
 * (src/model/simplified_dual_stream_model.py:370-415) with the emotion vector supplied by the
 * caller (openSMILE / emotion2vec are host-side providers, out of scope):
 * audio_dev (B, L) -> out_dev (B, 52).  state_dev (B,52) or NULL disables smoothing. */
int km_forward_audio(km_handle h, const float* audio_dev, int64_t B, int64_t L,
                     const float* emotion_dev, float* out_dev, float* state_dev, int32_t first,
                     void* stream);

/* km_forward_audio for B windows of ONE clip resident in HBM -- the eval-mode twin of km_train_step_clip, for the validation
 * pass between epochs.  Replaces the per-window slicing (src/data/sequential_dataset.py:156-209) + the per-window log-mel
 * (src/model/simplified_dual_stream_model.py:184-229) under the validation forward (src/train_sequential.py:257-259) without
 * materialising the (B, T * hop) windows.  Window b is samples [start_frames[b] * hop, + T * hop) of clip_dev (clip_len samples,
 * zero beyond), exactly what km_gather_windows would have copied; the start frames may come in any order and may repeat.
 * emotion_dev is (B, emotion_dim), one vector per window; state_dev / first as in km_forward_audio (the caller carries the
 * (B, 52) EMA state from batch to batch -- km_sequence_forward smooths along the frame axis of a clip instead and takes one
 * emotion vector per clip, so it cannot stand in).  The STFT frames the windows share are computed once -- max - min + T + 1 clip
 * frames + 2 zero-padded boundary frames per window instead of B * (T + 1) -- the dB reference of a window is the maximum over
 * its own T + 1 frames, and the fused core reads its rows through the start-frame table: out_dev and state_dev are
 * bit-identical to km_gather_windows + km_forward_audio.  min_start_frame / max_start_frame are HOST copies of the extremes of
 * start_frames_dev (they size the launches; nothing is read back, so the call can be captured into a hipGraph).  The span and
 * edge images belong to the inference context (no km_train_init needed) and only grow: a span wider, or a batch larger, than
 * any earlier call's allocates, so capture only after a warm-up call with that span.  Needs km_reserve(B, 0).
 *   km_forward_clip_supported   1 when km_forward_clip runs on this handle (after km_finalize), else 0: the fused core
 *                        (d_model 256, window 256, 8 heads) behind the 1024-point front end (not mel_two_frame), pad_mode
 *                        constant and hop_length >= n_fft / 2 (see km_train_clip_supported).  On any other handle
 *                        km_forward_clip returns KM_ERR_UNSUPPORTED, never another result -- unless option "clip_assemble"
 *                        is set, which adds the handles of km_clip_plan route 2 (they need km_reserve(B, T * hop): the windows
 *                        are assembled into the front end's workspace). */
int km_forward_clip_supported(km_handle h);
int km_forward_clip(km_handle h, const float* clip_dev, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                    int32_t min_start_frame, int32_t max_start_frame, const float* emotion_dev,
                    float* out_dev, float* state_dev, int32_t first, void* stream);

/* Throughput mode of km_forward_audio: a two-deep software pipeline ACROSS calls.  The front end (VALU/LDS bound
 * FFT) of call i runs on an internal stream concurrently with the fused core (fp32-MFMA bound) of call i-1, which
 * the hardware co-schedules on the same CUs (separate matrix and vector pipes); the power-mel workspace is double
 * buffered.  Differences from km_forward_audio:
 *   - out_dev (and state_dev) of call i are complete only after the NEXT pipelined call returns and the caller's
 *     stream has advanced past it, or after km_pipeline_flush(h, stream);
 *   - audio_dev / emotion_dev of call i must stay untouched until then as well.
 * EMA state is applied in call order.  Mixing with the non-pipelined entry points requires a flush in between. */
int km_forward_audio_pipelined(km_handle h, const float* audio_dev, int64_t B, int64_t L,
                               const float* emotion_dev, float* out_dev, float* state_dev, int32_t first,
                               void* stream);
int km_pipeline_flush(km_handle h, void* stream);

/* Sequence forward.  Replaces SequentialDualStreamModel.forward
 * (src/model/sequential_dual_stream_model.py:63-167): slides a mel_sequence_length-frame
 * window with stride_frames over each clip, one output frame per position, EMA reset at the
 * clip start.  audio_dev (B, L) -> out_dev (B, N, 52), N = km_sequence_num_outputs().
 * Windows are addressed in place inside the clip (no (B*N, window) copy is materialised) and processed
 * in tiles of the reserved workspace size.  The reference recomputes every window's STFT; here, because windows
 * start at multiples of the hop, the clip's STFT is computed ONCE ((N-1)*stride + T+1 frames) plus the two
 * zero-padded boundary frames of each window, and the core reads rows from both images -- bit-identical to the
 * per-window evaluation (KM_SEQ_PER_WINDOW=1 selects that for comparison).  This entry point may allocate (grow-only
 * clip-level buffers sized B*L) on first use, so capture it in a hipGraph only after a warm-up call of the same shape:
 * inside a stream capture a call that would have to grow them returns KM_ERR_WORKSPACE before it launches anything, as
 * km_forward_clip and km_train_step_clip do. */
int64_t km_sequence_num_outputs(km_handle h, int64_t L, int32_t stride_frames);
/* The temporal smoothing of a whole sequence, in place: x_dev (B, N, 52), y[0] = x[0], y[n] = alpha x[n] + (1 - alpha) y[n - 1]
 * along the frame axis with alpha = sigmoid(smoothing_alpha) -- what SequentialDualStreamModel.forward's per-position calls of
 * apply_temporal_smoothing add up to (src/model/sequential_dual_stream_model.py:99-151,
 * simplified_dual_stream_model.py:341-368).  It is the last step of km_sequence_forward(smooth = 1); exported so that a clip
 * whose output frames were computed in chunks on several GPUs (km_sequence_forward with smooth = 0 on each chunk, SURVEY.md
 * section 8e) is smoothed once, over the gathered frames. */
int km_ema_scan(km_handle h, float* x_dev, int64_t B, int64_t N, void* stream);
int km_sequence_forward(km_handle h, const float* audio_dev, int64_t B, int64_t L,
                        const float* emotion_dev, int32_t stride_frames, int32_t smooth,
                        float* out_dev, void* stream);
/* km_sequence_forward with a per-window emotion input taken from a TRACK per clip: track_dev (B, K, emotion_dim), e.g. the
 * emotion output of km_emotion_clip_build_batch.  It is km_sequence_forward in every respect (schedule, tiles, bit-identical
 * shared-frame and per-window paths, smoothing, growth rules) except where a window's emotion logit comes from.  Output frame i of
 * clip c ends, in clip coordinates, at e = min(clip_len, sample_offset + (i * stride_frames + T) * hop) and takes row
 * k = e < first_samples ? 0 : min((e - first_samples) / interval_samples, K - 1) of the clip's track.  With sample_offset = 0,
 * clip_len = L, first_samples = MIN and interval_samples = U of the emotion clip object this is km_emotion_clip_rows' mapping for
 * start frame i * stride_frames; sample_offset / clip_len let a chunk audio[:, s0 : s0 + L] of a clip of clip_len samples map as
 * the whole clip does (frames computed in chunks on several GPUs); first_samples = T * hop with interval_samples =
 * stride_frames * hop is the identity map, one row per window, for callers who bring their own per-window emotion.
 * The emotion branch runs ONCE per track row (B * K rows, not B * N windows: windows are 33 ms apart and rows 0.3 s), one small
 * kernel writes a logit per window from the closed form (no audio is read and no table comes from the host) and the core
 * launches read it.  KM_ERR_INVALID_ARG: K < 1, interval_samples < 1, negative first_samples or sample_offset,
 * clip_len < sample_offset + L, B * K beyond 2^31 - 1.  Two more grow-only buffers (B * K and B * N floats), allocated before the
 * first launch; the call neither synchronises nor reads back. */
int km_sequence_forward_track(km_handle h, const float* audio_dev, int64_t B, int64_t L,
                              const float* track_dev, int64_t K, int64_t first_samples, int64_t interval_samples,
                              int64_t sample_offset, int64_t clip_len, int32_t stride_frames, int32_t smooth,
                              float* out_dev, void* stream);

/* ---- attention maps and pre-weight outputs from the audio paths ------------------------------------------------------------
 * The reference treats the mel stream's attention map as an output of the model (DualStreamTrainer.train_step calls
 * model(audio, return_attention=True); SequentialTrainer logs outputs['mel_attention_weights'][0]).  These are km_forward_audio,
 * km_forward_clip and km_sequence_forward / km_sequence_forward_track with two more outputs, indexed like out_dev:
 *   raw_dev   (..., 52) or NULL        the sigmoid outputs before the stream weights and before any smoothing (km_core_forward)
 *   attn_dev  (..., 28, 80) or NULL    'mel_attention_weights', head-averaged as km_core_forward defines it
 * On handles of the fused shape out_dev and state_dev are bit-identical to the entry point without _attn (the ATTN instantiation
 * of the same fused core writes the map from the LDS image behind its O tile), and raw_dev / attn_dev are bit-identical across
 * the shared-frame and per-window schedules, any tile size, km_forward_audio_attn on the gathered windows and
 * km_forward_clip_attn on their start frames.  With the experimental split-bf16 core (core_split 3 / 6) a call that asks for
 * maps returns KM_ERR_UNSUPPORTED before it launches anything.  On generic shapes the GEMM-chain core writes both (the merged
 * d_model 512 launch is declined when a map is asked for, so bit equality with the plain call is not promised there).
 * km_sequence_forward_attn: exactly one of emotion_dev (B, emotion_dim) and track_dev (B, K, emotion_dim) is non-NULL; K ..
 * clip_len are km_sequence_forward_track's and are ignored with emotion_dev; the argument checks are that entry point's.
 * stats is NULL or an accumulator of km_attn_stats_create(28, 80): every tile's maps are added to it with one
 * km_attn_stats_update, in tile order.  With stats and attn_dev == NULL the maps never exist as a whole: they go to a grow-only
 * buffer of one tile (reserved windows x 28 x 80 floats) on the handle, allocated before the first launch and refused inside a
 * capture when it would have to grow, like the other sequence buffers. */
int km_forward_audio_attn(km_handle h, const float* audio_dev, int64_t B, int64_t L,
                          const float* emotion_dev, float* out_dev, float* state_dev, int32_t first,
                          float* raw_dev, float* attn_dev, void* stream);
int km_forward_clip_attn(km_handle h, const float* clip_dev, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                         int32_t min_start_frame, int32_t max_start_frame, const float* emotion_dev,
                         float* out_dev, float* state_dev, int32_t first, float* raw_dev, float* attn_dev, void* stream);
int km_sequence_forward_attn(km_handle h, const float* audio_dev, int64_t B, int64_t L,
                             const float* emotion_dev, const float* track_dev, int64_t K, int64_t first_samples,
                             int64_t interval_samples, int64_t sample_offset, int64_t clip_len, int32_t stride_frames,
                             int32_t smooth, float* out_dev, float* raw_dev, float* attn_dev, void* stats, void* stream);

/* ---- training step (data-parallel ready) -------------------------------------------------------------
 * Replaces the body of SequentialTrainer.train_epoch (src/train_sequential.py:158-181: forward, loss,
 * backward, clip_grad_norm_(1.0), AdamW.step) for the 28 tensors of DualStreamCrossAttention + smoothing_alpha.
 * Parameters, AdamW moments and gradients are FLAT fp32 vectors in state-dict order (km_train_param_offset);
 * the gradient bucket is caller-owned so that the data-parallel build can all-reduce it over RCCL between
 * km_train_step* and km_train_adamw.  Eval-mode arithmetic (dropout = 0); loss = mse_weight * MSE +
 * l1_weight * L1 of the (optionally EMA-smoothed) prediction against target (src/model/losses.py:112-121).
 *   km_train_init        allocate the training state for up to max_windows windows per step and upload the
 *                        currently loaded parameters (allocates; call after km_finalize)
 *   km_train_step        mel_dev (B,T_in,80), mel_short_dev (B,3,80), emotion_dev (B,ED), target_dev (B,52) ->
 *                        flat_grad_dev (n_params), loss_dev (1), out_dev (B,52) or NULL; ema_state_dev (B,52) or
 *                        NULL applies the model's temporal smoothing inside the forward as the reference does
 *   km_train_step_audio  same from audio_dev (B, L): runs the log-mel front end first (no gradient flows into
 *                        it in the reference either: NumPy round trip, simplified_dual_stream_model.py:184-229)
 *   km_train_step_clip   same for B windows of ONE clip resident in HBM: window b is samples [start_frames[b] * hop,
 *                        + T * hop) of clip_dev (clip_len samples, zero beyond), exactly what km_gather_windows would have
 *                        copied; the start frames may come in any order and may repeat.  Replaces the per-window slicing
 *                        (src/data/sequential_dataset.py:156-209) + the per-window log-mel
 *                        (src/model/simplified_dual_stream_model.py:184-229) under the step (src/train_sequential.py:158)
 *                        without materialising the (B, T * hop) windows: the STFT frames the windows share are computed
 *                        once -- max - min + T + 1 clip frames + 2 zero-padded boundary frames per window instead of
 *                        B * (T + 1) -- and everything behind the front end is km_train_step_audio's program, so loss,
 *                        out and flat_grad are bit-identical to km_gather_windows + km_train_step_audio.
 *                        min_start_frame / max_start_frame are HOST copies of the extremes of start_frames_dev (they size
 *                        the launches; nothing is read back from the device, so the step can be captured into a hipGraph).
 *                        A span wider than any earlier call's (km_train_init allocates max_windows + T + 1 frames) grows a
 *                        buffer: capture only after a warm-up call with that span.  Needs km_reserve(B, T * hop) like the
 *                        from-audio step.
 *   km_train_clip_supported   1 when km_train_step_clip runs on this handle (after km_train_init), else 0: the 1024-point
 *                        front end (not mel_two_frame) that writes the packed encoder input (where km_train_step_audio
 *                        packs in the front-end launch), pad_mode constant, and hop_length >= n_fft / 2 -- only then are
 *                        frames 0 and T the only frames of a window that see its zero padding (hop 533: frame 1 spans
 *                        samples 21 .. 1044; at the 60 fps shape, hop 266, frames 1 and T - 1 reach into it too).
 *                        km_train_step_clip on an unsupported handle returns KM_ERR_UNSUPPORTED, never another result.
 *                        Option "clip_assemble" adds the handles of km_clip_plan route 2 (any hop with T + 1 >= 2 E).
 *   km_train_adamw       grad-norm clipping (max_grad_norm <= 0 disables) + AdamW on the flat vectors; `step`
 *                        is the 1-based optimizer step for the bias correction
 *   km_train_get_params / km_train_set_params   flat master copy <-> host
 *   km_train_sync        make the inference kernels see the trained weights (device master -> host store ->
 *                        fold + pack + upload) */
int km_train_init(km_handle h, int64_t max_windows, void* stream);
int64_t km_train_num_params(km_handle h);
int64_t km_train_param_offset(km_handle h, const char* key);
int km_train_step(km_handle h, const float* mel_dev, int64_t B, int64_t T_in, const float* mel_short_dev,
                  const float* emotion_dev, const float* target_dev, float mse_weight, float l1_weight,
                  float* flat_grad_dev, float* loss_dev, float* out_dev, float* ema_state_dev, int32_t ema_first,
                  void* stream);
int km_train_step_audio(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* emotion_dev,
                        const float* target_dev, float mse_weight, float l1_weight, float* flat_grad_dev,
                        float* loss_dev, float* out_dev, float* ema_state_dev, int32_t ema_first, void* stream);
int km_train_clip_supported(km_handle h);
int km_train_step_clip(km_handle h, const float* clip_dev, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                       int32_t min_start_frame, int32_t max_start_frame, const float* emotion_dev, const float* target_dev,
                       float mse_weight, float l1_weight, float* flat_grad_dev, float* loss_dev, float* out_dev,
                       float* ema_state_dev, int32_t ema_first, void* stream);
int km_train_adamw(km_handle h, const float* flat_grad_dev, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float max_grad_norm, int64_t step, void* stream);
int km_train_get_params(km_handle h, float* flat_host, int64_t n);
int km_train_set_params(km_handle h, const float* flat_host, int64_t n);
int km_train_sync(km_handle h, void* stream);
/* AdamW state for checkpoints (the optimizer_state_dict of src/train_sequential.py:303-339): first and second moments as
 * flat vectors laid out like the parameters, and the two device-side step counters (all parameters, smoothing_alpha).
 * Both calls synchronise the device. */
int km_train_get_optimizer_state(km_handle h, float* exp_avg_host, float* exp_avg_sq_host, int64_t n, int32_t* steps2_host);
int km_train_set_optimizer_state(km_handle h, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t n,
                                 const int32_t* steps2_host);

/* The remaining terms of KoeMorphLoss (src/model/losses.py:29-178), ADDED to the mse/l1 terms of km_train_step*:
 *   perceptual  four group-weighted MSEs: mouth cols 12..31 x2.0, eye 0..11 x1.0, brow 32..43 x1.0, jaw 44..51 x1.5
 *               (losses.py:306-338; the optional audio-visual term needs audio_features and is not computed, as when
 *               the reference is called with audio_features=None)
 *   temporal    MSE of (pred - prev_pred) vs (target - prev_target)           (losses.py:185-200)
 *   velocity    L1 of the same differences                                    (losses.py:202-217)
 *   sparsity    mean |pred|                                                   (losses.py:219-224)
 *   smoothness  mean |pred[:, j+1] - pred[:, j]| over the 51 adjacent pairs    (losses.py:226-234)
 *   landmark    MSE of pred W^T vs target W^T, W = the loss module's fixed (136, 52) matrix (losses.py:380-412)
 * prev_pred_dev / prev_target_dev (B,52) are constants (no gradient); temporal and velocity are skipped when either
 * is NULL, landmark when landmark_w_dev is NULL -- as the reference skips them.  Pointers must stay valid for every
 * later km_train_step* call (they are read on the step's stream).  cfg = NULL switches the extra terms off. */
typedef struct km_loss_config {
    int32_t abi_version;             /* KM_ABI_VERSION: km_train_set_loss refuses anything else (the struct has grown) */
    float perceptual_weight, temporal_weight, sparsity_weight, smoothness_weight, landmark_weight, velocity_weight;
    const float* prev_pred_dev;
    const float* prev_target_dev;
    const float* landmark_w_dev;
    const float* audio_energy_dev;   /* (B) per-window audio energy (km_audio_energy) or NULL: adds the audio-visual term
                                        0.5 * (1 - cos(mean mouth activation, audio energy)) to the perceptual loss
                                        (PerceptualBlendshapeLoss.forward with audio_features, losses.py:340-378) */
    /* DualStreamLoss (src/train_dual_stream.py:434-516).  Its L1 / L2 terms are l1_weight / mse_weight of km_train_step*
     * (defaults there 1.0 / 0.1); the two others:
     *   ds_velocity    weight x MSE(pred - prev_predictions, target - prev_predictions)   (:489-495), prev_predictions =
     *                  ds_prev_pred_dev (B, 52), a constant (no gradient); skipped when NULL, as the reference skips it
     *   ds_separation  weight x mean over the batch of | mean(pred[:, MOUTH]) - mean(pred[:, EXPRESSION]) |  (:498-514;
     *                  index sets of src/model/dual_stream_attention.py:14-45).  The reference computes it only when both
     *                  attention maps are passed in; here weight > 0 switches it on */
    float ds_velocity_weight, ds_separation_weight;
    const float* ds_prev_pred_dev;
} km_loss_config;
int km_train_set_loss(km_handle h, const km_loss_config* cfg);
/* (B, T, D) or (B, 1, D) audio features -> (B) energies for km_loss_config.audio_energy_dev: mean over T of the L2 norm
 * over D, as PerceptualBlendshapeLoss._compute_audiovisual_loss reduces its audio_features (losses.py:352-358). */
int km_audio_energy(const float* features_dev, int64_t B, int64_t T, int64_t D, float* energy_dev, void* stream);

/* Training-mode dropout: the reference trains under model.train() (src/train_sequential.py:118) with dropout p = 0.1 on
 * the attention weights of both nn.MultiheadAttention modules and on the decoder's hidden layer
 * (src/model/dual_stream_attention.py:106, :115, :153).  p = 0 (the state after km_train_init) is eval-mode arithmetic.
 *   km_train_set_dropout        p in [0, 1); masks are drawn per step by a counter-based Philox4x32-10 generator keyed by
 *                               `seed` and a device-side step counter (a captured step draws fresh masks on every replay);
 *                               external_masks != 0: the step uses the masks last given to km_train_set_dropout_masks
 *                               (parity tests replay the masks of reference-generated fixtures)
 *   km_train_get_dropout_masks  keep flags (1 = kept) of the most recent step, for B windows: mel (B, H, 28, n_mels),
 *                               emo (B, H, 24), dec (B, 52, d_model / 2) bytes on the host -- the layout of
 *                               oracle.core.core_forward(drop_masks=...)
 *   km_train_set_dropout_masks  the reverse (host -> device) */
int km_train_set_dropout(km_handle h, float p, uint64_t seed, int32_t external_masks);
/* The device-side step counter of the mask generator (part of a training checkpoint: a resumed run draws the masks the
 * uninterrupted run would have drawn). */
int km_train_get_dropout_step(km_handle h, int64_t* step);
int km_train_set_dropout_step(km_handle h, int64_t step);

/* Overlapping the data-parallel gradient all-reduce with the end of the backward pass (new construction: the reference is
 * single-process).  The flat bucket is laid out so that the tensors the backward pass finishes last come last:
 *   km_train_grad_split   *early_floats = E: floats [0, E) of flat_grad (83 % at d_model 256) are final after phase P11 of
 *                         km_train_step*'s program (the last but one or two of its launches), the rest when the call's work completes
 *   km_train_wait_early   make `stream` wait (hipStreamWaitEvent) for that point of the most recent km_train_step*: a
 *                         side stream can then all-reduce flat_grad[0:E] while the launch stream still computes the tail */
int km_train_grad_split(km_handle h, int64_t* early_floats);
int km_train_wait_early(km_handle h, void* stream);
int km_train_get_dropout_masks(km_handle h, int64_t B, uint8_t* mel_host, uint8_t* emo_host, uint8_t* dec_host, void* stream);
int km_train_set_dropout_masks(km_handle h, int64_t B, const uint8_t* mel_host, const uint8_t* emo_host, const uint8_t* dec_host,
                               void* stream);

/* ---- legacy single-stream variant --------------------------------------------------------------------
 * SimplifiedKoeMorphModel (src/model/simplified_model.py:12-156), used by the reference's src/train.py,
 * scripts/rt_simplified.py and scripts/test_model.py: same librosa-style log-mel front end, a two-layer
 * per-frame audio encoder, ONE nn.MultiheadAttention with 52 learnable blendshape queries over the T_mel
 * encoded frames (the literal "52 x 256" attention of the north star), a 3-layer decoder + sigmoid per query
 * row and a mean over the 52 rows.  State-dict keys: audio_encoder.{0,3}.*, attention.*, decoder.{0,3,6}.*,
 * blendshape_queries.  The handle is used with km_load_param / km_finalize / km_reserve / km_destroy as usual.
 *   km_legacy_forward      audio_dev (B, L)            -> out_dev (B, 52)   (forward, :114-149)
 *   km_legacy_forward_mel  mel_dev (B, T_mel, 80)      -> out_dev (B, 52)   (everything after extract_mel_features) */
typedef struct km_legacy_config {
    int32_t abi_version;       /* KM_ABI_VERSION */
    int32_t d_model;           /* 256 */
    int32_t num_heads;         /* 8 */
    int32_t decoder_hidden;    /* 128 */
    int32_t num_blendshapes;   /* 52 */
    km_mel_config mel;
} km_legacy_config;
int km_legacy_create(const km_legacy_config* cfg, km_handle* out);
int km_legacy_forward(km_handle h, const float* audio_dev, int64_t B, int64_t L, float* out_dev, void* stream);
int km_legacy_forward_mel(km_handle h, const float* mel_dev, int64_t B, int64_t T_mel, float* out_dev, void* stream);

/* ---- training step of the legacy single-stream variant -------------------------------------------------------
 * What the reference's main trainer does to SimplifiedKoeMorphModel (src/train.py:82-96 builds it, :165-249 is the loop): the
 * model under .train() (src/model/simplified_model.py:44-72, :114-149), KoeMorphLoss (src/model/losses.py:89-178), backward,
 * clip_grad_norm_ and AdamW.  Default width only: d_model 256, 8 heads, decoder hidden 128, 52 blendshapes, 80 mel bins, any
 * number of frames; km_legacy_train_init on any other legacy handle returns KM_ERR_UNSUPPORTED, never another result.  The
 * km_train_* family keeps refusing legacy handles, this one refuses dual-stream handles.  Parameters, AdamW moments and the
 * gradient are FLAT fp32 vectors in state-dict order with 16-byte-aligned offsets, the gradient caller-owned.
 *   km_legacy_train_init         allocate the training state and the step's workspace for up to max_windows windows of up to
 *                                max_frames mel frames and upload the loaded parameters (allocates; call after km_finalize)
 *   km_legacy_train_num_params / km_legacy_train_param_offset   size of the flat vectors / offset of a state-dict key (-1: unknown)
 *   km_legacy_train_step_mel     mel_dev (B, T, 80), target_dev (B, 52) -> flat_grad_dev (all of it is written, nothing is
 *                                accumulated), loss_dev (1), out_dev (B, 52) or NULL: forward (simplified_model.py:129-147), loss =
 *                                mse_weight * MSE + l1_weight * L1 (losses.py:112-121) + the terms of km_legacy_train_set_loss,
 *                                backward (train.py:190-193).  Two calls with the same inputs and dropout step give the same bits;
 *                                no allocation, so the call can be captured into a hipGraph after one eager call
 *   km_legacy_train_step_audio   the same from audio_dev (B, L): km_mel_batch's front end (extract_mel_features, :79-112; no
 *                                gradient flows into it: a NumPy round trip in the reference), then the step from mel -- bit-identical
 *                                to km_mel_batch followed by km_legacy_train_step_mel.  Needs km_reserve(B, L)
 *   km_legacy_train_set_loss     the remaining KoeMorphLoss terms as km_train_set_loss takes them (perceptual, temporal, velocity,
 *                                sparsity, smoothness, landmark); the audio-visual and ds_* terms are KM_ERR_UNSUPPORTED here
 *   km_legacy_train_adamw        clip_grad_norm_ + AdamW.step (train.py:195-203); contract and implementation of km_train_adamw
 *   km_legacy_train_get_params / _set_params / _get_optimizer_state / _set_optimizer_state   as their km_train_* twins
 *                                (checkpoints, train.py:262-283)
 *   km_legacy_train_sync         km_legacy_forward* and the state dict (km_get_param) see the trained weights, as km_train_sync
 *   km_legacy_train_set_dropout  training-mode dropout of the five sites of the model (simplified_model.py:44-72): p in [0, 1),
 *                                masks drawn per step by the Philox4x32-10 generator of km_train_set_dropout, or given by the
 *                                caller (external_masks != 0); p = 0 (the state after init) is eval-mode arithmetic
 *   km_legacy_train_get_dropout_masks / _set_dropout_masks   keep flags (1 = kept) of a (B, T) step as bytes on the host:
 *                                enc1 (B, T, 256), enc2 (B, T, 256) behind the encoder's two ReLUs, attn (B, 8, 52, T) on the
 *                                softmaxed attention weights (as nn.MultiheadAttention applies its dropout), dec1 (B, 52, 128),
 *                                dec2 (B, 52, 128) behind the decoder's two ReLUs
 *   km_legacy_train_get_dropout_step / _set_dropout_step   the generator's device-side step counter (advanced by every step) */
int km_legacy_train_init(km_handle h, int64_t max_windows, int64_t max_frames, void* stream);
int64_t km_legacy_train_num_params(km_handle h);
int64_t km_legacy_train_param_offset(km_handle h, const char* key);
int km_legacy_train_step_mel(km_handle h, const float* mel_dev, int64_t B, int64_t T, const float* target_dev, float mse_weight,
                             float l1_weight, float* flat_grad_dev, float* loss_dev, float* out_dev, void* stream);
int km_legacy_train_step_audio(km_handle h, const float* audio_dev, int64_t B, int64_t L, const float* target_dev, float mse_weight,
                               float l1_weight, float* flat_grad_dev, float* loss_dev, float* out_dev, void* stream);
int km_legacy_train_set_loss(km_handle h, const km_loss_config* cfg);
int km_legacy_train_adamw(km_handle h, const float* flat_grad_dev, float lr, float beta1, float beta2, float eps,
                          float weight_decay, float max_grad_norm, int64_t step, void* stream);
int km_legacy_train_get_params(km_handle h, float* flat_host, int64_t n);
int km_legacy_train_set_params(km_handle h, const float* flat_host, int64_t n);
int km_legacy_train_get_optimizer_state(km_handle h, float* exp_avg_host, float* exp_avg_sq_host, int64_t n, int32_t* steps2_host);
int km_legacy_train_set_optimizer_state(km_handle h, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t n,
                                        const int32_t* steps2_host);
int km_legacy_train_sync(km_handle h, void* stream);
int km_legacy_train_set_dropout(km_handle h, float p, uint64_t seed, int32_t external_masks);
int km_legacy_train_get_dropout_step(km_handle h, int64_t* step);
int km_legacy_train_set_dropout_step(km_handle h, int64_t step);
int km_legacy_train_get_dropout_masks(km_handle h, int64_t B, int64_t T, uint8_t* enc1_host, uint8_t* enc2_host, uint8_t* attn_host,
                                      uint8_t* dec1_host, uint8_t* dec2_host, void* stream);
int km_legacy_train_set_dropout_masks(km_handle h, int64_t B, int64_t T, const uint8_t* enc1_host, const uint8_t* enc2_host,
                                      const uint8_t* attn_host, const uint8_t* dec1_host, const uint8_t* dec2_host, void* stream);

/* ---- legacy multi-layer model: KoeMorphModel (src/model/gaussian_face.py:29-268) -----------------------
 * The model behind create_koemorph_model / scripts/rt.py:283-304, eval mode: DualStreamEncoder on both feature streams
 * (Linear + ReLU + LayerNorm, then num_encoder_layers post-norm nn.TransformerEncoderLayer with 8 heads, 4 d feed-forward,
 * exact GELU; src/model/dual_stream_attention.py:296-390), their average, BlendshapeQueryEmbedding conditioned on the
 * previous frame (src/model/attention.py:481-514), num_attention_layers x [MultiHeadCrossAttention with the causal and
 * window masks of attention.py:208-246, residual, LayerNorm], BlendshapeDecoder (diagonal of output_proj, sigmoid,
 * 0.9 / 0.1 mix with the previous frame; src/model/decoder.py:108-177), learnable TemporalSmoother (exponential,
 * gaussian or median: decoder.py:278-340) and BlendshapeConstraints (decoder.py:434-466).  d_query must equal d_model (the reference's
 * residual `attn_out + attention_output` needs it; its default d_query = 128 does not run).  State-dict keys are the
 * reference's; the buffers of the smoother / constraints are NOT parameters here: the smoother state is the caller's
 * (B, 52) device array (zero it for reset_temporal_state).  A query row whose keys are all masked yields NaN, as in
 * the reference.
 *   km_koemorph_reserve  workspace for max_batch x max_frames
 *   km_koemorph_forward  mel_dev (B, T, mel_dim), emotion_dev (B, T, emotion_dim), audio_mask_dev (B, T) bytes, 1 = valid
 *                        frame, or NULL (padded frames are masked as keys in the encoder and in every cross-attention
 *                        layer, gaussian_face.py:180,204,224; what the encoder leaves AT padded positions is unspecified,
 *                        as in torch, and never reaches the output), prev_dev (B, 52) or NULL,
 *                        smoother_state_dev (B, 52) in/out or NULL (= apply_smoothing False), apply_constraints,
 *                        -> out_dev (B, 52), raw_dev (B, 52) or NULL, attn_dev (layers, B, H, 52, T) or NULL */
typedef struct km_koemorph_config {
    int32_t abi_version;            /* KM_ABI_VERSION */
    int32_t mel_dim;                /* 80 */
    int32_t emotion_dim;            /* 256 */
    int32_t d_model;                /* 256, a multiple of 8 and of num_heads */
    int32_t num_heads;              /* 8 */
    int32_t num_encoder_layers;     /* 2 */
    int32_t num_attention_layers;   /* 4 */
    int32_t decoder_hidden_dim;     /* 128 */
    int32_t decoder_layers;         /* 2 */
    int32_t decoder_activation;     /* 0 relu, 1 gelu (default), 2 swish = nn.SiLU, 3 leaky_relu(0.1)  (decoder.py:68-75) */
    int32_t causal;                 /* 1 */
    int32_t window_size;            /* 30; < 0 = None */
    int32_t use_temporal_smoothing; /* 1: temporal_smoother.alpha is a parameter */
    int32_t use_constraints;        /* 1 */
    int32_t num_blendshapes;        /* 52 */
    int32_t output_activation;      /* 0 sigmoid (default), 1 tanh, 2 none  (decoder.py:162-167) */
    int32_t smoothing_method;       /* TemporalSmoother (decoder.py:179-340), learnable=True as KoeMorphModel builds it:
                                       0 exponential: parameter temporal_smoother.alpha, state (B, 52);
                                       1 gaussian: parameter temporal_smoother.gaussian_weights (window), y = sum_k softmax(w)_k *
                                         ring[k] over the SLOTS of the history ring (:299-317: the weights go with the slot, not
                                         with the age of its content);
                                       2 median: torch.median over the ring's slots (:319-331; the lower middle value for an
                                         even window, NaN if a slot holds NaN).
                                       1 and 2 keep smoother_state_dev as (B, smoothing_window * 52 + 1) floats per call: each
                                       batch element's ring (window, 52) followed by its slot pointer; all zero = reset */
    int32_t smoothing_window;       /* 5 (TemporalSmoother's default; KoeMorphModel never passes another), 1..16 */
} km_koemorph_config;
int km_koemorph_create(const km_koemorph_config* cfg, km_handle* out);
int km_koemorph_reserve(km_handle h, int64_t max_batch, int64_t max_frames);
int km_koemorph_forward(km_handle h, const float* mel_dev, const float* emotion_dev, int64_t B, int64_t T,
                        const uint8_t* audio_mask_dev, const float* prev_dev, float* smoother_state_dev,
                        int32_t apply_constraints, float* out_dev, float* raw_dev, float* attn_dev, void* stream);

/* ---- KoeMorphModel: autoregressive rollout of whole clips on the device ---------------------------------
 * The model is autoregressive: frame i's output is frame i + 1's prev_blendshapes, and the smoother carries state.  One call renders
 * frames first_frame .. F - 1 of B clips from their per-frame rows mel_dev (B, F, mel_dim) and emotion_dev (B, F, emotion_dim)
 * (same F for every clip).  THE LAW: for i = first_frame .. F - 1 in order, T_i = min(i + 1, T), row i - first_frame of out_dev /
 * raw_dev (B, F - first_frame, 52) is km_koemorph_forward on the dense window of rows i - T_i + 1 .. i of every clip, B, T_i, no
 * audio mask, prev = the previous rendered frame's out (prev0_dev (B, 52) for i == first_frame; NULL: that one frame runs without
 * conditioning), smoother_state_dev (km_koemorph_forward's layouts; NULL = no smoothing) updated by every frame in turn and
 * left as the loop leaves it.  A clip's first T - 1 frames see SHORTER windows, not padded ones (the causal mask lets query q
 * see keys 0 .. q: a left-padded window would leave query 0 without a key).  first_frame > 0 continues a stream: pass the last
 * T - 1 rows already rendered as context, the previous call's last out as prev0_dev and the state; two calls give the bits of one.
 *   km_koemorph_rollout_reserve  workspace (a buffer group of its own; km_koemorph_forward's workspace grows to max_clips x
 *                        max_context as well) for calls of up to max_clips clips and T <= max_context, and the chunk length of
 *                        route 1.  Grow-only; it allocates, so not inside a stream capture
 *   km_koemorph_rollout  route 1 (the width of the fused kernels, T <= 32, option "kmm_no_fuse" off, 16-byte aligned row pointers):
 *                        frames with a short window (i < T - 1) as four launches each (window gather, encoder, decode, row scatter);
 *                        the others in chunks of chunk_frames as three launches per chunk: a gather of the chunk's B x frames
 *                        overlapping windows into a dense staging buffer, ONE encoder launch over all of them, ONE
 *                        kmmf_rollout_kernel launch (a workgroup per clip walks the serial chain with prev and the state in LDS).
 *                        Route 0 (any other width, T > 32, emotion_dim % 16 != 0, "kmm_no_fuse", misaligned rows): per frame a
 *                        window gather, the launches of km_koemorph_forward and a row scatter.  Launches on `stream` only: capturable.
 *                        KM_ERR_INVALID_ARG (the text names the entry point and the value): NULL mel_dev / emotion_dev / out_dev,
 *                        B, F or T < 1, first_frame outside 0 .. F - 1, a handle of another kind; KM_ERR_WORKSPACE: not reserved,
 *                        or reserved for fewer clips or a shorter context
 *   km_koemorph_rollout_plan  host only (after km_finalize_host), the function the call itself runs: out[0] route, out[1] chunks
 *                        (route 1), out[2] rendered frames with a short window, out[3] launches of the call (route 0 on the chain:
 *                        counted with prev0 given; without it the first frame makes two fewer), out[4] workspace floats of the
 *                        rollout group.  With the reserved chunk_frames, or 256 before any reserve; row pointers taken as aligned */
int km_koemorph_rollout_reserve(km_handle h, int64_t max_clips, int64_t max_context, int64_t chunk_frames);
int km_koemorph_rollout(km_handle h, const float* mel_dev, const float* emotion_dev, int64_t B, int64_t F, int64_t T, int64_t first_frame,
                        const float* prev0_dev, float* smoother_state_dev, int32_t apply_constraints, float* out_dev, float* raw_dev,
                        void* stream);
int km_koemorph_rollout_plan(km_handle h, int64_t B, int64_t F, int64_t T, int64_t first_frame, int64_t out[5]);

/* ---- KoeMorphModel: live streams with their last rows resident on the device -----------------------------
 * n_streams independent streams, out of phase.  THE LAW: stream s has a frame counter c_s, 0 after creation and after a reset of
 * that stream.  A step that gives it n_s new rows (0 <= n_s <= max_rows) renders n_s frames, in order; frame i = c_s + j is
 * km_koemorph_forward at B = 1 on the dense window of the stream's rows i - T_i + 1 .. i, T_i = min(i + 1, context_frames), no audio
 * mask, prev = the stream's previous rendered frame (frame 0 has none and runs unconditioned), the stream's OWN smoother state
 * (zeros after a reset, km_koemorph_forward's layouts for B = 1) updated by every frame.  Short windows are shorter windows, never
 * padded ones (the rollout's law).  Streams share nothing; a stream with n_s = 0 keeps ring, counter, previous frame and state, and
 * its rows of out_dev / raw_dev are not written.  The results are those of the per-stream km_koemorph_forward loop, bit for bit.
 * Served: the width of the fused kernels (d_model 256, 8 heads, 52 blendshapes, decoder width 128, mel_dim and emotion_dim multiples
 * of 16, at least one attention layer), context_frames <= 32, smoothing window <= 16, option "kmm_no_fuse" off (rollout route 1);
 * anything else is KM_ERR_UNSUPPORTED at creation, the text naming the entry point and the value.
 *   km_koemorph_stream_plan    host only (after km_finalize_host), the function create itself uses: out[0] 1 supported / 0 not (the
 *                        reason is km_last_error's text; the other values are 0), out[1] ring rows per stream = context_frames - 1 +
 *                        max_rows, out[2] launches per step (4), out[3] device memory of the engine in 4-byte units, out[4] LDS
 *                        bytes of the chain kernel, out[5] smoother-state floats per stream
 *   km_koemorph_stream_create  a buffer group of its own (rings, counters, previous frames, states, window table, encodings).
 *                        Allocates and synchronises the device: call it outside any stream capture.  A second create replaces the
 *                        first; km_destroy frees the group.  apply_smoothing / apply_constraints: km_koemorph_forward's switches
 *   km_koemorph_stream_step    mel_dev (n_streams, max_rows, mel_dim), emotion_dev (n_streams, max_rows, emotion_dim), both 16-byte
 *                        aligned; counts_dev (n_streams) int32 or NULL = max_rows for every stream, each clamped to 0 .. max_rows:
 *                        stream s brings rows 0 .. n_s - 1 of its block.  out_dev / raw_dev (or NULL) (n_streams, max_rows, 52): row
 *                        (s, j) = frame c_s + j for j < n_s, the others untouched; rendered_dev (n_streams) int32 or NULL receives
 *                        n_s.  FOUR launches on `stream` whatever the sizes and phases (row advance + window table, the encoder for
 *                        windows of <= 16 and of 17 .. 32 rows, the per-stream chains); no allocation, synchronisation or readback:
 *                        capturable
 *   km_koemorph_stream_reset   one launch: the streams with mask_dev[s] != 0 (NULL: all) become freshly created ones
 *   km_koemorph_stream_destroy frees the group and leaves the handle as it was before create (km_destroy does the same on its way)
 *   km_koemorph_stream_frames  frames_dev (n_streams) int64 <- the counters
 *   km_koemorph_stream_state   state_dev (n_streams, out[5]) and / or prev_dev (n_streams, 52), either may be NULL <- the smoother
 *                        states and the last rendered frames
 * KM_ERR_INVALID_ARG: NULL handle, a handle of another kind, n_streams / context_frames / max_rows < 1, no engine created, NULL or
 * misaligned row pointers. */
int km_koemorph_stream_plan(km_handle h, int64_t n_streams, int64_t context_frames, int64_t max_rows, int64_t out[6]);
int km_koemorph_stream_create(km_handle h, int64_t n_streams, int64_t context_frames, int64_t max_rows, int32_t apply_smoothing,
                              int32_t apply_constraints);
int km_koemorph_stream_step(km_handle h, const float* mel_dev, const float* emotion_dev, const int32_t* counts_dev, float* out_dev,
                            float* raw_dev, int32_t* rendered_dev, void* stream);
int km_koemorph_stream_reset(km_handle h, const uint8_t* mask_dev, void* stream);
int km_koemorph_stream_destroy(km_handle h);
int km_koemorph_stream_frames(km_handle h, int64_t* frames_dev, void* stream);
int km_koemorph_stream_state(km_handle h, float* state_dev, float* prev_dev, void* stream);

/* ---- KoeMorphModel: the rows of the streams from pushed audio -------------------------------------------
 * The audio front of the engine above: 16 kHz samples are pushed per stream and the mel and emotion rows km_koemorph_stream_step takes
 * come out with their per-stream counts; samples, counters and rows stay on the device.  THE LAW.
 *   Clock     hop = int(16000 / fps) (float64).  Stream s has received n_s samples since creation or its last reset; frame k is due as
 *             soon as n_s >= (k + 1) * hop.  After a push the stream has K = n_s / hop frames; the push renders frames c_s .. K - 1, in
 *             order (c_s: the count before it).  Integer arithmetic: the two tracks never drift apart or behind the audio.  Supported:
 *             hop >= 257 and fps >= 10 (30 fps: 533, 60 fps: 266); anything else is KM_ERR_UNSUPPORTED at creation.  max_rows =
 *             max_samples / hop + 1 bounds the frames of a push.
 *   Mel row k the row of the STFT frame centred on sample k * hop of the stream, in the configuration of MelSpectrogramExtractor
 *             (16000 Hz, 512 points, mel_dim HTK filters 80 .. 8000 Hz, "window" normalisation, log(mel + 1e-8)), reflected at the
 *             stream's first sample only: with hop >= 257 every frame has its 512 samples when it is due.  A function of the stream's
 *             samples alone -- not of the pushes they came in, of the other streams or of where the ring wraps.
 *   Emotion row k  a push that leaves stream s with new frames sets the window: a0 = the smallest multiple of 160 >= n_s - W (0 while
 *             n_s <= W, W = int(emotion_window_s * 16000)), len = n_s - a0, m = a0 / 160, nf = (len - 960) / 160 + 1 (0 for len < 960).
 *             The window's descriptors are the rows of km_egemaps_llds(samples a0 .. n_s - 1, normalize 1, fps 0).  Row k sits at
 *             p = (double)(k * hop) / 160.0, j = floor(p) - m, w = p - floor(p): frame 0 for j < 0 (creation rules it out), the last
 *             frame for j >= nf - 1, frame j for w == 0, otherwise fmaf((float)w, b - a, a) between frames j and j + 1, with
 *             km_egemaps_llds's exception for columns 10-24.  The row is emotion_dim wide, the descriptors first, zeros to the right;
 *             a window without a frame gives a row of zeros.  Emotion rows depend on the push schedule: the window ends where the push ends.
 *   km_koemorph_audio_plan      host only, the function create itself uses: out[0] 1 supported / 0 not (the reason is km_last_error's
 *                        text; the other values are 0), out[1] hop, out[2] max_rows, out[3] ring samples per stream (W + max_samples),
 *                        out[4] W, out[5] frames of a full window, out[6] launches of a push (7), out[7] bytes of the engine's
 *                        state on the device (rings, counters, tables, frame records; the two constant plans come on top)
 *   km_koemorph_audio_schedule  host only, the arithmetic of the advance kernel for one stream: samples before, samples pushed, the life's
 *                        origin in the ring -> out[0]
 *                        first new frame, out[1] new frames, out[2] a0, out[3] len, out[4] nf, out[5] m, out[6] samples after, out[7..9]
 *                        the window's slot for the ragged eGeMAPS kernels: stream (-1: nothing to compute), ring index of a0, nf
 *   km_koemorph_audio_create    a buffer group of its own on the handle, with a mel plan and an eGeMAPS plan.  Allocates and synchronises:
 *                        outside any stream capture.  A second create replaces the first; km_destroy frees the group.  Checks, each
 *                        refusal naming the entry point and the value: n_streams >= 1, a known feature set, W >= max_samples + hop +
 *                        1120 (KM_ERR_INVALID_ARG); a window of at most 2048 frames, emotion_dim at least the descriptor count
 *                        (KM_ERR_UNSUPPORTED)
 *   km_koemorph_audio_rows      samples_dev (n_streams, M), 1 <= M <= max_samples; counts_dev (n_streams) int32 or NULL = M, clamped to
 *                        0 .. M -> mel_rows_dev (n_streams, max_rows, mel_dim), emotion_rows_dev (n_streams, max_rows, emotion_dim),
 *                        row_counts_dev (n_streams) int32: row (s, j) is frame c_s + j for j < row_counts[s], the others untouched.
 *                        SEVEN launches on `stream`, one linear chain (advance, mel rows, the four record kernels of the ragged
 *                        eGeMAPS chain, descriptor rows); no allocation, synchronisation or readback: capturable, also in front of
 *                        km_koemorph_stream_step on the same three buffers
 *   km_koemorph_audio_reset     one launch: the streams with mask_dev[s] != 0 (NULL: all) start again at sample 0; the ring's write position
 *                        stays where it stands and becomes the new life's origin (sample i of a life at (origin + i) mod ring)
 *   km_koemorph_audio_samples   totals_dev (n_streams) int64 <- n_s
 *   km_koemorph_audio_destroy   frees the group (km_destroy does the same on its way) */
int km_koemorph_audio_plan(km_handle h, int64_t n_streams, double fps, double emotion_window_s, int64_t max_samples, int32_t feature_set,
                           int64_t out[8]);
int km_koemorph_audio_schedule(int64_t samples_before, int64_t pushed, int32_t hop, int64_t window_samples, int64_t ring_len, int64_t origin,
                               int32_t stream, int64_t out[10]);
int km_koemorph_audio_create(km_handle h, int64_t n_streams, double fps, double emotion_window_s, int64_t max_samples, int32_t feature_set);
int km_koemorph_audio_rows(km_handle h, const float* samples_dev, int64_t M, const int32_t* counts_dev, float* mel_rows_dev,
                           float* emotion_rows_dev, int32_t* row_counts_dev, void* stream);
int km_koemorph_audio_reset(km_handle h, const uint8_t* mask_dev, void* stream);
int km_koemorph_audio_samples(km_handle h, int64_t* totals_dev, void* stream);
int km_koemorph_audio_destroy(km_handle h);

/* ---- streaming: many concurrent speaker streams, state resident on the device -------------------------
 * Replaces, for all streams of this GPU at once, MelAudioBuffer.add_audio_frame / get_current_audio
 * (src/features/mel_sliding_window.py:70-140), MelSlidingWindowExtractor.process_audio_frame (:252-324) and
 * SimplifiedDualStreamModel.process_audio_frame_realtime (src/model/simplified_dual_stream_model.py:452-498).
 *   km_stream_create  n_streams rings of int(context_window_s * sr) samples; the ring hop is
 *                     int(sr / (1 / update_interval_s)) (= 532 for 0.0333 s, reference quirk); mel_cfg is the
 *                     sliding-window front end (n_fft 1024 / hop 533 / reflect / dB when built by the model,
 *                     simplified_dual_stream_model.py:122-131), out_frames = int(context_window / update_interval).
 *                     Allocates; call once, outside any graph capture.
 *   km_stream_push    samples_dev (n_streams, n_per_stream): one frame per stream; n_per_stream must be within
 *                     +/-1 of the ring hop (reference rejects others, :80-82) and is padded / truncated to it.
 *   km_stream_tick    emotion_dev (n_streams, emotion_dim) -> out_dev (n_streams, 52) for every stream whose ring
 *                     is full; ready_dev (n_streams) u8 mirrors MelAudioBuffer.is_full (rows of not-ready streams
 *                     are left untouched).  Per-stream EMA state lives in the handle.  The short-term rows are
 *                     the last three kept frames.  push + tick never allocate or synchronise: capture them in a
 *                     hipGraph and replay it per tick.  Five model shapes have a streaming core: d_model 256 /
 *                     8 heads / mel_sequence_length 256 (30 fps: update_interval 0.0333 s, front end hop 533),
 *                     d_model 512 / 8 or 16 heads / mel_sequence_length 512 (60 fps long context: update_interval
 *                     1/60 s, ring hop 266, front end hop 266, 512 frames per 8.5 s ring of which 510 are kept),
 *                     d_model 256 / 8 heads / mel_sequence_length 512 (the 60 fps recipe itself, same ring and front end) and
 *                     d_model 128 / 4 heads / mel_sequence_length 128 or 256 with 80 mel channels (the `fast` and `basic`
 *                     variants, 30 fps as the first shape; 255 kept rows of an 8.5 s ring, truncated to 128 at `fast`);
 *                     any other shape returns KM_ERR_UNSUPPORTED ("no kernel for d_model=...").
 *   km_stream_reset   clear rings, readiness and EMA state (MelSlidingWindowExtractor.reset :373-383). */
int km_stream_create(km_handle h, int64_t n_streams, double context_window_s, double update_interval_s,
                     const km_mel_config* mel_cfg);
int km_stream_push(km_handle h, const float* samples_dev, int64_t n_per_stream, void* stream);
int km_stream_tick(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* ready_dev, void* stream);
int km_stream_reset(km_handle h, void* stream);

/* ---- streams out of phase: a chunk FIFO per stream in front of its ring ----------------------------------------
 * Dual-stream handles with streams (km_stream_create) only; legacy and KoeMorphModel handles are refused as km_stream_* refuses
 * them.  Replaces, for all streams at once, the production model's real-time loop of scripts/rt.py: chunks of any size are
 * written into a consuming RingBuffer (:48-99) that drops what does not fit, one read(frame_samples) per inference step feeds
 * process_audio_frame_realtime (:343-372, src/model/simplified_dual_stream_model.py:452-507), and reset_realtime_state() is per
 * speaker.  km_stream_push / km_stream_tick keep serving streams that move in lockstep, unchanged.
 *   km_stream_fifo_create    call after km_stream_create: one FIFO of fifo_samples floats per stream (RingBuffer(int(
 *                            buffer_duration * sr)), 32000 by default) with its write_ptr, read_ptr and available (:51-56);
 *                            frame_samples is int(sr / target_fps) (533 at 30 fps, 266 at 60 fps).  Allocates: call it once,
 *                            outside any graph capture.  KM_ERR_INVALID_ARG without streams, for non-positive sizes, for
 *                            frame_samples not within +/-1 of the ring hop ("Frame size mismatch", mel_sliding_window.py:80-82)
 *                            and for fifo_samples < frame_samples (no read could ever succeed).  km_stream_create called again
 *                            frees the FIFOs together with the rings.
 *   km_stream_feed           RingBuffer.write (:58-79) for every stream: samples_dev (n_streams, n_per_stream); counts_dev
 *                            (n_streams) int32 or NULL = n_per_stream for all.  Stream s appends min(clamp(counts[s], 0,
 *                            n_per_stream), fifo_samples - available[s]) samples and drops the rest (:61-64).  May be called
 *                            several times between steps.
 *   km_stream_step           for every stream: read(frame_samples) (:81-99) -- a stream holding fewer samples does nothing on
 *                            this step; a stream that popped runs MelAudioBuffer.add_audio_frame on the frame (padded /
 *                            truncated to the ring hop, mel_sliding_window.py:84-91; is_full by :112); fired[s] = popped[s] &&
 *                            is_full[s], and only fired streams go through the emotion stream, the front end and the core with
 *                            the per-stream EMA.  A stream that did not fire -- a full ring that received no audio included --
 *                            keeps its out_dev row, EMA state, ring and started flag exactly as they were.  fired_dev (u8, may be
 *                            NULL); ready_dev (u8, may be NULL) mirrors is_full as km_stream_tick does; backlog_dev (int32, may
 *                            be NULL) = available[s] / frame_samples after the pop: while it is positive another step without a
 *                            feed drains the next whole frame.  The wall-clock gate of mel_sliding_window.py:267-269 is treated
 *                            as km_stream_tick treats it: steps are one audio hop apart.  Shapes as km_stream_tick, same
 *                            KM_ERR_UNSUPPORTED message.
 *   km_stream_reset_streams  for the streams with mask_dev[s] != 0 (u8): FIFO pointers (if FIFOs exist), ring write pointer and
 *                            frame count, is_full, started and the EMA state are cleared (MelSlidingWindowExtractor.reset
 *                            :373-383 + reset_temporal_state, simplified_dual_stream_model.py:417-419): the stream then behaves
 *                            as a freshly created one; every other stream is untouched.  Also works without FIFOs, with the
 *                            lockstep push / tick.  km_stream_reset keeps its meaning and empties the FIFOs too.
 * feed, step and reset_streams never allocate, synchronise or read anything back; feed + step capture into a hipGraph as one
 * linear chain. */
int km_stream_fifo_create(km_handle h, int64_t fifo_samples, int64_t frame_samples);
int km_stream_feed(km_handle h, const float* samples_dev, int64_t n_per_stream, const int32_t* counts_dev, void* stream);
int km_stream_step(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* fired_dev, uint8_t* ready_dev, int32_t* backlog_dev,
                   void* stream);
int km_stream_reset_streams(km_handle h, const uint8_t* mask_dev, void* stream);

/* ---- the model's other outputs from the live ticks ---------------------------------------------------------------
 * km_stream_tick / km_stream_step with two more outputs, indexed by stream (either may be NULL; with both NULL the calls ARE the
 * plain ones):
 *   raw_dev  (n_streams, 52)      the sigmoid values before the stream weights, the clamp and the EMA (km_core_forward's raw_dev)
 *   attn_dev (n_streams, 28, 80)  the mel stream's attention map, averaged over the heads as km_core_forward defines it; 16-byte
 *                                 aligned
 * A stream that is not computed -- not ready on a tick, not fired on a step -- keeps its rows of both exactly as it keeps its row
 * of out_dev.  out_dev, ready_dev, fired_dev, backlog_dev, the rings and the EMA state are bit-identical to the plain call's.  At
 * d_model 256 the map comes from the fused core's own attention-map instantiation; at d_model 512 from a dependent launch that
 * averages the heads' softmaxed scores of the computed streams (float32, heads added in the order 0 .. H - 1, then one multiply by
 * 1 / H).  The handle checks and refusals are those of km_stream_tick / km_stream_step, with their messages; a map asked for under
 * option core_split 3 / 6 is KM_ERR_UNSUPPORTED before anything is launched or popped.  No allocation, synchronisation or
 * readback: both capture, alone or in front of km_attn_stats_update_masked(acc, attn_dev, ready_dev / fired_dev, n_streams). */
int km_stream_tick_attn(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* ready_dev, float* raw_dev, float* attn_dev,
                        void* stream);
int km_stream_step_attn(km_handle h, const float* emotion_dev, float* out_dev, uint8_t* fired_dev, uint8_t* ready_dev, int32_t* backlog_dev,
                        float* raw_dev, float* attn_dev, void* stream);

/* ---- streaming the legacy SimplifiedKoeMorphModel: consuming FIFOs resident on the device ---------------------
 * Legacy handles (km_legacy_create, after km_finalize) only; the km_stream_* family above keeps refusing them and this one
 * refuses dual-stream and KoeMorphModel handles.  Replaces, for all streams at once, the real-time loop of
 * scripts/rt_simplified.py: RingBuffer (:46-97) and SimplifiedRealTimeInference.process_audio_chunk / inference_step (:374-399).
 *   km_legacy_stream_create  n_streams FIFOs of buffer_samples floats (int(buffer_duration * sr), :333) with their write_ptr,
 *                            read_ptr and available (:49-54), plus everything a tick needs (pop staging, power-mel, window
 *                            maxima, attention output; the workspace through km_reserve).  Allocates: call it once, outside
 *                            any graph capture.  KM_ERR_INVALID_ARG for non-positive arguments or audio_length >
 *                            buffer_samples; KM_ERR_UNSUPPORTED, naming the frame count, when 1 + audio_length / hop
 *                            (simplified_model.py:40) exceeds 32 or the handle is not d_model 256 / 8 heads / decoder hidden
 *                            128 behind the 1024-point front end.  Longer windows and other widths keep using
 *                            km_legacy_forward on windows the caller pops.
 *   km_legacy_stream_push    RingBuffer.write (:56-75) for every stream: samples_dev (n_streams, n_per_stream); counts_dev
 *                            (n_streams) int32, each clamped to 0 .. n_per_stream, or NULL = n_per_stream for all.  Stream s
 *                            appends min(count[s], buffer_samples - available[s]) samples and drops the rest (:59-62).
 *   km_legacy_stream_tick    RingBuffer.read(audio_length) + model(audio) (:378-399) for every stream: ready_dev[s] (u8, may
 *                            be NULL) = available[s] >= audio_length (:79-80); a ready stream consumes its window and gets
 *                            out_dev[s, :52]; the row and the FIFO of a stream that is not ready are left untouched.  Three
 *                            launches: pop, front end, model.
 *   km_legacy_stream_reset   empties the FIFOs and zeroes the pointers; the model itself has no temporal state
 *                            (simplified_model.py:155-157).
 * push and tick never allocate, synchronise or read anything back: capture them in a hipGraph (one linear chain) and replay
 * it per tick.  A later km_reserve that grows the workspace invalidates such a graph. */
int km_legacy_stream_create(km_handle h, int64_t n_streams, int64_t buffer_samples, int64_t audio_length);
int km_legacy_stream_push(km_handle h, const float* samples_dev, int64_t n_per_stream, const int32_t* counts_dev, void* stream);
int km_legacy_stream_tick(km_handle h, float* out_dev, uint8_t* ready_dev, void* stream);
int km_legacy_stream_reset(km_handle h, void* stream);

/* ---- measurement aid used by bench.py ------------------------------------------------------------
 * With stage timing enabled, km_forward_audio / km_forward_audio_pipelined record HIP events on the stream each
 * kernel is launched on, right before and after it (emotion logits, power-mel front end, fused core);
 * km_stage_times synchronises on the last event and returns the elapsed milliseconds of the most recent call:
 * ms[0] emotion, ms[1] front end, ms[2] core -- in pipelined mode these are the durations WHILE the other
 * call's kernel shares the chip, i.e. what rocprofv3 reports per dispatch.  Event records are not
 * graph-capturable: keep it off in production. */
int km_enable_stage_timing(km_handle h, int32_t enable);
int km_stage_times(km_handle h, float* ms3);

/* ---- eGeMAPSv02 functionals: the long-context emotion stream's feature extractor --------------------------------
 * Replaces the openSMILE call of OpenSMILEeGeMAPSExtractor._extract_features_from_audio
 * (src/features/opensmile_extractor.py:427-439): peak normalisation to [-1, 1] (:431-433), then the 88 eGeMAPSv02
 * functionals of the window (`opensmile.Smile(FeatureSet.eGeMAPSv02, FeatureLevel.Functionals).process_signal`, :227-235,
 * :439), for B windows of L samples at 16 kHz in one call.  openSMILE is a third-party package the reference neither
 * vendors nor pins: the arithmetic is the restatement of the published parameter set in oracle/egemaps.py (parity
 * unpinned; output order = openSMILE's feature order).
 *   km_egemaps_plan_create / _destroy   constant tables (windows, filterbank, log-frequency axis, ...) on the device
 *   km_egemaps_num_frames               10 ms frames of a window of L samples (60 ms frames, left aligned); at most 2048
 *   km_egemaps_workspace_floats         floats of caller-owned scratch km_egemaps_functionals needs for (B, L)
 *   km_egemaps_functionals              audio_dev (B, L) -> out_dev (B, 88); launches on `stream`, no allocation, no sync
 *   km_egemaps_records                  per-frame low-level descriptors of the last call on that workspace, (B, frames, 36)
 *                                       floats to the host (tests)
 *   km_egemaps_track_from_records       the pitch-track kernel alone on caller-written records rec_dev (B, nf, 36), in place:
 *                                       reads voicing, RMS, candidate frequencies / strengths, writes the F0 column (tests)
 *   km_egemaps_functionals_from_records the functionals kernel alone on caller-written records -> out_dev (B, 88) (tests)
 *                                       both: 1 <= nf <= 2048, 1 <= B <= 65535, the kernels km_egemaps_functionals launches */
int km_egemaps_plan_create(void** plan_out);
int km_egemaps_plan_destroy(void* plan);
int64_t km_egemaps_num_frames(int64_t L);
int64_t km_egemaps_workspace_floats(int64_t B, int64_t L);
int km_egemaps_functionals(void* plan, const float* audio_dev, int64_t B, int64_t L, int32_t normalize, float* work_dev,
                           int64_t work_floats, float* out_dev, void* stream);
int km_egemaps_records(const float* work_dev, int64_t B, int64_t L, float* rec_host, void* stream);
int km_egemaps_track_from_records(float* rec_dev, int64_t B, int64_t nf, void* stream);
int km_egemaps_functionals_from_records(const float* rec_dev, int64_t B, int64_t nf, float* out_dev, void* stream);
/* Windows beyond 2048 frames (20.5 s), opt-in: up to 2^20 samples (65.5 s, 6548 frames), the window limit of the `basic` back end.
 * The reference's long_context variant extracts eGeMAPS over 30 s (2995 frames).  The three per-frame kernels take any frame count;
 * the two per-window kernels (pitch track, functionals) have a second form that holds a long window in dynamic LDS and gives, on the
 * same records, the bits of the first form at every frame count up to 2048.
 *   km_egemaps_functionals_long              the contract of km_egemaps_functionals for L <= 2^20 (KM_ERR_UNSUPPORTED beyond: "a
 *                                            window of L samples, at most 1048576 (65.5 s)"); workspace from
 *                                            km_egemaps_workspace_floats, records by km_egemaps_records.  At 2048 frames or fewer it
 *                                            launches what km_egemaps_functionals launches
 *   km_egemaps_track_from_records_long       km_egemaps_track_from_records / _functionals_from_records for 1 <= nf <= 6548, ALWAYS
 *   km_egemaps_functionals_from_records_long on the long form of the kernel (tests: the equal-bits law) */
int km_egemaps_functionals_long(void* plan, const float* audio_dev, int64_t B, int64_t L, int32_t normalize, float* work_dev,
                                int64_t work_floats, float* out_dev, void* stream);
int km_egemaps_track_from_records_long(float* rec_dev, int64_t B, int64_t nf, void* stream);
int km_egemaps_functionals_from_records_long(const float* rec_dev, int64_t B, int64_t nf, float* out_dev, void* stream);
/* out (B, N) = x (B, K) w^T + b with w stored (N, K) like nn.Linear: the 264 -> 256 compression of the three concatenated
 * eGeMAPS windows (OpenSMILEeGeMAPSExtractor.get_concatenated_features, opensmile_extractor.py:575-590).  b may be NULL. */
int km_linear(const float* x_dev, const float* w_dev, const float* b_dev, int64_t B, int64_t K, int64_t N, float* out_dev, void* stream);
/* The GEMM kernel km_linear(B = M, K, N) runs on, for 16-byte aligned x and w (`batch` such products in one launch, as the
 * model's batched products are): 0 gemm_kernel (64 x 64 tile, any strides), gemm_nt_kernel 1 <2,2,true> (64 x 64),
 * 2 <4,2,true> (128 x 64), 3 <4,4,true> (128 x 128, K <= 256), 4 <4,4,false> (128 x 128, K > 256).  -1 for a bad argument.
 * Host only, no device needed: the tests name the kernel a product ran on with it. */
int km_gemm_kernel_choice(int64_t M, int64_t N, int64_t K, int64_t batch);
/* What the workgroups with linear ids 0 .. n_ids - 1 of a 1024-point front-end launch do, as the kernel itself derives it:
 * `windows` windows, per_window workgroups each, and -- group > 0 -- one emotion group workgroup per `group` windows in front of
 * them.  out (n_ids, 3) int32, on the host: kind (0 nothing: the surplus of the rounded-up grid, 1 the emotion logits of windows
 * [group b, group b + group), 2 front-end workgroup bx of window b), b, bx.  Host only, no device needed: the tests walk the mapping. */
int km_mel_role_table(int64_t windows, int32_t per_window, int32_t group, int64_t n_ids, int32_t* out);

/* ---- emotion vectors of many streams, from the pushed audio, resident on the device ------------------------------
 * An object of its own (not tied to a km_handle), on the current device.  Replaces, for n_streams speakers at once, one
 * OpenSMILEeGeMAPSExtractor(use_concatenation=True) per speaker (src/features/opensmile_extractor.py): its AudioBuffer (:29-154),
 * process_audio_frame / _extract_features (:287-318, :380-425), the three window slots (_update_window_features :460-502), the
 * Linear(264, 256) of get_concatenated_features (:559-608) and reset (:640-659).  With SR = 16000, per stream: a ring of
 * R = int((context_window_s + 2.0) * SR) samples with write_pos, is_full and total (int64 samples since creation or reset); the
 * window is [0, min(write_pos, C)) while the ring has not wrapped -- the OLDEST C samples once more than C have arrived, as
 * get_window does (:128-130) -- and the newest C = min(int(context_window_s * SR), R) samples ending at write_pos once it has.
 * Two deliberate deviations from the reference: time is audio time (a stream is due U = int(update_interval_s * SR) samples
 * after its last update, not update_interval_s of time.time() after it, :308-312), and an empty buffer's window of zeros
 * (:111-114) is never extracted -- a stream without audio has no features.
 *   km_emotion_stream_create           validates like the constructor (:204-209): context >= 1.0 s, 0.1 s <= interval <= context
 *                                      (KM_ERR_INVALID_ARG); 1 <= max_updates <= n_streams <= 4096 (KM_ERR_INVALID_ARG); the window
 *                                      must fit km_egemaps_num_frames(C) <= 2048 (KM_ERR_UNSUPPORTED).  Allocates everything.
 *   km_emotion_stream_set_compression  the Linear(264, 256) (:589-591): w_dev (256, 264) as nn.Linear stores it, b_dev (256); copied
 *   km_emotion_stream_push             AudioBuffer.append (:63-96) for every stream: samples_dev (n_streams, n_per_stream);
 *                                      counts_dev (n_streams) int32, each clamped to 0 .. n_per_stream, or NULL = n_per_stream for
 *                                      all.  A stream with count 0 is untouched.  n_per_stream > R: KM_ERR_INVALID_ARG
 *   km_emotion_stream_update           evaluates every stream once.  Eligible: total > 0, due (no features yet, or total -
 *                                      last_update_total >= U) and a window of at least int(0.5 * SR) samples (:388-389).  Of the
 *                                      eligible streams the max_updates that waited longest (total - last_update_total, never
 *                                      updated = -1; ties to the lowest index) are selected; the others wait for the next call.
 *                                      A selected stream: features = the 88 functionals of its window with peak normalisation
 *                                      (km_egemaps_functionals' kernels, reading the ring in place), NaN / +-Inf -> 0 (:450-452);
 *                                      empty 300 / 600 ms slots both take that vector and keep it until a reset (:478-490);
 *                                      last_update_total = total; emotion row = W concat(features, slot_300, slot_600) + b.
 *                                      Everything of a stream that was not selected is kept.  emotion_dev (n_streams, 256): every
 *                                      row (zero until the first update); valid_dev (u8, may be NULL): has features; updated_dev
 *                                      (u8, may be NULL): selected on this call.  KM_ERR_NOT_READY before set_compression
 *   km_emotion_stream_reset_streams    mask_dev (n_streams) u8, NULL = all: those streams become freshly created ones (ring
 *                                      zeroed, counters cleared, slots empty, zero emotion row); the others are untouched
 *   km_emotion_stream_features         features_dev (n_streams, 88) <- current features; slots_dev (n_streams, 2, 88) or NULL <-
 *                                      the 300 / 600 ms slots (device to device, on `stream`)
 * push, update and reset_streams never allocate, synchronise or read anything back, and their launch shapes depend only on
 * (n_streams, max_updates, n_per_stream): push + update capture into a hipGraph as one linear chain. */
int km_emotion_stream_create(void** es, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates);
int km_emotion_stream_destroy(void* es);
int km_emotion_stream_set_compression(void* es, const float* w_dev, const float* b_dev, void* stream);
int km_emotion_stream_push(void* es, const float* samples_dev, int64_t n_per_stream, const int32_t* counts_dev, void* stream);
int km_emotion_stream_update(void* es, float* emotion_dev, uint8_t* valid_dev, uint8_t* updated_dev, void* stream);
int km_emotion_stream_reset_streams(void* es, const uint8_t* mask_dev, void* stream);
int km_emotion_stream_features(void* es, float* features_dev, float* slots_dev, void* stream);

/* ---- the `basic` prosodic emotion features: EmotionExtractor._extract_basic on the device ------------------------------
 * Replaces the librosa calls of EmotionExtractor._extract_basic (src/features/emotion_extractor.py:503-545), which forward runs
 * once per batch row on the whole audio it was handed (:280-300): for a window y of L >= 1 samples at 16 kHz the nine values
 * [energy, zcr, spectral_centroid, f0_mean, f0_std, mean, std, max, min], raw, with no normalisation -- np.mean(y ** 2), the means
 * over frames of librosa.feature.zero_crossing_rate and librosa.feature.spectral_centroid, nanmean / nanstd of
 * librosa.yin(fmin=50, fmax=400), np.mean / std / max / min.  librosa is a third-party package the reference pins only as
 * >=0.10.0: the arithmetic is the restatement of its 0.10 defaults (frames of 2048 samples, hop 512, centred: F = 1 + L / 512)
 * in tests/prosody_cases.py and in the header of km_prosody.hip, and has not been checked against the package (PARITY UNPINNED).
 * One deliberate deviation: yin's difference function is the direct sum of squared differences, not librosa's FFT
 * autocorrelation with terms below 1e-6 zeroed; digital silence gives f0 = 400 either way.  Inputs are assumed finite.
 *   km_prosody_plan_create / _destroy   Hann window and twiddle tables on the device
 *   km_prosody_num_frames               frames of a window of L samples: 1 + L / 512 (0 for L < 1)
 *   km_prosody_workspace_floats         floats of caller-owned scratch for B windows of L samples (4 per frame); -1 for B or L < 1
 *   km_prosody_features                 audio_dev: B rows of L samples, row b at audio_dev + b * row_stride (row_stride >= L) ->
 *                                       out_dev (B, 9).  frames_dev (B, F, 4) or NULL: the per-frame records (Z_f, C_f, f0_f, i*),
 *                                       i* the chosen index into yin's 281 candidate periods (period 40 + i*); when given, the
 *                                       records are written there and work_dev may be NULL.  1 <= L <= 2^20 and 1 <= B <= 65535:
 *                                       below 1 KM_ERR_INVALID_ARG, above KM_ERR_UNSUPPORTED; a short workspace KM_ERR_WORKSPACE
 *   km_prosody_windows                  W windows of a resident clip: window w covers clip_dev[s, s + L) with s =
 *                                       start_samples_dev[w] (int32, on the device), shortened ON THE DEVICE to what the clip
 *                                       holds -> out_dev (W, 9), each row what km_prosody_features gives on the shortened window,
 *                                       bit for bit.  A window that holds nothing (s < 0 or s >= clip_len) writes a zero row.
 *                                       Limits of W and L as for B and L above; 1 <= clip_len < 2^31
 * Neither call allocates, synchronises or reads anything back; every sum has a fixed order that depends on L only, so a window
 * gives the same bits wherever it lies (dense row, clip, stream ring). */
int km_prosody_plan_create(void** plan_out);
int km_prosody_plan_destroy(void* plan);
int64_t km_prosody_num_frames(int64_t L);
int64_t km_prosody_workspace_floats(int64_t B, int64_t L);
int km_prosody_features(void* plan, const float* audio_dev, int64_t B, int64_t L, int64_t row_stride, float* work_dev, int64_t work_floats,
                        float* out_dev, float* frames_dev, void* stream);
int km_prosody_windows(void* plan, const float* clip_dev, int64_t clip_len, const int32_t* start_samples_dev, int64_t W, int64_t L,
                       float* work_dev, int64_t work_floats, float* out_dev, void* stream);
/* The emotion-stream object above in a second back end: the same rings, push, eligibility and selection rule, reset and capture
 * contract, but a selected stream's features are the nine values above of its window (km_prosody_features' kernels, reading the
 * ring in place), raw: no peak normalisation, no window slots, no compression layer.  The window may hold up to 2^20 samples
 * (KM_ERR_UNSUPPORTED beyond).  On such an object km_emotion_stream_update writes emotion_dev (n_streams, 9),
 * km_emotion_stream_features writes features_dev (n_streams, 9) and refuses a non-NULL slots_dev (KM_ERR_INVALID_ARG), and
 * km_emotion_stream_set_compression returns KM_ERR_INVALID_ARG; no call is needed before the first update. */
int km_emotion_stream_create_basic(void** es, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates);

/* ---- the emotion track of a resident clip: the offline producer of the model's emotion input ---------------------
 * What ONE emotion stream (above) holds after t samples of a clip, for every update time at once.  With SR, R, C, U and MIN as
 * km_emotion_stream_create computes them, a clip of n samples has K rows: K = 0 if n < MIN, else (n - MIN) / U + 1.  Row k
 * belongs to audio time t_k = MIN + k U; its window is what the stream's AudioBuffer returns after t_k samples, the quirk
 * included: [0, min(t_k, C)) while t_k < R, [t_k - C, t_k) from t_k >= R on -- the updates of a stream fed the clip in chunks of
 * gcd(MIN, U) samples with an update after every push.  features[k] = the 88 functionals of that window, peak-normalised,
 * NaN / +-Inf -> 0, by the kernels the streams run (the clip is read in place); emotion[k] = W concat(features[k], features[0],
 * features[0]) + b: the 300 / 600 ms slots are filled once per life and a clip is one life.  A training window that starts at
 * frame s, with T frames of hop h, ends at e = min(n, (s + T) h); its row is clamp((e - MIN) / U, 0, K - 1), the last update a
 * live stream would have made by then (the first one for a window that ends before it).
 *   km_emotion_clip_create           validates like km_emotion_stream_create; 1 <= max_slots <= 65535 windows are extracted per
 *                                    pass.  Allocates everything (slot table, scales, max_slots x frames x 36 records,
 *                                    max_slots x 88 functionals, the weights)
 *   km_emotion_clip_set_compression  w_dev (256, 264) as nn.Linear stores it, b_dev (256); copied
 *   km_emotion_clip_num_rows         K of a clip of clip_len samples (host arithmetic; 0 for a NULL object)
 *   km_emotion_clip_build            clip_dev (clip_len) -> features_out (K, 88) or NULL, emotion_out (K, 256), in
 *                                    ceil(K / max_slots) passes.  K = 0: nothing is launched, KM_OK.  clip_len > 2^30 (window
 *                                    starts are 32-bit): KM_ERR_INVALID_ARG.  KM_ERR_NOT_READY before set_compression
 *   km_emotion_clip_rows             emotion_track_dev (K, 256) of a clip of clip_len samples (K must be its num_rows),
 *                                    start_frames_dev (B) int32 -> emotion_out (B, 256), valid_out (B) u8 or NULL.  K = 0:
 *                                    zero rows, valid 0, as a stream without features
 *   km_emotion_clip_build_batch      clips_dev (B, L), B clips of ONE length -> features_out (B, K, 88), emotion_out (B, K, 256),
 *                                    each clip's slice bit-identical to km_emotion_clip_build of that clip.  Rows are numbered
 *                                    g = c K + k and a pass takes max_slots consecutive g, so passes are filled across clip
 *                                    boundaries: ceil(B K / max_slots) of them.  A row is compressed with features[0] of its OWN
 *                                    clip: from the pass itself when row (c, 0) lies in it, else from features_out[c, 0] that
 *                                    an earlier pass wrote -- which is why features_out is REQUIRED here.  K = 0 or B = 0:
 *                                    nothing is launched.  L > 2^30 or B K > 2^31 - 1: KM_ERR_INVALID_ARG
 * build, build_batch and rows never allocate, synchronise or read back; the launch shape of rows depends on B alone, so it can sit inside a
 * captured training step. */
int km_emotion_clip_create(void** ec, double context_window_s, double update_interval_s, int64_t max_slots);
int km_emotion_clip_destroy(void* ec);
int km_emotion_clip_set_compression(void* ec, const float* w_dev, const float* b_dev, void* stream);
int64_t km_emotion_clip_num_rows(void* ec, int64_t clip_len);
int km_emotion_clip_build(void* ec, const float* clip_dev, int64_t clip_len, float* features_out, float* emotion_out, void* stream);
int km_emotion_clip_build_batch(void* ec, const float* clips_dev, int64_t B, int64_t L, float* features_out, float* emotion_out,
                                void* stream);
int km_emotion_clip_rows(void* ec, const float* emotion_track_dev, int64_t K, int64_t clip_len, const int32_t* start_frames_dev, int64_t B,
                         int64_t hop, int64_t window_frames, float* emotion_out, uint8_t* valid_out, void* stream);
/* The `basic` back end of the track: row k is the nine raw prosodic values [energy, zcr, centroid, f0_mean, f0_std, mean, std, max,
 * min] of the SAME window, i.e. what one km_emotion_stream_create_basic stream holds after t_k samples of the clip, bit for bit, and
 * bit for bit km_prosody_features on that window: no peak normalisation, no 300 / 600 ms slots, no compression layer, no NaN scrub.
 * K, the windows and the window -> row mapping are the ones above.
 *   km_emotion_clip_create_basic     validates like km_emotion_clip_create, except that the window limit is the stream back end's:
 *                                    C <= 2^20 samples (65.5 s), else KM_ERR_UNSUPPORTED.  Holds a prosody plan; scratch is the
 *                                    slot table and max_slots x (1 + C / 512) x 4 floats of frame records
 *   km_emotion_clip_width            256 or 9: the row width of the object's tracks (host only; 0 for a NULL object)
 * On such an object
 *   km_emotion_clip_set_compression  KM_ERR_INVALID_ARG; no call is needed before the first build
 *   km_emotion_clip_build            emotion_out (K, 9); features_out must be NULL (KM_ERR_INVALID_ARG otherwise: there are no
 *                                    functionals).  The windows are read in place and every pass writes its rows straight into
 *                                    emotion_out (empty slots write nothing), so rows beyond K are never touched
 *   km_emotion_clip_build_batch      emotion_out (B, K, 9), features_out NULL; each clip's slice bit-identical to build of that clip
 *   km_emotion_clip_rows             emotion_track_dev (K, 9) -> emotion_out (B, 9); one launch of ceil(B / 16) workgroups
 *   km_emotion_clip_num_rows         unchanged
 * and, as above, none of them allocates, synchronises or reads back. */
int km_emotion_clip_create_basic(void** ec, double context_window_s, double update_interval_s, int64_t max_slots);
int km_emotion_clip_width(void* ec);
/* The eGeMAPS objects (km_emotion_stream_create, km_emotion_clip_create) with the window limit of km_egemaps_functionals_long: C <=
 * 2^20 samples, else KM_ERR_UNSUPPORTED "a window of C samples, at most 1048576 (65.5 s)".  Every other check, its text (under the
 * entry point's own name) and the order in which the refusals win are those of the plain entry points; all refusals come before any
 * device call and leave a null handle.  An object whose window has at most 2048 frames IS the plain object.  Beyond that every
 * call on the object is unchanged (push, update, set_compression, reset_streams, features; build, build_batch, rows; capture and
 * replay); the frame records take slots x frames x 36 floats of the object's one allocation (0.94 MB per slot at the limit), and
 * the per-window kernels of every slot, short windows included, are the long form. */
int km_emotion_stream_create_long(void** es, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates);
int km_emotion_clip_create_long(void** ec, double context_window_s, double update_interval_s, int64_t max_slots);
/* ---- the GeMAPS feature set: the emotion input of the reference's `fast` variant (configs/model/dual_stream.yaml: 10 s / 0.5 s,
 * feature_set "GeMAPS") ----
 * The 62 functionals of GeMAPS v01b are the 88 of eGeMAPSv02 without the spectral flux (5 values), MFCC 1-4 (16), the bandwidths of F2
 * and F3 (4) and the equivalent sound level (1): columns 20-29, 48, 49, 54, 55, 66-75, 80 and 87 removed, the other 62 in the order
 * the 88 have.  PARITY with openSMILE's own GeMAPSv01b -- values, and that its column order is this one -- is UNPINNED, as for the
 * whole eGeMAPS back end.  What is pinned: value j of a GeMAPS call IS, bit for bit, the value of the j-th kept column of the eGeMAPS
 * call on the same samples.  The frame kernel's GeMAPS form leaves out the previous frame's transform, the flux sum and the four DCT
 * sums and writes 0 to fields 5-9 of a frame record (36 floats, same layout); the functionals kernel's skips the seven contours and
 * the RMS sum nobody reads.  An unknown feature set is KM_ERR_INVALID_ARG everywhere.
 *   km_feature_set_width                     88 / 62, -1 for an unknown set
 *   km_egemaps_functionals_set               km_egemaps_functionals (long_windows 0) or km_egemaps_functionals_long (non-zero) with
 *                                            out_dev (B, width): their workspace, their refusals under this name; with set 0 their
 *                                            launches
 *   km_egemaps_functionals_from_records_set  the test hooks km_egemaps_functionals_from_records / _long (long_windows non-zero
 *                                            ALWAYS runs the long form) with out_dev (B, width)
 *   km_emotion_stream_create_set             km_emotion_stream_create / _create_long for a feature set; with set 0 exactly their object
 *   km_emotion_clip_create_set               km_emotion_clip_create / _create_long likewise
 *   km_emotion_stream_feature_width          88 / 62 / 9: the row width of `features` (host only; 0 for a NULL object)
 *   km_emotion_clip_feature_width
 * On a GeMAPS object set_compression takes w (256, 186) -- three windows of 62, concatenated as the 88 are; the reference hard-codes
 * Linear(264, 256) and so never compresses GeMAPS features, a deliberate deviation -- `features` is (n, 62), the slots (n, 2, 62),
 * build / build_batch write features_out (K, 62).  The sum over k is the sequential chain of the 88-value objects with the 78 terms of
 * the removed columns left out: an eGeMAPS object whose layer holds those weights in the kept columns and 0 elsewhere gives equal
 * emotion bits.  Every other call (rows, push, update, reset_streams, capture and replay) is unchanged. */
#define KM_FEATURE_SET_EGEMAPS 0
#define KM_FEATURE_SET_GEMAPS 1
int km_feature_set_width(int32_t feature_set);
int km_egemaps_functionals_set(void* plan, int32_t feature_set, int32_t long_windows, const float* audio_dev, int64_t B, int64_t L,
                               int32_t normalize, float* work_dev, int64_t work_floats, float* out_dev, void* stream);
int km_egemaps_functionals_from_records_set(int32_t feature_set, int32_t long_windows, const float* rec_dev, int64_t B, int64_t nf,
                                            float* out_dev, void* stream);
int km_emotion_stream_create_set(void** es, int64_t n_streams, double context_window_s, double update_interval_s, int64_t max_updates,
                                 int32_t feature_set, int32_t long_windows);
int km_emotion_clip_create_set(void** ec, double context_window_s, double update_interval_s, int64_t max_slots, int32_t feature_set,
                               int32_t long_windows);
int km_emotion_stream_feature_width(void* es);
int km_emotion_clip_feature_width(void* ec);
/* ---- eGeMAPS low-level descriptors per frame: the reference extractor's feature_level="LowLevelDescriptors"
 * (src/features/opensmile_extractor.py:220-225), and a per-frame emotion input on the model's frame grid ----
 * The 25 smoothed contours behind the 88 functionals, one row per frame, from the frame records of the calls above: columns 0-9 the
 * 3-frame average of loudness, alpha ratio, Hammarberg index, the two spectral slopes, spectral flux and MFCC 1-4; column 10 the
 * semitone (from 27.5 Hz) of the non-zero-smoothed F0, 0 in unvoiced frames; columns 11-24 jitter, shimmer, HNR, H1-H2, H1-A3 and
 * frequency, bandwidth, amplitude of F1, F2, F3, masked to voiced frames and smoothed over non-zero values, 0 in unvoiced frames.
 * GeMAPS: the 18 columns left without 5-9, 20 and 23.  The float32 statements are those of the functionals kernel.  PARITY of names,
 * order and values with openSMILE's own LowLevelDescriptors level is UNPINNED, as for the whole eGeMAPS back end.
 * Frame grid: fps == 0 gives the native rows, one per 10 ms frame.  Otherwise fps must be finite and within 1 .. 400
 * (KM_ERR_INVALID_ARG), there are int(L / 16000 * fps) rows (float64, in that order: the mel extractor's frame count), and row k sits
 * at frame coordinate p = k * 100.0 / fps, j = floor(p), w = p - j: the last frame for j >= nf - 1, frame j for w == 0, otherwise
 * fmaf((float)w, b - a, a) between frames j and j + 1 -- but columns 10-24 blend only where both are non-zero and else take the nearer
 * frame's value (the earlier at w == 0.5): a descriptor is never mixed with an unvoiced frame's 0.
 *   km_egemaps_lld_width          25 / 18, -1 for an unknown set
 *   km_egemaps_lld_frames         rows of the grid for a window of L samples; fps == 0: km_egemaps_num_frames(L); -1 for a bad fps
 *   km_egemaps_llds               audio_dev (B, L) -> out_dev (B, rows, width).  The checks, limits and refusal texts of
 *                                 km_egemaps_functionals_set under this name, its workspace (km_egemaps_workspace_floats; records by
 *                                 km_egemaps_records) and its launches up to the records, then one launch of the descriptor kernel.
 *                                 Launches only: no allocation, no synchronisation, capturable.  A grid of 0 rows launches nothing.
 *   km_egemaps_llds_from_records  the descriptor kernel alone on caller-written records rec_dev (B, nf, 36), 1 <= nf <= 6548 (tests);
 *                                 L_for_grid lays the grid (ignored with fps == 0, at most 2^20) */
int km_egemaps_lld_width(int32_t feature_set);
int64_t km_egemaps_lld_frames(int64_t L, double fps);
int km_egemaps_llds(void* plan, int32_t feature_set, int32_t long_windows, const float* audio_dev, int64_t B, int64_t L, int32_t normalize,
                    float* work_dev, int64_t work_floats, double fps, float* out_dev, void* stream);
int km_egemaps_llds_from_records(int32_t feature_set, const float* rec_dev, int64_t B, int64_t nf, int64_t L_for_grid, double fps,
                                 float* out_dev, void* stream);

/* ---- evaluation metrics: a streaming accumulator in device memory ------------------------------------------------
 * Replaces BlendshapeMetrics (src/model/losses.py:421-521) and compute_lip_sync_metrics (:524-583).  The reference
 * copies every batch to the host, concatenates the epoch and reduces it there; here (N, 52) rows are folded into a
 * float64 / integer state on the device (first-row-shifted moments per column, absolute and squared errors, frame-to-frame
 * differences carried ACROSS updates as torch.diff over the concatenation sees them, activity counts against float32(0.1),
 * moments of the mouth activity = sum of columns 12..31, and of an optional per-row audio energy).  Fixed-order
 * reductions: the same rows in the same calls give the same bits.
 *   km_metrics_create / _destroy   state + a workspace of partial records on the current device; the state starts empty
 *   km_metrics_reset               BlendshapeMetrics.reset (:432-436)
 *   km_metrics_update              BlendshapeMetrics.update (:438-449): pred_dev, target_dev (N, 52); audio_energy_dev (N)
 *                                  (km_audio_energy of the batch's audio features) or NULL.  Any N >= 0; N = 0 does nothing,
 *                                  calls beyond 2^24 rows are cut into pieces inside
 *   km_metrics_compute             BlendshapeMetrics.compute (:451-521) + compute_lip_sync_metrics (:540-583) over
 *                                  everything since the last reset: out_dev[KM_METRICS_COUNT] float32, finalised in
 *                                  float64 and rounded once.  The state is left as it is (compute, update, compute works)
 * reset / update / compute launch on `stream`, neither allocate nor synchronise nor read back, and can be captured.
 * out_dev, in the reference's key order:
 *    0 mae                   1 mse                 2 rmse                 3 max_bs_mae         4 min_bs_mae
 *    5 std_bs_mae            6 mean_correlation    7 min_correlation      8 temporal_consistency
 *    9 pred_smoothness      10 target_smoothness  11 pred_activity       12 target_activity   13 precision
 *   14 recall               15 f1_score
 *   16 mouth_mae            17 mouth_correlation  18 audiovisual_sync (0 unless an energy was given)
 *   19 rows (exact below 2^24)   20 valid_correlations (columns that passed the std() > 1e-6 gate of :479)
 *   21 has_energy (1 when any update came with an energy, else 0)
 * 8..10 are 0 while fewer than two rows were seen (the reference leaves the keys out, :492); before any row every entry
 * is 0 (the reference returns {}, :453-454). */
#define KM_METRICS_COUNT 22
int km_metrics_create(void** acc_out);
int km_metrics_destroy(void* acc);
int km_metrics_reset(void* acc, void* stream);
int km_metrics_update(void* acc, const float* pred_dev, const float* target_dev, const float* audio_energy_dev, int64_t N, void* stream);
int km_metrics_compute(void* acc, float* out_dev, void* stream);

/* ---- attention-map statistics: a streaming accumulator in device memory ---------------------------------------------------
 * Replaces the reductions AttentionVisualizer is built on (src/visualization/attention_viz.py: the mean map, :96-98, and the
 * mass per frequency band, :329-331) for maps that stay on the device: (rows, Q, K) float32 maps are folded into a float64 /
 * integer state, per query q over every map since the last reset
 *   sum[q][k]   the float64 sum of A                                   (compute: / rows, the mean map)
 *   ent[q]      the sum over maps of -sum_k A ln A, every term in float64 from the float32 entry, 0 for an entry of 0
 *                                                                      (compute: / rows, the mean entropy)
 *   peak[q][k]  the number of maps whose largest entry of query q is key k, ties to the lowest k (np.argmax); exact
 * Fixed-order reductions, no atomics: the same rows in the same calls with the same max_rows_per_launch give the same bits.
 *   km_attn_stats_create    Q = n_queries >= 1, K = n_keys a multiple of 4 up to 256 (28 x 80 for this model);
 *                           max_rows_per_launch = 0 is a default (4096), larger updates are cut into pieces inside
 *   km_attn_stats_shape     the Q and K of an accumulator
 *   km_attn_stats_update    attn_dev (rows, Q, K), 16-byte aligned; rows = 0 does nothing
 *   km_attn_stats_compute   out_dev[KM_ATTN_STATS_COUNT(Q, K)] float64: rows, the mean map (Q K), the mean entropy (Q), the peak
 *                           counts (Q K); all 0 before any row.  The state is left as it is (compute, update, compute works)
 *   km_attn_stats_update_masked  folds the rows of attn_dev (rows, Q, K) whose byte of mask_dev (rows) u8 is non-zero, in index
 *                           order: the state afterwards is bit-identical to km_attn_stats_update on those rows compacted into a
 *                           dense array, for any mask (all zero: nothing changes).  How many rows are selected stays on the device:
 *                           an ordered compaction writes an index table (allocated by create, max_rows_per_launch entries) and the
 *                           count, piece by piece as the dense update cuts them.  rows below 2^31.
 * reset / update / update_masked / compute launch on `stream`, neither allocate nor synchronise nor read back, and can be captured.
 *
 * One independent state per stream, for the maps of km_stream_tick_attn / km_stream_step_attn:
 *   km_attn_stats_streams_create   n_streams states (1 .. 65535) for Q x K maps
 *   km_attn_stats_streams_update   attn_dev (n_streams, Q, K), 16-byte aligned, and mask_dev (n_streams) u8: stream s takes its map
 *                                  when mask_dev[s] != 0.  No reduction across streams or rows: stream s's state is bit-identical
 *                                  to an accumulator of km_attn_stats_create that received the stream's selected maps one
 *                                  km_attn_stats_update(rows = 1) at a time, in order
 *   km_attn_stats_streams_reset    the streams with mask_dev[s] != 0 become fresh, the others are untouched; NULL: all
 *   km_attn_stats_streams_compute  out_dev (n_streams, KM_ATTN_STATS_COUNT(Q, K)) float64, one km_attn_stats_compute vector per stream
 * update / reset / compute neither allocate nor synchronise nor read back, and can be captured. */
#define KM_ATTN_STATS_COUNT(Q, K) (1 + (Q) * (K) + (Q) + (Q) * (K))
int km_attn_stats_create(void** acc_out, int32_t n_queries, int32_t n_keys, int64_t max_rows_per_launch);
int km_attn_stats_destroy(void* acc);
int km_attn_stats_shape(void* acc, int32_t* n_queries, int32_t* n_keys);
int km_attn_stats_reset(void* acc, void* stream);
int km_attn_stats_update(void* acc, const float* attn_dev, int64_t rows, void* stream);
int km_attn_stats_update_masked(void* acc, const float* attn_dev, const uint8_t* mask_dev, int64_t rows, void* stream);
int km_attn_stats_compute(void* acc, double* out_dev, void* stream);
int km_attn_stats_streams_create(void** acc_out, int64_t n_streams, int32_t n_queries, int32_t n_keys);
int km_attn_stats_streams_destroy(void* acc);
int km_attn_stats_streams_update(void* acc, const float* attn_dev, const uint8_t* mask_dev, void* stream);
int km_attn_stats_streams_reset(void* acc, const uint8_t* mask_dev, void* stream);
int km_attn_stats_streams_compute(void* acc, double* out_dev, void* stream);

/* ---- the loss by component: a streaming accumulator in device memory ------------------------------------------------
 * Replaces the `metrics` dict of KoeMorphLoss.forward (src/model/losses.py:111-183: one .item() per term and batch), the
 * per-batch criterion call + .item() reads of the reference's validate() (src/train_sequential.py:257-271) and the
 * per-sequence loss / smoothness lists it keeps (:273-290).  One update takes one batch (N, 52), N >= 1, and evaluates in
 * float64 the eval-mode value of every term km_train_step* adds (KoeMorphLoss's eight, perceptual with the audio-visual part
 * when cfg->audio_energy_dev is set, and DualStreamLoss's two), their weighted total
 * mse_weight * mse + l1_weight * l1 + sum cfg weight * term, and the rows' smoothness mean_j |pred[b, j+1] - pred[b, j]|.
 * The skip rules are km_loss_config's: temporal and velocity need prev_pred_dev and prev_target_dev, landmark landmark_w_dev,
 * ds_velocity ds_prev_pred_dev, ds_separation a weight > 0; a skipped term reports 0 and its update does not count in its
 * mean.  cfg = NULL evaluates mse and l1 only; cfg->abi_version is checked as in km_train_set_loss.  cfg is read during the
 * call (its device pointers on the stream).  Fixed-order float64 reductions, no floating-point atomics: the same rows in the
 * same calls give the same bits.  reset / update / compute launch on `stream`, neither allocate nor synchronise nor read
 * back, and can be captured.
 *   km_loss_terms_update    terms_dev (KM_LOSS_TERMS) or NULL: this batch's values, float32, indexed by KM_LOSS_TERM_*
 *   km_loss_terms_compute   out_dev (KM_LOSS_TERMS + 2): per term (and for the total) the mean over the UPDATES since the last
 *                           reset in which it was evaluated -- the reference averages per-batch losses (:286-287) -- then
 *                           [KM_LOSS_TERMS] the number of updates and [KM_LOSS_TERMS + 1] the mean over all ROWS of their
 *                           smoothness; all 0 before any update.  The state is left as it is */
enum {
    KM_LOSS_TERM_MSE = 0, KM_LOSS_TERM_L1 = 1, KM_LOSS_TERM_PERCEPTUAL = 2, KM_LOSS_TERM_TEMPORAL = 3, KM_LOSS_TERM_VELOCITY = 4,
    KM_LOSS_TERM_SPARSITY = 5, KM_LOSS_TERM_SMOOTHNESS = 6, KM_LOSS_TERM_LANDMARK = 7, KM_LOSS_TERM_DS_VELOCITY = 8,
    KM_LOSS_TERM_DS_SEPARATION = 9, KM_LOSS_TERM_TOTAL = 10
};
#define KM_LOSS_TERMS 11
int km_loss_terms_create(void** acc_out);
int km_loss_terms_destroy(void* acc);
int km_loss_terms_reset(void* acc, void* stream);
int km_loss_terms_update(void* acc, const km_loss_config* cfg, float mse_weight, float l1_weight,
                         const float* pred_dev, const float* target_dev, int64_t N, float* terms_dev, void* stream);
int km_loss_terms_compute(void* acc, float* out_dev, void* stream);

/* ---- sample-rate conversion: whole clips and stateful streams, on the device -------------------------------------------
 * Replaces the host-side conversion in front of every 16 kHz entry point (the reference's librosa.resample in
 * src/data/sequential_dataset.py:100-101; here scipy.signal.resample_poly) for audio that arrives at its capture rate.
 * up / down is the reduced ratio rate_out / rate_in.  The taps are the caller's: for resample_poly's filter,
 *     half_len = 10 max(up, down),   h[k] = up * fc sinc(fc (k - half_len)) kaiser_5.0[k] / (sum of those),   fc = 1 / max(up, down),
 * k = 0 .. 2 half_len (koemorph_amd.features.resample.resample_filter); half_len is taken as (n_taps - 1) / 2.  The library rounds
 * them to float32 once.  Output m of an input x[0..N) is
 *     y[m] = sum_j x[j] h[m down - j up + half_len]      (tap index within [0, 2 half_len], x zero outside [0, N)),
 * one float32 fmaf chain over ascending j; n_out(N) = ceil(N up / down).  A stream that has consumed N samples has emitted the
 * max(0, ceil((N up - half_len) / down)) outputs whose samples have all arrived; its state is the last ceil(2 half_len / up)
 * samples and one bounded integer, so nothing wraps however long it runs.  The same output index has the same bits from
 * km_resample_clip, from km_resampler_push under any chunking and from km_resampler_flush.
 *   km_resampler_create         n_streams 1 .. 65535; n_taps odd; up != down; KM_ERR_UNSUPPORTED when the polyphase table and one
 *                               tile's input span do not fit the kernels' 64 KiB of LDS (8000, 11025, 22050, 24000, 32000,
 *                               44100, 48000 and 96000 -> 16000 do)
 *   km_resampler_out_max        ceil(n_in_max up / down) + 1: a row length that holds whatever a push of n_in_max samples emits
 *   km_resampler_push           samples_dev (n_streams, n_per_stream), counts_dev (n_streams) or NULL (all) as in km_stream_feed;
 *                               stream s's new outputs go to out_dev + s out_stride, their number to out_counts_dev[s]; a stream
 *                               that brings nothing is untouched and reports 0.  out_stride >= ceil(n_per_stream up / down)
 *   km_resampler_flush          the streams of mask_dev (NULL: all) emit what they still owe up to n_out(N), as though zeros
 *                               followed, and are left reset; the others report 0.  out_stride >= ceil(half_len / down)
 *   km_resampler_reset_streams  those streams become freshly created ones (NULL: all)
 *   km_resample_clip            clip_dev (n_in) -> out_dev (n_out), n_out == ceil(n_in up / down); uses no stream state
 * push / flush / reset_streams / clip launch on `stream`, neither allocate nor synchronise nor read back, and can be captured. */
int km_resampler_create(void** rs, int64_t n_streams, int32_t up, int32_t down, const double* taps_host, int64_t n_taps);
int km_resampler_destroy(void* rs);
int km_resampler_out_max(void* rs, int64_t n_in_max, int64_t* n_out_max);
int km_resampler_push(void* rs, const float* samples_dev, int64_t n_per_stream, const int32_t* counts_dev,
                      float* out_dev, int64_t out_stride, int32_t* out_counts_dev, void* stream);
int km_resampler_flush(void* rs, const uint8_t* mask_dev, float* out_dev, int64_t out_stride, int32_t* out_counts_dev, void* stream);
int km_resampler_reset_streams(void* rs, const uint8_t* mask_dev, void* stream);
int km_resample_clip(void* rs, const float* clip_dev, int64_t n_in, float* out_dev, int64_t n_out, void* stream);

/* ---- run-time switches ---------------------------------------------------------------------------
 * Replaces what would be module attributes / environment switches on the reference side (the reference has none on
 * this path: every switch selects between two implementations of the SAME arithmetic, for A/B timing and for the
 * tests that pin one path against the other).  Names: "core_split" (0 | 3 | 6, experimental split-bf16 core),
 * "seq_per_window", "seq_assemble" (default 0; 1: sequence mode shares each clip's STFT frames at every shape and hop whose forward
 * call has a power path, assembling the windows into the workspace: km_sequence_plan route 2), "clip_assemble" (default 0; 1:
 * km_train_step_clip / km_forward_clip / km_forward_clip_attn also run on the handles they refuse by default, from a span image and
 * E edge rows a side per window: km_clip_plan route 2; a handle they accept keeps its launches and bits), "generic_staged", "mel_two_frame", "emotion_separate",
 * "emotion_rider" (default 0; 1: at d_model 256 the front-end launch computes each window's emotion logit inside one of that window's
 * workgroups, as it does at the other shapes, instead of in group workgroups at the head of the launch that read the weights once per group of windows; same bits), "no_ln_fusion", "no_db_fusion",
 * "no_score_fusion", "no_out_fusion", "no_v_fusion",
 * "no_core_merge" (the one-launch cores of d_model 512 and of d_model 256 / window 512 as the launches they replaced: km_core_route),
 * "core128" (default 0; 1: the forward calls at d_model 128 / 4 heads / window 128 or 256 run core128_kernel, route 4, instead of the
 * launch-per-product chain; the streams at those shapes run its streaming form either way),
 * "kmm_no_fuse" (km_koemorph_forward as the launch-per-step GEMM chain even at the width of the two fused kernels),
 * "legacy_no_enc_fusion" / "legacy_no_attn_fusion" / "legacy_no_tail_fusion" (km_legacy_forward's three fused kernels back to GEMM-chain launches), "train_op_per_launch" (timing aid:
 * every operation of the training program as its own launch), "train_bm32_below", "train_tail_groups", "train_split_min_k",
 * "train_no_dma" (the products of the training program on the register-staged tile instead of the LDS-DMA tile),
 * "train_attn_regs" (its attention blocks register-staged as in round 3), "train_no_fe_pack" (km_train_step_audio converts and
 * packs the front end's power-mel in phase 0 of the program instead of inside the front-end launch + on the channel encoder's
 * operand fragments), "train_colsum_gemm" (its column sums as ones-vector products on the matrix pipe), "train_no_ln_fuse" (a LayerNorm phase
 * instead of LayerNorm in the readers of the channel encoder's output) / "train_ln_fuse_rows" (the batch size, in key rows, up to which the readers do it).  A handle's switches start from the environment
 * variables KM_<NAME> read ONCE in km_create; no launch path reads the environment.  Unknown name: KM_ERR_INVALID_ARG. */
int km_set_option(km_handle h, const char* name, int64_t value);

/* ---- introspection used by the tests ------------------------------------------------- */
/* Copy a named host-side folded/packed buffer (after km_finalize_host) into out; returns its
 * length in floats via *n when out == NULL. */
int km_debug_buffer(km_handle h, const char* name, float* out, int64_t* n);
/* Which core the forward calls of a dual-stream handle run behind the front end (km_core_forward, km_forward_audio, the generic
 * branch of km_sequence_forward*), for the handle's shape and its switches as they stand; with_attention != 0: when the caller
 * asks for the attention map.  Host only, valid after km_finalize_host.  0: the fused d_model 256 / window 256 core; 1:
 * core512_kernel (d_model 512, 8 or 16 heads); 2: core256w_kernel (d_model 256, 8 heads, window 512, 80 channels -- the shape
 * of the reference's frame_rate=60 recipe); 3: the launch-per-product chain; 4: core128_kernel (d_model 128, 4 heads, window 128 or
 * 256, 80 channels -- the `fast` and `basic` variants -- with option core128 set; the default there is 3).  A call that asks for the
 * map takes 3 at every generic shape.  Negative: an error code. */
int km_core_route(km_handle h, int32_t with_attention);
/* The schedule km_sequence_forward / _track / _attn run for B clips of L samples at stride_frames, for the handle's shape, front end
 * and switches as they stand (with_attention != 0: the call asks for maps or brings an accumulator).  Host only, valid after
 * km_finalize_host; nothing is launched or allocated.  out[0] route: 0 per window (every window's T + 1 STFT frames); 1 the clip's
 * STFT once + two boundary frames per window, both images read by the fused core (the fused shape with hop >= n_fft / 2, zero
 * padding); 2 the clip's STFT once + the edge frames of every window, assembled per tile into the front end's workspace for the
 * core behind km_forward_audio's power path (option "seq_assemble", any hop, the fused shape and every generic shape whose forward
 * call has a power path; zero padding, clips of at least one window).  out[1] N = km_sequence_num_outputs.  out[2] the STFT frames
 * the call's front-end launches compute in total, discarded rows included: B N (T + 1) on route 0, B (nfc + 2 N) on route 1 and
 * B (nfc + 3 E N) on route 2, nfc = (N - 1) stride_frames + T + 1.  out[3] E = ceil((n_fft / 2) / hop): the frames at either end of
 * a window that see its zero padding.  KM_ERR_INVALID_ARG: NULL argument, B, L or stride_frames <= 0. */
int km_sequence_plan(km_handle h, int64_t B, int64_t L, int32_t stride_frames, int32_t with_attention, int64_t out[4]);
/* The schedule km_train_step_clip (training = 1), km_forward_clip (0) or km_forward_clip_attn (2) runs for B windows whose start
 * frames lie in [min_start_frame, max_start_frame], for the handle's shape, front end and switches as they stand.  Host only, valid
 * after km_finalize_host; nothing is launched or allocated.  out[0] route: 0 the call is refused (the Python wrappers gather the
 * windows: km_gather_windows + the from-audio call); 1 the default shared route (the span once + frames 0 and T of every window:
 * hop >= n_fft / 2, the packing front end for training, the fused core for the forward calls), whatever option "clip_assemble"
 * says; 2 option "clip_assemble" on a handle route 1 does not cover: the span once + two snippets of 2 E frames per window, then
 * the packed training input (the packing 1024-point front end, zero padding, T + 1 >= 2 E) or the windows assembled into the front
 * end's workspace for the core behind km_forward_audio's power path (the fused shape below hop n_fft / 2, core512, core256w, core128
 * under option "core128", the chain where maps are asked for; zero padding, T + 1 >= 2 E).  out[1] the span rows max - min + T + 1.
 * out[2] the STFT frames the call's front-end launches compute: B (T + 1) gathered, span + 2 B on route 1, span + 4 E B on route 2.
 * out[3] E = ceil((n_fft / 2) / hop).  km_train_clip_supported / km_forward_clip_supported answer 1 on routes 1 and 2.
 * KM_ERR_INVALID_ARG: NULL argument, B <= 0, min_start_frame < 0, max_start_frame < min_start_frame, training outside 0 .. 2. */
int km_clip_plan(km_handle h, int64_t B, int32_t min_start_frame, int32_t max_start_frame, int32_t training, int64_t out[4]);

/* ---- window producer for sequence training -------------------------------------------------------------
 * Replaces the per-window host slicing + H2D copies of KoeMorphSequentialDataset (src/data/sequential_dataset.py:
 * 136-209) for clips and labels resident in HBM.
 *   km_resample_labels  labels recorded at another frame rate -> target rate, exactly as _resample_blendshapes
 *                       (:136-154): dst[t,k] = float32(np.interp(np.linspace(0, n_src-1, n_dst)[t], arange(n_src),
 *                       src[:,k])) evaluated in float64 like numpy (bit-identical); n_dst = int(n_src * target/source)
 *                       is the caller's (host) computation
 *   km_gather_windows   window b starts at frame start_frames[b]: audio_out (B, window_samples) =
 *                       clip[start*hop : +window_samples] (zero beyond the clip), labels_out (B, window_frames, dims) =
 *                       labels[start : +window_frames] (:181-188), target_out (B, dims) = the label of the window's
 *                       last frame; any of the three outputs may be NULL */
int km_resample_labels(const float* src_dev, int64_t n_src, int32_t dims, int64_t n_dst, float* dst_dev, void* stream);
int km_gather_windows(const float* clip_dev, int64_t clip_len, const int32_t* start_frames_dev, int64_t B, int32_t hop,
                      int64_t window_samples, float* audio_out_dev, const float* labels_dev, int64_t n_label_frames,
                      int32_t window_frames, int32_t dims, float* labels_out_dev, float* target_out_dev, void* stream);

/* ---- wire encoding (host only, no GPU) -----------------------------------------------------------------
 * Byte-identical replacement for the per-frame json.dumps of the reference's output side (scripts/rt.py:209-231:
 * UDP datagrams and JSONL lines; src/data/io.py:119-131: dataset labels):
 *     {"timestamp": <float>, "blendshapes": [<n_values floats>]}
 * frames_host (n_frames, n_values) fp32 on the host, timestamps (n_frames) as time.time() doubles; floats are printed as
 * CPython prints ndarray.tolist() values (shortest round-trip repr of the float32 widened to double, 'Infinity' /
 * 'NaN' as json.dumps spells them).  Frame f occupies out[offsets[f] .. offsets[f+1]) (offsets has n_frames + 1 entries,
 * may be NULL); newline != 0 appends '\n' to every frame (JSONL).  Returns the number of bytes written, or a negative
 * number -(n) when `capacity` is too small (n bytes are certainly enough), or KM_ERR_INVALID_ARG. */
int64_t km_format_frames(const float* frames_host, int64_t n_frames, int32_t n_values, const double* timestamps,
                         int32_t newline, char* out, int64_t capacity, int64_t* offsets);

#ifdef __cplusplus
}
#endif
#endif /* KOEMORPH_H */
