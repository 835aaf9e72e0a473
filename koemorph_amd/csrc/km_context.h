// Internal definitions shared by the translation units of libkoemorph_hip.so.
// Not part of the public ABI (that is include/koemorph.h).
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "koemorph.h"
#include "km_devbuf.h"

namespace km {

constexpr int kNumMouth = 28;   // dual_stream_attention.py:14-45 (MOUTH_INDICES)
constexpr int kNumExpr = 24;    // EXPRESSION_INDICES
extern const int kMouthIdx[kNumMouth];
extern const int kExprIdx[kNumExpr];

struct HostParam {
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool loaded = false;
};

// A named host buffer produced by folding/packing, mirrored 1:1 on the device.
struct Packed {
    std::vector<float> host;
    DevBuf<float> dev;
};

#ifndef KM_EMO_GROUP
#define KM_EMO_GROUP 2              /* A/B builds: -DKM_EMO_GROUP=1 .. 12 (measured: profiles/emotion_groups.txt) */
#endif
constexpr int kMelRpWaves = 8;      // waves per workgroup of mel_power_rp_kernel
constexpr int kMelRpGroups = 4;     // filter groups a wave can hold (8 x 4 x 4 = up to 128 filters)
constexpr int kMelEmoGroup = KM_EMO_GROUP;   // windows per emotion group workgroup of mel_power_rp_kernel (emotion_group_d256; 1, 2, 3, 4, 8 and 12 measured, 2 the fastest step: profiles/emotion_groups.txt)
constexpr int kMelRpRow = 580;      // power-row stride in dwords (4 mod 64: see the mel stage), >= fbg_extent

// Sparse triangular mel filterbank + window for one front-end configuration.
struct MelPlan {
    km_mel_config cfg{};
    int n_freq = 0;                 // n_fft/2 + 1
    std::vector<float> window;      // n_fft, periodic Hann (optionally / sqrt(sum w^2))
    std::vector<float> twiddle;     // n_fft complex (cos, -sin) pairs: W_N^p
    std::vector<int32_t> fb_start;  // n_mels: first FFT bin with non-zero weight
    std::vector<int32_t> fb_count;  // n_mels: number of bins
    std::vector<int32_t> fb_offset; // n_mels: offset into fb_weight
    std::vector<float> fb_weight;   // concatenated non-zero weights
    // the same filters for mel_power_rp_kernel (km_host.cpp build_mel_plan): groups of four consecutive filters dealt to
    // the workgroup's waves (balanced by length); a lane owns one (frame, filter) pair and walks the filter four bins a step
    std::vector<int32_t> fbg_gid;   // [wave][slot]: group (filters 4 gid .. 4 gid + 3) or -1
    std::vector<int32_t> fbg_desc;  // [wave][slot][filter in group]: first bin / 4 | steps << 8 | tap offset (float4) << 16
    std::vector<float> fbg_weight;  // four taps x 1/4 per (filter, step), zero padded to the group's step count
    int fbg_extent = 0;             // 1 + the highest bin a step reads (the power rows are padded with zeros up to it)
    // device mirrors
    DevBuf<float> d_window, d_twiddle;
    DevBuf<int32_t> d_fb_start, d_fb_count, d_fb_offset;
    DevBuf<float> d_fb_weight;
    DevBuf<int32_t> d_fbg_gid, d_fbg_desc;
    DevBuf<float> d_fbg_weight;
    bool uploaded = false;          // set by upload_mel_plan once every mirror exists
};

// Run-time switches (km_set_option).  Seeded ONCE per handle, at creation, from the KM_* environment variables of
// the same name in upper case (tools/ab_*.sh); nothing on a launch path reads the environment.
struct Options {
    int core_split = 0;            // 3 / 6: split-bf16 variant of the fused core (experimental, never the default)
    int seq_per_window = 0;        // 1: sequence mode recomputes every window's STFT (the reference's schedule)
    int seq_assemble = 0;          // 1: sequence mode computes each clip's STFT once at every shape and hop whose forward call has a power path, and assembles the windows into the workspace (km_seq_assemble.hip; km_sequence_plan route 2)
    int clip_assemble = 0;         // 1: km_train_step_clip / km_forward_clip / km_forward_clip_attn also run on the handles they refuse by default (hop below n_fft / 2, no fused core): span image + E edge rows a side per window, packed or assembled into the workspace (km_clip_assemble.hip; km_clip_plan route 2)
    int generic_staged = 0;        // 1: generic core from a staged log-mel image instead of the power-mel workspace
    int mel_two_frame = 0;         // 1: two-frames-per-wave front end (A/B baseline)
    int emotion_separate = 0;      // 1: emotion logits in their own kernel
    int emotion_rider = 0;         // 1: d_model 256: the front end's per-window emotion rider instead of its group workgroups (A/B, and the tests' bit-identity witness)
    int no_ln_fusion = 0, no_db_fusion = 0, no_score_fusion = 0, no_out_fusion = 0, no_v_fusion = 0;   // generic chain A/B
    int legacy_no_merge = 0;       // 1: the legacy model's attention and tail as two launches instead of one (legacy_attn_tail_kernel)
    int no_core_merge = 0;         // 1: the d_model 512 core as its three launches (encoder + LayerNorm, scores, output) instead of one workgroup per window walking the three stages (core512_kernel); d_model 256 / window 512: the launch-per-product chain instead of core256w_kernel
    int core128 = 0;               // 1: the forward calls at d_model 128 / 4 heads / window 128 or 256 run core128_kernel (route 4) instead of the launch-per-product chain; the streams at those shapes run core128_stream_kernel either way
    int legacy_no_tail_fusion = 0; // 1: SimplifiedKoeMorphModel out_proj + decoder as four GEMM launches + a row kernel (A/B, tests)
    int legacy_no_enc_fusion = 0;  // 1: SimplifiedKoeMorphModel audio encoder + key / value projections as four GEMM launches (A/B, tests)
    int legacy_no_attn_fusion = 0; // 1: SimplifiedKoeMorphModel attention as two batched strided products + a row softmax (A/B, tests)
    int kmm_no_fuse = 0;           // 1: KoeMorphModel as the launch-per-step chain even at the fused kernels' width (A/B, tests)
    int train_no_split = 0;        // 1: no split-K of the long gradient products of the training step (A/B)
    int train_split_min_k = 0;     // > 0: split gradient products longer than this many rows into chains of about this length (A/B; default 1024 / 640)
    int train_alone_max = 0;       // > 0: a phase of up to this many workgroups gives its 32-row LDS-DMA tiles the 8-stage ring (default 256)
    int train_no_dy_split = 0;     // 1: dY = dKV Wkv as one product at every batch size (A/B of the two K halves summed by the LayerNorm backward); 2: two halves at every batch size (measured: 16 windows 0.1401 -> 0.1422 ms, 64: 0.2299 -> 0.2327)
    int train_ln_fuse_rows = 0;    // > 0: LayerNorm by the reader up to this many key rows per step (default 3200 = 40 windows of 80 channels)
    int train_no_ln_fuse = 0;      // 1: the training program keeps its LayerNorm phase (P2) instead of normalising in the readers of Y0 / E0 (LnXform)
    int train_colsum_gemm = 0;     // 1: column sums of the training program as products with a ones vector on the matrix pipe (rounds 2-4a) instead of OP_COLSUM
    int train_no_fe_pack = 0;      // 1: km_train_step_audio converts and packs the power-mel in phase 0 of the program (round 3/4 form) instead of inside the front-end launch
    int train_attn_regs = 0;       // 1: the attention blocks of the training program as the register-staged blocks of round 3 (A/B of the LDS-DMA blocks)
    int train_no_dma = 0;          // 1: the products of the training program run on the register-staged tile only (A/B of the LDS-DMA tile, km_gemm_dma_dev.h)
    int train_op_per_launch = 0;   // 1: every operation of the training program is its own launch (timing aid: rocprofv3 then shows each operation)
    int train_bm32_below = 0;      // > 0: products with fewer 64-row tiles than this run on 32-row tiles (A/B; default 192)
    int train_tail_groups = 0;     // > 0: workgroups of the loss tail (A/B; default: one per 4 windows, at most 32)
};
void options_from_env(Options& o);
int set_option(struct Context* c, const char* name, long long value);

// hipFuncSetAttribute applies to the CURRENT device: one bit per device and call site, not one per process
struct PerDeviceOnce {
    unsigned long long seen[4] = {0, 0, 0, 0};
    bool first(int device) {
        if (device < 0 || device >= 256) return true;
        const unsigned long long bit = 1ull << (device & 63);
        if (seen[device >> 6] & bit) return false;
        seen[device >> 6] |= bit;
        return true;
    }
};

// ---- the device memory of a handle, grouped by what is torn down and rebuilt as a unit: the reset of a group is the assignment of
// a fresh value (c->st = Streams{}), teardown is the destructor (km_devbuf.h) ----

// km_reserve
struct Workspace {
    int64_t windows = 0, samples = 0, frames = 0;
    int mels = 0;                  // mel bins per frame the power-mel / log-mel / short-term workspaces were sized for
    DevBuf<float> zemo;            // (windows)             emotion-stream logit
    DevBuf<float> zemo_win;        // (windows)             per-window copy of per-clip logits (generic sequence mode)
    DevBuf<float> melpow;          // (windows, frames, 80) power-mel
    DevBuf<unsigned> melmax;       // (windows)             max power (float bits)
    DevBuf<float> mel;             // (windows, frames, 80) log-mel
    DevBuf<float> mel_short;       // (windows, 3, 80)
    DevBuf<float> generic;         // generic (non-fused) core intermediates, generic_ws_floats() per window; KoeMorphModel: km_koemorph_reserve
};

// chunk FIFOs in front of the rings (km_stream_fifo_create / _feed / _step): one consuming FIFO per stream (RingBuffer
// semantics, scripts/rt.py:48-99), popped one frame per step straight into the stream's ring; len == 0 until created
struct ChunkFifos {
    int64_t len = 0; int frame = 0;
    DevBuf<float> samples;               // (n_streams, len)
    DevBuf<int> state;                   // (3, n_streams): write_ptr | read_ptr | available
    DevBuf<unsigned char> fire;          // (n_streams) this step popped a frame AND the ring is full: the gate of km_stream_step
};

// streaming state (km_stream_*): device-resident per-stream audio rings (MelAudioBuffer semantics); n_streams == 0 until created
struct Streams {
    int64_t n_streams = 0, ring_len = 0;
    int ring_hop = 0;
    DevBuf<float> ring;                  // (n_streams, ring_len)
    DevBuf<int> ring_wptr;               // (n_streams) write pointer == chronological start once full
    DevBuf<int> ring_frames;             // (n_streams) frames added
    DevBuf<unsigned char> ring_ready;    // (n_streams) is_full
    DevBuf<unsigned char> ring_started;  // (n_streams) EMA state valid
    DevBuf<float> ring_state;            // (n_streams, 52) EMA state
    MelPlan* plan = nullptr;
    int64_t out_frames = 0;
    ChunkFifos fifo;
};

// streaming state of the legacy model (km_legacy_stream_*): device-resident consuming FIFOs (RingBuffer semantics,
// scripts/rt_simplified.py:46-97); grow-only buffers, streams == 0 until km_legacy_stream_create
struct LegacyFifos {
    int64_t streams = 0, len = 0, window = 0;
    DevBuf<float> fifo;                  // (streams, len) samples
    DevBuf<int> state;                   // (3, streams): write_ptr | read_ptr | available
    DevBuf<float> stage;                 // (streams, window) the popped windows, chronological
    DevBuf<unsigned char> ready;         // (streams) this tick popped a window
    DevBuf<float> attn;                  // (streams, 52, 256) attention output of legacy_stream_kernel
};

// training state (km_train_* / km_legacy_train_*): flat fp32 master parameters + AdamW moments on the device, in state-dict order
struct TrainState {
    int64_t nparams = 0, windows = 0;
    int64_t early = 0;               // floats [0, early) of the gradient bucket are final when early_ev fires
    DevEvent early_ev;               // recorded by the step after the last phase that writes an early gradient
    bool early_recorded = false;
    std::map<std::string, int64_t> offset;
    DevBuf<float> params, m, v;
    DevBuf<float> wcep;              // (d, KP) the channel encoder weight with rows padded to KP floats (zeros): written with params (upload, AdamW)
    DevBuf<float> part, gnorm, loss;
    DevBuf<int> steps;               // device-side AdamW step counters (graph replay safe)
    // training step (km_trainp.hip): activation workspace, dropout masks and per-step mask counter
    DevBuf<float> act;
    DevBuf<float> split;             // partial outputs of the split-K gradient products of one step
    DevBuf<float> tail_part; DevBuf<unsigned> tail_ctr;   // per-workgroup sums of the loss tail + its arrival counter
    DevBuf<unsigned char> masks;     // mel (W,H,28,NK) | emo (W,H,24) | dec (W,52,DH), W = windows
    DevBuf<int> drop_ctr;            // device-side step counter of the mask generator (graph-replay safe)
    // training step of the legacy model (km_legacy_train.hip); parameters, moments and counters are the ones above
    DevBuf<float> l_ws;              // activations and their gradients, carved for (windows, l_frames)
    int64_t l_frames = 0;
    DevBuf<float> l_part;            // split-K partials of one weight gradient, then of its bias gradient
    DevBuf<unsigned char> l_masks;   // keep flags: enc1 | enc2 | attn | dec1 | dec2, packed for the step's (B, T)
    int64_t l_mask_B = 0, l_mask_T = 0;   // the (B, T) the masks on the device belong to
    // training from a resident clip (km_train_step_clip): power-mel of the clip span the batch touches (clip_span_rows, NK), then
    // (clip_edge, a view into the same allocation) every window's two zero-padded boundary frames (windows, 2, NK); sized by
    // km_train_init, the span grow-only afterwards
    DevBuf<float> clip_span; float* clip_edge = nullptr;
    int64_t clip_span_rows = 0;
};

// grow-only images of sequence mode and of the eval-mode forward from a resident clip
struct SeqBufs {
    // shared-frame sequence mode (km_sequence_forward): the clip image and its per-row maxima; the edge image and its maxima --
    // (windows, 2, NK) read by the fused core, or on the assembled route (windows, E, NK) left edges followed by E images of
    // (windows, 2, NK) right edges
    DevBuf<float> pow; DevBuf<unsigned> fmax; DevBuf<float> edge; DevBuf<unsigned> emax;
    // km_sequence_forward_track: the logits of the track's rows (clips * K) and of the sequence's windows (clips * N)
    DevBuf<float> ztrack, zwin;
    // km_sequence_forward_attn with an accumulator and no caller's map: the maps of ONE tile (ws.windows, 28, NK)
    DevBuf<float> attn;
    // km_forward_clip: the span image (rows, NK) and the edge image (windows, 2, NK) of launch_mel_clip_span, owned by the
    // inference context (no km_train_init needed)
    DevBuf<float> fwd_span, fwd_edge;
};

// grow-only images of the resident-clip calls on their assembled route (option clip_assemble, km_clip_assemble.hip)
struct ClipAsmBufs {
    DevBuf<float> span; DevBuf<unsigned> smax;   // (n_span, NK) clip frames min_start .. max_start + T and their per-row maxima
    DevBuf<float> snip;                          // (2 windows, Ls rounded up to 4) the first / last Ls = (2 E - 1) hop samples of every window
    DevBuf<float> edge; DevBuf<unsigned> emax;   // (2 windows, 2 E, NK) the snippets' frames and their per-row maxima
};

// km_koemorph_rollout_reserve: workspace of km_koemorph_rollout (km_koemorph_rollout.hip carves it), one allocation
struct RolloutBufs {
    int64_t clips = 0, context = 0, chunk = 0;   // what it was sized for; clips == 0 until reserved
    DevBuf<float> ws;
};

// km_koemorph_stream_create: the stream engine of a KoeMorphModel handle (km_koemorph_stream.hip); streams == 0 until created
struct KoeMorphStreams {
    int64_t streams = 0, context = 0, max_rows = 0, cap = 0, state_floats = 0;
    int smoothing = 0, constraints = 0;
    DevBuf<float> ring_mel, ring_emo;    // (streams, cap, mel_dim / emotion_dim) the last cap = context - 1 + max_rows rows, positions wrap
    DevBuf<long long> counter;           // (streams) frames since the stream's reset
    DevBuf<int> nstep;                   // (streams) frames of the current step
    DevBuf<float> prev, state;           // (streams, 52) the last rendered frame; (streams, state_floats) the smoother state
    DevBuf<int> table;                   // (streams * max_rows, 4) the step's window table (KmsWindow, km_kmmf.hip)
    DevBuf<float> xm, xe;                // (streams * max_rows, context, 256) encodings of the step's windows
};

// km_koemorph_audio_create: the audio front of the stream engine (km_koemorph_audio.hip); streams == 0 until created
struct EgmPlanDelete { void operator()(void* p) const; };   // km_egemaps_plan_destroy
struct KoeMorphAudio {
    int64_t streams = 0, max_samples = 0, ring_len = 0, W = 0, max_nf = 0, max_rows = 0;
    int hop = 0, rows_tile = 0, feature_set = 0;
    std::unique_ptr<MelPlan> mel;                // the 512-point plan of the stream's frame rate: owned here, so destroy frees its mirrors
    std::unique_ptr<void, EgmPlanDelete> egm;    // km_egemaps_plan_create
    DevBuf<float> ring;                          // (streams, ring_len) sample i of a life at i mod ring_len
    DevBuf<long long> total;                     // (streams) samples since the stream's reset
    DevBuf<int> origin;                          // (streams) ring index of the life's sample 0
    DevBuf<char> table, slots;                   // (streams) KmaEntry / EgmSlot of the push (km_koemorph_audio.h)
    DevBuf<float> scale, rec;                    // (streams), (streams, max_nf, 36): the ragged eGeMAPS kernels' peak scales and frame records
};

// two-deep pipeline across calls (km_forward_audio_pipelined)
struct PipeSlot {
    DevBuf<float> melpow; DevBuf<unsigned> melmax; DevBuf<float> zemo;
    bool dirty = true;
};
struct Pipeline {
    DevStream s1, s2;              // front end / core
    DevEvent ev_in[2], ev_mel[2], ev_core[2];
    PipeSlot slot[2];
    int64_t seq = 0, windows = 0, frames = 0;
};

struct Context {
    km_config cfg{};
    Options opt{};
    int kind = 0;                                // 0 dual-stream production model, 1 legacy SimplifiedKoeMorphModel, 2 legacy KoeMorphModel
    int legacy_hidden = 128;
    km_koemorph_config kmm{};                    // kind 2
    int64_t kmm_batch = 0, kmm_frames = 0;       // kind 2: reserved workspace (ws.generic)
    bool legacy_tail_fused = false;              // kind 1: the blob of legacy_tail_kernel exists as well (decoder 128 wide, 52 queries)
    bool legacy_fused = false;                   // kind 1: the blob of legacy_encoder_kernel exists (d_model 256, 80 mel bins, 8 heads)
    bool kmm_fused = false;                      // kind 2: the model has the width of the fused kernels (km_kmmf.hip) and their blobs exist
    int d = 0, H = 0, hd = 0, T = 0, KT = 0, ED = 0, DH = 0, NB = 0, NK = 0;
    std::map<std::string, HostParam> params;     // reference state-dict tensors (fp32 masters)
    std::vector<std::string> param_order;
    std::map<std::string, Packed> packed;        // folded / packed buffers
    bool host_finalized = false;
    bool dev_finalized = false;
    bool fused_ok = false;                       // (d,T,H) has the fused gfx950 kernel
    float alpha = 0.0f;                          // sigmoid(smoothing_alpha)
    int device = -1;

    std::vector<MelPlan*> mel_plans;             // [0] = cfg.mel

    DevBuf<unsigned> ws_chunkctr;                // chunk requests per window of mel_power_rp_kernel: zero between launches; outlives km_reserve
    Workspace ws;                                // km_reserve
    Streams st;                                  // km_stream_*
    LegacyFifos lf;                              // km_legacy_stream_*
    TrainState tr;                               // km_train_init / km_legacy_train_init
    bool tr_alpha_live = false;      // smoothing_alpha was in the last step's graph (see adamw_kernel)
    // settings of the training step: they outlive a second km_train_init / km_legacy_train_init
    km_loss_config tr_loss_cfg{};    // extra KoeMorphLoss terms (all weights 0 = off)
    float tr_dropout_p = 0.f;        // training-mode dropout probability (0 = eval-mode arithmetic)
    int tr_dropout_mode = 0;         // 0: masks drawn per step (Philox), 1: masks supplied by the caller (km_train_set_dropout_masks)
    unsigned long long tr_dropout_seed = 0;
    SeqBufs seq;                                 // km_sequence_forward*, km_forward_clip
    ClipAsmBufs clipasm;                         // km_train_step_clip / km_forward_clip with option clip_assemble
    Pipeline pipe;                               // km_forward_audio_pipelined
    RolloutBufs ro;                              // kind 2: km_koemorph_rollout
    KoeMorphStreams ks;                          // kind 2: km_koemorph_stream_*
    KoeMorphAudio ka;                            // kind 2: km_koemorph_audio_*
    bool stage_timing = false;
    DevEvent stage_ev[6];                        // emo b/e, mel e, core b/e
    bool melmax_dirty = true;      // ws.melmax may hold stale maxima (see launch_mel_power)

    Context() = default;
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ~Context() { for (MelPlan* p : mel_plans) delete p; }   // everything else frees itself (km_devbuf.h)
};

void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);   // (also declared by km_devbuf.h)

// km_host.cpp
int finalize_host(Context* c);
MelPlan* build_mel_plan(const km_mel_config& cfg);
MelPlan* find_or_add_plan(Context* c, const km_mel_config& cfg);

// km_core.hip
int launch_emotion(Context* c, const float* emo, int64_t B, float* zemo, void* stream);
int launch_core_fused(Context* c, const float* mel, int64_t B, int64_t T_in, const float* mel_short,
                      const float* zemo, float* out, float* raw, float* attn, float* state, int first,
                      void* stream);
// fused variant: reads the workspace power-mel + window maxima, applies the log/dB conversion on load.  CoreSrc says where
// the B windows' rows and their EMA come from (CoreArgs in km_core.hip): build one with the functions below it
struct SeqCore {          // shared-frame sequence mode: frame f of window i of a clip is row i stride + f of the clip's image
    const float* pow;     // (clips, nfc, 80) clip-level power-mel
    const float* edge;    // (clips * n_per_clip, 2, 80) first / last frame of every window
    int nfc, stride, n_per_clip;
};
struct ClipTable {        // km_forward_clip: rows addressed by a start-frame table
    const float* span;    // (n_span, 80) ONE span image, row r = clip frame min_start + r
    const float* edge;    // (windows, 2, 80)
    int n_span;
    const int* start; int min_start;   // (windows) window b begins at row start[b] - min_start
};
struct CoreSrc {
    float* state; int first;                 // EMA state (B, 52) or null
    int64_t win0; int zemo_div;              // sequence mode: window b of the launch takes the logit zemo[(win0 + b) / zemo_div]
    int64_t n_use;                           // streams: frames kept by the truncate / repeat-last policy (0: all)
    const unsigned char* ready; unsigned char* started;   // streams: windows with ready[b] == 0 are skipped, first = !started[b]
    const SeqCore* seq;                      // rows of the strided images instead of the workspace, or null
    const ClipTable* tab;                    // ... of the span image through the table, or null
    float* raw; float* attn;                 // (B, 52) / (B, 28, 80) rows of window 0 of the launch, or null (with_outputs)
};
// rows of the workspace (launch_mel_power wrote them), the caller's EMA state
inline CoreSrc core_workspace(float* state, int first) { return {state, first, 0, 1, 0, nullptr, nullptr, nullptr, nullptr}; }
// ... for windows win0 .. of a sequence, n_per_clip of them sharing a clip's logit; no EMA here (launch_ema_scan follows)
inline CoreSrc core_workspace_seq(int64_t win0, int n_per_clip) { return {nullptr, 1, win0, n_per_clip, 0, nullptr, nullptr, nullptr, nullptr}; }
inline CoreSrc core_strided(const SeqCore* s, int64_t win0) { return {nullptr, 1, win0, s->n_per_clip, 0, nullptr, nullptr, s, nullptr}; }
// ... the same two sources with a logit per WINDOW of the sequence (km_sequence_forward_track: zemo is (clips * n_per_clip))
inline CoreSrc core_workspace_seq_win(int64_t win0) { return {nullptr, 1, win0, 1, 0, nullptr, nullptr, nullptr, nullptr}; }
inline CoreSrc core_strided_win(const SeqCore* s, int64_t win0) { return {nullptr, 1, win0, 1, 0, nullptr, nullptr, s, nullptr}; }
inline CoreSrc core_table(const ClipTable* t, float* state, int first) { return {state, first, 0, 1, 0, nullptr, nullptr, nullptr, t}; }
// the handle's streams: rows of the workspace, EMA state and flags of the rings
// (gate: the per-stream flags the kernel skips on -- is_full for km_stream_tick, this step's fire flags for km_stream_step)
inline CoreSrc core_stream(Context* c, const unsigned char* gate = nullptr) {
    return {c->st.ring_state, 0, 0, 1, c->st.out_frames, gate ? gate : c->st.ring_ready, c->st.ring_started, nullptr, nullptr};
}
// any of the sources above with the pre-weight sigmoid values and / or the head-averaged attention map written as well (attn set:
// the ATTN instantiation of the same source; the split-bf16 variants have none and refuse)
inline CoreSrc with_outputs(CoreSrc s, float* raw, float* attn) { s.raw = raw; s.attn = attn; return s; }
int launch_core_fused_db(Context* c, MelPlan* p, int64_t B, int64_t n_frames, const float* zemo, float* out, void* stream,
                         const CoreSrc& src);
int launch_seq_window_max(Context* c, const unsigned* fmax, const unsigned* emax, int64_t nw, int64_t win0, int nfc, int stride,
                          int n_per_clip, int n_frames, void* stream);
// km_forward_clip: the maximum over each window's OWN n_frames rows of the span / edge images (found through the table) -> ws.melmax
int launch_clip_window_max(Context* c, const float* span, const float* edge, const int* start, int64_t B, int min_start,
                           int64_t n_span, int n_frames, void* stream);
int launch_ema_scan(Context* c, float* x, int64_t B, int64_t N, void* stream);
int launch_smooth(Context* c, float* x, float* state, int64_t B, int first, void* stream);

// km_train.hip
int train_refresh_padded_weights(Context* c, void* stream);
int train_adamw(Context* c, const float* flat_grad, float lr, float b1, float b2, float eps, float wd, float max_norm,
                int64_t step, void* stream);

// km_trainp.hip
int64_t trainp_act_floats(Context* c, int64_t* fixed);
int64_t trainp_kp(Context* c);
int64_t trainp_mask_alloc_bytes(Context* c, int64_t windows);
int trainp_mask_sizes(Context* c, int64_t B, int64_t* mel, int64_t* emo, int64_t* dec);
int trainp_copy_masks(Context* c, int64_t B, unsigned char* mel, unsigned char* emo, unsigned char* dec, int to_device, void* stream);
// from-audio training step: the front end's power-mel + window maxima, converted and packed by phase 0 of the program
struct LogParams;
// packed: the front end wrote 10 log10(power) into the packed input itself (MelPack); the readers finish the dB conversion
struct TrainAudioSrc { const float* melpow; const unsigned* melmax; int n_frames; const LogParams* lp; bool packed; };
// what km_train_step, km_train_step_audio and km_train_step_clip hand through unchanged from their own arguments
struct TrainStepArgs {
    const float* emo; const float* target; float mse_w, l1_w; float* flat_grad; float* loss_dev; float* out_dev;
    float* ema_state; int ema_first; void* stream;
};
int train_forward_backward(Context* c, const float* mel, int64_t B, int64_t T_in, const float* mel_short, const float* xp_dev,
                           const TrainAudioSrc* asrc, const TrainStepArgs& a);
int launch_audio_energy(const float* feats, int64_t B, int64_t T, int64_t D, float* out, void* stream);

// km_legacy_train.hip
bool legacy_train_supported(Context* c);
int legacy_train_init(Context* c, int64_t max_windows, int64_t max_frames, void* stream);
float* legacy_train_mel_buffer(Context* c);
int legacy_train_step(Context* c, const float* mel, int64_t B, int64_t T, const float* target, float mse_w, float l1_w, float* grad,
                      float* loss_dev, float* out_dev, void* stream);
int legacy_train_copy_masks(Context* c, int64_t B, int64_t T, unsigned char* const host[5], int to_device, void* stream);

// km_generic.hip
int64_t generic_ws_floats(Context* c);
int64_t legacy_ws_floats(Context* c, int64_t frames);
int finalize_host_legacy(Context* c);
int finalize_host_koemorph(Context* c);
int64_t koemorph_ws_floats(Context* c, int64_t T);
int reserve_koemorph(Context* c, int64_t max_batch, int64_t max_frames);     // km_api.hip: what km_koemorph_reserve does behind its guards
int launch_koemorph(Context* c, const float* mel, const float* emo, int64_t B, int64_t T, const unsigned char* kvalid, const float* prev,
                    float* state, int apply_constraints, float* out, float* raw, float* attn, void* stream);
struct LegacyPowSrc { const float* melpow; unsigned* melmax; const LogParams* lp; };      // the front end's power-mel as the legacy model's input
bool legacy_pow_ok(Context* c);
int launch_legacy(Context* c, const float* mel, int64_t B, int64_t T_mel, float* out, void* stream, const LegacyPowSrc* pow_src = nullptr);
int launch_gather_clip_logits(Context* c, const float* zclip, float* zwin, int64_t nw, int64_t w0, int wins_per_clip, void* stream);
// km_sequence_forward_track: window j of clip c ends at e = min(clip_len, sample_offset + j step + window) and takes the logit of
// track row k = e < first ? 0 : min((e - first) / interval, K - 1): zwin[c n_per_clip + j] = ztrack[c K + k]
struct SeqTrackMap { int64_t K, first, interval, sample_offset, clip_len, step, window; };
int launch_seq_track_logits(Context* c, const float* ztrack, float* zwin, int64_t total, int n_per_clip, const SeqTrackMap& m, void* stream);
int launch_core_generic_packed(Context* c, const float* xp, int64_t B, const float* zemo, float* out, float* raw, float* attn,
                               void* stream);
float* generic_packed_x(Context* c, int64_t B);
int launch_core_generic_power(Context* c, MelPlan* plan, int64_t B, int64_t n_frames, const float* zemo, float* out,
                              float* raw, float* attn, void* stream);
int launch_core_generic(Context* c, const float* mel, int64_t B, int64_t T_in, const float* mel_short, const float* zemo,
                        float* out, float* raw, float* attn, void* stream);
// the streams on the shapes with a one-launch generic core (d_model 512 / 8 or 16 heads; 256 / 8 heads / window 512; 128 / 4 heads /
// window 128 or 256): the shape's streaming kernel over the rings' power-mel.  raw (S, 52) / attn (S, 28, 80, 16-byte aligned) or
// null: the pre-weight sigmoid values and the head-averaged map of the computed streams
int launch_core_stream(Context* c, MelPlan* plan, int64_t S, int64_t n_frames, const float* zemo, float* out, void* stream,
                       const unsigned char* gate = nullptr, float* raw = nullptr, float* attn = nullptr);
// the handle's shape has a streaming core: the fused one (d_model 256, 8 heads, window 256) or one of those
bool stream_core_ok(Context* c);
// the forward calls have a power path: the fused core, or a generic core that reads the power-mel workspace and converts to dB itself
bool core_takes_power(Context* c, bool with_attention);
// ... and the core on it, for the B windows whose rows and maxima are in the workspace: the fused core with `src` as it is; on the
// generic shapes the logits src.win0 / src.zemo_div names (gathered into ws.zemo_win unless the divisor is 1), then the streaming
// core for a stream source, else launch_core_generic_power with src.raw / src.attn and launch_smooth where src.state is set
int launch_core_power(Context* c, MelPlan* plan, int64_t B, int64_t n_frames, const float* zemo, float* out, void* stream, const CoreSrc& src);
// km_core_route: 0 fused d_model 256 core, 1 core512_kernel, 2 core256w_kernel, 3 the launch-per-product chain, 4 core128_kernel
int core_route(Context* c, bool with_attention);

// km_mel.hip
// Shared-frame sequence mode: the front end writes n_rows rows per window (row r = STFT frame r * frame_mul) into
// `pow` and the per-row maxima (float bits, zero-initialised by the caller) into `fmax`, instead of the workspace.
struct SeqFrames {
    float* pow;        // (B, n_rows, n_mels)
    unsigned* fmax;    // (B, n_rows)
    int64_t n_rows;
    int frame_mul;
};
// packed training input written by the front end itself (MelArgs::pack_*): xt (B, n_mels, KP), T long frames per row
struct MelPack { float* xt; int T, KP; };
// Where a front-end launch takes its B windows of L samples from; build one with the functions below.
struct MelSrc {
    const float* audio; int64_t B, L;
    int64_t clip_len, win_step, win0; int wins_per_clip;      // window w is global window g = win0 + w: clip g / wins_per_clip, offset (g % wins_per_clip) win_step
    const int* ring_start; const unsigned char* ready;        // rings: window b is read from ring_start[b] (mod L), skipped while ready[b] == 0
};
inline MelSrc mel_windows(const float* audio, int64_t B, int64_t L) { return {audio, B, L, L, 0, 0, 1, nullptr, nullptr}; }   // audio (B, L)
// windows win0 .. win0 + B - 1 of L samples cut from clips (n, clip_len), wins_per_clip per clip, win_step samples apart (zero past the clip's end)
inline MelSrc mel_clip_windows(const float* clips, int64_t clip_len, int64_t B, int64_t L, int64_t win_step, int64_t win0, int wins_per_clip) {
    return {clips, B, L, clip_len, win_step, win0, wins_per_clip, nullptr, nullptr};
}
inline MelSrc mel_rings(Context* c, const unsigned char* gate = nullptr) {
    return {c->st.ring, c->st.n_streams, c->st.ring_len, c->st.ring_len, 0, 0, 1, c->st.ring_wptr, gate ? gate : c->st.ring_ready};
}
// What a launch may carry, at most one of: the windows' emotion logits from the same kernel (mel_fuses_emotion, one window per clip)
// -- emo_group = 0: the per-window rider inside the last workgroup of each window; emo_group = kMelEmoGroup (d_model 256 / hidden
// 128 only: mel_emotion_grouped): ceil(B / emo_group) extra workgroups in front of the grid, one per group of windows --, rows into a
// SeqFrames image instead of the workspace (mel_rp_ok, no rings), the packed training input (mel_packs, a plain batch)
struct MelCarry { const float* emotion = nullptr; float* zemo = nullptr; const SeqFrames* seq = nullptr; const MelPack* pack = nullptr; int emo_group = 0; };
inline MelCarry mel_emotion(const float* emotion, float* zemo, int emo_group = 0) { return {emotion, zemo, nullptr, nullptr, emo_group}; }
inline MelCarry mel_to_frames(const SeqFrames* seq) { return {nullptr, nullptr, seq, nullptr, 0}; }
inline MelCarry mel_to_pack(const MelPack* pack) { return {nullptr, nullptr, nullptr, pack, 0}; }
int launch_mel_power(Context* c, MelPlan* p, const MelSrc& src, void* stream, const MelCarry& carry = {});
// true when launch_mel_power launches mel_power_rp_kernel, the row-parallel 1024-point kernel
bool mel_rp_ok(Context* c, MelPlan* p);
bool clip_frames_shared(Context* c, MelPlan* p);   // windows at multiples of the hop share the clip's STFT frames (km_mel.hip)
bool mel_packs(Context* c, MelPlan* p, int64_t n_frames, int64_t T);
// Training from a resident clip (km_train_step_clip).  Window b of the batch is samples [start[b] hop, + T hop) of the clip.
// launch_mel_clip_span: ONE front-end launch writes `span` (n_span, n_mels) = the power-mel of clip frames min_start ..
// min_start + n_span - 1 (frame f of window b is row start[b] - min_start + f for f = 1 .. T - 1) and `edge` (B, 2, n_mels) =
// frames 0 and T of every window, the two that see its zero padding.  launch_train_clip_pack: from both images the packed
// encoder input xt (B, n_mels, KP) as MelPack leaves it and the window maxima into ws.melmax.
int launch_mel_clip_span(Context* c, MelPlan* p, const float* clip, int64_t clip_len, const int* start_frames, int64_t B,
                         int min_start, int64_t n_span, int T, float* span, float* edge, void* stream);
int launch_train_clip_pack(Context* c, MelPlan* p, const float* span, const float* edge, const int* start_frames, int64_t B,
                           int min_start, int64_t n_span, int T, int KP, float* xt, void* stream);
bool mel_fuses_emotion(Context* c, MelPlan* p);
// true when that launch carries the logits in group workgroups (d_model 256 / hidden 128, unless the option emotion_rider asks for the rider)
bool mel_emotion_grouped(Context* c, MelPlan* p);
int mel_role_table(int64_t windows, int per_window, int group, int64_t n_ids, int32_t* out);   // km_mel_role_table
// the windows' emotion logits and their power-mel: one launch with the group workgroups or the rider where mel_fuses_emotion holds, else
// launch_emotion and the plain front end.  emo_done: recorded between the two (stage timing of the fused shape), or null
int launch_mel_power_with_logits(Context* c, MelPlan* p, const MelSrc& src, const float* emotion, float* zemo, void* stream,
                                 hipEvent_t emo_done = nullptr);
// ws.melmax all-zero ahead of launches that raise or store maxima in a freshly (re)allocated workspace (melmax_dirty)
int clear_stale_maxima(Context* c, void* stream);

// km_seq_assemble.hip
// Sequence mode, assembled route: windows win0 .. win0 + nw - 1 of `total` (n_per_clip per clip, `stride` frames apart) written into
// ws.melpow (nw, T + 1, NK) and their maxima stored into ws.melmax, from the clip image pow (clips, nfc, NK), the left-edge image
// left (total, E, NK: frames 0 .. E - 1 of every window) and the right-edge images right (E, total, 2, NK: row 1 of image j is
// frame T - j), with the per-row maxima the front end left beside each (float bits).  NK % 4 == 0, images 16-byte aligned.
struct SeqAssemble {
    const float* pow; const unsigned* fmax; const float* left; const unsigned* lmax; const float* right; const unsigned* rmax;
    int64_t total; int nfc, stride, n_per_clip, E, T;
};
int launch_seq_assemble(Context* c, const SeqAssemble& s, int64_t nw, int64_t win0, void* stream);
// ... and the two arrays of per-row maxima zeroed by one kernel launch ahead of the front-end launches that raise them
int launch_seq_zero_maxima(unsigned* fmax, int64_t n_fmax, unsigned* emax, int64_t n_emax, void* stream);
int ensure_chunk_counters(Context* c, int64_t windows, void* stream);

// km_clip_assemble.hip
// The schedule of a resident-clip call on B windows whose start frames lie in [min_start, max_start]; mode 0 km_forward_clip,
// 1 km_train_step_clip, 2 km_forward_clip_attn.  route 0: refused (the caller gathers the windows); 1: the default shared route
// (launch_mel_clip_span: n_span + 2 B frames); 2: option clip_assemble (n_span + 4 E B frames).
struct ClipPlan { int route, E; int64_t n_span, stft_frames; };
ClipPlan clip_plan(Context* c, int64_t B, int64_t min_start, int64_t max_start, int mode);
// the span and edge images of route 2 into c->clipasm (grow-only: refused inside a stream capture, before any launch)
int launch_clip_images(Context* c, MelPlan* plan, const float* clip, int64_t clip_len, const int* start_frames, int64_t B, int min_start,
                       int64_t n_span, int E, void* stream);
// ... from them ws.melpow (B, T + 1, NK) and ws.melmax (B), as launch_mel_power leaves them for the windows
int launch_clip_assemble(Context* c, const int* start_frames, int64_t B, int min_start, int64_t n_span, int E, void* stream);
// ... or the packed encoder input xt (B, n_mels, KP) as MelPack leaves it, and ws.melmax
int launch_clip_pack_edges(Context* c, MelPlan* p, const int* start_frames, int64_t B, int min_start, int64_t n_span, int E, int KP, float* xt,
                           void* stream);
int launch_ring_push(Context* c, const float* samples, int64_t n_per_stream, void* stream);

// km_legacy_stream.hip: the FIFOs of km_legacy_stream_* (Context::lf)
int launch_lfifo_push(Context* c, const float* samples, int64_t n_per_stream, const int* counts, void* stream);
int launch_lfifo_pop(Context* c, unsigned char* ready_out, void* stream);
// ... and the chunk FIFOs of km_stream_* (Context::st.fifo): write, pop one frame into the ring, reset the masked streams
int launch_sfifo_push(Context* c, const float* samples, int64_t n_per_stream, const int* counts, void* stream);
int launch_sfifo_pop_ring(Context* c, unsigned char* fire_out, unsigned char* ready_out, int* backlog_out, void* stream);
int launch_stream_reset_masked(Context* c, const unsigned char* mask, void* stream);
// km_kmmf.hip: SimplifiedKoeMorphModel behind the front end for every stream with ready[s] != 0, windows of Tm <= 32 frames
int launch_legacy_stream_model(Context* c, const float* melpow, unsigned* melmax, const unsigned char* ready, int64_t S, int Tm,
                               const LogParams& lp, float* O, float* out, void* stream);
// launch_mel_power + the log-mel image(s) / the packed log-mel image of the generic core; the window maxima are left at zero
int launch_mel(Context* c, MelPlan* p, const MelSrc& src, int64_t out_frames, float* mel_long, float* mel_short, void* stream);
int launch_mel_packed(Context* c, MelPlan* p, const MelSrc& src, float* xp, int T, int KP, void* stream);
int upload_mel_plan(MelPlan* p);

}  // namespace km

// the opaque handle type of the public header
struct km_context : public km::Context {};
