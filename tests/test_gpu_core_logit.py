"""The attention core pinned in LOGIT space against the float64 oracle, on every kernel path.

tests/test_gpu_core.py compares `blendshapes` = clamp(c_i sigmoid(z)) at 2e-6 absolute.  c_i = (softmax(mel_weights)_i +
softmax(emotion_weights)_i) / 2 is about 1/52 and the sigmoid's slope at most 1/4, so an error in the decoder logit z arrives
~200 times smaller: 2e-6 on the output admits 4e-4 on z, which is 1300 times the float32 rounding noise at `init` weights -- a
kernel that staged the three short-term frames in reverse order would pass there.  Here every case recovers the sigmoid value s
of EVERY coefficient (`raw` where the entry point returns it, otherwise out / c_i with c_i in float64; after an EMA, the EMA is
undone in float64 with the state read back from the device) and measures (oracle/core.py)

    e = |s - s64| / (s64 (1 - s64))              the first-order error of the logit, s64 from the float64 oracle
    a = |A - A64| / max_k A64                    per (window, query) row of the head-averaged attention map

THE BOUND: e <= K x max(yardstick, 2^-23) + R x 2^-24 / (1 - s64), entry by entry, and a <= K x max(yardstick, 2^-23) + 2^-24.
The yardstick is the largest e (a) of the float32 oracle -- torch's float32 restatement -- on the same parameters and inputs,
computed in the test; the last term is what float32 storage can add, a derived quantity and not a tolerance: R = 1 for `raw`
(the store of s), R = 3 for s recovered as out / c_i, where out = fl(c32 x s32) carries the rounding of s, the float32
representation of c_i and the rounding of the product (core.OUT_OVER_C_ROUNDINGS).  With R = 1 the recovery of the d512 / 16-head
golden, whose |z| reaches 8.13 (1 / (1 - s) = 3400), would sit at 1.7 x the bound on storage alone.
The floor 2^-23 is one float32 ulp at 1.  K = 4 (core_logit_cases.K), one value for the whole file: the kernels sum in another
order than torch (MFMA k-blocks, folded weights, a base-2 softmax, v_rsq_f32), and the first run on the MI355X showed up to 3.7
yardsticks in e and 3.1 in a (table below); 4 is the next whole number, and the largest that still lets every planted fault of
tests/test_oracle_core.py::test_planted_faults_break_the_bound_on_a_stand_in_kernel exceed the bound at `init` AND `trained`
weights (one value column x 1.001 at `init` weights is 1.2 x the bound at K = 4 and would pass at K = 8).  BOTH MARGINS ARE THIN:
4 against 3.72 observed on one side, a stand-in fault at 1.2 x the bound on the other.  A compiler or runtime update that reorders
one sum can move a case past the bound.  If that happens, measure, and give the path a derived term or fix the kernel; raising K
hides the smallest faults (see the planted-fault table below for what the file catches on real faulted builds).  The kernels are
deterministic, so the figures repeat bit for bit.  Every case asserts |z64| <= 8 so that 1 / (s (1 - s)) stays below 3000.
After an EMA the recovery itself rounds: y = alpha x + (1 - alpha) prev in float32 is three roundings of at most 2^-24 max(x,
prev) each plus the representation of alpha and 1 - alpha, so undoing it in float64 is exact to 5 x 2^-24 max(x, prev) / alpha;
that term, divided by c_i s64 (1 - s64), is added to the bound of those calls (EMA_ROUNDINGS below).

Inputs travel as views into larger NaN-filled allocations (a read outside a tensor meets NaN), rows of `mel` from T on are NaN
(a kernel that multiplied them by zero instead of skipping them would turn NaN), and the from-audio paths are compared with the
oracle fed the DEVICE's own features (Engine.mel_batch / mel_extract, which tests/test_gpu_mel_power.py pins), so that the core
is isolated from the front end.

Every case prints `CORELOGIT|group|case|gpu max e|yardstick e|e / bound|gpu max a|yardstick a|a / bound` before it asserts.

OBSERVED (MI355X, K = 4, floor 2^-23; "x yard" = largest GPU error / max(yardstick, floor), "/ bound" = largest error / its bound)
  group         lines  e x yard  e / bound  closest case in e                     a x yard  a / bound  closest case in a
  fused           147    2.41     0.601     sharp77 zeroch raw                      2.12     0.519     trained301 mel01
  fused t_in       60    3.72     0.379     trained t_in=255 out/c                  1.81     0.443     trained t_in=256
  emotion z        36    3.18     0.324     trained d64 ED256 core_forward_z
  forward_audio    48    3.18     0.363     init click first
  stream            8    2.76     0.383     S=300 push 256 first
  sequence          8    0.82     0.199     per_window=0 stride=3 N=10
  d512            168    2.65     0.373     trained H8 merged t_in=513 out/c        3.11     0.761     trained H16 merged t_in=513
  d64 T32          60    1.92     0.345     init H4 mel01 t_in=31 out/c             1.71     0.416     trained H4 mel01 t_in=1
  d256 T128        60    1.95     0.330     init H8 randn t_in=127 out/c            3.03     0.744     trained H8 randn t_in=128
  d256 T160        60    1.92     0.340     init H16 mel01 t_in=250 out/c           2.68     0.660     trained H16 randn t_in=159
  geometry         28    2.79     0.333     d256 B=257 out/c                        2.55     0.628     d512 B=2
  golden (tests/test_gpu_core.py, 33 lines): closest 0.614 (core_d256_trunc_T300 attention); d512 H16 out / c_i 0.387
The closest case of all is the attention map of d512 / 16 heads / merged / trained at t_in = 513: 0.761 of its bound; in e it is
`raw` of sharp77 / zeroch at 0.601.  No kernel missed the bound, so no kernel source changed.

PLANTED FAULTS (library built with each fault, MI355X; failing tests of the previous tests/test_gpu_core.py, 22 tests, and of
this file, 134 tests, of which cases on `init` / `trained`-derived parameter sets):
  fault                                             previous file   this file   init   trained
  short-term frames staged in reverse order               9            70        23      27
  last long frame (row T-1) := row T-2                    6            60        18      22
  LayerNorm epsilon 1e-5 -> 1e-6                          8           111        36      44
  softmax scale x 1.0005                                 11            99        24      39
  one column of the folded value weight x 1.001           8            98        27      42
  emotion encoder's last input column dropped            10            92        28      34
The previous file caught all six as well, most through the goldens with `trained` weights (and the attention map's 2e-6); this
file fails each of them at `init` and at `trained` weights (the first two were planted in the caller-provided-mel loader only).
"""
import numpy as np
import pytest
import torch

import core_logit_cases as cc
from core_logit_cases import EMA_ROUNDINGS, K, ema_term, engine_for, guarded, judge, make_inputs, make_params, run_core  # noqa: F401
from koemorph_amd import synth
from koemorph_amd.engine import Engine, MelConfig
from oracle import core

pytestmark = pytest.mark.gpu
EXPR0 = core.EXPRESSION_INDICES[0]


# ---- fused d256 kernel: parameter sets x inputs, and every t_in ------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(kind, seed, **kw):
        key = (kind, seed, tuple(sorted(kw.items())))
        if key not in cache:
            d, T = kw.get("d_model", 256), kw.get("mel_sequence_length", 256)
            params = make_params(kind, seed, d, T)
            cache[key] = (params, engine_for(params, **kw))
        return cache[key]
    yield get
    for _, e in cache.values():
        e.close()


@pytest.mark.parametrize("ik", cc.INPUT_KINDS)
@pytest.mark.parametrize("pk,seed", [("init", 77), ("init", 5), ("trained", 77), ("trained", 12), ("trained", 301), ("sharp", 77),
                                      ("bias0", 77), ("offset", 77)])
def test_fused_core_parameter_sets_and_inputs(engines, pk, seed, ik):
    params, e = engines(pk, seed)
    assert e.fused
    run_core(e, "fused", f"{pk}{seed} {ik}", params, make_inputs(ik, 900 + seed, 3, 257))


T_INS = [1, 2, 3, 100, 255, 256, 257, 258, 300, 700]


@pytest.mark.parametrize("t_in", T_INS)
@pytest.mark.parametrize("pk", ["init", "trained"])
def test_fused_core_every_input_length(engines, pk, t_in):
    params, e = engines(pk, 77)
    run_core(e, "fused t_in", f"{pk} t_in={t_in}", params, make_inputs("mel01", 40 + t_in, 3, t_in))


def test_bias0_case_has_zero_variance_rows_in_the_oracle(engines):
    """The premise of the bias0 / zeroch cases, checked on the float64 oracle: with a zero encoder bias a channel that is zero in
    every frame has exactly zero variance and its LayerNorm row is exactly beta.  The C ABI does not expose the kernel's LayerNorm
    rows; the kernel is judged on this input through the logit and attention bound like every other case."""
    params, e = engines("bias0", 77)
    mel, short, emo = make_inputs("zeroch", 31, 4, 256)
    ref, o = run_core(e, "fused", "bias0 zeroch rows", params, (mel, short, emo))
    with torch.no_grad():
        y = core.core_forward(params, mel, short, emo, dtype=torch.float64, return_intermediates=True)["_y"].numpy()
    assert np.array_equal(y[:, [0, 37, 79]], np.broadcast_to(params["mel_norm.bias"].astype(np.float64), (4, 3, 256)))


# ---- emotion stream: emotion_logit + core_forward_z -------------------------------------------------------------------------------
@pytest.mark.parametrize("d,T,H,ED", [(256, 256, 8, 256), (256, 256, 8, 250), (256, 256, 8, 87), (256, 256, 8, 1), (256, 256, 8, 300),
                                      (512, 512, 8, 256), (512, 512, 16, 99), (64, 32, 4, 256), (64, 32, 4, 33)])
@pytest.mark.parametrize("pk", ["init", "trained"])
def test_emotion_logit_and_core_forward_z(pk, d, T, H, ED):
    """emotion_kernel_d256 (d 256, emotion_dim <= 256) and emotion_kernel (the rest) against the oracle's emotion-stream logit
    -- the 24 expression columns of z -- with emotion dims that are no multiple of the kernels' 16- and 64-wide steps, 7 windows
    (4 per workgroup) and the tensor 4 bytes off alignment; then core_forward_z on those logits in the logit measure."""
    B = 7
    params = make_params(pk, 50 + ED, d, T, ED)
    e = engine_for(params, d_model=d, num_heads=H, mel_sequence_length=T, emotion_dim=ED)
    mel, short, _ = make_inputs("mel01", 60 + ED, B, T + 1, T)
    emo = synth.normal(61 + ED, (B, ED))
    ref = core.logit_reference(params, mel, short, emo, num_heads=H, mel_sequence_length=T)
    with torch.no_grad():
        z32 = core.core_forward(params, mel, short, emo, num_heads=H, mel_sequence_length=T, return_intermediates=True)["_z"].numpy()
    z64 = ref["z64"][:, EXPR0]
    assert np.array_equal(ref["z64"][:, core.EXPRESSION_INDICES], np.broadcast_to(z64[:, None], (B, 24)))
    ge = guarded(emo, guard=1281)
    assert ge.data_ptr() % 16 == 4
    z = e.emotion_logit(ge)
    zg = z.cpu().numpy().astype(np.float64)
    yard = float(np.abs(z32[:, EXPR0] - z64).max())
    bound = K * max(yard, core.LOGIT_FLOOR) + core.LOGIT_U * np.abs(z64)
    err = np.abs(zg - z64)
    print(f"CORELOGIT|emotion z|{pk} d{d} ED{ED}|{err.max():.3e}|{yard:.3e}|{(err / bound).max():.3f}|nan|nan|nan")
    assert np.isfinite(zg).all() and (err <= bound).all(), (float(err.max()), yard)
    e.reserve(B)                                          # core_forward_z is the bare launch: the workspace is the caller's business
    out = e.core_forward_z(guarded(mel), guarded(short), z)
    judge("emotion z", f"{pk} d{d} ED{ED} core_forward_z", ref, s=core.recover_sigmoid(out.cpu().numpy(), params), out_over_c=True)
    e.close()


# ---- from audio (FUSE_DB): the oracle is fed the device's own features -------------------------------------------------------------
L_PROD = 136448


def audio_case(name, B=3):
    if name in ("uniform", "speech"):
        return synth.make_audio(11, B, L_PROD, name)
    if name == "silence":                                 # window maximum 0: the log_eps / amin floor
        return np.zeros((B, L_PROD), np.float32)
    if name == "click":
        a = np.zeros((B, L_PROD), np.float32)
        for b in range(B):
            a[b, 40000 + 533 * b + b] = 0.9
        return a
    if name == "short":                                   # fewer frames than the window: the zero-pad branch
        return synth.make_audio(12, B, 50000, "speech")
    if name == "L136000":                                 # 256 frames, no 257th
        return synth.make_audio(13, B, 136000, "uniform")
    raise KeyError(name)


@pytest.mark.parametrize("name", ["uniform", "speech", "silence", "click", "short", "L136000"])
@pytest.mark.parametrize("pk", ["init", "trained"])
def test_forward_audio_in_logit_space(engines, pk, name):
    """km_forward_audio: dB conversion inside the core's load.  Two consecutive calls on one engine, the second with first=False
    on other audio: the EMA epilogue (undone with the state the device held before the call) and the re-zeroed window maxima."""
    params, e = engines(pk, 77)
    B = 3
    a0 = audio_case(name, B)
    a1 = np.ascontiguousarray(a0[::-1] * np.float32(0.5)) if name != "silence" else audio_case("speech", B)[:, :a0.shape[1]]
    emo = synth.normal(14, (B, 256))
    ge = guarded(emo)
    state = torch.zeros(B, 52, device="cuda")
    prev = None
    for call, audio in enumerate((a0, a1)):
        ga = guarded(audio)
        out = e.forward_audio(ga, ge, state=state, first=(call == 0)).cpu().numpy()
        assert np.array_equal(out, state.cpu().numpy())
        long, short = e.mel_batch(ga)
        ref = core.logit_reference(params, long.cpu().numpy(), short.cpu().numpy(), emo)
        if call == 0:
            judge("forward_audio", f"{pk} {name} first", ref, s=core.recover_sigmoid(out, params), out_over_c=True)
        else:
            x = core.undo_ema(out, prev)
            judge("forward_audio", f"{pk} {name} ema", ref, s=core.recover_sigmoid(x, params), extra=ema_term(ref["out64"], prev, params), out_over_c=True)
        plain = e.forward_audio(ga, ge).cpu().numpy()     # no state: the same windows unsmoothed
        judge("forward_audio", f"{pk} {name} call{call} nostate", ref, s=core.recover_sigmoid(plain, params), out_over_c=True)
        prev = out.astype(np.float64)


# ---- streaming tick and graph replay -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 300])
def test_streaming_ticks_in_logit_space(S):
    """km_stream_tick: the ring (136 000 samples, 532 per push) is full after 256 pushes; the tick keeps 255 of the front end's 256
    frames (int(8.5 / 0.0333)), zero-pads the 256th and takes the short-term rows from the last three kept.  Checked: the tick that
    fills the ring (EMA starts), the two after it, and a replayed tick of the captured graph; the EMA is undone with the previous
    tick's output, which is the device's state.  Before the ring is full, `out` stays what it was, bit for bit, and ready is 0.
    StreamEngine.push takes one frame for EVERY stream, so all rings fill in lockstep: a launch with ready and not-ready streams
    side by side cannot be produced through this API and is not covered here."""
    from koemorph_amd.streaming import StreamEngine
    params = make_params("trained", 61)
    e, fe = engine_for(params), engine_for(params)       # fe: the same front end on a handle of its own, whose workspace may grow
    se = StreamEngine(e, S)
    assert se.ring_hop == 532
    RING, FULL = 136000, 256
    pool = synth.make_audio(62, S, 532 * 37, "speech" if S == 3 else "uniform")
    emo = synth.normal(63, (S, 256))
    ge = guarded(emo)
    sentinel = torch.from_numpy(synth.uniform(64, (S, 52), 0.25, 0.75)).cuda()
    se.out.copy_(sentinel)
    ring = np.zeros((S, RING), np.float32)
    w, prev = 0, None
    for n in range(1, FULL + 4):
        chunk = np.ascontiguousarray(pool[:, (n % 37) * 532:(n % 37 + 1) * 532] * np.float32(0.5 + 0.125 * ((n // 37) % 5)))
        ring[:, (w + np.arange(532)) % RING] = chunk
        w = (w + 532) % RING
        if n == FULL + 3:
            se.capture(532)
            out, ready = se.replay(guarded(chunk), ge)
        else:
            se.push(guarded(chunk))
            out, ready = se.tick(ge)
        if n < FULL:
            if n in (1, 2, 100, FULL - 1):
                assert not bool(ready.any()) and torch.equal(out, sentinel), n
            continue
        assert bool(ready.all()), n
        got = out.cpu().numpy()
        feats = fe.mel_extract(se.mel, guarded(np.roll(ring, -w, axis=1)), out_frames=255).cpu().numpy()
        ref = core.logit_reference(params, feats, feats[:, -3:], emo)
        label = f"S={S} push {n}" + (" replay" if n == FULL + 3 else "")
        if n == FULL:
            judge("stream", label + " first", ref, s=core.recover_sigmoid(got, params), out_over_c=True)
        else:
            judge("stream", label + " ema", ref, s=core.recover_sigmoid(core.undo_ema(got, prev), params),
                  extra=ema_term(ref["out64"], prev, params), out_over_c=True)
        prev = got.astype(np.float64)
    e.close()
    fe.close()


# ---- sequence_forward: shared frames and per-window ---------------------------------------------------------------------------------
@pytest.mark.parametrize("per_window", [0, 1])
@pytest.mark.parametrize("stride,extra", [(1, 4), (3, 7)])
def test_sequence_forward_in_logit_space(per_window, stride, extra):
    """km_sequence_forward(smooth=False): the clip-level frame image (seq_pow), the per-window edge frames (seq_edge) and the
    per-window emotion logits of a clip (zemo_div); option seq_per_window selects the per-window evaluation of the same windows.
    A call takes clips of ONE length (audio is (B, L)), so the two clip lengths are two calls of two clips each, each on a fresh
    engine whose workspace is reserved for exactly 4 windows (the tile is the reserved window count, and reserve never shrinks):
    every clip has N >= 5 windows, so clip 0 straddles tiles 0 and 1 and clip 1 starts inside a tile (win0 != 0).  The features
    for the oracle come from a second engine, so that its mel_batch cannot grow the first one's tile."""
    params = make_params("trained", 77)
    fe = engine_for(params)
    hop, W = 533, 256 * 533
    for clip_extra in (extra, extra + 2):
        e = engine_for(params)
        e.set_option("seq_per_window", per_window)
        L = W + hop * stride * clip_extra + 17
        audio = synth.make_audio(70 + clip_extra, 2, L, "speech")
        emo = synth.normal(71, (2, 256))
        N = e.sequence_num_outputs(L, stride)
        assert N >= 5
        out = e.sequence_forward(guarded(audio), guarded(emo), stride_frames=stride, smooth=False, max_tile=4).cpu().numpy()
        assert out.shape == (2, N, 52)
        wins = np.stack([audio[b, i * stride * hop:i * stride * hop + W] for b in range(2) for i in range(N)])
        assert wins.shape == (2 * N, W)
        assert e._reserved[0] == 4                        # the tile really was 4 windows
        long, short = fe.mel_batch(guarded(wins))
        ref = core.logit_reference(params, long.cpu().numpy(), short.cpu().numpy(), np.repeat(emo, N, axis=0))
        judge("sequence", f"per_window={per_window} stride={stride} N={N}", ref,
              s=core.recover_sigmoid(out.reshape(2 * N, 52), params), out_over_c=True)
        e.close()
    fe.close()


# ---- generic chain -------------------------------------------------------------------------------------------------------------------
def t_ins(T):
    return sorted({max(1, T - 37), T - 1, T, T + 1, T + 90})


@pytest.mark.parametrize("no_merge", [0, 1])
@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("pk", ["init", "trained"])
def test_generic_d512_from_mel_and_audio(pk, H, no_merge):
    """d_model 512, window 512: core512_kernel (one launch) and the three launches behind option no_core_merge."""
    params = make_params(pk, 88, 512, 512)
    e = engine_for(params, d_model=512, num_heads=H, mel_sequence_length=512, mel=MelConfig.model_batch(target_fps=60))
    assert not e.fused and e.mel.hop_length == 266
    e.set_option("no_core_merge", no_merge)
    tag = f"{pk} H{H} {'three launches' if no_merge else 'merged'}"
    for t_in in t_ins(512):
        run_core(e, "d512", f"{tag} t_in={t_in}", params, make_inputs("mel01", 80 + t_in, 2, t_in, 512), H=H, T=512)
    emo = synth.normal(81, (2, 256))
    for name, L in (("speech", 512 * 266), ("uniform", 512 * 266 - 300), ("speech", 40000)):
        ga, ge = guarded(synth.make_audio(82, 2, L, name)), guarded(emo)
        for call in range(2):                             # twice: the window maxima were handed back clean
            out = e.forward_audio(ga, ge).cpu().numpy()
            long, short = e.mel_batch(ga)
            ref = core.logit_reference(params, long.cpu().numpy(), short.cpu().numpy(), emo, num_heads=H, mel_sequence_length=512)
            judge("d512", f"{tag} audio {name} L={L} call{call}", ref, s=core.recover_sigmoid(out, params), out_over_c=True)
    e.close()


@pytest.mark.parametrize("d,T,H", [(64, 32, 4), (256, 128, 8), (256, 160, 16)])
@pytest.mark.parametrize("pk", ["init", "trained"])
def test_generic_other_shapes(pk, d, T, H):
    params = make_params(pk, 91, d, T)
    e = engine_for(params, d_model=d, num_heads=H, mel_sequence_length=T)
    assert not e.fused
    for t_in in t_ins(T):
        for ik in ("mel01", "randn"):
            run_core(e, f"d{d} T{T}", f"{pk} H{H} {ik} t_in={t_in}", params, make_inputs(ik, 90 + t_in, 3, t_in, T), H=H, T=T)
    e.close()


# ---- launch geometry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 513, 1100])
@pytest.mark.parametrize("d,T,H", [(256, 256, 8), (512, 512, 8)])
def test_launch_geometry(d, T, H, B):
    """Every window of the batch is bit-identical to the same window run in a batch of three (so the checked sample speaks for all
    of them), and windows 0, B-1 and ~30 spread ones meet the bound against the float64 oracle."""
    params = make_params("trained", 77, d, T)
    e = engine_for(params, d_model=d, num_heads=H, mel_sequence_length=T)
    mel, short, emo = synth.make_core_inputs(1000 + B, B, T + 1)
    mel[:, T:] = np.nan
    gm, gs, ge = guarded(mel), guarded(short), guarded(emo)
    o = e.core_forward(gm, gs, ge, return_attention=True)
    full, raw, attn = o["blendshapes"], o["raw"], o["mel_attention_weights"]
    assert torch.equal(e.core_forward(gm, gs, ge)["blendshapes"], full)
    for lo in range(0, B, 3):
        hi = min(lo + 3, B)
        o3 = e.core_forward(gm[lo:hi], gs[lo:hi], ge[lo:hi], return_attention=True)
        assert torch.equal(o3["blendshapes"], full[lo:hi]) and torch.equal(o3["raw"], raw[lo:hi]), (B, lo)
        assert torch.equal(o3["mel_attention_weights"], attn[lo:hi]), (B, lo)
    pick = sorted({0, B - 1} | {int(i) for i in np.linspace(0, B - 1, 30)})
    ref = core.logit_reference(params, mel[pick], short[pick], emo[pick], num_heads=H, mel_sequence_length=T)
    judge("geometry", f"d{d} B={B} raw", ref, s=raw.cpu().numpy()[pick], a=attn.cpu().numpy()[pick])
    judge("geometry", f"d{d} B={B} out/c", ref, s=core.recover_sigmoid(full.cpu().numpy()[pick], params), out_over_c=True)
    e.close()


def test_cases_of_this_file_run_with_core_split_off():
    """core_split (3 / 6, the split-bf16 form) stays opt-in.  engine_for() sets the option to 0 on every engine of this file, so no
    case above can have run the split images even where the environment presets it; and an engine left at its defaults gives the
    same bits as one with the option set to 0.  (tests/test_gpu_core.py holds the on / off / on comparison.)"""
    import os
    assert os.environ.get("KM_CORE_SPLIT", "0") == "0"
    params = make_params("trained", 77)
    plain = Engine()
    plain.load_state_dict(params)
    plain.finalize()
    e = engine_for(params)
    audio, emo = guarded(synth.make_audio(3, 3, L_PROD, "speech")), guarded(synth.normal(4, (3, 256)))
    assert torch.equal(plain.forward_audio(audio, emo), e.forward_audio(audio, emo))
    long, short = e.mel_batch(audio)
    assert torch.equal(plain.core_forward(long, short, emo)["blendshapes"], e.core_forward(long, short, emo)["blendshapes"])
    plain.close()
    e.close()
