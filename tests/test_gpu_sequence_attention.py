"""Attention maps and `raw` from the audio paths (km_forward_audio_attn, km_forward_clip_attn, km_sequence_forward_attn;
``Engine.*(return_attention=True, stats=...)``, ``SequentialDualStreamModel.forward(return_attention=True)``,
``render_sequential --attention-summary``).

On the fused shape `blendshapes` are the bits of the call without the maps, and the maps and `raw` are the same bits however the
windows were scheduled: shared frames, per-window, tile 4 or 2048, ``forward_audio`` on the gathered windows, ``forward_clip`` on
their start frames.  The values are held to the bound of tests/test_gpu_core_logit.py (its docstring derives it; K =
core_logit_cases.K): the float64 oracle fed the DEVICE's own features, ``core.attention_verdict`` on the maps and
``core.logit_verdict`` on `raw`.  Every case prints `SEQATTN|case|e max|e / bound|a max|a / bound` before it asserts.
Clips are 136 448 + extra x 533 samples: (stride, extra) = (1, 4) and (3, 7) give N = 5 and 3 windows per clip, and with a tile
of 4 windows a tile boundary falls inside a clip."""
import json
import logging

import numpy as np
import pytest
import torch

import attn_stats_cases as ac
from core_logit_cases import K, guarded, make_params
from koemorph_amd import synth
from koemorph_amd._lib import KM_ERR_UNSUPPORTED, KoeMorphError, check, load
from koemorph_amd.engine import Engine, MelConfig, sequence_track_row
from koemorph_amd.metrics import AttentionStats
from oracle import core

pytestmark = pytest.mark.gpu

HOP, T = 533, 256
W = T * HOP
CASES = [(1, 4), (3, 7)]
FIRST, INTERVAL, TRACK_ROWS = 8000, 4800, 3


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def engine_for(params, **kw):
    e = Engine(**kw)
    e.load_state_dict(params)
    e.finalize()
    e.set_option("core_split", 0)
    return e


def clip_length(extra):
    return 136448 + extra * HOP


def gathered(audio, N, stride, hop=HOP, window=W):
    """The (B N, window) windows of the clips, zero-padded past the clip end, in the order of the outputs."""
    B, L = audio.shape
    wins = np.zeros((B * N, window), np.float32)
    for b in range(B):
        for i in range(N):
            seg = audio[b, i * stride * hop:i * stride * hop + window]
            wins[b * N + i, :seg.shape[0]] = seg
    return wins


class Source:
    """One emotion source of a sequence call: a vector per clip, or a (B, 3, 256) track with first = 8000, interval = 4800."""

    def __init__(self, kind, B, L, N, stride, T_=T, hop=HOP):
        self.kind = kind
        if kind == "vector":
            self.emo = synth.normal(71, (B, 256))
            self.rows = np.repeat(self.emo, N, axis=0)
            self.dev = guarded(self.emo)
        else:
            self.trk = synth.normal(72, (B, TRACK_ROWS, 256))
            k = [sequence_track_row(i, TRACK_ROWS, FIRST, INTERVAL, 0, L, stride, T_, hop) for i in range(N)]
            self.rows = np.stack([self.trk[b, k[i]] for b in range(B) for i in range(N)])
            self.dev = guarded(self.trk)

    def call(self, e, audio, stride, **kw):
        if self.kind == "vector":
            return e.sequence_forward(audio, self.dev, stride, **kw)
        return e.sequence_forward_track(audio, self.dev, FIRST, INTERVAL, stride, **kw)


def judge(label, ref, raw, attn):
    zmax = float(np.abs(ref["z64"]).max())
    assert zmax <= core.LOGIT_Z_MAX, f"{label}: |z64| reaches {zmax}, choose other parameters"
    e_max, e_ratio = core.logit_verdict(raw, ref, K)
    a_max, a_ratio = core.attention_verdict(attn, ref, K)
    print(f"SEQATTN|{label}|{e_max:.3e}|{e_ratio:.3f}|{a_max:.3e}|{a_ratio:.3f}")
    assert e_ratio <= 1.0, f"{label}: logit error of raw {e_max:.3e} is {e_ratio:.2f} x its bound (yardstick {ref['yard_e']:.3e})"
    assert a_ratio <= 1.0, f"{label}: attention error {a_max:.3e} is {a_ratio:.2f} x its bound (yardstick {ref['yard_a']:.3e})"
    assert np.abs(attn.astype(np.float64).sum(-1) - 1.0).max() < 1e-5


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("blendshapes", "raw", "mel_attention_weights"))


# ---- 1: the fused shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vector", "track"])
@pytest.mark.parametrize("stride,extra", CASES)
@pytest.mark.parametrize("pk", ["init", "trained"])
def test_fused_sequence_maps_every_schedule_and_the_oracle(pk, stride, extra, kind):
    params = make_params(pk, 77)
    small, big = engine_for(params), engine_for(params)          # small: never reserved beyond 4 windows, so its tile is 4
    L = clip_length(extra)
    audio = synth.make_audio(70 + extra, 2, L, "speech")
    ga = guarded(audio)
    N = small.sequence_num_outputs(L, stride)
    assert N == (5 if stride == 1 else 3)
    src = Source(kind, 2, L, N, stride)
    # blendshapes: the bits of the call without the maps, smoothed or not
    for smooth in (True, False):
        plain = src.call(small, ga, stride, smooth=smooth, max_tile=4)
        o = src.call(small, ga, stride, smooth=smooth, max_tile=4, return_attention=True)
        assert set(o) == {"blendshapes", "raw", "mel_attention_weights"}
        assert o["blendshapes"].shape == (2, N, 52) and o["raw"].shape == (2, N, 52) and o["mel_attention_weights"].shape == (2, N, 28, 80)
        assert torch.equal(o["blendshapes"], plain), smooth
        if smooth:
            smoothed = o
    assert small._reserved[0] == 4                               # the tile really was 4 windows
    assert torch.equal(smoothed["raw"], o["raw"]) and torch.equal(smoothed["mel_attention_weights"], o["mel_attention_weights"])
    assert not torch.equal(smoothed["blendshapes"], o["blendshapes"])
    # the same bits from the per-window schedule, one tile, and forward_audio on the gathered windows
    small.set_option("seq_per_window", 1)
    assert same(src.call(small, ga, stride, smooth=False, max_tile=4, return_attention=True), o)
    small.set_option("seq_per_window", 0)
    assert same(src.call(big, ga, stride, smooth=False, max_tile=2048, return_attention=True), o)
    gw = guarded(gathered(audio, N, stride))
    fa = big.forward_audio(gw, guarded(src.rows), return_attention=True)
    assert torch.equal(fa["blendshapes"], big.forward_audio(gw, guarded(src.rows)))
    flat = {k: v.reshape(2 * N, *v.shape[2:]) for k, v in o.items()}
    assert same(fa, flat)
    # the values: the float64 oracle on the device's own features
    long, short = big.mel_batch(gw)
    ref = core.logit_reference(params, long.cpu().numpy(), short.cpu().numpy(), src.rows)
    judge(f"{pk} stride={stride} N={N} {kind}", ref, flat["raw"].cpu().numpy(), flat["mel_attention_weights"].cpu().numpy())
    small.close()
    big.close()


def test_nothing_is_written_outside_the_outputs():
    """km_sequence_forward_attn on out / raw / attn views inside NaN-filled allocations, shared-frame and per-window, tile 4: the
    guards stay NaN and the views hold what the Engine call returns."""
    params = make_params("trained", 77)
    e = engine_for(params)
    stride, extra = 1, 4
    L = clip_length(extra)
    audio, emo = guarded(synth.make_audio(70 + extra, 2, L, "speech")), guarded(synth.normal(71, (2, 256)))
    N = e.sequence_num_outputs(L, stride)
    want = e.sequence_forward(audio, emo, stride, smooth=False, max_tile=4, return_attention=True)
    lib, G = load(), 1280
    for per_window in (0, 1):
        e.set_option("seq_per_window", per_window)
        bufs = {}
        for name, n in (("blendshapes", 2 * N * 52), ("raw", 2 * N * 52), ("mel_attention_weights", 2 * N * 28 * 80)):
            bufs[name] = torch.full((n + 2 * G,), float("nan"), device="cuda")
        p = {k: v.data_ptr() + 4 * G for k, v in bufs.items()}
        check(lib.km_sequence_forward_attn(e._h, audio.data_ptr(), 2, L, emo.data_ptr(), None, 0, 0, 0, 0, 0, stride, 0, p["blendshapes"],
                                           p["raw"], p["mel_attention_weights"], None, torch.cuda.current_stream().cuda_stream))
        for name, b in bufs.items():
            assert torch.isnan(b[:G]).all() and torch.isnan(b[-G:]).all(), (per_window, name)
            assert torch.equal(b[G:-G], want[name].reshape(-1)), (per_window, name)
    e.close()


def test_forward_clip_with_maps():
    """Start frames out of order, one repeated; then a second call with first=False on the carried state."""
    params = make_params("trained", 77)
    e = engine_for(params)
    assert e.forward_clip_supported()
    clip = synth.make_audio(74, 1, clip_length(4), "speech")[0]
    gc = guarded(clip)
    starts = [3, 0, 3, 1]
    wins = guarded(np.stack([clip[s * HOP:s * HOP + W] for s in starts]))
    sp, sa, sg = (torch.zeros(4, 52, device="cuda") for _ in range(3))
    for call, first in enumerate((True, False)):
        emo = guarded(synth.normal(75 + call, (4, 256)))
        plain = e.forward_clip(gc, starts, emo, state=sp, first=first)
        o = e.forward_clip(gc, starts, emo, state=sa, first=first, return_attention=True)
        assert torch.equal(o["blendshapes"], plain) and torch.equal(sa, sp), call
        fa = e.forward_audio(wins, emo, state=sg, first=first, return_attention=True)
        assert same(o, fa) and torch.equal(sg, sa), call
        assert torch.equal(o["mel_attention_weights"][0], o["mel_attention_weights"][2])        # the repeated start frame
        assert not torch.equal(o["mel_attention_weights"][0], o["mel_attention_weights"][1])
    long, short = e.mel_batch(wins)
    ref = core.logit_reference(params, long.cpu().numpy(), short.cpu().numpy(), synth.normal(76, (4, 256)))
    judge("forward_clip first=False", ref, o["raw"].cpu().numpy(), o["mel_attention_weights"].cpu().numpy())
    e.close()


# ---- 2: the generic path -----------------------------------------------------------------------------------------------------------
def test_generic_path_small_shape_is_within_the_oracle_bound():
    """d_model 64, window 32, 4 heads: the GEMM-chain core writes the maps and raw; blendshapes within the bound (bit equality with
    the plain call is not promised on generic shapes)."""
    d, Tw, H = 64, 32, 4
    params = make_params("trained", 91, d, Tw)
    kw = dict(d_model=d, num_heads=H, mel_sequence_length=Tw, mel=MelConfig.model_batch(target_fps=30))
    e, fe = engine_for(params, **kw), engine_for(params, **kw)
    assert not e.fused
    L = Tw * HOP + 4 * HOP + 50
    clips = synth.make_audio(103, 3, L)
    for stride in (1, 2):
        N = e.sequence_num_outputs(L, stride)
        assert N == (5 if stride == 1 else 3)
        trk = synth.normal(104, (3, N, 256))                      # the identity map: one row per window
        o = e.sequence_forward_track(guarded(clips), guarded(trk), Tw * HOP, stride * HOP, stride, smooth=False, max_tile=4,
                                     return_attention=True)
        assert o["blendshapes"].shape == (3, N, 52) and o["raw"].shape == (3, N, 52) and o["mel_attention_weights"].shape == (3, N, 28, 80)
        long, short = fe.mel_batch(guarded(gathered(clips, N, stride, HOP, Tw * HOP)))
        ref = core.logit_reference(params, long.cpu().numpy(), short.cpu().numpy(), trk.reshape(3 * N, 256), num_heads=H, mel_sequence_length=Tw)
        judge(f"generic d{d} T{Tw} stride={stride}", ref, o["raw"].reshape(3 * N, 52).cpu().numpy(),
              o["mel_attention_weights"].reshape(3 * N, 28, 80).cpu().numpy())
        s = core.recover_sigmoid(o["blendshapes"].reshape(3 * N, 52).cpu().numpy(), params)
        e_max, e_ratio = core.logit_verdict(s, ref, K, core.OUT_OVER_C_ROUNDINGS)
        print(f"SEQATTN|generic stride={stride} out/c|{e_max:.3e}|{e_ratio:.3f}|nan|nan")
        assert e_ratio <= 1.0
        # a vector per clip through the same entry point
        v = synth.normal(105, (3, 256))
        ov = e.sequence_forward(guarded(clips), guarded(v), stride, smooth=False, max_tile=4, return_attention=True)
        refv = core.logit_reference(params, long.cpu().numpy(), short.cpu().numpy(), np.repeat(v, N, axis=0), num_heads=H, mel_sequence_length=Tw)
        judge(f"generic d{d} T{Tw} stride={stride} vector", refv, ov["raw"].reshape(3 * N, 52).cpu().numpy(),
              ov["mel_attention_weights"].reshape(3 * N, 28, 80).cpu().numpy())
    e.close()
    fe.close()


# ---- 3: stats= alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vector", "track"])
def test_stats_alone_equals_an_accumulator_fed_the_returned_maps(kind):
    params = make_params("trained", 77)
    e = engine_for(params)
    stride, extra = 1, 4
    L = clip_length(extra)
    ga = guarded(synth.make_audio(70 + extra, 2, L, "speech"))
    N = e.sequence_num_outputs(L, stride)
    src = Source(kind, 2, L, N, stride)
    acc = AttentionStats()
    out = src.call(e, ga, stride, max_tile=4, stats=acc)
    assert isinstance(out, torch.Tensor) and torch.equal(out, src.call(e, ga, stride, max_tile=4))
    assert acc.rows == 2 * N and e._reserved[0] == 4
    got = acc.compute()
    maps = src.call(e, ga, stride, max_tile=4, return_attention=True)["mel_attention_weights"].reshape(2 * N, 28, 80)
    twin = AttentionStats()
    for w0 in range(0, 2 * N, 4):                                # the tiles of the call
        twin.update(maps[w0:w0 + 4])
    want = twin.compute()
    assert got["rows"] == want["rows"] == 2 * N and np.array_equal(got["peak_hist"], want["peak_hist"])
    assert got["mean_map"].tobytes() == want["mean_map"].tobytes() and got["entropy"].tobytes() == want["entropy"].tobytes()
    ac.assert_within_bounds(got, maps.cpu().numpy())
    # maps returned AND accumulated in one call: the same bits again
    both = AttentionStats()
    o = src.call(e, ga, stride, max_tile=4, return_attention=True, stats=both)
    assert torch.equal(o["mel_attention_weights"].reshape(2 * N, 28, 80), maps) and ac.pack(both.compute()).tobytes() == ac.pack(got).tobytes()
    # the handle's tile buffer is reused: a second stats-only call is captured (a call that had to grow a buffer would be refused
    # inside a capture) and its replay accumulates the same bits
    acc.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        again = src.call(e, ga, stride, max_tile=4, stats=acc)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(again, out) and ac.pack(acc.compute()).tobytes() == ac.pack(got).tobytes()
    del g
    with pytest.raises(ValueError):
        src.call(e, ga, stride, max_tile=4, stats=AttentionStats(28, 40))
    for a in (acc, twin, both):
        a.close()
    e.close()


def test_split_core_refuses_maps_before_it_launches_anything():
    params = make_params("trained", 77)
    e = engine_for(params)
    L = clip_length(4)
    ga, emo = guarded(synth.make_audio(74, 2, L, "speech")), guarded(synth.normal(71, (2, 256)))
    before = e.sequence_forward(ga, emo, 1, max_tile=4).clone()
    quiet = guarded(synth.make_audio(720, 4, W) * 1e-3)
    q0 = e.forward_audio(quiet, emo.repeat(2, 1)).clone()
    e.set_option("core_split", 3)
    acc = AttentionStats()
    for call in (lambda: e.sequence_forward(ga, emo, 1, max_tile=4, return_attention=True),
                 lambda: e.sequence_forward(ga, emo, 1, max_tile=4, stats=acc),
                 lambda: e.forward_audio(quiet, emo.repeat(2, 1), return_attention=True)):
        with pytest.raises(KoeMorphError, match="split-bf16") as err:
            call()
        assert err.value.code == KM_ERR_UNSUPPORTED
    assert acc.compute()["rows"] == 0
    e.set_option("core_split", 0)
    # nothing was launched: no front end ran, so the window maxima are as clean as they were and both paths give their bits
    assert torch.equal(e.forward_audio(quiet, emo.repeat(2, 1)), q0)
    assert torch.equal(e.sequence_forward(ga, emo, 1, max_tile=4), before)
    acc.close()
    e.close()


def test_argument_checks_of_the_sequence_entry_point():
    from koemorph_amd._lib import KM_ERR_INVALID_ARG
    params = make_params("trained", 77)
    e = engine_for(params)
    L = clip_length(4)
    ga, emo, trk = guarded(synth.make_audio(74, 2, L)), guarded(synth.normal(71, (2, 256))), guarded(synth.normal(72, (2, 3, 256)))
    e.reserve(4, W)
    out = torch.empty(2, 5, 52, device="cuda")
    lib, st = load(), torch.cuda.current_stream().cuda_stream

    def call(emo_p=None, trk_p=None, K_=3, first=FIRST, interval=INTERVAL, offset=0, clip_len=L, stats=None):
        return lib.km_sequence_forward_attn(e._h, ga.data_ptr(), 2, L, emo_p, trk_p, K_, first, interval, offset, clip_len, 1, 1,
                                            out.data_ptr(), None, None, stats, st)

    assert call(emo_p=emo.data_ptr()) == 0 and call(trk_p=trk.data_ptr()) == 0
    assert call() == KM_ERR_INVALID_ARG and call(emo_p=emo.data_ptr(), trk_p=trk.data_ptr()) == KM_ERR_INVALID_ARG
    assert call(emo_p=emo.data_ptr(), K_=0, interval=0, clip_len=0) == 0          # the track arguments are ignored with emotion_dev
    for kw in (dict(K_=0), dict(interval=0), dict(first=-1), dict(offset=-1), dict(clip_len=L - 1), dict(offset=5)):
        assert call(trk_p=trk.data_ptr(), **kw) == KM_ERR_INVALID_ARG, kw
    wrong = AttentionStats(28, 40)
    assert call(emo_p=emo.data_ptr(), stats=wrong._handle(out.device)) == KM_ERR_INVALID_ARG
    wrong.close()
    torch.cuda.synchronize()
    e.close()


# ---- 4: the models and the tool ------------------------------------------------------------------------------------------------------
def full_state(params, alpha=0.8):
    sd = {"dual_stream_attention." + k: torch.from_numpy(v) for k, v in params.items()}
    sd["smoothing_alpha"] = torch.tensor(alpha)
    return sd


def test_sequential_model_returns_the_maps_from_one_call(caplog):
    from koemorph_amd.features import ClipEmotion
    from koemorph_amd.model import SequentialDualStreamModel
    params = make_params("trained", 77)
    stride, extra = 3, 7
    L = clip_length(extra)
    audio = dev(synth.make_audio(70 + extra, 2, L, "speech"))
    N = 3
    v = dev(synth.normal(71, (2, 256)))
    m = SequentialDualStreamModel(stride_frames=stride).cuda().eval()
    m.load_state_dict(full_state(params))
    calls = []
    eng = m.dual_stream_attention.engine()
    for name in ("mel_batch", "core_forward", "smooth", "forward_audio"):        # the per-window loop went through these
        setattr(eng, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(getattr(eng, name), name))
    plain = m(audio, emotion_features=v)
    o = m(audio, return_attention=True, emotion_features=v)
    assert not calls, calls
    assert torch.equal(o["blendshapes"], plain["blendshapes"]) and o["num_frames"] == N
    assert o["mel_attention_weights"].shape == (2, N, 28, 80)
    assert o["emotion_attention_weights"].shape == (2, N, 24, 1) and bool((o["emotion_attention_weights"] == 1).all())
    assert torch.equal(o["mel_attention_weights"], eng.sequence_forward(audio, v, stride, return_attention=True)["mel_attention_weights"])
    assert torch.equal(m.prev_blendshapes, plain["blendshapes"][:, -1])
    # an accumulator through the model, with and without the maps
    acc = AttentionStats()
    assert torch.equal(m(audio, emotion_features=v, attention_stats=acc)["blendshapes"], plain["blendshapes"])
    ac.assert_within_bounds(acc.compute(), o["mel_attention_weights"].reshape(2 * N, 28, 80).cpu().numpy())
    acc.close()
    # the clips' own emotion tracks
    torch.manual_seed(4321)
    ce = ClipEmotion(compression_layer=torch.nn.Linear(264, 256))
    mc = SequentialDualStreamModel(stride_frames=stride, clip_emotion=ce).cuda().eval()
    mc.load_state_dict(full_state(params))
    with caplog.at_level(logging.WARNING):
        auto = mc(audio)
        oc = mc(audio, return_attention=True)
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
    assert oc["emotion_backend"] == "egemaps_track" and torch.equal(oc["blendshapes"], auto["blendshapes"])
    assert oc["mel_attention_weights"].shape == (2, N, 28, 80)
    ot = mc(audio, return_attention=True, emotion_track=ce.build_batch(audio)[0])
    assert torch.equal(ot["mel_attention_weights"], oc["mel_attention_weights"]) and torch.equal(ot["blendshapes"], auto["blendshapes"])
    ce.close()


def test_render_sequential_writes_the_attention_summary(tmp_path):
    from scipy.io import wavfile
    from koemorph_amd.scripts import render_sequential
    params = make_params("trained", 77)
    L = clip_length(7)
    pcm = np.round(synth.make_audio(77, 1, L, "speech")[0] * 32767.0).astype(np.int16)
    wav, ckpt, out, summ = tmp_path / "a.wav", tmp_path / "ckpt.pth", tmp_path / "out.jsonl", tmp_path / "sub" / "attn.json"
    wavfile.write(str(wav), 16000, pcm)
    torch.save({"epoch": 0, "global_step": 0, "model_state_dict": full_state(params),
                "model_config": {"d_model": 256, "num_heads": 8, "mel_sequence_length": 256}}, ckpt)
    assert render_sequential.main(["--model_path", str(ckpt), "--input_audio", str(wav), "--output_json", str(out), "--stride", "2",
                                   "--attention-summary", str(summ)]) == 0
    lines = out.read_text().splitlines()
    s = json.loads(summ.read_text())
    assert set(s) == {"rows", "mean_map", "entropy", "peak_hist", "band_mean", "band_share"}
    assert s["rows"] == len(lines) == 4
    mean_map = np.asarray(s["mean_map"])
    assert mean_map.shape == (28, 80) and np.asarray(s["peak_hist"]).sum() == 28 * len(lines)
    assert abs(sum(s["band_share"].values()) - mean_map.mean() * 4) < 1e-12
    assert np.abs(mean_map.sum(1) - 1.0).max() < 1e-5 and set(s["band_mean"]) == {"low", "mid_low", "mid_high", "high"}
    # without the switch the frames are the same and no summary is written
    out2 = tmp_path / "out2.jsonl"
    assert render_sequential.main(["--model_path", str(ckpt), "--input_audio", str(wav), "--output_json", str(out2), "--stride", "2"]) == 0
    assert out2.read_text() == out.read_text()
