"""Training and validation from a resident clip with option clip_assemble (km_clip_plan route 2): the span of the clip once, two
snippets of 2 E frames per window through the unchanged front end, then clip_pack_edges_kernel (the packed training input) or
clip_assemble_kernel (the front end's workspace, for the core behind km_forward_audio's power path) of km_clip_assemble.hip.

Every comparison is equality of bits with the path that is pinned to the float64 oracle: training against
``Trainer.forward_backward(km_gather_windows(clip, starts))`` (loss, out, the whole gradient bucket), forward against
``Engine.forward_audio`` on the gathered windows (out and the EMA state; with maps: raw and the maps).  The twin of every engine is an
engine with the same weights and the option off.  No tolerance anywhere.

Shapes: the 60 fps recipe (d_model 256, 8 heads, window 512, hop 266), d_model 512 at hop 266, `fast` at hop 533 (forward only,
with core128), the fused shape at hop 266, and d_model 64 / window 32 at hops 266 (E = 2) and 200 (E = 3: frames T - 2 .. T of the
packed tail columns are all edge rows; km_sequence_plan reports route 2 there too, asserted below).  B <= 9.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import clip_assemble_cases as cc
from core_logit_cases import guarded
from koemorph_amd import _lib, synth
from koemorph_amd._lib import KM_ERR_UNSUPPORTED, KoeMorphError, check, load
from koemorph_amd.data import SequentialKoeMorphDataset
from koemorph_amd.engine import Engine, _ptr, _stream_ptr
from koemorph_amd.training import Trainer

pytestmark = pytest.mark.gpu

BMAX = 9
TRAIN_SHAPES = [("d256 w512", 266), ("d512 h8", 266), ("fused", 266), ("d64 w32", 266), ("d64 w32", 200)]
FORWARD_SHAPES = TRAIN_SHAPES + [("fast", 533)]
EXTRA_OPTIONS = {"fast": {"core128": 1}}
EXTRA_FRAMES = 40          # the last full window of a clip starts at frame 40


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def clip_samples(name, hop):
    return (cc.SHAPES[name][2] + EXTRA_FRAMES) * hop + 77


def make_clip(name, hop, seed, kind="speech"):
    return synth.make_audio(seed, 1, clip_samples(name, hop), kind)[0]


def gather(clip_dev, starts, name, hop):
    """km_gather_windows: the (B, T hop) tensor the pinned path runs on."""
    W = cc.SHAPES[name][2] * hop
    st = dev(np.asarray(starts, np.int32))
    out = torch.empty(len(starts), W, device="cuda")
    check(load().km_gather_windows(clip_dev.data_ptr(), clip_dev.shape[0], st.data_ptr(), len(starts), hop, W, out.data_ptr(),
                                   None, 0, 0, 0, None, None, torch.cuda.current_stream().cuda_stream))
    return out


def make_engine(name, hop, assemble, **options):
    e = cc.new_engine(name, hop, **{**EXTRA_OPTIONS.get(name, {}), **options})
    e.finalize()
    if assemble:
        e.set_option("clip_assemble", 1)
    return e


class Pair:
    """An engine with the option on and its twin with the option off, same weights, each with a trainer where asked."""

    def __init__(self, name, hop, train=True, **trkw):
        self.name, self.hop = name, hop
        self.T, self.ED = cc.SHAPES[name][2], cc.SHAPES[name][3]
        self.ec, self.eg = make_engine(name, hop, True), make_engine(name, hop, False)
        trkw.setdefault("use_smoothing", False)
        self.tc = Trainer(self.ec, max_windows=BMAX, l1_weight=0.1, **trkw) if train else None
        self.tg = Trainer(self.eg, max_windows=BMAX, l1_weight=0.1, **trkw) if train else None

    def inputs(self, B, seed):
        return dev(synth.normal(seed, (B, self.ED))), dev(synth.uniform(seed + 1, (B, 52), 0, 1))

    def result(self, tr, B):
        torch.cuda.synchronize()
        return float(tr.loss.item()), tr.out[:B].clone(), tr.flat_grad.clone()

    def train_both(self, tag, clip_dev, starts, seed, extremes=None):
        B = len(starts)
        emo, target = self.inputs(B, seed)
        lo, hi = extremes if extremes else (min(starts), max(starts))
        assert self.tc.clip_supported() and not self.tg.clip_supported()
        assert self.ec.clip_plan(B, lo, hi, training=True)["route"] == 2
        self.tc.forward_backward_clip(clip_dev, dev(np.asarray(starts, np.int32)) if extremes else starts, emo, target, extremes=extremes)
        self.tg.forward_backward(gather(clip_dev, starts, self.name, self.hop), emo, target)
        assert_same_step(tag, self.result(self.tc, B), self.result(self.tg, B))

    def forward_both(self, tag, clip_dev, starts, seed, state=None, first=True, extremes=None, attention=False):
        """forward_clip on the option-on engine against forward_audio on the gathered windows on its twin; `state`: a pair of
        (B, 52) EMA states, one per engine, carried by the caller."""
        B = len(starts)
        emo = self.inputs(B, seed)[0]
        lo, hi = extremes if extremes else (min(starts), max(starts))
        assert self.ec.forward_clip_supported() and not self.eg.forward_clip_supported()
        assert self.ec.clip_plan(B, lo, hi, forward_attention=attention)["route"] == 2
        sc_, sg_ = state if state is not None else (None, None)
        got = self.ec.forward_clip(clip_dev, dev(np.asarray(starts, np.int32)) if extremes else starts, emo, state=sc_, first=first,
                                   extremes=extremes, return_attention=attention)
        want = self.eg.forward_audio(gather(clip_dev, starts, self.name, self.hop), emo, state=sg_, first=first, return_attention=attention)
        torch.cuda.synchronize()
        if attention:
            for key in ("blendshapes", "raw", "mel_attention_weights"):
                assert torch.equal(got[key], want[key]), (tag, key, float((got[key] - want[key]).abs().max()))
        else:
            assert torch.equal(got, want), (tag, float((got - want).abs().max()))
        if state is not None:
            assert torch.equal(sc_, sg_), (tag, "state")
        return got

    def close(self):
        self.tc = self.tg = None
        self.ec.close(); self.eg.close()


def assert_same_step(tag, a, b):
    assert a[0] == b[0], (tag, "loss", a[0], b[0])
    assert torch.equal(a[1], b[1]), (tag, "out", float((a[1] - b[1]).abs().max()))
    if not torch.equal(a[2], b[2]):
        bad = torch.nonzero(a[2] != b[2]).flatten()
        raise AssertionError(f"{tag}: flat_grad differs in {bad.numel()} of {a[2].numel()} entries, first at {int(bad[0])}, max "
                             f"{float((a[2] - b[2]).abs().max()):.3e}")


@pytest.fixture(scope="module", autouse=True)
def nothing_left_for_later_modules():
    """Every engine here is closed where it was made; should a failing test have left one behind, it is collected now, not inside
    another module's capture or between its readings of the memory counter."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def pairs():
    cache = {}

    def get(name, hop):
        if (name, hop) not in cache:
            cache[(name, hop)] = Pair(name, hop, train=(name, hop) in TRAIN_SHAPES)
        return cache[(name, hop)]
    yield get
    for p in cache.values():
        p.close()


def start_cases(T):
    """name -> (start frames, extremes or None).  The clip has T + 40 frames and 77 samples: the last full window starts at 40."""
    return {
        "0 1 2 9": ([0, 1, 2, 9], None),
        "unordered with a repeat": ([31, 7, 19, 7, 40, 2, 25, 13, 7], None),
        "one window, min_start > 0": ([21], None),
        "past clip_len": ([38, 41, 45, 60, T + 39], None),              # 41+: zeros at the end; T + 39: one frame and 77 samples
        "every window past the clip": ([T + 41, T + 50, 4000], None),
        "min_start > 0, dense": (list(range(10, 18)), None),
        "extremes wider than the batch's": ([12, 15, 13], (3, 30)),
    }


# ---- 1: equal bits with the gathered step / forward, case after case on ONE handle (so every call but the first is a second call) ----
@pytest.mark.parametrize("name,hop", TRAIN_SHAPES)
def test_training_step_equals_the_gathered_step(pairs, name, hop):
    p = pairs(name, hop)
    clip = dev(make_clip(name, hop, 700 + hop))
    for i, (case, (starts, extremes)) in enumerate(start_cases(p.T).items()):
        p.train_both(f"{name} hop {hop} {case}", clip, starts, 710 + i, extremes)
    p.train_both(f"{name} hop {hop} 0 1 2 9 again", clip, [0, 1, 2, 9], 710)


@pytest.mark.parametrize("name,hop", FORWARD_SHAPES)
def test_forward_equals_forward_audio_on_the_gathered_windows(pairs, name, hop):
    """out and the EMA state the caller carries: first call, then first=False on the same batch size."""
    p = pairs(name, hop)
    clip = dev(make_clip(name, hop, 720 + hop))
    for i, (case, (starts, extremes)) in enumerate(start_cases(p.T).items()):
        state = (torch.zeros(len(starts), 52, device="cuda"), torch.zeros(len(starts), 52, device="cuda"))
        a = p.forward_both(f"{name} hop {hop} {case}", clip, starts, 730 + i, state, True, extremes)
        b = p.forward_both(f"{name} hop {hop} {case} (second call)", clip, starts, 740 + i, state, False, extremes)
        assert not torch.equal(a, b)
    out = p.forward_both(f"{name} hop {hop} no state", clip, [0, 1, 2, 9], 750)
    assert len({out[i].cpu().numpy().tobytes() for i in range(4)}) == 4            # the windows differ


@pytest.mark.parametrize("name,hop", [s for s in FORWARD_SHAPES if s[0] != "fast"])
def test_maps_equal_forward_audio_on_the_gathered_windows(pairs, name, hop):
    """km_forward_clip_attn: the chain (or the fused core's ATTN form) behind the assembled workspace."""
    p = pairs(name, hop)
    clip = dev(make_clip(name, hop, 760 + hop))
    for i, starts in enumerate(([0, 1, 2, 9], [31, 7, 19, 7, 40], [p.T + 39, 5])):
        state = (torch.zeros(len(starts), 52, device="cuda"), torch.zeros(len(starts), 52, device="cuda"))
        p.forward_both(f"{name} hop {hop} maps {i}", clip, starts, 770 + i, state, True, attention=True)


def test_fast_needs_core128_for_its_power_path():
    """d_model 128 at hop 533: E = 1 without a fused core.  With core128 the forward runs on the new route (above); without it
    the forward call has no power path, the plan says 0 and the entry refuses as it always did; with maps asked for likewise."""
    e = make_engine("fast", 533, True, core128=0)
    assert e.clip_plan(4, 0, 9)["route"] == 0 and not e.forward_clip_supported()
    clip, emo = dev(make_clip("fast", 533, 780)), dev(synth.normal(781, (4, 256)))
    with pytest.raises(KoeMorphError, match="fused core"):
        e.forward_clip(clip, [0, 1, 2, 9], emo)
    e.set_option("core128", 1)
    assert e.clip_plan(4, 0, 9)["route"] == 2 and e.forward_clip_supported()
    assert e.clip_plan(4, 0, 9, forward_attention=True)["route"] == 0
    with pytest.raises(KoeMorphError, match="fused core"):
        e.forward_clip(clip, [0, 1, 2, 9], emo, return_attention=True)
    assert e.forward_clip(clip, [0, 1, 2, 9], emo).shape == (4, 52)
    e.close()


def test_e3_runs_where_sequence_mode_reports_route_2():
    e = cc.new_engine("d64 w32", 200, seq_assemble=1, clip_assemble=1)
    e.finalize_host()
    assert e.sequence_plan(40 * 200)["route"] == 2 and e.sequence_plan(40 * 200)["edge_frames_per_side"] == 3
    assert e.clip_plan(4, 0, 9, training=True) == {"route": 2, "span_rows": 42, "stft_frames": 42 + 48, "edge_frames_per_side": 3}
    e.close()


# ---- 2: the dB reference: stale maxima ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hop", [("d256 w512", 266), ("fused", 266), ("d64 w32", 200)])
def test_quiet_after_loud_and_a_silent_first_window(pairs, name, hop):
    p = pairs(name, hop)
    T = p.T
    loud = np.clip(make_clip(name, hop, 800, "uniform") * np.float32(8.0), -1.0, 1.0).astype(np.float32)
    quiet = (make_clip(name, hop, 801) * np.float32(1e-3)).astype(np.float32)
    silent = make_clip(name, hop, 802).copy()
    silent[:T * hop + 512] = 0.0                            # window 0 is zeros (maximum 0), and so is the left edge of window 1
    starts = [0, 1, 2, 9]
    outs = {}
    for i, (label, a) in enumerate((("loud", loud), ("quiet", quiet), ("silent", silent), ("quiet again", quiet))):
        clip = dev(a)
        p.train_both(f"{name} {label}", clip, starts, 810)
        outs[label] = p.forward_both(f"{name} {label}", clip, starts, 811).clone()
        p.forward_both(f"{name} {label} maps", clip, starts, 811, attention=True)
    assert torch.equal(outs["quiet"], outs["quiet again"]) and not torch.equal(outs["quiet"], outs["loud"])
    # a from-audio step and a forward_audio on the option-on handle behind them: the maxima were handed back clean
    W = T * hop
    qa = dev(synth.make_audio(812, 4, W) * np.float32(1e-3))
    emo, target = p.inputs(4, 813)
    p.tc.forward_backward(qa, emo, target)
    p.tg.forward_backward(qa, emo, target)
    assert_same_step(f"{name} from-audio step behind the clip steps", p.result(p.tc, 4), p.result(p.tg, 4))
    assert torch.equal(p.ec.forward_audio(qa, emo), p.eg.forward_audio(qa, emo))


@pytest.mark.parametrize("name,hop", [("d256 w512", 266), ("d64 w32", 266)])
def test_forward_audio_is_unchanged_by_clip_calls(pairs, name, hop):
    """No aliasing between the images and the inference workspace: forward_audio on a fixed batch before and after."""
    p = pairs(name, hop)
    W = p.T * hop
    fixed, emo = dev(synth.make_audio(820, 5, W)), p.inputs(5, 821)[0]
    before = p.ec.forward_audio(fixed, emo).clone()
    before_maps = p.ec.forward_audio(fixed, emo, return_attention=True)
    clip = dev(np.clip(make_clip(name, hop, 822, "uniform") * np.float32(8.0), -1.0, 1.0).astype(np.float32))
    p.train_both(f"{name} between", clip, [3, 4, 5, 6, 7, 30, 1], 823)
    p.forward_both(f"{name} between", clip, [3, 4, 5, 6, 7, 30, 1], 824)
    assert torch.equal(p.ec.forward_audio(fixed, emo), before)
    after_maps = p.ec.forward_audio(fixed, emo, return_attention=True)
    for key in before_maps:
        assert torch.equal(after_maps[key], before_maps[key]), key


# ---- 3: guard regions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hop", [("d256 w512", 266), ("fused", 266), ("d64 w32", 200)])
def test_nothing_outside_out_raw_and_the_maps_is_written(pairs, name, hop):
    p = pairs(name, hop)
    e = p.ec
    B, starts = 5, [9, 0, 40, 41, 3]
    clip, emo = guarded(make_clip(name, hop, 830)), guarded(synth.normal(831, (B, p.ED)))
    want = e.forward_clip(clip, starts, emo, return_attention=True)
    plain = e.forward_clip(clip, starts, emo)
    out, out2, raw = (guarded(np.zeros((B, 52), np.float32)) for _ in range(3))
    attn = guarded(np.zeros((B, 28, 80), np.float32))
    st = dev(np.asarray(starts, np.int32))
    stream = _stream_ptr(clip.device)
    check(e._lib.km_forward_clip_attn(e._h, _ptr(clip), clip.shape[0], _ptr(st), B, 0, 41, _ptr(emo), _ptr(out), None, 1, _ptr(raw), _ptr(attn),
                                      stream))
    check(e._lib.km_forward_clip(e._h, _ptr(clip), clip.shape[0], _ptr(st), B, 0, 41, _ptr(emo), _ptr(out2), None, 1, stream))
    torch.cuda.synchronize()
    assert torch.equal(out, want["blendshapes"]) and torch.equal(raw, want["raw"]) and torch.equal(attn, want["mel_attention_weights"])
    assert torch.equal(out2, plain)
    for t in (out, out2, raw, attn):
        base = t._base
        assert base.numel() == t.numel() + 2 * 1280
        assert torch.isnan(base[:1280]).all() and torch.isnan(base[-1280:]).all() and not torch.isnan(t).any()
    for t in (clip, emo):
        assert torch.isnan(t._base[:1280]).all() and torch.isnan(t._base[-1280:]).all() and not torch.isnan(t).any()
    # the training step reads the same guarded clip
    emo_t, target = guarded(synth.normal(832, (B, p.ED))), guarded(synth.uniform(833, (B, 52), 0, 1))
    p.tc.forward_backward_clip(clip, starts, emo_t, target)
    p.tg.forward_backward(gather(clip, starts, name, hop), emo_t, target)
    assert_same_step(f"{name} guarded", p.result(p.tc, B), p.result(p.tg, B))


# ---- 4: hipGraph replay ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hop", [("d256 w512", 266), ("d64 w32", 200)])
def test_captured_clip_step_replays_on_other_start_frames_and_clip_contents(name, hop):
    p = Pair(name, hop, use_smoothing=True)
    a, b = dev(make_clip(name, hop, 840)), dev(make_clip(name, hop, 841))
    buf = a.clone()
    emo0, target0 = p.inputs(8, 842)
    first = [0, 39, 1, 2, 3, 4, 5, 6]                       # one eager step: EMA past its first call, the images at the recorded width
    p.tc.forward_backward_clip(buf, first, emo0, target0)
    p.tg.forward_backward(gather(buf, first, name, hop), emo0, target0)
    assert_same_step("eager", p.result(p.tc, 8), p.result(p.tg, 8))
    p.tc.capture_clip(buf, 8, 0, 39)
    replays = ((a, [0, 1, 2, 3, 4, 5, 6, 7]), (b, [39, 12, 30, 31, 32, 5, 5, 0]), (a, [20, 21, 22, 23, 24, 25, 26, 27]), (b, [0, 1, 2, 3, 4, 5, 6, 7]))
    for i, (samples, starts) in enumerate(replays):
        emo, target = p.inputs(8, 850 + 2 * i)
        buf.copy_(samples)
        p.tc.replay_clip(starts, emo, target)
        p.tg.forward_backward(gather(samples, starts, name, hop), emo, target)
        assert_same_step(f"replay {i}", p.result(p.tc, 8), p.result(p.tg, 8))
        assert torch.equal(p.tc.ema_state, p.tg.ema_state), i
    p.tc._gc_graph = None
    p.close()


@pytest.mark.parametrize("name,hop", [("d256 w512", 266), ("fast", 533), ("fused", 266)])
def test_captured_forward_clip_replays_on_other_start_frames_and_clip_contents(name, hop):
    p = Pair(name, hop, train=False)
    B = 6
    a, b = dev(make_clip(name, hop, 860)), dev(make_clip(name, hop, 861))
    buf, emo_buf = a.clone(), torch.zeros(B, p.ED, device="cuda")
    starts_buf = torch.zeros(B, dtype=torch.int32, device="cuda")
    state_c, state_g = torch.zeros(B, 52, device="cuda"), torch.zeros(B, 52, device="cuda")
    out = torch.empty(B, 52, device="cuda")
    side = torch.cuda.Stream()                                # a warm-up call at the recorded span, on the capturing stream's side
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p.ec.forward_clip(buf, starts_buf, emo_buf, state=state_c, first=True, extremes=(0, 39), out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    p.eg.forward_audio(gather(buf, [0] * B, name, hop), emo_buf, state=state_g, first=True)
    assert torch.equal(state_c, state_g)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p.ec.forward_clip(buf, starts_buf, emo_buf, state=state_c, first=False, extremes=(0, 39), out=out)
    for i, (samples, starts) in enumerate(((b, [39, 12, 30, 5, 5, 0]), (a, [0, 1, 2, 3, 4, 5]), (b, [20, 21, 22, 23, 24, 25]))):
        emo = p.inputs(B, 870 + i)[0]
        buf.copy_(samples); emo_buf.copy_(emo); starts_buf.copy_(dev(np.asarray(starts, np.int32)))
        graph.replay()
        want = p.eg.forward_audio(gather(samples, starts, name, hop), emo, state=state_g, first=False)
        torch.cuda.synchronize()
        assert torch.equal(out, want), (i, float((out - want).abs().max()))
        assert torch.equal(state_c, state_g), i
    del graph
    p.close()


# ---- 5: the trainer of the 60 fps recipe ----------------------------------------------------------------------------------------
def write_pair(d, name, seconds, seed):
    n = int(seconds * 16000)
    wavfile.write(d / f"{name}.wav", 16000, synth.uniform(seed, (n,), -0.5, 0.5).astype(np.float32))
    F = int(seconds * 30)
    labels = synth.uniform(seed + 1, (F, 52), 0, 1).astype(np.float32)
    with open(d / f"{name}.jsonl", "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


def test_one_epoch_and_validation_at_60_fps_equal_the_gathered_epoch(tmp_path, monkeypatch):
    """d_model 256, 8 heads, window 512, hop 266; two clips of 522 and 518 labelled frames at batch 4: 11 and 7 windows, i.e.
    batches of 4, 4, 3 and 4, 3 -- a file change and a short last batch.  from_clip + clip_assemble against the gathered epoch: the loss, the
    weights and the optimizer state, bit for bit, dropout on; then validate(components=True): the same numbers."""
    from koemorph_amd.scripts import train_sequential as ts
    write_pair(tmp_path, "a", 8.7, 40)
    write_pair(tmp_path, "b", 8.65, 50)
    kw = dict(window_frames=512, target_fps=60, shuffle_files=False, loop_dataset=False, batch_size=4)
    sizes = [b["target"].shape[0] for b in SequentialKoeMorphDataset(tmp_path, **kw)]
    assert sizes == [4, 4, 3, 4, 3]
    steps, forwards = [], []
    orig_step, orig_forward = Trainer.step_clip, Engine.forward_clip
    monkeypatch.setattr(Trainer, "step_clip", lambda self, *a, **k: steps.append(self.clip_supported()) or orig_step(self, *a, **k))
    monkeypatch.setattr(Engine, "forward_clip", lambda self, *a, **k: forwards.append(int(a[1].numel())) or orig_forward(self, *a, **k))
    res = []
    for from_clip in (True, False):
        eng = cc.new_engine("d256 w512", 266, params=cc.params_for("d256 w512", seed=7))
        eng.finalize()
        data = SequentialKoeMorphDataset(tmp_path, resident_windows=from_clip, **kw)
        st = ts.SequentialTrainer(eng, data, data, learning_rate=1e-3, l1_weight=0.1, from_clip=from_clip, clip_assemble=from_clip, seed=3)
        if from_clip:
            assert eng.clip_plan(4, 0, 3, training=True)["route"] == 2 and st.trainer.clip_supported() and eng.forward_clip_supported()
        else:
            assert not st.trainer.clip_supported() and not eng.forward_clip_supported()
        m = st.train_epoch()
        v = st.validate(components=True)
        res.append((m["total"], m["batches"], st.state_dict(), st.trainer.optimizer_state(), v))
        eng.close()
    assert steps == [True] * 5 and forwards == sizes           # every step and every validation batch ran from the resident clip
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] == 5
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    oc, og = res[0][3], res[1][3]
    for key in ("exp_avg", "exp_avg_sq"):
        for k in oc[key]:
            assert torch.equal(oc[key][k], og[key][k]), (key, k)
    assert torch.equal(oc["steps"], og["steps"]) and oc["dropout_step"] == og["dropout_step"] > 0
    assert torch.equal(oc["ema_state"], og["ema_state"])
    assert res[0][4] == res[1][4] and res[0][4]["batches"] == 5 and list(res[0][4]["sequence_stats"]) == ["a", "b"]


# ---- 6: with the option off, and with it on where the default route runs ---------------------------------------------------------
def test_option_off_keeps_the_refusals_and_their_texts():
    e = make_engine("d512 h8", 266, False)
    tr = Trainer(e, max_windows=4, use_smoothing=False)
    lib = load()
    clip = dev(make_clip("d512 h8", 266, 880))
    starts = dev(np.asarray([0, 1, 2, 9], np.int32))
    emo, target = dev(synth.normal(881, (4, 256))), dev(synth.uniform(882, (4, 52), 0, 1))
    out = torch.empty(4, 52, device="cuda")
    e.reserve(4, 512 * 266)
    stream = torch.cuda.current_stream().cuda_stream
    for on in (0, 1, 0):
        e.set_option("clip_assemble", on)
        assert lib.km_train_clip_supported(e._h) == on and lib.km_forward_clip_supported(e._h) == on
        assert e.clip_plan(4, 0, 9, training=True)["route"] == e.clip_plan(4, 0, 9)["route"] == 2 * on
    rc = lib.km_train_step_clip(e._h, clip.data_ptr(), clip.shape[0], starts.data_ptr(), 4, 0, 9, emo.data_ptr(), target.data_ptr(), 1.0, 0.0,
                                tr.flat_grad.data_ptr(), tr.loss.data_ptr(), tr.out.data_ptr(), None, 1, stream)
    assert rc == KM_ERR_UNSUPPORTED
    msg = lib.km_last_error()
    assert b"hop >= n_fft / 2 (hop 266, n_fft 1024)" in msg and b"km_gather_windows" in msg and b"km_train_step_audio" in msg
    rc = lib.km_forward_clip(e._h, clip.data_ptr(), clip.shape[0], starts.data_ptr(), 4, 0, 9, emo.data_ptr(), out.data_ptr(), None, 1, stream)
    assert rc == KM_ERR_UNSUPPORTED
    msg = lib.km_last_error()
    assert b"needs the fused core (d_model 256, window 256, 8 heads)" in msg and b"(hop 266, n_fft 1024)" in msg and b"km_forward_audio" in msg
    # the wrappers gather: equal to the gathered step because it is the gathered step
    tr.forward_backward_clip(clip, [0, 1, 2, 9], emo, target)
    a = (float(tr.loss.item()), tr.out[:4].clone(), tr.flat_grad.clone())
    tr.forward_backward(gather(clip, [0, 1, 2, 9], "d512 h8", 266), emo, target)
    assert_same_step("gathered by the wrapper", a, (float(tr.loss.item()), tr.out[:4].clone(), tr.flat_grad.clone()))
    # reflect padding stays refused with the option on
    r = cc.new_engine("d64 w32", 266, reflect=True, clip_assemble=1)
    r.finalize()
    assert not r.forward_clip_supported() and not Trainer(r, max_windows=2).clip_supported()
    r.close()
    e.close()


def test_option_on_at_the_default_shape_is_the_default_route():
    """The fused shape at hop 533: km_clip_plan route 1 with the option on and off, and the same bits from either handle."""
    on, off = make_engine("fused", 533, True), make_engine("fused", 533, False)
    t_on, t_off = Trainer(on, max_windows=8, use_smoothing=False), Trainer(off, max_windows=8, use_smoothing=False)
    clip = dev(make_clip("fused", 533, 890))
    starts = [31, 7, 19, 7, 40, 2, 25, 13]
    emo, target = dev(synth.normal(891, (8, 256))), dev(synth.uniform(892, (8, 52), 0, 1))
    for e in (on, off):
        assert e.clip_plan(8, 2, 40, training=True) == e.clip_plan(8, 2, 40) == {"route": 1, "span_rows": 295, "stft_frames": 295 + 16,
                                                                                "edge_frames_per_side": 1}
    live = load().km_live_device_bytes
    held = live()
    res = []
    for e, tr in ((on, t_on), (off, t_off)):
        tr.forward_backward_clip(clip, starts, emo, target)
        state = torch.zeros(8, 52, device="cuda")
        o = e.forward_clip(clip, starts, emo, state=state)
        maps = e.forward_clip(clip, starts, emo, return_attention=True)
        torch.cuda.synchronize()
        res.append(((float(tr.loss.item()), tr.out[:8].clone(), tr.flat_grad.clone()), o, state, maps))
    assert_same_step("option on at the default shape", res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    for key in res[0][3]:
        assert torch.equal(res[0][3][key], res[1][3][key]), key
    gathered = make_engine("fused", 533, False)
    t_g = Trainer(gathered, max_windows=8, use_smoothing=False)
    t_g.forward_backward(gather(clip, starts, "fused", 533), emo, target)
    assert_same_step("the default route against the gathered step", res[1][0], (float(t_g.loss.item()), t_g.out[:8].clone(), t_g.flat_grad.clone()))
    # both handles grew the same buffers: the option-on handle allocated no image of the new route
    assert on._lib.km_live_device_bytes() >= held
    on.close(); off.close(); gathered.close()


# ---- 7: memory ------------------------------------------------------------------------------------------------------------------
def test_the_images_go_with_the_engine():
    live = _lib.load().km_live_device_bytes
    base = live()
    e = make_engine("d64 w32", 266, True)
    tr = Trainer(e, max_windows=4, use_smoothing=False)
    held = live()
    clip = dev(make_clip("d64 w32", 266, 900))
    tr.forward_backward_clip(clip, [0, 1, 2, 9], dev(synth.normal(901, (4, 256))), dev(synth.uniform(902, (4, 52), 0, 1)))
    grown = live()
    e.forward_clip(clip, list(range(9)), dev(synth.normal(903, (9, 256))))
    torch.cuda.synchronize()
    assert live() > grown > held > base                     # the span, snippet and edge images; a larger batch grows them
    del tr
    e.close()
    assert live() == base


def test_leak_check_passes():
    """tools/leak_check.py, two cycles in a process of its own: the library's count of live device bytes returns to its baseline."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "leak_check.py")], env={**os.environ, "REPS": "1"}, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "leak over 1 cycles: 0 bytes" in res.stdout
