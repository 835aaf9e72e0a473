"""The training step from a resident clip (km_train_step_clip / Trainer.forward_backward_clip): the windows of a batch share
the clip's STFT frames -- one front-end launch over the span + two boundary frames per window, one pack kernel -- and the
program behind the front end is km_train_step_audio's.

The bar is bit-identity with the pinned path, ``forward_backward(km_gather_windows(...))`` (tests/test_gpu_train_audio.py pins
that one to the float64 oracle): the frames are the same arithmetic, one frame per wave, whichever launch computes them, the
window maximum is a maximum over the same numbers, and ``db10`` is one function.  No tolerance anywhere below except in the one
direct oracle check, which restates test_gpu_train_audio's tier-A bounds through its own ``check``.

The window maxima live in a workspace no entry point reads back; "clean maxima afterwards" is therefore checked by what
depends on it: a quiet from-audio step and ``Engine.forward_audio`` behind a loud clip step give what they give without it.
"""
import ctypes
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import test_gpu_train_audio as ta
from koemorph_amd import synth
from koemorph_amd._lib import KM_ERR_UNSUPPORTED, KoeMorphError, check, load
from koemorph_amd.data import SequentialKoeMorphDataset
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.training import Trainer

pytestmark = pytest.mark.gpu

C3 = ta.C3
HOP, T = 533, 256
W = T * HOP


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_clip(seed, n_samples):
    return synth.make_audio(seed, 1, n_samples)[0]


def gather(clip_dev, starts, hop=HOP, window=W):
    """km_gather_windows: the (B, window) tensor the parent path trains on."""
    st = dev(np.asarray(starts, np.int32))
    out = torch.empty(len(starts), window, device="cuda")
    check(load().km_gather_windows(clip_dev.data_ptr(), clip_dev.shape[0], st.data_ptr(), len(starts), hop, window, out.data_ptr(),
                                   None, 0, 0, 0, None, None, torch.cuda.current_stream().cuda_stream))
    return out


def trainer(params, B, c=C3, mel_cfg=None, **kw):
    kw.setdefault("use_smoothing", False)
    return Trainer(ta.engine(params, c, mel_cfg), max_windows=B, **kw)


def result(tr, B):
    torch.cuda.synchronize()
    return float(tr.loss.item()), tr.out[:B].cpu().numpy().copy(), tr.flat_grad.cpu().numpy().copy()


def assert_same(tag, a, b):
    assert a[0] == b[0], (tag, "loss", a[0], b[0])
    assert np.array_equal(a[1], b[1]), (tag, "out", np.abs(a[1] - b[1]).max())
    if not np.array_equal(a[2], b[2]):
        bad = np.flatnonzero(a[2] != b[2])
        raise AssertionError(f"{tag}: flat_grad differs in {bad.size} of {a[2].size} entries, first at {bad[0]}, max "
                             f"{np.abs(a[2] - b[2]).max():.3e}")


def both_paths(tag, clip, starts, seed, params=None, **trkw):
    """One step on each path with a trainer of its own; returns the clip trainer."""
    B = len(starts)
    params = params if params is not None else synth.make_core_params(seed, style="trained")
    emo, target = dev(synth.normal(seed + 1, (B, 256))), dev(synth.uniform(seed + 2, (B, 52), 0, 1))
    clip_dev = dev(clip)
    tr_c, tr_g = trainer(params, B, **trkw), trainer(params, B, **trkw)
    assert tr_c.clip_supported()
    tr_c.forward_backward_clip(clip_dev, starts, emo, target)
    tr_g.forward_backward(gather(clip_dev, starts), emo, target)
    assert_same(tag, result(tr_c, B), result(tr_g, B))
    return tr_c, tr_g, clip_dev, emo, target


# ---- 1: bit-identity with the gathered step ------------------------------------------------------------------------------
N_CLIP = 300 * HOP + 77          # 300 full frames and a few samples: the last full window starts at frame 44

CASES = {
    "dense8": list(range(10, 18)),
    "stride3": list(range(0, 24, 3)),
    "shuffled_repeat": [31, 7, 19, 7, 40, 2, 25, 13],
    "single": [21],
    "first_and_last_full_window": [0, 44, 20, 43],
    "tail_past_clip_end": [41, 44, 45, 60, 130, 299],          # 45+: zeros at the end, 299: 77 samples, the rest zero
    "dense64": list(range(0, 64)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_clip_step_is_bit_identical_to_the_gathered_step(name):
    """loss, out and every gradient entry, np.array_equal.  dense64: split-K and the LayerNorm phase; tail_past_clip_end:
    windows whose samples beyond clip_len read as zeros, as the gather fills them (start 60 + 256 = 316 > 300 frames)."""
    starts = CASES[name]
    n = N_CLIP if name != "dense64" else 330 * HOP + 5
    tr_c, tr_g, clip_dev, emo, target = both_paths(name, make_clip(500 + len(starts), n), starts, 510 + len(name), l1_weight=0.1)
    # clean window maxima: the same quiet from-audio batch behind either step
    quiet = dev(synth.make_audio(520, len(starts), W) * 1e-3)
    tr_c.forward_backward(quiet, emo, target)
    tr_g.forward_backward(quiet, emo, target)
    assert_same(name + " (from-audio step behind it)", result(tr_c, len(starts)), result(tr_g, len(starts)))


def test_clip_step_when_every_window_lies_beyond_the_clip():
    """Start frames past the end: all-zero windows (every power at the amin floor), not an out-of-bounds read."""
    both_paths("beyond", make_clip(530, 40 * HOP), [40, 41, 100, 4000], 531)


# ---- 2: dropout, EMA, optimizer steps -------------------------------------------------------------------------------------
def test_clip_step_with_dropout_and_ema_over_two_steps_and_three_optimizer_steps():
    """Dropout 0.1 (same seed and step counter on both trainers), EMA inside the forward across consecutive steps, then
    three step_clip against three step: parameters and AdamW moments equal bit for bit."""
    params = synth.make_core_params(541, style="trained")
    clip = dev(make_clip(542, N_CLIP))
    kw = dict(use_smoothing=True, dropout=0.1, seed=77, l1_weight=0.1, lr=3e-3)
    tr_c, tr_g = trainer(params, 8, **kw), trainer(params, 8, **kw)
    for step in range(5):
        starts = list(range(8 * step, 8 * step + 8))
        emo, target = dev(synth.normal(550 + step, (8, 256))), dev(synth.uniform(560 + step, (8, 52), 0, 1))
        if step < 2:
            tr_c.forward_backward_clip(clip, starts, emo, target)
            tr_g.forward_backward(gather(clip, starts), emo, target)
        else:
            tr_c.step_clip(clip, dev(np.asarray(starts, np.int32)), emo, target, extremes=(starts[0], starts[-1]))
            tr_g.step(gather(clip, starts), emo, target)
        assert_same(f"step {step}", result(tr_c, 8), result(tr_g, 8))
        assert torch.equal(tr_c.ema_state, tr_g.ema_state), step
    sc, sg = tr_c.optimizer_state(), tr_g.optimizer_state()
    for key in ("exp_avg", "exp_avg_sq"):
        for k in sc[key]:
            assert torch.equal(sc[key][k], sg[key][k]), (key, k)
    assert sc["dropout_step"] == sg["dropout_step"] > 0 and torch.equal(sc["steps"], sg["steps"])
    shapes = {k: v.shape for k, v in params.items()}
    pc, pg = tr_c.params(shapes), tr_g.params(shapes)
    for k in shapes:
        assert np.array_equal(pc[k], pg[k]), k


# ---- 3: hipGraph replay ----------------------------------------------------------------------------------------------------
def test_captured_clip_step_replays_bit_identically_on_changed_start_frames():
    params = synth.make_core_params(571, style="trained")
    clip = dev(make_clip(572, N_CLIP))
    tr_g, tr_e = trainer(params, 8, use_smoothing=True), trainer(params, 8, use_smoothing=True)
    emo0, target0 = dev(synth.normal(573, (8, 256))), dev(synth.uniform(574, (8, 52), 0, 1))
    for tr in (tr_g, tr_e):              # one eager step: EMA past its first call, span image at the recorded width
        tr.forward_backward_clip(clip, [0, 39, 1, 2, 3, 4, 5, 6], emo0, target0)
    tr_g.capture_clip(clip, 8, 0, 39)
    for i, starts in enumerate(([0, 1, 2, 3, 4, 5, 6, 7], [39, 12, 30, 31, 32, 5, 5, 0], [20, 21, 22, 23, 24, 25, 26, 27])):
        emo, target = dev(synth.normal(580 + i, (8, 256))), dev(synth.uniform(590 + i, (8, 52), 0, 1))
        tr_g.replay_clip(starts, emo, target)
        tr_e.forward_backward_clip(clip, starts, emo, target)
        assert_same(f"replay {i}", result(tr_g, 8), result(tr_e, 8))
    with pytest.raises(ValueError):
        tr_g.replay_clip([40, 1, 2, 3, 4, 5, 6, 7], emo0, target0)


# ---- 4: inference behind a clip step ---------------------------------------------------------------------------------------
def test_forward_audio_is_unchanged_by_a_clip_step():
    """Clean window maxima and no aliasing between the clip images and the inference workspace: forward_audio on a fixed quiet
    batch before and after a loud clip step (no optimizer step, no weight sync: the inference weights are the same)."""
    params = synth.make_core_params(601, style="trained")
    e = ta.engine(params, C3)
    tr = Trainer(e, max_windows=8, use_smoothing=False)
    quiet, emo = dev(synth.make_audio(602, 8, W) * 1e-3), dev(synth.normal(603, (8, 256)))
    before = e.forward_audio(quiet, emo).clone()
    tr.forward_backward_clip(dev(make_clip(604, N_CLIP)), list(range(8)), emo, dev(synth.uniform(605, (8, 52), 0, 1)))
    after = e.forward_audio(quiet, emo)
    assert torch.equal(before, after)


# ---- 5: straight against the float64 oracle --------------------------------------------------------------------------------
def test_clip_step_matches_the_float64_oracle():
    """8 stride-1 windows cut from the clip on the host -> oracle.mel.mel_batch -> oracle.core.core_loss_and_grads, within
    test_gpu_train_audio's tier-A bounds (its ``check``, unchanged: loss 2e-6 relative, out 2e-6, gradients 1e-5 of each
    tensor's largest entry)."""
    params = synth.make_core_params(611, style="trained")
    clip = make_clip(612, N_CLIP)
    starts = list(range(5, 13))
    windows = np.stack([clip[s * HOP:s * HOP + W] for s in starts])
    emo, target = synth.normal(613, (8, 256)), synth.uniform(614, (8, 52), 0, 1)
    tr = trainer(params, 8, l1_weight=0.1)
    loss = float(tr.forward_backward_clip(dev(clip), starts, dev(emo), dev(target)).item())
    got = (loss, tr.out[:8].cpu().numpy().copy(), tr.grads({k: v.shape for k, v in params.items()}))
    want = ta.oracle_step(params, ta.oracle_features(windows), emo, target, C3, l1=0.1)
    ta.check("clip step vs oracle", got, want)


# ---- 6: shapes that cannot share frames ------------------------------------------------------------------------------------
def test_60fps_shape_reports_unsupported_and_still_trains_through_the_gather():
    """d_model 512, T 512, hop 266 < n_fft / 2: frames 1 and T - 1 see the window's padding as well, so the windows do not
    share their interior frames with the clip.  km_train_clip_supported is 0, the C entry refuses with a message, and
    Trainer.forward_backward_clip gathers: equal to the gathered step because it is the gathered step."""
    c = dict(d=512, H=8, T=512)
    cfg = MelConfig.model_batch(target_fps=60)
    assert cfg.hop_length == 266
    params = synth.make_core_params(621, 512, 512, 256, "trained")
    clip = dev(make_clip(622, 540 * 266))
    starts = [0, 1, 2, 9]
    emo, target = dev(synth.normal(623, (4, 256))), dev(synth.uniform(624, (4, 52), 0, 1))
    tr_c, tr_g = trainer(params, 4, c, cfg), trainer(params, 4, c, cfg)
    lib = load()
    assert lib.km_train_clip_supported(tr_c._h) == 0 and not tr_c.clip_supported()
    tr_c.engine.reserve(4, 512 * 266)
    st = dev(np.asarray(starts, np.int32))
    rc = lib.km_train_step_clip(tr_c._h, clip.data_ptr(), clip.shape[0], st.data_ptr(), 4, 0, 9, emo.data_ptr(), target.data_ptr(), 1.0, 0.0,
                                tr_c.flat_grad.data_ptr(), tr_c.loss.data_ptr(), tr_c.out.data_ptr(), None, 1,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == KM_ERR_UNSUPPORTED
    assert b"hop" in lib.km_last_error()
    with pytest.raises(KoeMorphError):
        check(rc)
    tr_c.forward_backward_clip(clip, starts, emo, target)
    tr_g.forward_backward(gather(clip, starts, 266, 512 * 266), emo, target)
    assert_same("60 fps fallback", result(tr_c, 4), result(tr_g, 4))
    # the default shape is supported only once the training state exists
    e = ta.engine(synth.make_core_params(625), C3)
    assert lib.km_train_clip_supported(e._h) == 0
    assert Trainer(e, max_windows=2).clip_supported()


def test_clip_step_argument_errors():
    tr = trainer(synth.make_core_params(631), 4)
    clip, emo, target = dev(make_clip(632, 300 * HOP)), dev(synth.normal(633, (4, 256))), dev(synth.uniform(634, (4, 52), 0, 1))
    with pytest.raises(ValueError):                                        # device start frames without their host extremes
        tr.forward_backward_clip(clip, dev(np.arange(4, dtype=np.int32)), emo, target)
    with pytest.raises(KoeMorphError):                                     # extremes the wrong way round
        tr.forward_backward_clip(clip, dev(np.arange(4, dtype=np.int32)), emo, target, extremes=(3, 0))
    with pytest.raises(KoeMorphError):                                     # more windows than km_train_init sized
        tr.forward_backward_clip(clip, list(range(5)), dev(synth.normal(635, (5, 256))), dev(synth.uniform(636, (5, 52), 0, 1)))


# ---- 7: data set and trainer -----------------------------------------------------------------------------------------------
def write_pair(d, name, seconds, seed):
    n = int(seconds * 16000)
    audio = synth.uniform(seed, (n,), -0.5, 0.5).astype(np.float32)
    wavfile.write(d / f"{name}.wav", 16000, audio)
    F = int(seconds * 30)
    labels = synth.uniform(seed + 1, (F, 52), 0, 1).astype(np.float32)
    with open(d / f"{name}.jsonl", "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


def test_resident_window_batches_and_one_epoch_from_the_clip(tmp_path):
    """Two clips of 267 and 264 frames at batch 5: 12 and 9 windows, so both end in a short batch and the file changes in
    between (EMA reset).  resident_windows batches carry gather()'s labels, targets and indices; one epoch with from_clip ends
    with the same loss and the same weights as one epoch on gathered batches, dropout on."""
    from koemorph_amd.scripts import train_sequential as ts
    write_pair(tmp_path, "a", 8.9, 40)
    write_pair(tmp_path, "b", 8.8, 50)
    kw = dict(shuffle_files=False, loop_dataset=False, batch_size=5)
    got = list(SequentialKoeMorphDataset(tmp_path, resident_windows=True, **kw))
    want = list(SequentialKoeMorphDataset(tmp_path, **kw))
    assert len(got) == len(want) >= 4 and {b["target"].shape[0] for b in want} > {5}
    for g, w in zip(got, want):
        assert "audio" not in g and g["clip_audio"].dim() == 1 and g["start_frames_dev"].dtype == torch.int32
        assert torch.equal(g["start_frames_dev"].cpu().long(), w["start_frames"])
        for k in ("blendshapes", "target", "file_indices", "window_indices", "start_frames"):
            assert torch.equal(g[k], w[k]), k
        assert g["file_names"] == w["file_names"]
        assert torch.equal(gather(g["clip_audio"], g["start_frames"].tolist()), w["audio"])
    res = []
    for from_clip in (True, False):
        eng = Engine(); eng.load_state_dict(synth.make_core_params(0)); eng.finalize()
        st = ts.SequentialTrainer(eng, SequentialKoeMorphDataset(tmp_path, resident_windows=from_clip, **kw), learning_rate=1e-3,
                                  l1_weight=0.1, from_clip=from_clip, seed=3)
        m = st.train_epoch()
        res.append((m["total"], m["batches"], st.state_dict()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] == len(want)
    for (k, a), (_, b) in zip(res[0][2].items(), res[1][2].items()):
        assert torch.equal(a, b), k
    # resident batches with from_clip off, or with an emotion provider, are gathered: still the same epoch
    eng = Engine(); eng.load_state_dict(synth.make_core_params(0)); eng.finalize()
    st = ts.SequentialTrainer(eng, SequentialKoeMorphDataset(tmp_path, resident_windows=True, **kw), learning_rate=1e-3,
                              l1_weight=0.1, from_clip=False, seed=3)
    assert st.train_epoch()["total"] == res[1][0]
