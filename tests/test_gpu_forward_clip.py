"""The eval-mode forward from a resident clip (km_forward_clip / Engine.forward_clip): the windows of a batch share the
clip's STFT frames -- one front-end launch over the span + two boundary frames per window -- the dB reference of a window is
the maximum over its own 257 frames, and the fused core finds its rows through the start-frame table.

The bar is bit-identity (``torch.equal``) with ``km_gather_windows`` + ``Engine.forward_audio`` on the same handle: the
frames are the same arithmetic whichever launch computes them, a maximum does not depend on the order, the emotion logits of
emotion_kernel_d256 are those of the rider inside forward_audio's front end, and behind phase 0 the core is one program.
Production fused shape throughout (d_model 256, T 256, 80 mels, n_fft 1024, hop 533); the clip is T + 40 frames and a bit.
"""
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from koemorph_amd import synth
from koemorph_amd._lib import KM_ERR_INVALID_ARG, KM_ERR_UNSUPPORTED, KM_PAD_REFLECT, KoeMorphError, check, load
from koemorph_amd.data import SequentialKoeMorphDataset
from koemorph_amd.engine import Engine, MelConfig

pytestmark = pytest.mark.gpu

HOP, T = 533, 256
W = T * HOP
N_CLIP = (T + 40) * HOP + 77         # the last full window starts at frame 40


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def gather(clip_dev, starts, hop=HOP, window=W):
    st = dev(np.asarray(starts, np.int32))
    out = torch.empty(len(starts), window, device="cuda")
    check(load().km_gather_windows(clip_dev.data_ptr(), clip_dev.shape[0], st.data_ptr(), len(starts), hop, window, out.data_ptr(),
                                   None, 0, 0, 0, None, None, torch.cuda.current_stream().cuda_stream))
    return out


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    e.load_state_dict(synth.make_core_params(701, style="trained"))
    e.finalize()
    assert e.forward_clip_supported()
    return e


@pytest.fixture(scope="module")
def clip():
    return dev(synth.make_audio(702, 1, N_CLIP)[0])


def emotion(seed, B):
    return dev(synth.normal(seed, (B, 256)))


def both(e, clip_dev, starts, emo, state_c=None, state_g=None, first=True):
    got = e.forward_clip(clip_dev, starts, emo, state=state_c, first=first)
    want = e.forward_audio(gather(clip_dev, starts), emo, state=state_g, first=first)
    return got, want


CASES = {
    "dense8": list(range(10, 18)),                           # 1: B = 8, stride 1
    "stride3_b5": list(range(4, 19, 3)),                     # 2: B = 5, stride 3
    "single": [21],                                          # 3: B = 1
    "unordered_repeat": [7, 0, 7, 31, 2],                    # 4: any order, a repeat (and min_start = 0)
    "tail_past_clip_end": [0, 40, 41, 60, 130, 295, 400],    # 5: zero tail (41+), window wholly beyond the clip (400), min_start 0
}


@pytest.mark.parametrize("name", list(CASES))
def test_forward_clip_is_bit_identical_to_the_gathered_forward(eng, clip, name):
    starts = CASES[name]
    emo = emotion(710 + len(starts), len(starts))
    sc, sg = torch.zeros(len(starts), 52, device="cuda"), torch.zeros(len(starts), 52, device="cuda")
    got, want = both(eng, clip, starts, emo, sc, sg, first=True)
    assert torch.equal(got, want), (name, (got - want).abs().max().item())
    assert torch.equal(sc, sg)
    # device start frames with host extremes, no state: the same bits again
    st = dev(np.asarray(starts, np.int32))
    again = eng.forward_clip(clip, st, emo, extremes=(min(starts), max(starts)))
    assert torch.equal(again, want)
    # clean window maxima: a quiet gathered batch behind it gives what it gives on a fresh engine state
    quiet = dev(synth.make_audio(720, len(starts), W) * 1e-3)
    a = eng.forward_audio(quiet, emo).clone()
    eng.forward_clip(clip, starts, emo)
    assert torch.equal(eng.forward_audio(quiet, emo), a)


def test_all_zero_clip(eng):
    """Silence: every power at the amin floor, the window maximum 0 -- the dB clamp path."""
    z = torch.zeros(N_CLIP, device="cuda")
    starts = [0, 1, 5, 40]
    got, want = both(eng, z, starts, emotion(730, 4))
    assert torch.equal(got, want) and torch.isfinite(got).all()


def test_two_chained_calls_carry_the_state(eng, clip):
    """first=True then first=False with the caller's (B, 52) state: out and state equal after each call."""
    sc, sg = torch.zeros(8, 52, device="cuda"), torch.zeros(8, 52, device="cuda")
    for i, (starts, first) in enumerate(((list(range(0, 8)), True), (list(range(8, 16)), False))):
        got, want = both(eng, clip, starts, emotion(740 + i, 8), sc, sg, first=first)
        assert torch.equal(got, want), i
        assert torch.equal(sc, sg), i


def test_graph_replay_on_two_start_frame_tables(eng, clip):
    """After one warm-up call with the span, forward_clip is captured for a fixed span (min 0, max 39) and replayed on two
    different tables inside it; each replay equals eager."""
    B = 8
    starts_dev = dev(np.arange(B, dtype=np.int32))
    emo, out, state = emotion(750, B), torch.empty(B, 52, device="cuda"), torch.zeros(B, 52, device="cuda")
    eng.forward_clip(clip, [0, 39, 1, 2, 3, 4, 5, 6], emo, state=state, first=True)          # warm-up: span image at the recorded width
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.forward_clip(clip, starts_dev, emo, state=state, first=False, extremes=(0, 39), out=out)
    for i, starts in enumerate(([39, 12, 30, 31, 32, 5, 5, 0], [20, 21, 22, 23, 24, 25, 26, 27])):
        starts_dev.copy_(torch.from_numpy(np.asarray(starts, np.int32)))
        s0 = dev(synth.uniform(760 + i, (B, 52), 0, 1))
        state.copy_(s0)
        g.replay()
        torch.cuda.synchronize()
        se = s0.clone()
        want = eng.forward_audio(gather(clip, starts), emo, state=se, first=False)
        assert torch.equal(out, want), i
        assert torch.equal(state, se), i


def test_sequence_forward_is_undisturbed(eng, clip):
    """km_sequence_forward on the same clip before and after a forward_clip call: identical bytes (the stride path and its
    buffers are untouched)."""
    audio, emo1 = clip[None, :], emotion(770, 1)
    before = eng.sequence_forward(audio, emo1, stride_frames=1).clone()
    eng.forward_clip(clip, [3, 9, 40, 0], emotion(771, 4))
    after = eng.sequence_forward(audio, emo1, stride_frames=1)
    assert before.shape[1] == 41 and torch.equal(before, after)


def test_argument_errors(eng, clip):
    lib, st = load(), torch.cuda.current_stream().cuda_stream
    starts, emo, out = dev(np.arange(4, dtype=np.int32)), emotion(780, 4), torch.empty(4, 52, device="cuda")
    eng.reserve(4, 0)
    call = lambda clip_p, n, st_p, B, lo, hi, emo_p, out_p: lib.km_forward_clip(eng._h, clip_p, n, st_p, B, lo, hi, emo_p, out_p, None, 1, st)
    ok = (clip.data_ptr(), clip.shape[0], starts.data_ptr(), 4, 0, 3, emo.data_ptr(), out.data_ptr())
    assert call(*ok) == 0
    for i, bad in ((0, None), (2, None), (6, None), (7, None), (3, 0), (3, -1), (1, 0)):
        args = list(ok); args[i] = bad
        assert call(*args) == KM_ERR_INVALID_ARG, (i, bad)
    assert call(ok[0], ok[1], ok[2], 4, 3, 0, ok[6], ok[7]) == KM_ERR_INVALID_ARG          # min > max
    assert call(ok[0], ok[1], ok[2], 4, -1, 3, ok[6], ok[7]) == KM_ERR_INVALID_ARG         # negative start frame
    with pytest.raises(ValueError):                                                        # device start frames without extremes
        eng.forward_clip(clip, starts, emo)
    with pytest.raises(ValueError):
        eng.forward_clip(clip, [0, 1, 2], emo)                                             # 3 windows, 4 emotion rows
    torch.cuda.synchronize()


# ---- which handles share frames: km_forward_clip_supported / km_train_clip_supported ---------------------------------------------
# Expected (forward, train), written out from the derivations in the library, not from what it returns:
#   both     the row-parallel 1024-point front end (n_fft 1024, not mel_two_frame), zero (constant) padding -- the span and
#            edge images are built for zeros --, 2 hop >= n_fft (frame f of a window spans [f hop - n_fft / 2, f hop + n_fft / 2),
#            so only then do frames 1 .. T - 1 stay clear of the window's padding: 2 * 533 >= 1024, 2 * 266 = 532 < 1024)
#   forward  + the fused core without its split-bf16 variant (core_split 3 has no table variant); the training options and
#            the dB constants do not matter to it
#   train    + the packing front end: neither train_no_fe_pack nor train_no_dma, log mode dB with top_db == db_add and
#            db_scale > 0 (under a negative scale the floor becomes a ceiling); core_split does not matter to it
# Every row is the supported base (fused shape, n_fft 1024, hop 533, constant padding, (dB + 80) / 80) with the named change.
SUPPORT_TABLE = [
    # mel config changes                        options                            forward  train
    ({},                                        {},                                1, 1),
    (dict(db_scale=2.0),                        {},                                1, 1),     # positive scale, top_db == db_add
    (dict(db_scale=-1.0 / 80.0),                {},                                1, 0),     # negative scale, top_db == db_add
    (dict(top_db=60.0),                         {},                                1, 0),     # top_db != db_add
    (dict(pad_mode=KM_PAD_REFLECT),             {},                                0, 0),
    (dict(hop_length=266),                      {},                                0, 0),
    (dict(n_fft=512),                           {},                                0, 0),     # 2 * 533 >= 512, but not the 1024-point kernel
    (dict(n_fft=512, hop_length=266),           {},                                0, 0),     # 2 * 266 >= 512 as well
    (dict(hop_length=266, pad_mode=KM_PAD_REFLECT), {},                            0, 0),
    ({},                                        dict(mel_two_frame=1),             0, 0),
    ({},                                        dict(core_split=3),                0, 1),
    ({},                                        dict(train_no_fe_pack=1),          1, 0),
    ({},                                        dict(train_no_dma=1),              1, 0),
    ({},                                        dict(core_split=3, train_no_dma=1), 0, 0),
    ({},                                        dict(train_no_fe_pack=1, train_no_dma=1), 1, 0),
    (dict(db_scale=-1.0 / 80.0),                dict(core_split=3),                0, 0),
    (dict(hop_length=266),                      dict(core_split=3, train_no_fe_pack=1), 0, 0),
    (dict(n_fft=512),                           dict(mel_two_frame=1),             0, 0),
]


def test_clip_supported_predicates_over_front_end_configurations_and_options():
    """km_forward_clip_supported and km_train_clip_supported on handles of the fused shape: one per mel configuration of
    SUPPORT_TABLE, the options switched on the live handle and back.  No forward or training launch: km_finalize, and
    km_train_init (one window) because km_train_clip_supported is 0 by contract before the training state exists."""
    lib = load()
    params = synth.make_core_params(795)
    handles = {}
    for mel_kw, opts, want_fwd, want_train in SUPPORT_TABLE:
        key = tuple(sorted(mel_kw.items()))
        if key not in handles:
            e = Engine(mel=MelConfig(**mel_kw))
            e.load_state_dict(params)
            e.finalize()
            assert lib.km_train_clip_supported(e._h) == 0                       # no training state yet
            check(lib.km_train_init(e._h, 1, torch.cuda.current_stream().cuda_stream))
            handles[key] = e
        e = handles[key]
        for k, v in opts.items():
            e.set_option(k, v)
        try:
            got = (lib.km_forward_clip_supported(e._h), lib.km_train_clip_supported(e._h))
        finally:
            for k in opts:
                e.set_option(k, 0)
        assert got == (want_fwd, want_train), (mel_kw, opts, got)
    torch.cuda.synchronize()


# ---- the 60 fps shape: no shared frames, no fused core ------------------------------------------------------------------
def write_pair(d, name, seconds, seed, fps=30):
    n = int(seconds * 16000)
    wavfile.write(d / f"{name}.wav", 16000, synth.uniform(seed, (n,), -0.5, 0.5).astype(np.float32))
    F = int(seconds * fps)
    labels = synth.uniform(seed + 1, (F, 52), 0, 1).astype(np.float32)
    with open(d / f"{name}.jsonl", "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / float(fps), "blendshapes": labels[i].tolist()}) + "\n")


def test_60fps_shape_reports_unsupported_and_validation_gathers(tmp_path):
    """d_model 512, window 512, hop 266 < n_fft / 2: forward_clip_supported() is false, km_forward_clip returns
    KM_ERR_UNSUPPORTED, and validate(components=True) on resident-window batches runs through the gathered path with the
    default call's total."""
    from koemorph_amd.scripts import train_sequential as ts
    cfg = MelConfig.model_batch(target_fps=60)
    assert cfg.hop_length == 266
    e = Engine(d_model=512, num_heads=8, mel_sequence_length=512, mel=cfg)
    e.load_state_dict(synth.make_core_params(790, 512, 512, 256, "trained"))
    e.finalize()
    lib = load()
    assert lib.km_forward_clip_supported(e._h) == 0 and not e.forward_clip_supported()
    clip = dev(synth.make_audio(791, 1, 540 * 266)[0])
    starts, emo, out = dev(np.asarray([0, 1, 2, 9], np.int32)), emotion(792, 4), torch.empty(4, 52, device="cuda")
    e.reserve(4, 512 * 266)
    rc = lib.km_forward_clip(e._h, clip.data_ptr(), clip.shape[0], starts.data_ptr(), 4, 0, 9, emo.data_ptr(), out.data_ptr(), None, 1,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == KM_ERR_UNSUPPORTED and b"hop" in lib.km_last_error()
    with pytest.raises(KoeMorphError):
        e.forward_clip(clip, [0, 1, 2, 9], emo)
    write_pair(tmp_path, "a", 8.7, 60, fps=60)               # 522 frames: 11 windows of 512 at batch 4 -> 4 + 4 + 3
    data = SequentialKoeMorphDataset(tmp_path, resident_windows=True, window_frames=512, shuffle_files=False, loop_dataset=False,
                                     batch_size=4, target_fps=60)
    assert data.hop_length == 266
    calls = []
    orig = Engine.forward_clip
    Engine.forward_clip = lambda self, *a, **k: calls.append(1) or orig(self, *a, **k)
    try:
        st = ts.SequentialTrainer(e, data, data, from_clip=True, dropout=0.0)
        v0 = st.validate()
        v1 = st.validate(components=True)
    finally:
        Engine.forward_clip = orig
    assert not calls and v1["batches"] == v0["batches"] >= 2
    # the default call reduces each batch's n <= 4 * 52 squared errors in float32 (worst case n roundings of 2^-24, + the squares'
    # and the division's), the component call in float64 with one float32 rounding of the mean
    assert abs(v1["total"] - v0["total"]) <= (4 * 52 + 3) * 2.0 ** -24 * v0["total"]
    assert set(v1["sequence_stats"]) == {"a"} and v1["sequence_stats"]["a"]["batches"] == v0["batches"]
