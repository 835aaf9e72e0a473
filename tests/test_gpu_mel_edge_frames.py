"""Edge frames of mel_power_rp_kernel: the frames that touch the padding or a ring's wrap point go through the out-of-line
loader (load_frame_rp_edge: block-wise, one memory round trip), and the last frame of a window with n_frames % 16 == 1 is a
chunk of its own.  Interior frames take the frame loop's fast path.

a. the same samples give the same row, bit for bit, whether a frame is an edge frame (or the lone last frame) of one clip or an
   interior frame of an ordinary chunk of another: clip A against A extended at its tail (B) and at its head (C) by what the
   padding would have supplied.  Rows are ln(P + eps) with no per-window reference, so rows of different clips compare directly.
b. oracle parity (run_case / judge of test_gpu_mel_power.py, its yardstick) at the frame counts around the chunk size.
c. the last frame feeds the window maximum: forward_audio with the loudest samples in the last frame only, against the oracle
   chain and against the staged pipeline.
d. a ring whose wrap point lies inside the first frame on one tick and inside the last (257th) frame on another.
e. the training front end's packed rows at 17 frames against the phase-0 conversion.
"""
import numpy as np
import pytest
import torch

from koemorph_amd import synth
from koemorph_amd.engine import Engine, MelConfig
from oracle import models
from test_gpu_mel_power import PROD, dev, eng, mel_config, run_case  # noqa: F401  (eng: module-scoped fixture)

pytestmark = pytest.mark.gpu

WINDOWS = 3


def _rows(e, kw, audio):
    y = e.mel_extract(mel_config(kw), dev(audio)).clone()
    assert bool(torch.isfinite(y).all())
    return y


def _extended(a, n, pad, tail):
    """a with n samples behind it (tail) or ahead of it, as the padding supplies them: zeros, or the reflection about the clip's
    last / first sample (np.pad(mode='reflect'): A[L - 2 - k] behind, A[1 + k] read backwards ahead)."""
    ext = np.zeros((a.shape[0], n), np.float32)
    if pad == "reflect":
        m = min(n, a.shape[1] - 1)                 # (the reflection holds L - 1 samples; no frame compared here reads further)
        if tail:
            ext[:, :m] = a[:, ::-1][:, 1:1 + m]
        else:
            ext[:, n - m:] = a[:, m:0:-1]
    return np.ascontiguousarray(np.concatenate([a, ext] if tail else [ext, a], axis=1))


@pytest.mark.parametrize("pad", ["reflect", "constant"])
@pytest.mark.parametrize("hop,n", [(533, 17), (266, 33)])
def test_edge_and_lone_frames_equal_interior_frames(eng, hop, n, pad):
    kw = dict(PROD, hop=hop, pad_mode=pad)
    L = (n - 1) * hop
    a = synth.make_audio(4000 + hop, WINDOWS, L, "uniform")
    ya = _rows(eng, kw, a)
    assert ya.shape == (WINDOWS, n, 80)
    # tail: twice the length; rows 0 .. n - 1 see the same samples, the last ones now from the clip instead of the padding
    yb = _rows(eng, kw, _extended(a, L, pad, tail=True))
    assert yb.shape[1] == 2 * n - 1
    assert torch.equal(ya, yb[:, :n]), (hop, pad, "tail", float((ya - yb[:, :n]).abs().max()))
    # head: ceil(512 / hop) hops ahead; row f of A is row f + h of C, where frame 0 and the lone last frame of A are interior
    # frames of ordinary chunks
    h = -(-512 // hop)
    yc = _rows(eng, kw, _extended(a, h * hop, pad, tail=False))
    assert yc.shape[1] == n + h
    assert torch.equal(ya, yc[:, h:]), (hop, pad, "head", float((ya - yc[:, h:]).abs().max()))


def _parity_cases():
    out = []
    for hop in (533, 266):
        for n in (1, 2, 16, 17, 18, 33, 49):
            L = (n - 1) * hop + 5
            for pad in ("constant", "reflect"):
                if pad == "constant" or L > 512:
                    out.append((hop, n, pad))
    return out


@pytest.mark.parametrize("hop,n,pad", _parity_cases())
def test_oracle_parity_where_the_chunk_count_switches(eng, hop, n, pad):
    L = (n - 1) * hop + 5
    kw = dict(PROD, hop=hop, pad_mode=pad)
    y0 = run_case(eng, f"edge frames hop={hop} n={n} {pad}", synth.make_audio(4100 + n, WINDOWS, L, "uniform"), kw)
    assert y0.shape == (WINDOWS, n, 80)


@pytest.fixture(scope="module")
def model_eng():
    e = Engine()
    e.load_state_dict(synth.make_core_params(7, style="trained"))
    e.finalize()
    yield e
    e.close()


def test_lone_frame_reaches_the_window_maximum(model_eng):
    """3 windows x 8528 samples = 17 frames at hop 533; frame 16 spans the samples from 8016 on, frame 15 ends at 8507: the loud
    samples lie in frame 16 alone, so the window maximum (the dB reference of every row) comes from the lone frame."""
    L = 16 * 533
    audio = 0.01 * synth.make_audio(4200, WINDOWS, L, "uniform")
    audio[:, 8510:] = synth.make_audio(4201, WINDOWS, L - 8510, "uniform")
    assert np.abs(audio[:, 8510:]).max() > 10 * np.abs(audio[:, :8510]).max()
    emo = synth.normal(4202, (WINDOWS, 256))
    orc = models.SimplifiedOracle(synth.make_core_params(7, style="trained"))
    want = orc.forward(audio, emo, smooth=False)["blendshapes"]
    got = model_eng.forward_audio(dev(audio), dev(emo))
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"EDGEFRAMES|forward_audio, maximum in the lone frame|{err:.2e}")
    assert err < 1e-4, err
    assert err < 5e-6, err
    long, short = model_eng.mel_batch(dev(audio))
    assert long.shape[1] == 17
    staged = model_eng.core_forward(long, short, dev(emo))["blendshapes"]
    assert torch.equal(got, staged)
    assert torch.equal(model_eng.forward_audio(dev(audio), dev(emo)), got)


# ---- ring: 257 frames (136448 samples), pushes of 530 ------------------------------------------------------------------------
RING_LEN, RING_HOP, RING_CW, RING_UI = 136448, 530, 8.528, 0.03315


def _wrap_ticks():
    """The first tick (of a full ring) whose wrap point lies inside frame 0's samples, and the first inside frame 256's:
    logical sample q sits at (w + q) mod RING_LEN, w the write pointer; frame 0 reads q in [0, 512), frame 256 q in
    [135936, 136448)."""
    found, n = {}, -(-RING_LEN // RING_HOP)
    while len(found) < 2 and n < 100000:
        w = (n * RING_HOP) % RING_LEN
        if "first" not in found and RING_LEN - 512 < w < RING_LEN:
            found["first"] = n
        if "last" not in found and 0 < w < 512:
            found["last"] = n
        n += 1
    return found


def test_ring_wrap_inside_the_first_and_the_last_frame():
    from koemorph_amd.streaming import StreamEngine, stream_shape
    S = 3
    shape = stream_shape(RING_CW, RING_UI, 533)
    assert shape == dict(ring_len=RING_LEN, ring_hop=RING_HOP, n_frames=257, stream_out_frames=257)
    ticks = _wrap_ticks()
    assert set(ticks) == {"first", "last"}
    cfg = MelConfig.sliding_window(n_fft=1024, hop_length=533)
    e = Engine(mel=cfg)
    e.load_state_dict(synth.make_core_params(7, style="trained"))
    e.finalize()
    se = StreamEngine(e, S, context_window=RING_CW, update_interval=RING_UI, mel=cfg)
    assert se.ring_hop == RING_HOP
    pool = synth.make_audio(4300, S, RING_HOP * 67, "uniform")
    emo = dev(synth.normal(4301, (S, 256)))
    ring = np.zeros((S, RING_LEN), np.float32)
    state = torch.zeros(S, 52, device="cuda")
    w, first = 0, True
    for n in range(1, max(ticks.values()) + 1):
        chunk = pool[:, (n % 67) * RING_HOP:(n % 67 + 1) * RING_HOP] * np.float32(0.25 + 0.125 * ((n // 67) % 7))
        se.push(dev(chunk))
        ring[:, (w + np.arange(RING_HOP)) % RING_LEN] = chunk
        w = (w + RING_HOP) % RING_LEN
        if n in ticks.values():
            out, ready = se.tick(emo)
            assert bool(ready.all())
            want = e.forward_audio(dev(np.roll(ring, -w, axis=1)), emo, state=state, first=first)
            assert torch.equal(out, want), (n, w, float((out - want).abs().max()))
            assert float(want.std()) > 1e-3
            first = False
    e.close()


def test_training_pack_at_17_frames():
    """The from-audio training step at 2 windows of 17 frames (window 16: the 17th frame is the second of the three short rows
    and a chunk of its own): the front end's packed rows against the phase-0 conversion (train_no_fe_pack), at the tolerances of
    test_front_end_packed_input_agrees_with_the_phase_0_conversion."""
    from koemorph_amd.training import Trainer
    d, H, T, B = 64, 4, 16, 2
    params = synth.make_core_params(3, d, T, 256, "trained")
    L = T * 533
    audio, emo, target = dev(synth.make_audio(4400, B, L)), dev(synth.normal(4401, (B, 256))), dev(synth.uniform(4402, (B, 52), 0, 1))
    res = []
    for no_pack in (0, 1):
        e = Engine(d_model=d, num_heads=H, mel_sequence_length=T)
        e.load_state_dict(params)
        e.finalize()
        e.set_option("train_no_fe_pack", no_pack)
        tr = Trainer(e, max_windows=B, lr=1e-3, dropout=0.1)
        tr.set_dropout(0.1, seed=5)
        loss = float(tr.forward_backward(audio, emo, target).item())
        res.append((loss, tr.flat_grad.cpu().numpy().copy()))
        e.close()
    (l0, g0), (l1, g1) = res
    assert np.isfinite(l1) and np.abs(g1).max() > 0
    print(f"EDGEFRAMES|training pack at 17 frames|loss {abs(l0 - l1):.2e}|gradient {np.abs(g0 - g1).max() / np.abs(g1).max():.2e}")
    np.testing.assert_allclose(l0, l1, rtol=2e-6)
    assert np.abs(g0 - g1).max() <= 2e-5 * np.abs(g1).max()
