"""Device-resident streaming (km_stream_*) at the 60 fps long-context shape -- d_model 512, window 512, 8 / 16 heads,
update_interval 1/60 (ring hop 266), front end n_fft 1024 at hop 266 with reflect padding -- against the per-stream oracle
pipeline: MelAudioBuffer ring -> sliding-window dB mel -> core (float64) with last-3-kept-rows short rows -> EMA.

Tolerance.  The yardstick is the float64 oracle (tests/stream_d512_cases.py), never a second GPU path.  The project holds 5e-6
for the d_model 512 from-audio output against the oracle (tests/test_gpu_models.py, BASELINE config 4) and 2e-5 for the d_model
256 stream test.  Largest |hip - oracle| over the checked ticks x streams x 52 coefficients, one run on an MI355X:
    short ring (1.0 s), 8 heads    8.196e-08
    short ring (1.0 s), 16 heads   8.941e-08
    full ring (8.5 s), 8 heads     3.353e-08
BOUND[heads] is the largest figure of that head count times a margin of just under 4 (input-dependent rounding): 3.2e-7 and
3.5e-7, fifteen times below the existing d512 bound.  A wrong short-row choice, a wrong dB reference or a missed zero row shows
up at 1e-2 and above.
"""
import numpy as np
import pytest
import torch

import stream_d512_cases as sc
from koemorph_amd import synth
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.streaming import StreamEngine
from oracle import buffers

pytestmark = pytest.mark.gpu
BOUND = {8: 3.2e-7, 16: 3.5e-7}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def engine512(heads):
    e = Engine(d_model=512, num_heads=heads, mel_sequence_length=512, mel=MelConfig.model_batch(target_fps=60))
    e.load_state_dict(sc.params())
    e.finalize()
    return e


@pytest.mark.parametrize("heads", [8, 16])
def test_short_ring_matches_oracle(heads):
    """U = 60 kept rows of 61 computed, far below T = 512: zero rows 60 .. 511, short rows = kept rows 57 .. 59, and for stream 2
    a dB reference that lies in the dropped frame 60.  Frames of 266 / 267 samples alternately; the write pointer wraps at tick 60."""
    S = sc.SHORT_S
    se = StreamEngine(engine512(heads), S, context_window=sc.SHORT_CW, update_interval=sc.UI60)
    assert se.ring_hop == 266 and se.shape == dict(ring_len=16000, ring_hop=266, n_frames=61, stream_out_frames=60)
    emo = sc.short_emotion()
    sms = [sc.smoother() for _ in range(S)]
    worst = 0.0
    for t, frame in enumerate(sc.short_frames()):
        se.push(dev(frame))
        out, ready = se.tick(dev(emo))
        full = t >= sc.SHORT_FIRST_READY
        assert bool(ready.cpu().all()) == full and bool(ready.cpu().any()) == full, t
        if not full:
            assert not bool(out.cpu().any())             # no row is written before its ring is full
            continue
        got = out.cpu().numpy()
        for s in range(S):
            if t in sc.SHORT_CHECKED:
                want = sms[s](sc.short_expected(heads, t)[s:s + 1])
                worst = max(worst, float(np.abs(got[s] - want[0]).max()))
            else:   # keep the oracle EMA in step without paying for the mel: feed it the GPU value back
                sms[s].prev = got[s:s + 1].copy()
    assert worst < BOUND[heads], worst


def test_full_ring_matches_oracle_and_graph_replay():
    """8.5 s: ring 136000 samples, 512 frames computed, U = 510 kept, two zero rows.  Oracle on four ticks after the ring fills;
    from tick 513 on one engine replays a captured push + tick (pinned readback as the last node) while a second engine, fed the
    same samples, runs them eagerly: identical bits."""
    S, TICKS, FIRST, GRAPH_FROM = 2, 517, 511, 513
    emo = synth.normal(43, (S, 256))
    audio = synth.make_audio(42, S, 267 * TICKS)
    a, b = (StreamEngine(engine512(8), S, update_interval=sc.UI60) for _ in range(2))
    assert a.shape == dict(ring_len=136000, ring_hop=266, n_frames=512, stream_out_frames=510)
    rings = [buffers.MelAudioBufferOracle(8.5, sc.SR, sc.UI60) for _ in range(S)]
    sms = [sc.smoother() for _ in range(S)]
    host_out = torch.empty(S, 52).pin_memory()
    emo_d = dev(emo)
    worst, checked = 0.0, 0
    for t in range(TICKS):
        frame = audio[:, t * 267:(t + 1) * 267]
        fd = dev(frame)
        if t == GRAPH_FROM:
            a.capture(host_out=host_out)                 # default frame size: ring_hop + 1 = 267
            assert tuple(a._g_samples.shape) == (S, 267)
        if t >= GRAPH_FROM:
            out, ready = a.replay(fd, emo_d)
            torch.cuda.synchronize()
            assert np.array_equal(host_out.numpy(), out.cpu().numpy())
        else:
            a.push(fd)
            out, ready = a.tick(emo_d)
        b.push(fd)
        out_b, ready_b = b.tick(emo_d)
        assert torch.equal(out, out_b) and torch.equal(ready, ready_b), t
        for s in range(S):
            rings[s].add_audio_frame(frame[s])
        assert bool(ready.cpu().all()) == rings[0].is_full == (t >= FIRST)
        if t < FIRST:
            continue
        got = out.cpu().numpy()
        for s in range(S):
            if t in (511, 512, 514, 515):
                want = sms[s](sc.oracle_blendshapes(rings[s].get_current_audio(), emo[s], 8, 8.5))
                worst = max(worst, float(np.abs(got[s] - want[0]).max()))
                checked += 1
            else:
                sms[s].prev = got[s:s + 1].copy()
    assert checked == 8 and worst < BOUND[8], worst


def test_rows_and_state_of_a_stream_that_is_not_ready_are_left_alone():
    """Across the fill boundary: while the ring fills, a tick writes neither the stream's out row (a sentinel survives) nor its
    EMA state; reset() clears readiness, out and state, so the first ready tick after a refill is again the unsmoothed value --
    bit for bit what the first run gave -- and the second one is smoothed from it, not from anything older."""
    S = sc.SHORT_S
    se = StreamEngine(engine512(16), S, context_window=sc.SHORT_CW, update_interval=sc.UI60)
    emo = dev(sc.short_emotion())
    frames = [dev(f) for f in sc.short_frames()]

    def fill_and_two(sentinel):
        se.out.fill_(sentinel)
        for t in range(sc.SHORT_FIRST_READY):
            se.push(frames[t])
            out, ready = se.tick(emo)
            assert not bool(ready.any()) and bool((out == sentinel).all()), t
        res = []
        for t in (sc.SHORT_FIRST_READY, sc.SHORT_FIRST_READY + 1):
            se.push(frames[t])
            out, ready = se.tick(emo)
            assert bool(ready.all())
            res.append(out.clone())
        return res

    first = fill_and_two(7.0)
    assert float(first[0].max()) <= 1.0 and not torch.equal(first[0], first[1])
    se.reset()
    assert not bool(se.out.any()) and not bool(se.ready.any())
    again = fill_and_two(-3.0)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    # the first ready tick carries no history: the unsmoothed oracle value
    want = sc.short_expected(16, sc.SHORT_FIRST_READY)
    assert np.abs(first[0].cpu().numpy() - want).max() < BOUND[16]


def test_other_shapes_still_refuse():
    e = Engine(d_model=128, num_heads=4, mel_sequence_length=64)
    e.load_state_dict(synth.make_core_params(5, 128, 64, 256, "trained"))
    e.finalize()
    se = StreamEngine(e, 2, context_window=1.0)
    se.push(torch.zeros(2, se.ring_hop, device="cuda"))
    with pytest.raises(KoeMorphError, match="no kernel for d_model=128, mel_sequence_length=64, heads=4"):
        se.tick(torch.zeros(2, 256, device="cuda"))
