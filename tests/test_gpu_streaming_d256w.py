"""Device-resident streaming (km_stream_*) at the shape of the reference's frame_rate=60 recipe -- d_model 256, 8 heads, window
512, update_interval 1/60 (ring hop 266), front end n_fft 1024 at hop 266 with reflect padding -- served by
core256w_stream_kernel, against the per-stream oracle pipeline of tests/test_gpu_streaming_d512.py: MelAudioBuffer ring ->
sliding-window dB mel -> core (float64) with last-3-kept-rows short rows -> EMA.

Tolerance.  The yardstick is the float64 oracle (tests/stream_d256w_cases.py), never a second GPU path.  Largest |hip - oracle|
over the checked ticks x streams x 52 coefficients, one run on an MI355X:
    short ring (1.0 s), six checked ticks x 3 streams          3.353e-08
    full ring (8.5 s), four oracle ticks x 2 streams           7.451e-08
BOUND is the larger figure times 4 (2.98e-7), the margin tests/test_gpu_streaming_d512.py takes for input-dependent rounding; it
is below 2e-5, the project's d_model 256 stream bound.  A wrong short-row choice, a wrong dB reference or a missed zero row shows up at
1e-2 and above.
"""
import numpy as np
import pytest
import torch

import stream_d256w_cases as wc
import stream_d512_cases as sc
from core_logit_cases import K
from koemorph_amd import synth
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEngine
from oracle import buffers, core

pytestmark = pytest.mark.gpu
MEASURED = dict(short=3.353e-08, full=7.451e-08)
BOUND = 4 * max(MEASURED.values())
assert BOUND <= 2e-5


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def engine256w():
    e = Engine(d_model=wc.D_MODEL, num_heads=wc.HEADS, mel_sequence_length=wc.WINDOW, mel=MelConfig.model_batch(target_fps=60))
    e.load_state_dict(wc.params())
    e.finalize()
    assert e.core_route() == 2
    return e


def test_short_ring_matches_oracle():
    """U = 60 kept rows of 61 computed, far below T = 512: zero rows 60 .. 511, short rows = kept rows 57 .. 59, and for stream 2
    a dB reference that lies in the dropped frame 60.  Frames of 266 / 267 samples alternately; the write pointer wraps at tick 60."""
    S = sc.SHORT_S
    se = StreamEngine(engine256w(), S, context_window=sc.SHORT_CW, update_interval=sc.UI60)
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
                want = sms[s](wc.short_expected(t)[s:s + 1])
                worst = max(worst, float(np.abs(got[s] - want[0]).max()))
            else:   # keep the oracle EMA in step without paying for the mel: feed it the GPU value back
                sms[s].prev = got[s:s + 1].copy()
    print(f"STREAM256W|short ring|{worst:.3e}")
    assert worst < BOUND, worst


def test_full_ring_matches_oracle_and_graph_replay():
    """8.5 s: ring 136000 samples, 512 frames computed, U = 510 kept, two zero rows.  Oracle on four ticks after the ring fills;
    from tick 513 on one engine replays a captured push + tick (pinned readback as the last node) while a second engine, fed the
    same samples, runs them eagerly: identical bits."""
    S, TICKS, FIRST, GRAPH_FROM = 2, 517, 511, 513
    emo = synth.normal(43, (S, 256))
    audio = synth.make_audio(42, S, 267 * TICKS)
    a, b = (StreamEngine(engine256w(), S, update_interval=sc.UI60) for _ in range(2))
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
                want = sms[s](wc.oracle_blendshapes(rings[s].get_current_audio(), emo[s], 8.5))
                worst = max(worst, float(np.abs(got[s] - want[0]).max()))
                checked += 1
            else:
                sms[s].prev = got[s:s + 1].copy()
    print(f"STREAM256W|full ring|{worst:.3e}")
    assert checked == 8 and worst < BOUND, worst


def test_rows_and_state_of_a_stream_that_is_not_ready_are_left_alone():
    """Across the fill boundary: while the ring fills, a tick writes neither the stream's out row (a sentinel survives) nor its
    EMA state; reset() clears readiness, out and state, so the first ready tick after a refill is again the unsmoothed value --
    bit for bit what the first run gave -- and the second one is smoothed from it, not from anything older."""
    S = sc.SHORT_S
    se = StreamEngine(engine256w(), S, context_window=sc.SHORT_CW, update_interval=sc.UI60)
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
    want = wc.short_expected(sc.SHORT_FIRST_READY)
    assert np.abs(first[0].cpu().numpy() - want).max() < BOUND


# ---- streams out of phase ------------------------------------------------------------------------------------------------------------
FRAME = 266                  # int(16000 / 60): what a step pops
JOIN, RESET_AT, STEPS = 10, 65, 130          # stream 1 brings its first frame at step 10; stream 2 is reset before step 65
FULL_AFTER = 61              # frames of 266 samples that fill the 16000-sample ring


def chunk_audio():
    return synth.make_audio(47, 3, FRAME * STEPS)


def popped(audio, s, j):
    """The j-th frame stream s ever pops: every stream consumes its own audio in order."""
    return audio[s, j * FRAME:(j + 1) * FRAME]


def test_chunked_engine_late_joiner_and_reset_stream_equal_the_lockstep_engine():
    """ChunkedStreamEngine on the short ring: stream 0 in step from the start, stream 1 ten steps late, stream 2 reset before step 65
    and refilled.  Every fired row is, bit for bit, the row the lockstep engine gives at the same frame of that stream's life; a row
    that did not fire keeps the step's sentinel; fired and ready follow the frame counts."""
    audio, emo = chunk_audio(), dev(sc.short_emotion())
    se = ChunkedStreamEngine(engine256w(), 3, context_window=sc.SHORT_CW, update_interval=sc.UI60)
    assert se.chunk == dict(fifo_samples=32000, frame_samples=FRAME, ring_hop=266)
    got, fired = np.zeros((STEPS, 3, 52), np.float32), np.zeros((STEPS, 3), bool)
    taken = [0, 0, 0]                                    # frames each stream has brought so far
    life_start = [0, JOIN, 0]                            # the step at which the stream's current life began
    frame_of = {}                                        # (step, stream) -> (life, index of the popped frame within the life)
    for t in range(STEPS):
        if t == RESET_AT:
            se.reset_streams(dev(np.array([0, 0, 1], np.uint8)))
            assert not bool(se.out[2].any()) and bool(se.out[0].any())
            life_start[2] = t
        chunk, counts = np.zeros((3, FRAME), np.float32), np.zeros(3, np.int32)
        for s in range(3):
            if s == 1 and t < JOIN:
                continue
            chunk[s], counts[s] = popped(audio, s, taken[s]), FRAME
            frame_of[(t, s)] = (int(s == 2 and t >= RESET_AT), t - life_start[s])
            taken[s] += 1
        se.out.fill_(1000.0 + t)
        se.feed(dev(chunk), dev(counts))
        out, f = se.step(emo)
        got[t], fired[t] = out.cpu().numpy(), f.cpu().numpy().astype(bool)
        want_fired = [(t, s) in frame_of and frame_of[(t, s)][1] >= FULL_AFTER - 1 for s in range(3)]
        assert fired[t].tolist() == want_fired and se.ready.cpu().numpy().astype(bool).tolist() == want_fired, t
        assert not se.backlog.cpu().numpy().any()
        for s in range(3):
            if not fired[t, s]:
                assert bool((got[t, s] == 1000.0 + t).all()), (t, s)
    # the lockstep twin: life 0 of every stream side by side, then (after reset()) life 1 of stream 2 alone
    twin = StreamEngine(engine256w(), 3, context_window=sc.SHORT_CW, update_interval=sc.UI60)
    rows = {}
    for life, n in ((0, STEPS), (1, STEPS - RESET_AT)):
        if life:
            twin.reset()
        for k in range(n):
            frame = np.zeros((3, FRAME), np.float32)
            for s in range(3):
                j = k if life == 0 else RESET_AT + k
                if (life == 0 and j < taken[s] and not (s == 2 and j >= RESET_AT)) or (life == 1 and s == 2):
                    frame[s] = popped(audio, s, j)
            twin.push(dev(frame))
            o, r = twin.tick(emo)
            assert bool(r.cpu().all()) == (k >= FULL_AFTER - 1)
            rows[(life, k)] = o.cpu().numpy()
    compared = 0
    for (t, s), (life, k) in frame_of.items():
        if fired[t, s]:
            assert np.array_equal(got[t, s], rows[(life, k)][s]), (t, s, life, k)
            compared += 1
    assert compared == (STEPS - 60) + (STEPS - JOIN - 60) + (RESET_AT - 60) + (STEPS - RESET_AT - 60)


def test_step_with_the_attention_outputs():
    """One step with return_attention=True, at the step where streams 0 and 2 fire for the first time and the late stream 1 does
    not: out, fired and ready are those of the plain step on a twin engine, bit for bit; the rows of stream 1 in out, raw and the
    map are untouched; raw times the stream weights is out (no EMA history yet); the map of a fired stream meets the attention
    bound of tests/test_gpu_core_logit.py against the oracle on the device's own features of the stream's ring."""
    audio, emo = chunk_audio(), sc.short_emotion()
    emo_d = dev(emo)
    plain, attn = (ChunkedStreamEngine(engine256w(), 3, context_window=sc.SHORT_CW, update_interval=sc.UI60) for _ in range(2))
    extra = attn.attention_outputs()
    rings = [buffers.MelAudioBufferOracle(sc.SHORT_CW, sc.SR, sc.UI60) for _ in range(3)]
    for t in range(FULL_AFTER):
        chunk, counts = np.zeros((3, FRAME), np.float32), np.zeros(3, np.int32)
        for s in range(3):
            if s == 1 and t < JOIN:
                continue
            chunk[s], counts[s] = popped(audio, s, t - (JOIN if s == 1 else 0)), FRAME
            rings[s].add_audio_frame(chunk[s])
        last = t == FULL_AFTER - 1
        for se in (plain, attn):
            se.out.fill_(1000.0 + t)
            se.feed(dev(chunk), dev(counts))
        out_p, fired_p = plain.step(emo_d)
        if last:
            extra["raw"].fill_(-7.0)
            extra["mel_attention_weights"].fill_(-7.0)
            out_a, fired_a, got = attn.step(emo_d, return_attention=True)
        else:
            out_a, fired_a = attn.step(emo_d)
        assert torch.equal(out_p, out_a) and torch.equal(fired_p, fired_a) and torch.equal(plain.ready, attn.ready), t
    assert fired_a.cpu().tolist() == [1, 0, 1]
    raw, maps, out = got["raw"].cpu().numpy(), got["mel_attention_weights"].cpu().numpy(), out_a.cpu().numpy()
    assert (raw[1] == -7.0).all() and (maps[1] == -7.0).all() and (out[1] == 1000.0 + FULL_AFTER - 1).all()
    fe = engine256w()                                     # the stream's front end on a handle of its own
    for s in (0, 2):
        assert rings[s].is_full
        win = rings[s].get_current_audio().astype(np.float32)
        feats = fe.mel_extract(attn.mel, dev(win[None]), out_frames=attn.shape["stream_out_frames"]).cpu().numpy()
        ref = core.logit_reference(wc.params(), feats, feats[:, -3:], emo[s:s + 1], num_heads=wc.HEADS, mel_sequence_length=wc.WINDOW)
        a_max, a_ratio = core.attention_verdict(maps[s][None], ref, K)
        print(f"STREAM256W|map stream {s}|{a_max:.3e}|{a_ratio:.3f}")
        assert a_ratio <= 1.0, (s, a_max, a_ratio)
        assert np.abs(maps[s].astype(np.float64).sum(-1) - 1.0).max() < 1e-5
        d = np.abs(core.recover_sigmoid(out[s][None], wc.params()) - raw[s][None].astype(np.float64))
        assert (d <= 3 * core.LOGIT_U * ref["s64"] + 1e-45).all(), (s, float(d.max()))
    fe.close()
