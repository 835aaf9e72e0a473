"""Device-resident streaming (km_stream_*) at the reference's `fast` (d_model 128, 4 heads, window 128, emotion_dim 256) and `basic`
(window 256, emotion_dim 9) variants at 30 fps -- update_interval 0.0333 (ring hop 532), front end n_fft 1024 at hop 533 with reflect
padding -- served by core128_stream_kernel, against the per-stream oracle pipeline of tests/stream_d128_cases.py: MelAudioBuffer ring
-> sliding-window dB mel -> core (float64) with last-3-kept-rows short rows -> EMA.  Frames of 532 / 533 samples alternate.

Tolerance.  The yardstick is the float64 oracle, never a second GPU path.  Largest |hip - oracle| over the checked ticks x streams x
52 coefficients, one run on an MI355X (every test prints its figure as `STREAM128|...` before it asserts):
    short ring (1.0 s), six checked ticks x 3 streams     fast 1.863e-08    basic 2.980e-08
    truncating ring (4.4 s), four ticks x 2 streams       fast 9.313e-09
    full ring (8.5 s), four ticks x 2 streams             fast 1.676e-08    basic 1.118e-08
BOUND is the largest figure times 4 (1.19e-7), the margin tests/test_gpu_streaming_d512.py and _d256w.py take for input-dependent rounding; it
is below 2e-5, the project's d_model 256 stream bound.  A wrong short-row choice, a wrong dB reference or a missed zero row shows up at
1e-2 and above.
"""
import numpy as np
import pytest
import torch

import stream_d128_cases as dc
from core_logit_cases import K
from koemorph_amd import _lib, synth
from koemorph_amd._lib import KM_ERR_UNSUPPORTED, KoeMorphError
from koemorph_amd.engine import Engine
from koemorph_amd.metrics import StreamAttentionStats
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEngine
from oracle import core

pytestmark = pytest.mark.gpu
MEASURED = {("short", "fast"): 1.863e-08, ("short", "basic"): 2.980e-08, ("trunc", "fast"): 9.313e-09, ("full", "fast"): 1.676e-08,
            ("full", "basic"): 1.118e-08}
BOUND = 4 * max(MEASURED.values())
assert BOUND <= 2e-5
VARIANTS = list(dc.VARIANTS)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def engine128(name):
    T, ED, _ = dc.VARIANTS[name]
    e = Engine(d_model=dc.D_MODEL, num_heads=dc.HEADS, mel_sequence_length=T, emotion_dim=ED)
    e.load_state_dict(dc.params(name))
    e.finalize()
    assert not e.fused and e.mel.hop_length == dc.MEL_HOP and e.core_route() == 3     # the forward calls keep the chain by default
    return e


@pytest.mark.parametrize("name", VARIANTS)
def test_short_ring_matches_oracle(name):
    """U = 30 kept rows of 31 computed, below T: zero rows 30 .. T - 1, short rows = kept rows 27 .. 29, and for stream 2 a dB
    reference that lies in the dropped frame 30.  The write pointer wraps at tick 30."""
    S = dc.SHORT_S
    se = StreamEngine(engine128(name), S, context_window=dc.SHORT_CW)
    assert se.ring_hop == 532 and se.shape == dict(ring_len=16000, ring_hop=532, n_frames=31, stream_out_frames=30)
    emo = dc.short_emotion(name)
    sms = [dc.smoother() for _ in range(S)]
    worst = 0.0
    for t, frame in enumerate(dc.short_frames()):
        se.push(dev(frame))
        out, ready = se.tick(dev(emo))
        full = t >= dc.SHORT_FIRST_READY
        assert bool(ready.cpu().all()) == full and bool(ready.cpu().any()) == full, t
        if not full:
            assert not bool(out.cpu().any())             # no row is written before its ring is full
            continue
        got = out.cpu().numpy()
        for s in range(S):
            if t in dc.SHORT_CHECKED:
                want = sms[s](dc.short_expected(name, t)[s:s + 1])
                worst = max(worst, float(np.abs(got[s] - want[0]).max()))
            else:   # keep the oracle EMA in step without paying for the mel: feed it the GPU value back
                sms[s].prev = got[s:s + 1].copy()
    print(f"STREAM128|short ring {name}|{worst:.3e}")
    assert worst < BOUND, worst


def run_long_ring(name, cw, shape, first, checks, graph_from, ticks, seed):
    """Two streams on a ring of `cw` seconds.  Oracle on the ticks `checks`; with `graph_from`, one engine replays a captured push +
    tick (533-sample frames, pinned readback as the last node) from that tick on while a second engine, fed the same samples, runs
    them eagerly: identical bits on every tick."""
    S = 2
    emo = synth.normal(seed + 1, (S, dc.VARIANTS[name][1]))
    audio = synth.make_audio(seed, S, 533 * ticks)
    a = StreamEngine(engine128(name), S, context_window=cw)
    b = StreamEngine(engine128(name), S, context_window=cw) if graph_from else None
    assert a.shape == shape
    rings = [dc.ring(cw) for _ in range(S)]
    sms = [dc.smoother() for _ in range(S)]
    host_out = torch.empty(S, 52).pin_memory()
    emo_d = dev(emo)
    worst, checked, pos = 0.0, 0, 0
    for t in range(ticks):
        n = 533 if graph_from and t >= graph_from else dc.frame_len(t)
        frame = audio[:, pos:pos + n]
        pos += n
        fd = dev(frame)
        if t == graph_from:
            a.capture(host_out=host_out)                 # default frame size: 533
            assert tuple(a._g_samples.shape) == (S, 533)
        if graph_from and t >= graph_from:
            out, ready = a.replay(fd, emo_d)
            torch.cuda.synchronize()
            assert np.array_equal(host_out.numpy(), out.cpu().numpy())
        else:
            a.push(fd)
            out, ready = a.tick(emo_d)
        if b is not None:
            b.push(fd)
            out_b, ready_b = b.tick(emo_d)
            assert torch.equal(out, out_b) and torch.equal(ready, ready_b), t
        for s in range(S):
            rings[s].add_audio_frame(frame[s])
        assert bool(ready.cpu().all()) == rings[0].is_full == (t >= first)
        if t < first:
            continue
        got = out.cpu().numpy()
        for s in range(S):
            if t in checks:
                want = sms[s](dc.oracle_blendshapes(name, rings[s].get_current_audio(), emo[s], cw))
                worst = max(worst, float(np.abs(got[s] - want[0]).max()))
                checked += 1
            else:
                sms[s].prev = got[s:s + 1].copy()
    assert checked == 2 * len(checks)
    return worst


def test_truncating_ring_matches_oracle():
    """4.4 s at `fast`: ring 70400 samples, 133 frames computed, U = 132 kept > T = 128.  Long rows are kept rows 0 .. 127, short rows
    kept rows 129 .. 131: the r < tv branch of the streaming row policy with U > T.  Four oracle ticks after the ring fills."""
    worst = run_long_ring("fast", 4.4, dict(ring_len=70400, ring_hop=532, n_frames=133, stream_out_frames=132), first=132,
                          checks=(132, 133, 135, 136), graph_from=0, ticks=137, seed=52)
    print(f"STREAM128|truncating ring fast|{worst:.3e}")
    assert worst < BOUND, worst


@pytest.mark.parametrize("name", VARIANTS)
def test_full_ring_matches_oracle_and_graph_replay(name):
    """8.5 s: ring 136000 samples, 256 frames computed, U = 255 kept: one zero row at `basic`, truncation to 128 at `fast`.  Oracle on
    four ticks after the ring fills; from tick 257 on a captured push + tick against an eager twin."""
    worst = run_long_ring(name, 8.5, dict(ring_len=136000, ring_hop=532, n_frames=256, stream_out_frames=255), first=255,
                          checks=(255, 256, 258, 259), graph_from=257, ticks=261, seed=42)
    print(f"STREAM128|full ring {name}|{worst:.3e}")
    assert worst < BOUND, worst


def test_rows_state_and_maps_of_a_stream_that_is_not_ready_are_left_alone():
    """Across the fill boundary: while the ring fills, a tick writes neither the stream's out row (a sentinel survives), nor its rows
    of raw and the map, nor its EMA state; reset() clears readiness, out and state, so the first ready tick after a refill is again
    the unsmoothed value -- bit for bit what the first run gave -- and the second one is smoothed from it, not from anything older."""
    name, S = "fast", dc.SHORT_S
    se = StreamEngine(engine128(name), S, context_window=dc.SHORT_CW)
    emo = dev(dc.short_emotion(name))
    frames = [dev(f) for f in dc.short_frames()]
    extra = se.attention_outputs()

    def fill_and_two(sentinel):
        se.out.fill_(sentinel)
        extra["raw"].fill_(sentinel)
        extra["mel_attention_weights"].fill_(sentinel)
        for t in range(dc.SHORT_FIRST_READY):
            se.push(frames[t])
            out, ready, got = se.tick(emo, return_attention=True)
            assert not bool(ready.any()) and bool((out == sentinel).all()), t
            assert bool((got["raw"] == sentinel).all()) and bool((got["mel_attention_weights"] == sentinel).all()), t
        res = []
        for t in (dc.SHORT_FIRST_READY, dc.SHORT_FIRST_READY + 1):
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
    want = dc.short_expected(name, dc.SHORT_FIRST_READY)
    assert np.abs(first[0].cpu().numpy() - want).max() < BOUND


# ---- streams out of phase ------------------------------------------------------------------------------------------------------------
FRAME = 533                  # int(16000 / 30): what a step pops
JOIN, RESET_AT, STEPS = 10, 35, 70           # stream 1 brings its first frame at step 10; stream 2 is reset before step 35
FULL_AFTER = 31              # frames of 533 samples that fill the 16000-sample ring


def chunk_audio():
    return synth.make_audio(47, 3, FRAME * STEPS)


def popped(audio, s, j):
    """The j-th frame stream s ever pops: every stream consumes its own audio in order."""
    return audio[s, j * FRAME:(j + 1) * FRAME]


def test_chunked_engine_late_joiner_and_reset_stream_equal_the_lockstep_engine():
    """ChunkedStreamEngine on the short ring at `basic`: stream 0 in step from the start, stream 1 ten steps late, stream 2 reset before
    step 35 and refilled.  Every fired row is, bit for bit, the row the lockstep engine gives at the same frame of that stream's life;
    a row that did not fire keeps the step's sentinel; fired and ready follow the frame counts.  The last step is a captured feed +
    step."""
    name = "basic"
    audio, emo = chunk_audio(), dev(dc.short_emotion(name))
    se = ChunkedStreamEngine(engine128(name), 3, context_window=dc.SHORT_CW)
    assert se.chunk == dict(fifo_samples=32000, frame_samples=FRAME, ring_hop=532)
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
        if t == STEPS - 1:
            se.capture(FRAME)
        se.out.fill_(1000.0 + t)
        if t == STEPS - 1:
            out, f = se.replay(dev(chunk), dev(counts), emo)
        else:
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
    twin = StreamEngine(engine128(name), 3, context_window=dc.SHORT_CW)
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
    full = FULL_AFTER - 1
    assert compared == (STEPS - full) + (STEPS - JOIN - full) + (RESET_AT - full) + (STEPS - RESET_AT - full)


@pytest.mark.parametrize("name", VARIANTS)
def test_step_with_the_attention_outputs(name):
    """One step with return_attention=True, at the step where streams 0 and 2 fire for the first time and the late stream 1 does
    not: out, fired and ready are those of the plain step on a twin engine, bit for bit; the rows of stream 1 in out, raw and the
    map are untouched; raw and the map of a fired stream meet the bounds of tests/test_gpu_core_logit.py (K = 4) against the oracle on
    the device's own features of the stream's ring; the map's rows sum to 1.  Then a capture with the masked statistics update in the
    graph is accepted and one replay of it fires the three streams."""
    T, ED, _ = dc.VARIANTS[name]
    audio, emo = chunk_audio(), dc.short_emotion(name)
    emo_d = dev(emo)
    plain, attn = (ChunkedStreamEngine(engine128(name), 3, context_window=dc.SHORT_CW) for _ in range(2))
    extra = attn.attention_outputs()
    rings = [dc.ring(dc.SHORT_CW) for _ in range(3)]
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
    fe = engine128(name)                                  # the stream's front end on a handle of its own
    for s in (0, 2):
        assert rings[s].is_full
        win = rings[s].get_current_audio().astype(np.float32)
        feats = fe.mel_extract(attn.mel, dev(win[None]), out_frames=attn.shape["stream_out_frames"]).cpu().numpy()
        ref = core.logit_reference(dc.params(name), feats, feats[:, -3:], emo[s:s + 1], num_heads=dc.HEADS, mel_sequence_length=T)
        assert float(np.abs(ref["z64"]).max()) <= core.LOGIT_Z_MAX
        e_max, e_ratio = core.logit_verdict(raw[s][None], ref, K)
        a_max, a_ratio = core.attention_verdict(maps[s][None], ref, K)
        print(f"STREAM128|{name} raw and map stream {s}|{e_max:.3e}|{e_ratio:.3f}|{a_max:.3e}|{a_ratio:.3f}")
        assert e_ratio <= 1.0, (s, e_max, e_ratio)
        assert a_ratio <= 1.0, (s, a_max, a_ratio)
        assert np.abs(maps[s].astype(np.float64).sum(-1) - 1.0).max() < 1e-5
        d = np.abs(core.recover_sigmoid(out[s][None], dc.params(name)) - raw[s][None].astype(np.float64))
        assert (d <= 3 * core.LOGIT_U * ref["s64"] + 1e-45).all(), (s, float(d.max()))
    fe.close()
    # stats= in a capture: the next frame of every stream, all three rings full by then for streams 0 and 2
    per = StreamAttentionStats(3)
    attn.capture(FRAME, return_attention=True, stats=per)
    chunk = np.stack([popped(audio, s, FULL_AFTER - (JOIN if s == 1 else 0)) for s in range(3)])
    out_g, fired_g, got_g = attn.replay(dev(chunk), None, emo_d)
    plain.feed(dev(chunk))
    out_p, fired_p = plain.step(emo_d)
    assert torch.equal(out_g, out_p) and torch.equal(fired_g, fired_p) and fired_g.cpu().tolist() == [1, 0, 1]
    assert [st["rows"] for st in per.compute()] == [1, 0, 1]
    per.close()


def test_refusals():
    """d_model 128 / window 64 keeps its refusal and its text; maps under core_split 3 are refused before anything is popped."""
    e = Engine(d_model=128, num_heads=4, mel_sequence_length=64)
    e.load_state_dict(synth.make_core_params(5, 128, 64, 256, "trained"))
    e.finalize()
    se = ChunkedStreamEngine(e, 2, context_window=1.0)
    se.feed(torch.zeros(2, 1024, device="cuda"))
    for call in (lambda: se.tick(torch.zeros(2, 256, device="cuda")), lambda: se.step(torch.zeros(2, 256, device="cuda")),
                 lambda: se.step(torch.zeros(2, 256, device="cuda"), return_attention=True)):
        with pytest.raises(KoeMorphError, match="no kernel for d_model=128, mel_sequence_length=64, heads=4") as err:
            call()
        assert err.value.code == KM_ERR_UNSUPPORTED
    e.close()
    name = "fast"
    a = ChunkedStreamEngine(engine128(name), 2, context_window=dc.SHORT_CW)
    emo = dev(dc.short_emotion(name)[:2])
    a.feed(dev(synth.make_audio(61, 2, 3 * FRAME)))
    a.step(emo)
    before = a.backlog.clone()
    assert before.cpu().tolist() == [2, 2]
    a.engine.set_option("core_split", 3)
    a.out.fill_(7.0)
    for call in (lambda: a.step(emo, return_attention=True), lambda: a.tick(emo, return_attention=True)):
        with pytest.raises(KoeMorphError, match="split-bf16") as err:
            call()
        assert err.value.code == KM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(a.backlog, before) and float(a.out.min()) == 7.0 == float(a.out.max())
    a.engine.set_option("core_split", 0)
    a.step(emo)
    assert torch.equal(a.backlog, before - 1)
    a.engine.close()


def test_streams_give_their_memory_back():
    live = _lib.load().km_live_device_bytes
    base = live()
    e = engine128("fast")
    se = ChunkedStreamEngine(e, 4, context_window=dc.SHORT_CW)               # km_stream_create + km_stream_fifo_create
    assert live() > base
    emo = dev(synth.normal(71, (4, 256)))
    for t in range(FULL_AFTER):
        se.feed(dev(synth.make_audio(72 + t, 4, FRAME)))
        out, fired = se.step(emo)
    assert fired.cpu().tolist() == [1, 1, 1, 1]
    se.push(dev(synth.make_audio(70, 4, 532)))
    out, ready = se.tick(emo)
    torch.cuda.synchronize()
    assert ready.cpu().tolist() == [1, 1, 1, 1] and bool(out.any())
    e.close()
    assert live() == base
