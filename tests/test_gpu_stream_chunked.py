"""Streams out of phase (km_stream_fifo_create / _feed / _step / _reset_streams, ChunkedStreamEngine) on the two schedules of
tests/stream_chunked_cases.py, against
  * the lockstep engine (StreamEngine.push / tick) fed the frames each stream popped: identical bits, because the step's gate
    only removes workgroups from launches that are otherwise those of a tick;
  * the per-stream float64 oracle: RingBufferOracle -> MelAudioBufferOracle -> oracle.mel.mel_sliding_window ->
    core.core_forward_np (float64) -> TemporalSmootherOracle(0.8), at the (step, stream) pairs the schedules name;
  * the host simulation of the flags and backlogs, on every step.

Tolerance.  The yardstick of the values is the float64 oracle.  Largest |hip - oracle| over the checked pairs x 52 coefficients,
one run on an MI355X:
    Schedule A (d_model 512, 8 heads, 1.0 s ring), 6 pairs    5.960e-08
    Schedule B (d_model 256, 8 heads, 8.5 s ring), 6 pairs    4.470e-08
BOUND_A and BOUND_B are four times these figures (the margin rule of tests/test_gpu_streaming_d512.py: input-dependent
rounding), below the project's 5e-6 for d_model 512 and 2e-5 for d_model 256.
"""
import functools

import numpy as np
import pytest
import torch

import stream_chunked_cases as cc
import stream_d512_cases as sc
from koemorph_amd import _lib, synth
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEngine
from oracle import core, mel as omel

pytestmark = pytest.mark.gpu
BOUND_A, BOUND_B = 4 * 5.960e-08, 4 * 4.470e-08
assert BOUND_A < 5e-6 and BOUND_B < 2e-5
PARAMS_B_SEED = 61


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the cases' arrays are read-only


def sentinel(t):
    return 1000.0 + t          # no coefficient comes near it, and it differs from step to step


def engine512(heads):
    e = Engine(d_model=512, num_heads=heads, mel_sequence_length=512, mel=MelConfig.model_batch(target_fps=60))
    e.load_state_dict(sc.params())
    e.finalize()
    return e


def chunked_a(heads):
    c = cc.SCHEDULES["A"]
    se = ChunkedStreamEngine(engine512(heads), c["n_streams"], context_window=c["context_window"], update_interval=c["update_interval"],
                             buffer_duration=c["fifo_samples"] / cc.SR)
    assert se.chunk == dict(fifo_samples=1600, frame_samples=266, ring_hop=266)
    assert se.shape == dict(ring_len=16000, ring_hop=266, n_frames=61, stream_out_frames=60)
    return se


@functools.lru_cache(maxsize=None)
def run_a(heads, steps, with_resets):
    """One pass of the chunked engine over Schedule A with `out` set to the step's sentinel before every step: per step the rows,
    fired, ready and backlog, and the rows right after each reset_streams.  Computed once per argument set; not to be modified."""
    c = cc.SCHEDULES["A"]
    S = c["n_streams"]
    se = chunked_a(heads)
    emo = dev(cc.emotion("A"))
    cnt, x = cc.counts_table("A", steps), cc.chunks("A", steps)
    rec = dict(out=np.zeros((steps, S, 52), np.float32), fired=np.zeros((steps, S), bool), ready=np.zeros((steps, S), bool),
               backlog=np.zeros((steps, S), np.int32), after_reset={})
    for t in range(steps):
        if with_resets and t in c["resets"]:
            mask = torch.zeros(S, dtype=torch.bool, device="cuda")
            mask[list(c["resets"][t])] = True
            se.reset_streams(mask)
            rec["after_reset"][t] = se.out.cpu().numpy().copy()
        se.out.fill_(sentinel(t))
        se.feed(dev(x[t]), dev(cnt[t]))
        out, fired = se.step(emo)
        rec["out"][t], rec["fired"][t] = out.cpu().numpy(), fired.cpu().numpy().astype(bool)
        rec["ready"][t], rec["backlog"][t] = se.ready.cpu().numpy().astype(bool), se.backlog.cpu().numpy()
    return rec


@functools.lru_cache(maxsize=None)
def run_twin_a(heads, steps):
    """The lockstep engine of the same shape and stream count: tick k of life l pushes every stream's k-th popped frame of that
    life (zeros once a stream has none left).  -> {life: (rows (n, S, 52), ready (n, S))}."""
    c, sim = cc.SCHEDULES["A"], cc.simulate("A", steps)
    S = c["n_streams"]
    se = StreamEngine(engine512(heads), S, context_window=c["context_window"], update_interval=c["update_interval"])
    emo = dev(cc.emotion("A"))
    res = {}
    for life in range(int(sim["life"].max()) + 1):
        seqs = [[f for _, l, f in sim["pops"][s] if l == life] for s in range(S)]
        n = max(len(q) for q in seqs)
        if life:
            se.reset()
        rows, ready = np.zeros((n, S, 52), np.float32), np.zeros((n, S), bool)
        for k in range(n):
            frame = np.zeros((S, c["frame_samples"]), np.float32)
            for s in range(S):
                if k < len(seqs[s]):
                    frame[s] = seqs[s][k]
            se.push(dev(frame))
            o, r = se.tick(emo)
            rows[k], ready[k] = o.cpu().numpy(), r.cpu().numpy().astype(bool)
        res[life] = (rows, ready)
    return res


def check_bit_identity(heads, steps):
    sim, got, twin = cc.simulate("A", steps), run_a(heads, steps, True), run_twin_a(heads, steps)
    compared = 0
    for s in range(cc.SCHEDULES["A"]["n_streams"]):
        k_of_life = {}
        for t, life, _ in sim["pops"][s]:
            k = k_of_life.get(life, 0)
            k_of_life[life] = k + 1
            rows, ready = twin[life]
            assert got["ready"][t, s] == ready[k, s] and got["fired"][t, s] == ready[k, s], (t, s, k)
            if ready[k, s]:
                assert np.array_equal(got["out"][t, s], rows[k, s]), (t, s, k, float(np.abs(got["out"][t, s] - rows[k, s]).max()))
                compared += 1
    assert compared == int(sim["fired"].sum()) and compared >= 5
    return compared


def test_schedule_a_bit_identical_to_the_lockstep_engine():
    """The k-th row the chunked engine fires for a stream equals, bit for bit, the row a plain StreamEngine gives at the k-th
    frame of that stream (each life of stream 2 separately), and the ready flags agree -- through the pause of stream 0, the idle
    steps of stream 1, the overflow of stream 3 and the reset of stream 2."""
    assert check_bit_identity(8, 152) == 82 + 57 + 12 + 92


def test_schedule_a_first_90_steps_16_heads():
    check_bit_identity(16, 90)


def test_schedule_a_matches_oracle():
    """The pairs: first fire of streams 3, 1 and 2 (EMA 'first' branch), stream 0's first row after its pause (smoothed from
    its last row ten steps earlier), stream 2's first row after the reset ('first' again) and its second (smoothed from it)."""
    sim, got = cc.simulate("A"), run_a(8, 152, True)
    emo = np.array(cc.emotion("A"))          # a copy: the oracle makes tensors of its rows
    worst = 0.0
    for (t, s), win in sorted(sim["windows"].items()):
        want = sc.oracle_blendshapes(win, emo[s], 8, cc.SCHEDULES["A"]["context_window"])
        sm, prev = sc.smoother(), cc.previous_fire(sim, t, s)
        if prev is not None:               # the EMA history: the row the device gave at the stream's previous fire
            sm.prev = got["out"][prev, s][None].copy()
        err = float(np.abs(got["out"][t, s] - sm(want)[0]).max())
        print(f"schedule A step {t} stream {s}: max |hip - oracle| = {err:.3e}")
        worst = max(worst, err)
    print(f"schedule A: worst = {worst:.3e}")
    assert len(sim["windows"]) == 6 and worst < BOUND_A, worst


def test_schedule_a_nothing_else_moves():
    """Rows of streams that did not fire keep the step's sentinel; fired, ready and backlog are the host oracle's on every step;
    reset_streams zeroes the row of stream 2 alone; and the rows of streams 0, 1 and 3 are, on every step, those of a second
    engine that is fed the same data and never reset."""
    sim, got, calm = cc.simulate("A"), run_a(8, 152, True), run_a(8, 152, False)
    assert np.array_equal(got["fired"], sim["fired"]) and np.array_equal(got["ready"], sim["ready"])
    assert np.array_equal(got["backlog"], sim["backlog"])
    for t in range(152):
        for s in range(4):
            row = got["out"][t, s]
            if sim["fired"][t, s]:
                assert float(np.abs(row).max()) <= 1.0 + 1e-6, (t, s)
            else:
                assert bool((row == sentinel(t)).all()), (t, s)
    after = got["after_reset"][85]
    assert not after[2].any() and np.array_equal(after[[0, 1, 3]], got["out"][84][[0, 1, 3]])
    others = [0, 1, 3]
    assert np.array_equal(got["fired"][:, others], calm["fired"][:, others])
    assert np.array_equal(got["out"][:, others], calm["out"][:, others])
    assert calm["fired"][85:145, 2].all()                # the engine that was not reset went on firing stream 2


# ---- Schedule B ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params_b():
    return synth.make_core_params(PARAMS_B_SEED, style="trained")


def chunked_b():
    e = Engine()
    e.load_state_dict(params_b())
    e.finalize()
    se = ChunkedStreamEngine(e, cc.SCHEDULES["B"]["n_streams"])
    assert se.chunk == dict(fifo_samples=32000, frame_samples=533, ring_hop=532) and se.shape["ring_len"] == 136000
    return se


def test_schedule_b_matches_oracle_and_graph_replay():
    """The full 8.5 s ring at 30 fps (533-sample frames into a ring of hop 532).  From step 280 on one engine replays a captured
    feed + step with the pinned readback as the last node while an eager twin receives the same chunks: identical bits; flags and
    backlog follow the host oracle on every step; the float64 oracle at six pairs."""
    c, sim = cc.SCHEDULES["B"], cc.simulate("B")
    S, T, GRAPH_FROM = c["n_streams"], c["steps"], 280
    a, b = chunked_b(), chunked_b()
    emo = np.array(cc.emotion("B"))
    emo_d = dev(emo)
    cnt, x = cc.counts_table("B"), cc.chunks("B")
    host_out = torch.empty(S, 52).pin_memory()
    rows = np.zeros((T, S, 52), np.float32)
    for t in range(T):
        xd, cd = dev(x[t]), dev(cnt[t])
        if t == GRAPH_FROM:
            a.capture(c["n_max"], host_out=host_out)
        if t >= GRAPH_FROM:
            out, fired = a.replay(xd, cd, emo_d)
            torch.cuda.synchronize()
            assert np.array_equal(host_out.numpy(), out.cpu().numpy()), t
        else:
            a.feed(xd, cd)
            out, fired = a.step(emo_d)
        b.feed(xd, cd)
        out_b, fired_b = b.step(emo_d)
        assert torch.equal(out, out_b) and torch.equal(fired, fired_b), t
        assert torch.equal(a.ready, b.ready) and torch.equal(a.backlog, b.backlog), t
        assert np.array_equal(fired.cpu().numpy().astype(bool), sim["fired"][t]), t
        assert np.array_equal(a.ready.cpu().numpy().astype(bool), sim["ready"][t]), t
        assert np.array_equal(a.backlog.cpu().numpy(), sim["backlog"][t]), t
        rows[t] = out.cpu().numpy()
    worst = 0.0
    for (t, s), win in sorted(sim["windows"].items()):
        feats = omel.mel_sliding_window(win, n_fft=1024, hop=533)
        want = core.core_forward_np(params_b(), feats[None], feats[None, -3:], emo[s:s + 1], dtype=torch.float64)["blendshapes"]
        sm, prev = sc.smoother(), cc.previous_fire(sim, t, s)
        if prev is not None:
            sm.prev = rows[prev, s][None].copy()
        err = float(np.abs(rows[t, s] - sm(want.astype(np.float32))[0]).max())
        print(f"schedule B step {t} stream {s}: max |hip - oracle| = {err:.3e}")
        worst = max(worst, err)
    print(f"schedule B: worst = {worst:.3e}")
    assert len(sim["windows"]) == 6 and worst < BOUND_B, worst


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _lib.load()
    e = Engine()
    e.load_state_dict(synth.make_core_params(3))
    e.finalize()
    h = e._h
    samples, emo = torch.zeros(2, 533, device="cuda"), torch.zeros(2, 256, device="cuda")
    out = torch.full((2, 52), 7.0, device="cuda")
    mask = torch.ones(2, dtype=torch.uint8, device="cuda")
    assert lib.km_stream_fifo_create(h, 32000, 533) == _lib.KM_ERR_INVALID_ARG and b"km_stream_create first" in lib.km_last_error()
    assert lib.km_stream_reset_streams(h, mask.data_ptr(), None) == _lib.KM_ERR_INVALID_ARG
    se = StreamEngine(e, 2)
    # feed or step before km_stream_fifo_create
    assert lib.km_stream_feed(h, samples.data_ptr(), 533, None, None) == _lib.KM_ERR_INVALID_ARG
    assert b"km_stream_fifo_create first" in lib.km_last_error()
    assert lib.km_stream_step(h, emo.data_ptr(), out.data_ptr(), None, None, None, None) == _lib.KM_ERR_INVALID_ARG
    assert b"km_stream_fifo_create first" in lib.km_last_error()
    # sizes
    assert lib.km_stream_fifo_create(h, 32000, 500) == _lib.KM_ERR_INVALID_ARG
    assert b"Frame size mismatch: expected ~532, got 500" in lib.km_last_error()
    assert lib.km_stream_fifo_create(h, 500, 533) == _lib.KM_ERR_INVALID_ARG and b"no read could ever succeed" in lib.km_last_error()
    assert lib.km_stream_fifo_create(h, 0, 533) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_stream_fifo_create(h, 32000, 0) == _lib.KM_ERR_INVALID_ARG
    with pytest.raises(ValueError, match="Frame size mismatch"):
        ChunkedStreamEngine(e, 2, frame_samples=500)
    # km_stream_create called again frees the FIFOs together with the rings
    assert lib.km_stream_fifo_create(h, 32000, 533) == _lib.KM_OK
    assert lib.km_stream_feed(h, samples.data_ptr(), 533, None, None) == _lib.KM_OK
    se = StreamEngine(e, 2)
    assert lib.km_stream_feed(h, samples.data_ptr(), 533, None, None) == _lib.KM_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0        # no refused call wrote a row
    e.close()


def test_masked_reset_without_fifos():
    """km_stream_reset_streams on the lockstep path (no FIFOs): a full stream starts over -- not ready, its row left alone, and
    after a refill its first row is again the unsmoothed one, bit for bit what the first fill gave -- while its neighbours go on."""
    S = sc.SHORT_S
    se = StreamEngine(engine512(8), S, context_window=sc.SHORT_CW, update_interval=sc.UI60)
    lib, emo = _lib.load(), dev(sc.short_emotion())
    frames = [dev(f) for f in sc.short_frames()]
    n = sc.SHORT_FIRST_READY + 1

    def fill(ready_before):
        for t in range(n):
            se.push(frames[t])
            out, ready = se.tick(emo)
            assert ready.cpu().tolist() == (ready_before if t < n - 1 else [1] * S), t
        return out.clone()

    first = fill([0] * S)
    mask = torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda")
    assert lib.km_stream_reset_streams(se.engine._h, mask.data_ptr(), None) == _lib.KM_OK
    se.out[1].fill_(7.0)
    again = fill([1, 0, 1])
    assert torch.equal(again[1], first[1]) and not torch.equal(again[0], first[0])


def test_legacy_handle_is_refused():
    from koemorph_amd.model import SimplifiedKoeMorphModel
    import legacy_stream_cases as lc
    m = SimplifiedKoeMorphModel().cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in lc.params().items()})
    lib, h, _ = m._handle()
    buf = torch.zeros(2, 600, device="cuda")
    for rc in (lib.km_stream_fifo_create(h, 32000, 533), lib.km_stream_feed(h, buf.data_ptr(), 533, None, None),
               lib.km_stream_step(h, buf.data_ptr(), buf.data_ptr(), None, None, None, None),
               lib.km_stream_reset_streams(h, buf.data_ptr(), None)):
        assert rc == _lib.KM_ERR_INVALID_ARG and b"dual-stream handle" in lib.km_last_error()


def test_other_shapes_keep_the_message_of_tick():
    e = Engine(d_model=128, num_heads=4, mel_sequence_length=64)
    e.load_state_dict(synth.make_core_params(5, 128, 64, 256, "trained"))
    e.finalize()
    se = ChunkedStreamEngine(e, 2, context_window=1.0)
    se.feed(torch.zeros(2, 1024, device="cuda"))
    with pytest.raises(KoeMorphError, match="no kernel for d_model=128, mel_sequence_length=64, heads=4"):
        se.step(torch.zeros(2, 256, device="cuda"))
