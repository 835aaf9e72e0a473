"""km_resampler_push / _flush / _reset_streams (StreamResampler) on the schedule of tests/resample_cases.py: three streams at 48 kHz
and at 44.1 kHz, chunks of 0, 1, 7, 160, 1024 and 1600 samples with different counts per stream, a stream that joins late and
pauses, a stream that is reset mid-way and refilled.

The yardstick is Resampler.clip on each life's concatenated input (itself pinned to the float64 oracle by
tests/test_gpu_resample.py): what a stream emitted must be its first emitted(N) outputs BIT FOR BIT, and after a flush all
n_out(N) of them.  No tolerance anywhere in this file.
"""
import functools

import numpy as np
import pytest
import torch

import resample_cases as rc
from koemorph_amd import synth
from koemorph_amd.engine import Engine
from koemorph_amd.features import Resampler
from koemorph_amd.features import resample as rs
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEmotion, StreamResampler

pytestmark = pytest.mark.gpu
RATES = (48000, 44100)


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the cases' arrays are read-only


def mask_of(streams):
    m = torch.zeros(rc.STREAMS, dtype=torch.bool, device="cuda")
    m[list(streams)] = True
    return m


@functools.lru_cache(maxsize=None)
def clip_of_lives(rate_in):
    """[stream][life] -> Resampler.clip of the life's whole input (numpy; an empty life gives an empty array)."""
    r = Resampler(rate_in, rc.RATE_OUT)
    out = [[r.clip(dev(x)).cpu().numpy() if x.size else np.zeros(0, np.float32) for _, x in lives] for lives in rc.stream_lives(rate_in)]
    r.close()
    return out


@functools.lru_cache(maxsize=None)
def run(rate_in, graph):
    """One pass over the schedule -> per stream and life what it emitted: dict(pushed=[s][life] arrays, flushed=[s] arrays (last
    life), counts=(STEPS, STREAMS) reported per step, partial=the counts of the partial flush).  graph: every push is the replay
    of one captured push on static buffers."""
    counts, resets = rc.schedule()
    chunks = rc.stream_chunks(rate_in)
    sr = StreamResampler(rc.STREAMS, rate_in, rc.RATE_OUT)
    assert sr.out_max(rc.N_MAX) == rs.n_out(rc.N_MAX, sr.up, sr.down) + 1
    pushed = [[[]] for _ in range(rc.STREAMS)]
    reported = np.zeros((rc.STEPS, rc.STREAMS), np.int32)
    g = None
    if graph:
        x_static = torch.zeros(rc.STREAMS, rc.N_MAX, device="cuda")
        c_static = torch.zeros(rc.STREAMS, dtype=torch.int32, device="cuda")
        sr.push(x_static, c_static)                        # counts of 0: touches nothing, creates the output buffers
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, out_counts = sr.push(x_static, c_static)
    for t in range(rc.STEPS):
        if t in resets:
            sr.reset_streams(mask_of(resets[t]))
            for s in resets[t]:
                pushed[s].append([])
        if graph:
            x_static.copy_(dev(chunks[t]))
            c_static.copy_(dev(counts[t]))
            g.replay()
        else:
            out, out_counts = sr.push(dev(chunks[t]), dev(counts[t]))
        o, c = out.cpu().numpy(), out_counts.cpu().numpy()
        reported[t] = c
        for s in range(rc.STREAMS):
            pushed[s][-1].append(o[s, :c[s]].copy())
    # flush streams 0 and 2 first: stream 1 must report 0 and keep its state for the flush that follows
    out, out_counts = sr.flush(mask_of((0, 2)))
    o, partial = out.cpu().numpy().copy(), out_counts.cpu().numpy().copy()
    flushed = [o[s, :partial[s]].copy() for s in range(rc.STREAMS)]
    out, out_counts = sr.flush()
    o, c = out.cpu().numpy(), out_counts.cpu().numpy()
    flushed[1] = o[1, :c[1]].copy()
    rest = c.copy()
    sr.close()
    return dict(pushed=[[np.concatenate(life) if life else np.zeros(0, np.float32) for life in lives] for lives in pushed],
                flushed=flushed, counts=reported, partial=partial, rest=rest)


@pytest.mark.parametrize("rate_in", RATES)
def test_streams_emit_the_clip_outputs_bit_for_bit(rate_in):
    up, down, _, half_len = rc.plan(rate_in)
    counts, _ = rc.schedule()
    got, want, lives = run(rate_in, False), clip_of_lives(rate_in), rc.stream_lives(rate_in)
    assert [len(v) for v in lives] == [1, 1, 2]
    for s in range(rc.STREAMS):
        for i, (_, x) in enumerate(lives[s]):
            e = rs.emitted(x.size, up, down, half_len)
            assert got["pushed"][s][i].shape == (e,), (s, i)
            assert np.array_equal(got["pushed"][s][i], want[s][i][:e]), (s, i)          # the reset life equals a fresh stream's
        whole = np.concatenate([got["pushed"][s][-1], got["flushed"][s]])
        assert whole.shape == want[s][-1].shape == (rs.n_out(lives[s][-1][1].size, up, down),), s
        assert np.array_equal(whole, want[s][-1]), s
    # the counts every push reported are the streaming law's, step by step; a stream that brings nothing reports 0
    plans = [rs.StreamPlan(up, down, half_len) for _ in range(rc.STREAMS)]
    _, resets = rc.schedule()
    for t in range(rc.STEPS):
        for s in resets.get(t, ()):
            plans[s].reset()
        assert [plans[s].push(int(counts[t, s])) for s in range(rc.STREAMS)] == got["counts"][t].tolist(), t
    assert np.all(got["counts"][counts == 0] == 0) and (counts == 0).sum() >= 6
    assert got["partial"][1] == 0 and got["partial"].tolist() == [plans[0].flush(), 0, plans[2].flush()]
    assert got["rest"].tolist() == [0, plans[1].flush(), 0]                              # flushed streams are fresh: nothing owed


@pytest.mark.parametrize("rate_in", RATES)
def test_graph_replay_is_the_eager_run(rate_in):
    a, b = run(rate_in, False), run(rate_in, True)
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["partial"], b["partial"])
    for s in range(rc.STREAMS):
        assert len(a["pushed"][s]) == len(b["pushed"][s])
        for x, y in zip(a["pushed"][s] + [a["flushed"][s]], b["pushed"][s] + [b["flushed"][s]]):
            assert x.size and np.array_equal(x, y), s


def test_arguments_are_checked():
    sr = StreamResampler(2, 48000)
    with pytest.raises(ValueError, match="samples"):
        sr.push(torch.zeros(3, 16, device="cuda"))
    with pytest.raises(ValueError, match="counts"):
        sr.push(torch.zeros(2, 16, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        sr.reset_streams(torch.zeros(3, dtype=torch.bool, device="cuda"))
    x, out, oc = torch.zeros(2, 300, device="cuda"), torch.zeros(2, 99, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    code = sr._lib.km_resampler_push(sr._h, x.data_ptr(), 300, None, out.data_ptr(), 99, oc.data_ptr(), None)       # 300 / 3 = 100 > 99
    assert code != 0 and b"out_stride" in sr._lib.km_last_error()
    out, oc = sr.push(x)                                   # counts None: every stream brings all 300
    assert out.shape == (2, 101) and oc.tolist() == [90, 90]
    sr.close()
    with pytest.raises(ValueError):
        StreamResampler(2, 16000)


def test_resampler_emotion_and_chunked_engine_in_one_capture():
    """48 kHz chunks of 1600 samples for two streams: StreamResampler.push -> StreamEmotion.push / update -> ChunkedStreamEngine.feed /
    step recorded in one capture, replayed against an eager twin that is fed the resampler's own output tensors: identical bits."""
    n, chunk, prefill, steps = 2, 1600, 250, 12
    torch.manual_seed(1234)
    layer = torch.nn.Linear(264, 256)

    def pair():
        e = Engine()
        e.load_state_dict(synth.make_core_params(61, style="trained"))
        e.finalize()
        return StreamEmotion(n, 1.0, 0.3, compression_layer=layer), ChunkedStreamEngine(e, n)

    audio = synth.make_audio(933, n, (prefill + steps) * chunk) * np.array([[0.8], [0.3]], np.float32)
    sr = StreamResampler(n, 48000)
    (sa, ca), (sb, cb) = pair(), pair()
    assert ca.frame_samples == 533
    x_static = torch.zeros(n, chunk, device="cuda")
    graph = None
    fired_any = updated_any = False
    total = 0
    for t in range(prefill + steps):
        x = dev(audio[:, t * chunk:(t + 1) * chunk])
        if t < prefill:
            out, out_counts = sr.push(x)
            sa.push(out, out_counts)
            emo_a, _ = sa.update()
            ca.feed(out, out_counts)
            ca.step(emo_a)
        else:
            if graph is None:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out, out_counts = sr.push(x_static)
                    sa.push(out, out_counts)
                    sa.update()
                    ca.feed(out, out_counts)
                    ca.step(sa.emotion)
            x_static.copy_(x)
            graph.replay()
        sb.push(out, out_counts)
        emo_b, upd_b = sb.update()
        cb.feed(out, out_counts)
        out_b, fired_b = cb.step(emo_b)
        if t < prefill:
            continue
        torch.cuda.synchronize()
        total += int(out_counts[0])
        assert out_counts.tolist() in ([533, 533], [534, 534]), t
        assert torch.equal(sa.emotion, sb.emotion) and torch.equal(sa.updated, sb.updated) and torch.equal(sa.valid, sb.valid), t
        assert torch.equal(ca.out, cb.out) and torch.equal(ca.fired, cb.fired) and torch.equal(ca.ready, cb.ready), t
        fired_any |= bool(fired_b.any())
        updated_any |= bool(upd_b.any())
    assert fired_any and updated_any and total == steps * chunk // 3
    sa.close()
    sb.close()
    sr.close()
