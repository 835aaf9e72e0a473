"""The emotion streams in their `basic` back end (km_emotion_stream_create_basic, StreamEmotion(backend="basic")) on the first three
streams of schedule S of tests/stream_emotion_cases.py: context 1.0 s, so 48 000-sample rings and 16 000-sample windows of 32 frames.

Who updates, and on which window, is checked against the host oracle on every step.  What an update computes is checked BIT FOR BIT
against ``BasicEmotion()(window[None])[0]`` on the oracle's window: the kernels read the samples where they lie in the stream's ring
-- across its wrap -- but run the same arithmetic in the same order, so no tolerance is needed and none is given.
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

import stream_d128_cases as dc
import stream_emotion_cases as ec
from koemorph_amd import _lib
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.engine import Engine
from koemorph_amd.features import BasicEmotion
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEmotion

pytestmark = pytest.mark.gpu
N = 3                   # streams 0 .. 2 of schedule S: steady 1600, steady 1024, late joiner that is reset before step 30
GRAPH_M = 1600          # the largest chunk of those three
GRAPH_FROM = 8
SHAPE = dict(ring_len=48000, window_len=16000, update_samples=4800, min_samples=8000, max_frames=32)


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def basic():
    return BasicEmotion("cuda")


_REF = {}


def reference(window: np.ndarray) -> np.ndarray:
    key = hashlib.sha1(np.ascontiguousarray(window).tobytes()).hexdigest()
    if key not in _REF:
        _REF[key] = basic()(dev(window)[None])[0].cpu().numpy()
    return _REF[key]


def rows_of(t):
    return ec.chunks()[t][:N]


@functools.lru_cache(maxsize=None)
def simulate(max_updates=None, with_reset=True):
    o = ec.EmotionStreamOracle(N, ec.CONTEXT, ec.INTERVAL, max_updates)
    out = []
    for t in range(ec.STEPS):
        if with_reset:
            for s in ec.RESETS.get(t, ()):
                o.reset(s)
        out.append(o.step(rows_of(t)))
    return out


def make(max_updates=None):
    se = StreamEmotion(N, ec.CONTEXT, ec.INTERVAL, max_updates=max_updates, backend="basic")
    assert se.shape == SHAPE and tuple(se.emotion.shape) == (N, 9) and se.compression_layer is None
    return se


def snapshot(se):
    torch.cuda.synchronize()
    return dict(updated=se.updated.cpu().numpy().copy(), valid=se.valid.cpu().numpy().copy(), features=se.features.cpu().numpy(),
                emotion=se.emotion.cpu().numpy().copy())


@functools.lru_cache(maxsize=None)
def run(max_updates=None, with_reset=True, graph=False, only=None, start=0):
    se = make(max_updates)
    out = []
    for t in range(ec.STEPS):
        if t < start:
            continue
        row = rows_of(t)
        if with_reset and t in ec.RESETS:
            mask = torch.zeros(N, dtype=torch.bool, device="cuda")
            mask[list(ec.RESETS[t])] = True
            se.reset_streams(mask)
        if only is not None:
            row = [c if s == only else c[:0] for s, c in enumerate(row)]
        if graph and t == GRAPH_FROM:
            se.capture(GRAPH_M)
        x, cnt = ec.padded(row, GRAPH_M if graph and t >= GRAPH_FROM else None)
        if graph and t >= GRAPH_FROM:
            se.replay(dev(x), dev(cnt))
        else:
            se.push(dev(x), dev(cnt))
            se.update()
        out.append(snapshot(se))
    se.close()
    return out


def same(a, b, s=None):
    sl = slice(None) if s is None else s
    return all(np.array_equal(a[k][sl].view(np.uint8) if a[k].dtype != np.uint8 else a[k][sl],
                              b[k][sl].view(np.uint8) if b[k].dtype != np.uint8 else b[k][sl]) for k in a)


@pytest.mark.parametrize("cap", [None, 2])
def test_schedule_s_flags_and_rows(cap):
    sim, got = simulate(cap), run(cap)
    n_updates, wrapped = 0, 0
    total = np.zeros(N, np.int64)
    for t, (want, g) in enumerate(zip(sim, got)):
        for s in ec.RESETS.get(t, ()):
            total[s] = 0
        total += [len(c) for c in rows_of(t)]
        upd = np.zeros(N, np.uint8)
        upd[want["updated"]] = 1
        assert np.array_equal(g["updated"], upd), (t, g["updated"], want["updated"])
        assert np.array_equal(g["valid"], np.array(want["valid"], np.uint8)), t
        assert len(want["updated"]) <= (cap or N)
        assert np.array_equal(bits(g["emotion"]), bits(g["features"])), t          # no layer in between: the same nine numbers
        for s in range(N):
            if s in want["windows"]:
                ref = reference(want["windows"][s])
                assert np.array_equal(bits(g["emotion"][s]), bits(ref)), (t, s, len(want["windows"][s]), g["emotion"][s], ref)
                n_updates += 1
                wrapped += int(total[s] > SHAPE["ring_len"] and total[s] % SHAPE["ring_len"] < SHAPE["window_len"])
            elif t in ec.RESETS and s in ec.RESETS[t]:
                assert not g["emotion"][s].any() and not g["valid"][s], (t, s)
            elif t > 0:
                assert np.array_equal(bits(got[t - 1]["emotion"][s]), bits(g["emotion"][s])) and got[t - 1]["valid"][s] == g["valid"][s], (t, s)
            if not want["valid"][s]:
                assert not g["emotion"][s].any(), (t, s)
    assert n_updates == sum(len(w["updated"]) for w in sim) and n_updates > 20
    assert wrapped > 0                                        # some windows straddled the end of their ring
    if cap == 2:
        assert any(len(w["updated"]) == 2 for w in sim)


def test_reset_stream_is_a_fresh_one_and_neighbours_do_not_notice():
    (t0, (s0,)), = ec.RESETS.items()
    with_reset, without = run(None), run(None, with_reset=False)
    fresh = run(None, with_reset=False, only=s0, start=t0)
    assert any(r["updated"][s0] for r in fresh) and with_reset[t0 - 1]["valid"][s0]
    for t in range(t0, ec.STEPS):
        assert same(with_reset[t], fresh[t - t0], s0), t
        for s in range(N):
            if s != s0:
                assert same(with_reset[t], without[t], s), (t, s)
    assert not same(with_reset[-1], without[-1], s0)


def test_graph_replay_is_the_eager_run():
    eager, replayed = run(None), run(None, graph=True)
    assert len(eager) == len(replayed) == ec.STEPS
    for t, (a, b) in enumerate(zip(eager, replayed)):
        assert same(a, b), t


def engine_basic():
    T, ED, _ = dc.VARIANTS["basic"]
    e = Engine(d_model=dc.D_MODEL, num_heads=dc.HEADS, mel_sequence_length=T, emotion_dim=ED)
    e.load_state_dict(dc.params("basic"))
    e.finalize()
    return e


def test_emotion_and_chunked_engine_in_one_capture_at_the_basic_shape():
    """push + update of the basic emotion streams and feed + step of the chunked engine at d_model 128, window 256, emotion_dim 9,
    recorded one after the other in the same capture with ``se.emotion`` as the step's input, replayed against an eager twin."""
    n, frame, prefill, steps = 3, 533, 36, 12

    def pair():
        return StreamEmotion(n, 1.0, 0.3, backend="basic"), ChunkedStreamEngine(engine_basic(), n, context_window=dc.SHORT_CW)

    audio = np.stack([ec.speechlike(900 + 7 * s, 2.0) * g for s, g in enumerate((0.8, 0.3, 0.5))]).astype(np.float32)
    assert audio.shape[1] >= (prefill + steps) * frame
    (sa, ca), (sb, cb) = pair(), pair()
    x_static = torch.zeros(n, frame, device="cuda")
    graph = None
    fired_any = updated_any = False
    for t in range(prefill + steps):
        x = dev(audio[:, t * frame:(t + 1) * frame])
        sb.push(x)
        emo_b, upd_b = sb.update()
        cb.feed(x)
        out_b, fired_b = cb.step(emo_b)
        if t < prefill:
            sa.push(x)
            emo_a, _ = sa.update()
            ca.feed(x)
            ca.step(emo_a)
            continue
        if graph is None:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                sa.push(x_static)
                sa.update()
                ca.feed(x_static)
                ca.step(sa.emotion)
        x_static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sa.emotion, sb.emotion) and torch.equal(sa.updated, sb.updated) and torch.equal(sa.valid, sb.valid), t
        assert torch.equal(ca.out, cb.out) and torch.equal(ca.fired, cb.fired) and torch.equal(ca.ready, cb.ready), t
        fired_any |= bool(fired_b.any())
        updated_any |= bool(upd_b.any())
    assert fired_any and updated_any and bool(sb.emotion.any())
    sa.close()
    sb.close()


def test_refusals():
    with pytest.raises(ValueError, match="compression"):
        StreamEmotion(N, ec.CONTEXT, ec.INTERVAL, backend="basic", compression_layer=torch.nn.Linear(264, 256))
    with pytest.raises(ValueError, match="backend"):
        StreamEmotion(N, ec.CONTEXT, ec.INTERVAL, backend="emotion2vec")
    se = make()
    with pytest.raises(AttributeError, match="slots"):
        se.slots
    import ctypes as C
    w = torch.zeros(256, 264, device="cuda")
    assert se._lib.km_emotion_stream_set_compression(se._h, w.data_ptr(), w.data_ptr(), None) == _lib.KM_ERR_INVALID_ARG
    f = torch.zeros(N, 9, device="cuda")
    assert se._lib.km_emotion_stream_features(se._h, f.data_ptr(), w.data_ptr(), None) == _lib.KM_ERR_INVALID_ARG
    with pytest.raises(KoeMorphError, match="samples per stream"):
        se.push(torch.zeros(N, SHAPE["ring_len"] + 1, device="cuda"))
    se.update()                                               # no set_compression is needed, and nothing is due
    assert not snapshot(se)["updated"].any()
    se.close()
    h = C.c_void_p()
    assert se._lib.km_emotion_stream_create_basic(C.byref(h), N, 66.0, 0.3, 1) == _lib.KM_ERR_UNSUPPORTED and not h.value


def test_device_memory_returns_after_close():
    lib = _lib.load()
    basic()
    torch.cuda.synchronize()
    base = lib.km_live_device_bytes()
    se = make()
    assert lib.km_live_device_bytes() > base + N * SHAPE["ring_len"] * 4
    x, cnt = ec.padded(rows_of(0))
    se.push(dev(x), dev(cnt))
    se.update()
    torch.cuda.synchronize()
    se.close()
    assert lib.km_live_device_bytes() == base


def test_the_egemaps_back_end_next_to_it_gives_the_bits_it_gave():
    """An eGeMAPS StreamEmotion before and after a basic one has run in the same process: the same flags, features, slots and rows."""
    torch.manual_seed(1234)
    layer = torch.nn.Linear(264, 256)

    def egemaps_run():
        se = StreamEmotion(N, ec.CONTEXT, ec.INTERVAL, compression_layer=layer)
        out = []
        for t in range(12):
            x, cnt = ec.padded(rows_of(t))
            se.push(dev(x), dev(cnt))
            se.update()
            torch.cuda.synchronize()
            out.append(dict(updated=se.updated.cpu().numpy().copy(), valid=se.valid.cpu().numpy().copy(), features=se.features.cpu().numpy(),
                            slots=se.slots.cpu().numpy(), emotion=se.emotion.cpu().numpy().copy()))
        se.close()
        return out

    before = egemaps_run()
    assert any(r["updated"].any() for r in before)
    sb = make()
    for t in range(12):
        x, cnt = ec.padded(rows_of(t))
        sb.push(dev(x), dev(cnt))
        sb.update()
    assert bool(sb.valid.any())
    after = egemaps_run()                                     # while the basic object is still alive
    sb.close()
    for t, (a, b) in enumerate(zip(before, after)):
        assert same(a, b), t
