"""Emotion vectors of many streams on the device (km_emotion_stream_*, koemorph_amd.streaming.StreamEmotion) on schedule S of
tests/stream_emotion_cases.py.

Who updates, and on which window, is checked against the host oracle on every step.  What an update computes is checked BIT FOR
BIT against the pinned B = 1 path, ``EGeMAPSEngine.functionals(window[None])[0]`` on the oracle's window: the ragged kernels read
the samples where they lie in the stream's ring, but a frame's arithmetic is the same code, so no tolerance is needed and none is
given.  The 264 -> 256 product alone has a bound, the worst-case rounding of a 264-term float32 dot product plus bias in any order:
|got - exact| <= 265 * 2^-24 * (|W| . |x| + |b|) per output (gamma_265 with unit roundoff 2^-24, derived, not measured).
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

import stream_emotion_cases as ec
from koemorph_amd import synth
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.engine import Engine
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEmotion, emotion_stream_shape
from oracle.buffers import AudioBufferOracle

pytestmark = pytest.mark.gpu
GRAPH_M = 4000          # the largest chunk of schedule S
GRAPH_FROM = 8          # the graph run is eager up to here (two streams have features by then), captured and replayed from here on


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the cases' arrays are read-only


@functools.lru_cache(maxsize=None)
def layer():
    torch.manual_seed(1234)
    return torch.nn.Linear(264, 256)


@functools.lru_cache(maxsize=None)
def egemaps():
    return EGeMAPSEngine("cuda")


_REF = {}


def reference(window: np.ndarray) -> np.ndarray:
    """The pinned B = 1 path on one window, NaN / Inf -> 0 as the extractor does; computed once per distinct window."""
    key = hashlib.sha1(np.ascontiguousarray(window).tobytes()).hexdigest()
    if key not in _REF:
        f = egemaps().functionals(dev(window)[None])[0].cpu().numpy()
        _REF[key] = np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)
    return _REF[key]


def make(max_updates=None):
    se = StreamEmotion(ec.N_STREAMS, ec.CONTEXT, ec.INTERVAL, max_updates=max_updates, compression_layer=layer())
    assert se.shape == ec.SHAPE_S
    return se


def snapshot(se):
    torch.cuda.synchronize()
    return dict(updated=se.updated.cpu().numpy().copy(), valid=se.valid.cpu().numpy().copy(), features=se.features.cpu().numpy(),
                slots=se.slots.cpu().numpy(), emotion=se.emotion.cpu().numpy().copy())


@functools.lru_cache(maxsize=None)
def run(max_updates=None, with_reset=True, graph=False, only=None, start=0):
    """Schedule S from step `start` on a fresh StreamEmotion -> one snapshot per step.  only: feed that stream alone."""
    se = make(max_updates)
    out = []
    for t, row in enumerate(ec.chunks()):
        if t < start:
            continue
        if with_reset and t in ec.RESETS:
            mask = torch.zeros(ec.N_STREAMS, dtype=torch.bool, device="cuda")
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
    """Bitwise equality of two snapshots (of stream s alone, if given)."""
    sl = slice(None) if s is None else s
    return all(np.array_equal(a[k][sl].view(np.uint8) if a[k].dtype != np.uint8 else a[k][sl],
                              b[k][sl].view(np.uint8) if b[k].dtype != np.uint8 else b[k][sl]) for k in a)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1, 2: schedule S ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [None, 2])
def test_schedule_s_flags_features_and_slots(cap):
    sim, got = ec.simulate(cap), run(cap)
    n_updates = 0
    first_features = {}                                     # (stream, step of the life's first update) -> its features
    for t, (want, g) in enumerate(zip(sim, got)):
        upd = np.zeros(ec.N_STREAMS, np.uint8)
        upd[want["updated"]] = 1
        assert np.array_equal(g["updated"], upd), (t, g["updated"], want["updated"])
        assert np.array_equal(g["valid"], np.array(want["valid"], np.uint8)), t
        assert len(want["updated"]) <= (cap or ec.N_STREAMS)
        for s in range(ec.N_STREAMS):
            if s in want["windows"]:
                ref = reference(want["windows"][s])
                assert np.array_equal(bits(g["features"][s]), bits(ref)), (t, s, len(want["windows"][s]),
                                                                           float(np.abs(g["features"][s] - ref).max()))
                if want["slot_from"][s] == t:
                    first_features[(s, t)] = ref
                n_updates += 1
            elif t in ec.RESETS and s in ec.RESETS[t]:
                assert not g["features"][s].any() and not g["slots"][s].any() and not g["emotion"][s].any() and not g["valid"][s], (t, s)
            elif t > 0:
                for k in ("features", "slots", "emotion", "valid"):
                    assert np.array_equal(bits(got[t - 1][k][s]) if k != "valid" else got[t - 1][k][s],
                                          bits(g[k][s]) if k != "valid" else g[k][s]), (t, s, k)
            if want["slot_from"][s] is not None:
                first = first_features[(s, want["slot_from"][s])]
                assert np.array_equal(bits(g["slots"][s, 0]), bits(first)) and np.array_equal(bits(g["slots"][s, 1]), bits(first)), (t, s)
            else:
                assert not g["slots"][s].any() and not g["features"][s].any() and not g["emotion"][s].any(), (t, s)
    assert n_updates == (ec.UPDATES_UNCAPPED if cap is None else ec.UPDATES_CAP2)


@pytest.mark.parametrize("cap", [None, 2])
def test_schedule_s_emotion_rows(cap):
    sim, got = ec.simulate(cap), run(cap)
    W = layer().weight.detach().numpy().astype(np.float64)
    b = layer().bias.detach().numpy().astype(np.float64)
    worst, checked = 0.0, 0
    for t, (want, g) in enumerate(zip(sim, got)):
        for s in want["updated"]:
            x = np.concatenate([g["features"][s], g["slots"][s, 0], g["slots"][s, 1]]).astype(np.float64)
            exact = W @ x + b
            bound = 265 * 2.0 ** -24 * (np.abs(W) @ np.abs(x) + np.abs(b))
            err = np.abs(g["emotion"][s].astype(np.float64) - exact)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (t, s, float((err / bound).max()))
            checked += 1
    print(f"schedule S cap {cap}: {checked} rows, worst error / bound = {worst:.3f}")
    assert checked == (ec.UPDATES_UNCAPPED if cap is None else ec.UPDATES_CAP2)


# ---- 3: reset -----------------------------------------------------------------------------------------------------------------
def test_reset_stream_is_a_fresh_one_and_neighbours_do_not_notice():
    (t0, (s0,)), = ec.RESETS.items()
    with_reset, without = run(None), run(None, with_reset=False)
    fresh = run(None, with_reset=False, only=s0, start=t0)
    assert any(r["updated"][s0] for r in fresh) and with_reset[t0 - 1]["valid"][s0]
    for t in range(t0, ec.STEPS):
        assert same(with_reset[t], fresh[t - t0], s0), t
        for s in range(ec.N_STREAMS):
            if s != s0:
                assert same(with_reset[t], without[t], s), (t, s)
    assert not same(with_reset[-1], without[-1], s0)             # the reset did change stream 2
    # reset(): everything
    se = make()
    for row in ec.chunks()[:8]:
        x, cnt = ec.padded(row)
        se.push(dev(x), dev(cnt))
        se.update()
    assert se.valid.any()
    se.reset()
    z = snapshot(se)
    assert not any(z[k].any() for k in z)
    se.update()
    assert not snapshot(se)["updated"].any()
    se.close()


# ---- 4: graph replay ----------------------------------------------------------------------------------------------------------
def test_graph_replay_is_the_eager_run():
    eager, replayed = run(None), run(None, graph=True)
    assert len(eager) == len(replayed) == ec.STEPS
    for t, (a, b) in enumerate(zip(eager, replayed)):
        assert same(a, b), t


def test_emotion_and_chunked_engine_in_one_capture():
    """push + update of the emotion streams and feed + step of the chunked engine, recorded one after the other in the same capture
    with ``se.emotion`` as the step's input: one linear chain, replayed against an eager twin."""
    n, frame, prefill, steps = 3, 533, 250, 12

    def pair():
        e = Engine()
        e.load_state_dict(synth.make_core_params(61, style="trained"))
        e.finalize()
        return StreamEmotion(n, 1.0, 0.3, compression_layer=layer()), ChunkedStreamEngine(e, n)

    audio = np.stack([ec.speechlike(900 + 7 * s, 9.0) * g for s, g in enumerate((0.8, 0.3, 0.5))]).astype(np.float32)
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
    assert fired_any and updated_any
    sa.close()
    sb.close()


# ---- 5: the full-size edge ----------------------------------------------------------------------------------------------------
def test_default_shape_wrapped_ring():
    """20 s window, 1 995 frames against the 2 048 the kernels hold; 22.5 s in 80 000-sample chunks, so that the 22 s ring wraps."""
    n, chunk, pushes = 2, 80000, 5
    sh = emotion_stream_shape()
    assert sh["max_frames"] == 1995 and chunk * pushes > sh["ring_len"]
    audio = np.stack([np.concatenate([ec.speechlike(1100 + 50 * s + k, 2.5) for k in range(10)])[:chunk * pushes] * g
                      for s, g in enumerate((0.7, 0.2))]).astype(np.float32)
    assert audio.shape == (n, chunk * pushes)
    se = StreamEmotion(n, compression_layer=layer())
    bufs = [AudioBufferOracle(22.0) for _ in range(n)]
    for k in range(pushes):
        x = audio[:, k * chunk:(k + 1) * chunk]
        se.push(dev(x))
        _, upd = se.update()
        assert upd.all()                                              # 5 s of audio since the last update: every stream is due
        for s in range(n):
            bufs[s].append(x[s])
    got = se.features.cpu().numpy()
    for s in range(n):
        assert bufs[s].full
        win = bufs[s].get_window(20.0)
        assert len(win) == 320000
        ref = reference(win)
        assert np.array_equal(bits(got[s]), bits(ref)), (s, float(np.abs(got[s] - ref).max()))
    se.close()
    with pytest.raises(ValueError, match="at most 2048"):
        StreamEmotion(n, context_window=20.6)


def test_counts_are_clamped_and_a_zero_count_leaves_the_stream_alone():
    x = dev(np.stack([ec.audio(s)[:9000] for s in range(ec.N_STREAMS)]))
    a, b = make(), make()
    a.push(x, torch.tensor([9000, 12000, -3, 0, 8500], dtype=torch.int32, device="cuda"))       # beyond m, negative, zero
    b.push(x, torch.tensor([9000, 9000, 0, 0, 8500], dtype=torch.int32, device="cuda"))
    a.update()
    b.update()
    sa, sb = snapshot(a), snapshot(b)
    assert same(sa, sb) and list(sa["updated"]) == [1, 1, 0, 0, 1]
    assert np.array_equal(bits(sa["features"][4]), bits(reference(ec.audio(4)[:8500])))
    a.close()
    b.close()


# ---- 6: refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    se = make()
    with pytest.raises(KoeMorphError, match="samples per stream"):
        se.push(torch.zeros(ec.N_STREAMS, ec.SHAPE_S["ring_len"] + 1, device="cuda"))           # m > R
    se.push(torch.zeros(ec.N_STREAMS, ec.SHAPE_S["ring_len"], device="cuda"))                   # m = R is a whole ring
    for bad in (0, ec.N_STREAMS + 1):
        with pytest.raises(ValueError, match="max_updates"):
            StreamEmotion(ec.N_STREAMS, ec.CONTEXT, ec.INTERVAL, max_updates=bad)
    with pytest.raises(ValueError, match="at least 0.1"):
        StreamEmotion(ec.N_STREAMS, ec.CONTEXT, 0.05)
    with pytest.raises(ValueError, match="mask"):
        se.reset_streams(torch.zeros(ec.N_STREAMS + 1, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="counts"):
        se.push(torch.zeros(ec.N_STREAMS, 16, device="cuda"), torch.zeros(ec.N_STREAMS, dtype=torch.int64, device="cuda"))
    # the library refuses by itself what the Python layer catches first
    import ctypes as C
    lib, h = se._lib, C.c_void_p()
    for args in ((ec.N_STREAMS, 1.0, 0.3, 0), (ec.N_STREAMS, 1.0, 0.3, ec.N_STREAMS + 1), (ec.N_STREAMS, 1.0, 0.05, 1),
                 (ec.N_STREAMS, 0.5, 0.3, 1), (ec.N_STREAMS, 1.0, 1.5, 1), (ec.N_STREAMS, 20.6, 0.3, 1)):
        assert lib.km_emotion_stream_create(C.byref(h), *args) != 0 and not h.value, args
    se.close()
