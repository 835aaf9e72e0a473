"""Host side of the streams out of phase (no GPU): the schedules of tests/stream_chunked_cases.py really contain the situations
the GPU tests are about -- recomputed here with the oracle classes, so that those tests cannot pass vacuously -- the arithmetic of
chunked_stream_shape, and the presence of the public pieces."""
import numpy as np
import pytest

import stream_chunked_cases as cc


def test_schedule_a_contains_every_situation():
    sim = cc.simulate("A")
    fired, ready, popped, dropped = sim["fired"], sim["ready"], sim["popped"], sim["dropped"]
    first = [int(np.argmax(fired[:, s])) for s in range(4)]
    assert first == [60, 78, 80, 60]
    assert fired.sum(axis=0).tolist() == [82, 57, 12, 92]
    idle_full = (ready & ~popped).sum(axis=0).tolist()
    assert idle_full == [10, 17, 0, 0]                                   # idle-while-full: stream 0's pause, stream 1 between chunks
    assert dropped.sum(axis=0).tolist() == [0, 0, 0, 5000]               # overflow drop
    assert int((dropped[:, 3] > 0).sum()) >= 5
    # late join: stream 2 pops nothing for 20 steps and is the last to fire
    assert not popped[:20, 2].any() and popped[20:85, 2].all() and first[2] > max(first[0], first[3])
    # reset of a full stream followed by a refill: 5 rows before the reset, none for 60 steps, 7 after
    assert int(fired[:85, 2].sum()) == 5 and ready[84, 2] and not ready[85, 2]
    assert not fired[85:145, 2].any() and fired[145:, 2].all() and int(fired[145:, 2].sum()) == 7
    assert sim["life"][84, 2] == 0 and sim["life"][85, 2] == 1 and not sim["life"][:, [0, 1, 3]].any()
    # steps on which some but not all streams fire, and the patterns that occur
    partial = [t for t in range(fired.shape[0]) if 0 < fired[t].sum() < 4]
    assert len(partial) >= 5 and len({tuple(r) for r in fired.tolist()}) == 7
    # a backlog to drain: stream 3 holds whole frames after its pop on most steps
    assert int(sim["backlog"][:, 3].max()) == 5 and int((sim["backlog"][:, 1] > 0).sum()) >= 5
    # the oracle pairs are what the GPU test says they are
    assert cc.previous_fire(sim, 110, 0) == 99 and cc.previous_fire(sim, 145, 2) is None and cc.previous_fire(sim, 146, 2) == 145
    for s, t in ((1, 78), (3, 60), (2, 80)):
        assert cc.previous_fire(sim, t, s) is None
    assert sorted(sim["windows"]) == sorted(cc.SCHEDULES["A"]["oracle_pairs"]) and len(sim["windows"]) <= 10
    assert all(w.shape == (16000,) for w in sim["windows"].values())


def test_schedule_a_first_90_steps_keep_the_reset():
    sim = cc.simulate("A", 90)
    full = cc.simulate("A")
    assert np.array_equal(sim["fired"], full["fired"][:90]) and sim["life"][89, 2] == 1
    assert int(sim["fired"][:, 2].sum()) == 5 and (sim["ready"] & ~sim["popped"])[:, 1].any()
    assert sum(1 for r in sim["fired"] if 0 < r.sum() < 4) >= 5


def test_schedule_b_contains_every_situation():
    sim = cc.simulate("B")
    fired, ready, popped = sim["fired"], sim["ready"], sim["popped"]
    assert [int(np.argmax(fired[:, s])) for s in range(3)] == [255, 255, 275]
    assert int((ready & ~popped)[:, 1].sum()) >= 5                       # stream 1 idles with a full ring
    assert int(sim["dropped"].sum()) == 0
    # every popped frame has 533 samples and the ring keeps 532 of them
    assert sim["truncated"] == [len(p) for p in sim["pops"]] and all(len(f) == 533 for p in sim["pops"] for _, _, f in p)
    assert len(sim["windows"]) <= 8 and all(w.shape == (136000,) for w in sim["windows"].values())
    assert cc.previous_fire(sim, 261, 1) == 258 and not popped[259:261, 1].any()
    # from step 280 on (the replayed part) some steps fire all streams and some do not
    assert fired[280:].all(axis=1).any() and not fired[280:].all()


def test_chunked_stream_shape():
    from koemorph_amd.streaming import chunked_stream_shape, stream_shape
    assert chunked_stream_shape() == dict(fifo_samples=32000, frame_samples=533, ring_hop=532)
    assert chunked_stream_shape(8.5, 1.0 / 60.0) == dict(fifo_samples=32000, frame_samples=266, ring_hop=266)
    assert chunked_stream_shape(1.0, 1.0 / 60.0, buffer_duration=0.1) == dict(fifo_samples=1600, frame_samples=266, ring_hop=266)
    assert chunked_stream_shape(frame_samples=531)["frame_samples"] == 531
    assert chunked_stream_shape()["ring_hop"] == stream_shape(8.5, 0.0333, 533)["ring_hop"]
    with pytest.raises(ValueError, match="Frame size mismatch: expected ~532, got 500"):
        chunked_stream_shape(frame_samples=500)
    with pytest.raises(ValueError, match="no read could ever succeed"):
        chunked_stream_shape(buffer_duration=0.03)                      # 480 samples < 533
    with pytest.raises(ValueError, match="positive"):
        chunked_stream_shape(buffer_duration=0.0)
    with pytest.raises(ValueError, match="positive"):
        chunked_stream_shape(frame_samples=0)


def test_public_pieces_exist():
    from koemorph_amd import _lib, streaming
    assert issubclass(streaming.ChunkedStreamEngine, streaming.StreamEngine)
    for m in ("feed", "step", "reset_streams", "capture", "replay"):
        assert callable(getattr(streaming.ChunkedStreamEngine, m))
    lib = _lib.load()
    for name in ("km_stream_fifo_create", "km_stream_feed", "km_stream_step", "km_stream_reset_streams"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.KM_ABI_VERSION == 2 and lib.km_abi_version() == 2
