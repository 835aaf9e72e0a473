"""Host half of the device-resident emotion streams: the shape arithmetic, the host oracle of schedule S against the mirror's
AudioBuffer and against every stream simulated alone, and the seven exports.  No GPU."""
import os
import re

import numpy as np
import pytest

import stream_emotion_cases as ec
from koemorph_amd import _lib
from koemorph_amd.features.opensmile_extractor import AudioBuffer
from koemorph_amd.streaming import emotion_stream_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("km_emotion_stream_create", "km_emotion_stream_destroy", "km_emotion_stream_set_compression", "km_emotion_stream_push",
           "km_emotion_stream_update", "km_emotion_stream_reset_streams", "km_emotion_stream_features")


def test_shape_arithmetic_and_refusals():
    assert emotion_stream_shape() == dict(ring_len=352000, window_len=320000, update_samples=4800, min_samples=8000, max_frames=1995)
    assert emotion_stream_shape(ec.CONTEXT, ec.INTERVAL) == ec.SHAPE_S
    assert emotion_stream_shape(20.5, 0.3)["max_frames"] == 2045              # the longest window the functionals kernel holds
    with pytest.raises(ValueError, match="at most 2048"):
        emotion_stream_shape(20.6, 0.3)                                       # 2055 frames
    with pytest.raises(ValueError, match="Context window"):
        emotion_stream_shape(0.9, 0.3)
    with pytest.raises(ValueError, match="at least 0.1"):
        emotion_stream_shape(20.0, 0.05)
    with pytest.raises(ValueError, match="larger than context"):
        emotion_stream_shape(1.0, 1.5)
    with pytest.raises(ValueError, match="16 kHz"):
        emotion_stream_shape(20.0, 0.3, sample_rate=8000)


def test_schedule_s_is_what_the_tests_say_it_is():
    for cap, total in ((None, ec.UPDATES_UNCAPPED), (2, ec.UPDATES_CAP2)):
        sim = ec.simulate(cap)
        assert sum(len(r["updated"]) for r in sim) == total
        assert max(len(r["updated"]) for r in sim) <= (cap or ec.N_STREAMS)
    sim = ec.simulate(None)
    lengths = {len(w) for r in sim for w in r["windows"].values()}
    assert min(lengths) == 8000 and max(lengths) == 16000 and {8192, 13312, 11200} <= lengths     # not multiples of the 160-sample hop
    assert any(n % 160 for n in lengths)
    first = {s: next(t for t, r in enumerate(sim) if s in r["updated"]) for s in range(ec.N_STREAMS)}
    assert first[2] > first[0]                                                                    # the late join
    assert not any(4 in r["updated"] for r in sim[25:31])                                         # the pause
    assert not sim[30]["valid"][2] and sim[29]["valid"][2] and sim[-1]["valid"][2]                # the reset and the refill
    assert sim[29]["slot_from"][2] != sim[-1]["slot_from"][2]
    # with the cap, a stream that lost keeps its place in the queue: it is served on a later step, never dropped
    capped = ec.simulate(2)
    assert any(set(a["updated"]) != set(b["updated"]) for a, b in zip(sim, capped))


def test_oracle_windows_equal_the_mirror_audio_buffer():
    """AudioBuffer (the mirror of the reference's class, host numpy) driven with the same chunks returns the oracle's window at
    every update: the growing window, the stale 'oldest C' window of an unwrapped ring and the wrapped ring."""
    sim = ec.simulate(None)
    bufs = [AudioBuffer(ec.CONTEXT + 2.0) for _ in range(ec.N_STREAMS)]
    kinds = set()
    for t, row in enumerate(ec.chunks()):
        for s in ec.RESETS.get(t, ()):
            bufs[s].reset()
        for s, c in enumerate(row):
            if len(c):
                bufs[s].append(np.array(c))
        for s, win in sim[t]["windows"].items():
            got = bufs[s].get_window(ec.CONTEXT)
            assert got.dtype == np.float32 and np.array_equal(got, win), (t, s)
            b = bufs[s]
            kinds.add("wrapped" if b.is_full else ("stale" if b.write_pos > len(win) else "growing"))
    assert kinds == {"growing", "stale", "wrapped"}


def test_streams_do_not_interact_without_a_cap():
    sim = ec.simulate(None)
    for s in range(ec.N_STREAMS):
        assert ec.simulate_alone(s) == [t for t, r in enumerate(sim) if s in r["updated"]], s


def test_header_and_signature_table_name_the_exports():
    text = open(os.path.join(ROOT, "include", "koemorph.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in EXPORTS:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert hasattr(_lib.load(), "km_emotion_stream_update")
