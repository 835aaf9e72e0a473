"""Host logic of the legacy model's streams (no GPU): the shape arithmetic of LegacyStreamEngine, the command line of
scripts/rt_simplified.py and the invariants of the case generator the GPU tests rely on (tests/legacy_stream_cases.py)."""
import numpy as np
import pytest

import legacy_stream_cases as lc
from koemorph_amd.streaming import legacy_stream_shape


def test_frame_counts_and_limits():
    assert legacy_stream_shape(2.0, 16000, 533, 16000) == dict(buffer_samples=32000, n_frames=31, supported=True)
    assert legacy_stream_shape(2.0, 17055, 533, 16000)["n_frames"] == 32 and legacy_stream_shape(2.0, 17055, 533, 16000)["supported"]
    s = legacy_stream_shape(2.0, 17056, 533, 16000)
    assert s["n_frames"] == 33 and not s["supported"]
    assert legacy_stream_shape(2.0, 16523, 533, 16000)["n_frames"] == 32 and legacy_stream_shape(2.0, 16522, 533, 16000)["n_frames"] == 31
    assert legacy_stream_shape(2.0, 1600, 533, 16000)["n_frames"] == 4
    assert legacy_stream_shape(0.5, 8000, 533, 16000)["buffer_samples"] == 8000
    with pytest.raises(ValueError, match="exceeds the buffer"):
        legacy_stream_shape(2.0, 32001, 533, 16000)
    with pytest.raises(ValueError):
        legacy_stream_shape(2.0, 0, 533, 16000)


def test_cli_arguments_are_the_reference_ones():
    from koemorph_amd.scripts import rt_simplified
    p = rt_simplified.build_parser()
    a = p.parse_args(["--model_path", "m.pth"])
    assert (a.sample_rate, a.target_fps, a.chunk_size, a.audio_length, a.output_mode, a.host, a.port, a.device) == \
        (16000, 30.0, 1024, 16000, "udp", "127.0.0.1", 9001, "auto")
    assert a.input_file is None and a.output_file is None and a.duration is None and a.no_audio is False
    a = p.parse_args(["--model_path", "m.pth", "--input_file", "a.wav", "--audio_length", "8000", "--chunk_size", "512",
                      "--output_mode", "file", "--output_file", "o.jsonl", "--duration", "2.5", "--no_audio"])
    assert (a.input_file, a.audio_length, a.chunk_size, a.output_mode, a.output_file, a.duration, a.no_audio) == \
        ("a.wav", 8000, 512, "file", "o.jsonl", 2.5, True)
    with pytest.raises(SystemExit):
        p.parse_args(["--model_path", "m.pth", "--output_mode", "tcp"])
    with pytest.raises(SystemExit):
        p.parse_args([])


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_every_case_mixes_ready_and_waiting_streams(name):
    c, sim = lc.CASES[name], lc.simulate(name)
    ready = sim["ready"]
    assert ready.shape == (c["rounds"], c["n_streams"])
    mixed = [r for r in range(c["rounds"]) if ready[r].any() and not ready[r].all()]
    assert mixed, "no tick with some streams ready and some not"
    assert ready.any(axis=0).all(), "a stream that never becomes ready checks nothing"
    assert (c["counts"] >= 0).all() and (c["counts"] <= c["n_per_stream"]).all()
    assert 1 + c["audio_length"] // lc.HOP <= 32
    for r in range(c["rounds"]):
        for s in range(c["n_streams"]):
            w = sim["windows"][r][s]
            assert (w is not None) == bool(ready[r, s]) and (w is None or w.shape == (c["audio_length"],))


def test_phase_case_overflows_and_wraps():
    sim = lc.simulate("phase")
    assert sim["truncated"] >= 1, "no write truncated by a full FIFO"
    assert sim["write_straddles"] >= 1 and sim["read_wraps"] >= 1
    first = [int(np.argmax(sim["ready"][:, s])) for s in range(3)]
    assert len(set(first)) == 3, f"the streams become ready on the same tick: {first}"


@pytest.mark.parametrize("name", ["T32", "T32min"])
def test_edge_cases_have_reads_that_straddle_the_end_of_the_ring(name):
    assert lc.simulate(name)["read_straddles"] >= 1


def test_stale_case_schedule():
    ready = lc.simulate("stale")["ready"]
    assert ready[:, 0].tolist() == [True, False, False, True] and ready[:, 1].all()
    x = lc.chunks("stale")
    assert np.abs(x[0, 0]).max() > 50.0 and np.abs(x[3, 0]).max() < 0.01
