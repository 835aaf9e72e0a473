"""Device-resident streams of SimplifiedKoeMorphModel (km_legacy_stream_*, LegacyStreamEngine, scripts/rt_simplified.py) against
the per-stream float64 reference of tests/legacy_stream_cases.py: RingBufferOracle FIFO -> oracle mel -> float64 model.

Tolerance: 2e-5, the project's existing bound for this model from audio against the oracle (tests/test_gpu_models.py:274); it is
the yardstick for every comparison here.  Each test prints the largest |hip - reference| it saw before it asserts.
"""
import json
import wave

import numpy as np
import pytest
import torch

import legacy_stream_cases as lc
from koemorph_amd import _lib, synth
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.model import SimplifiedKoeMorphModel
from koemorph_amd.streaming import LegacyStreamEngine

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the cases' arrays are read-only


def make_model():
    m = SimplifiedKoeMorphModel().cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in lc.params().items()})
    return m


def make_engine(name):
    c = lc.CASES[name]
    return LegacyStreamEngine(make_model(), c["n_streams"], buffer_duration=c["buffer_samples"] / 16000.0, audio_length=c["audio_length"])


def run_case(eng, name):
    """Every round of the case, eagerly: (out (rounds, S, 52) with the sentinel where nothing was written, ready (rounds, S))."""
    c, x = lc.CASES[name], lc.chunks(name)
    outs, readys = [], []
    for r in range(c["rounds"]):
        eng.push(dev(x[r]), dev(c["counts"][r]))
        eng.out.fill_(SENTINEL)
        out, ready = eng.tick()
        outs.append(out.cpu().numpy().copy())
        readys.append(ready.cpu().numpy().astype(bool))
    return np.stack(outs), np.stack(readys)


def check_case(name):
    got, ready = run_case(make_engine(name), name)
    sim, want = lc.simulate(name), lc.reference(name)
    assert np.array_equal(ready, sim["ready"]), (ready, sim["ready"])
    assert np.all(got[~ready] == SENTINEL), "a stream that was not ready had its row written"
    err = float(np.abs(got[ready] - want[ready]).max())
    print(f"legacy stream case {name}: {int(ready.sum())} windows, max |hip - float64 reference| = {err:.3e}")
    return got, ready, want, err


def test_short_ring_streams_out_of_phase():
    """3 streams, 12 push + tick rounds: ready on different ticks, one FIFO overflowing, write and read pointers wrapping.
    Observed on an MI355X: max |hip - float64 reference| = 8.960e-08 over the 21 popped windows (bound 2e-5); the other cases of this
    file: 1.277e-07 (4 frames), 8.915e-08 (32 frames), 1.157e-07 (smallest 32-frame window), 1.133e-07 (stale maximum), 6.819e-08 (script)."""
    _, ready, _, err = check_case("phase")
    assert ready.sum() >= 12 and err < lc.BOUND


@pytest.mark.parametrize("name", ["T4", "T32", "T32min"])
def test_frame_count_edges(name):
    """4 frames, 32 frames (no zero row, full key tile) and the smallest 32-frame window (odd length: scalar pop path)."""
    _, _, _, err = check_case(name)
    assert err < lc.BOUND


def test_too_many_frames_is_refused_at_construction():
    with pytest.raises(KoeMorphError, match="frames") as e:
        LegacyStreamEngine(make_model(), 2, buffer_duration=2.0, audio_length=17056)
    assert e.value.code == _lib.KM_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="exceeds the buffer"):
        LegacyStreamEngine(make_model(), 2, buffer_duration=1.0, audio_length=16001)


def test_stale_window_maximum():
    """A loud window, two ticks with nothing to pop, then a quiet window: its dB reference must be its own maximum."""
    got, ready, want, err = check_case("stale")
    assert ready[:, 0].tolist() == [True, False, False, True]
    last = float(np.abs(got[3, 0] - want[3, 0]).max())
    print(f"quiet window after the loud one: max |hip - reference| = {last:.3e}")
    assert last < lc.BOUND and err < lc.BOUND


def test_graph_replay_equals_eager_bit_for_bit():
    c, x = lc.CASES["phase"], lc.chunks("phase")
    eager, graph = make_engine("phase"), make_engine("phase")
    graph.capture(c["n_per_stream"])
    counts = torch.zeros(c["n_streams"], dtype=torch.int32, device="cuda")

    def rounds(lo, hi):
        for r in range(lo, hi):
            counts.copy_(dev(c["counts"][r]))
            eager.push(dev(x[r]), counts)
            eager.out.fill_(SENTINEL)
            graph.out.fill_(SENTINEL)
            eo, er = eager.tick()
            go, gr = graph.replay(dev(x[r]), counts)
            torch.cuda.synchronize()
            assert np.array_equal(er.cpu().numpy(), gr.cpu().numpy()), r
            assert np.array_equal(eo.cpu().numpy(), go.cpu().numpy()), r
        return er.cpu().numpy()

    seen = rounds(0, 5)
    assert seen.any()
    eager.reset()
    graph.reset()
    rounds(5, 8)
    # after the reset the FIFOs restart empty: the last round's flags against FIFO oracles that start at round 5
    from oracle import buffers
    fifos = [buffers.RingBufferOracle(c["buffer_samples"]) for _ in range(c["n_streams"])]
    for r in range(5, 8):
        for s, f in enumerate(fifos):
            f.write(x[r, s, :int(c["counts"][r, s])])
        want_last = [f.read(c["audio_length"]) is not None for f in fifos]
    assert graph.ready.cpu().numpy().astype(bool).tolist() == want_last


def test_handle_discipline():
    from koemorph_amd.engine import Engine, MelConfig
    lib = _lib.load()
    e = Engine()
    e.load_state_dict(synth.make_core_params(3))
    e.finalize()
    assert lib.km_legacy_stream_create(e._h, 2, 32000, 16000) == _lib.KM_ERR_INVALID_ARG
    assert b"legacy handle" in lib.km_last_error()
    out = torch.full((2, 52), SENTINEL, device="cuda")
    assert lib.km_legacy_stream_tick(e._h, out.data_ptr(), None, None) == _lib.KM_ERR_INVALID_ARG
    e.close()
    m = make_model()
    _, h, _ = m._handle()
    cfg = MelConfig.sliding_window(n_fft=1024, hop_length=533).to_c()
    import ctypes as C
    assert lib.km_stream_create(h, 2, 8.5, 0.0333, C.byref(cfg)) == _lib.KM_ERR_INVALID_ARG
    assert b"dual-stream handle" in lib.km_last_error()
    samples = torch.zeros(2, 1000, device="cuda")
    assert lib.km_legacy_stream_tick(h, out.data_ptr(), None, None) == _lib.KM_ERR_INVALID_ARG         # before create
    assert b"km_legacy_stream_create first" in lib.km_last_error()
    assert lib.km_legacy_stream_push(h, samples.data_ptr(), 1000, None, None) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_legacy_stream_reset(h, None) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_legacy_stream_create(h, 0, 32000, 16000) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_legacy_stream_create(h, 2, 16000, 16001) == _lib.KM_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert float(out.min()) == SENTINEL and float(out.max()) == SENTINEL        # nothing was launched on it


def test_rt_simplified_file_round_trip(tmp_path):
    from koemorph_amd.scripts import rt_simplified
    from oracle import buffers
    ckpt, wav, jsonl = tmp_path / "model.pth", tmp_path / "in.wav", tmp_path / "out.jsonl"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in lc.params().items()}}, ckpt)
    pcm = np.round(synth.make_audio(306, 1, 48000)[0] * 32767.0).astype(np.int16)           # 3 s
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    sent = rt_simplified.main(["--model_path", str(ckpt), "--input_file", str(wav), "--output_mode", "file", "--output_file", str(jsonl),
                               "--chunk_size", "1024"])
    audio = pcm.astype(np.float32) / 32768.0
    fifo, want = buffers.RingBufferOracle(32000), []
    for p in range(0, len(audio), 1024):
        chunk = audio[p:p + 1024]
        fifo.write(np.pad(chunk, (0, 1024 - len(chunk))))
        w = fifo.read(16000)
        if w is not None:
            want.append(lc.forward_window(w))
    lines = [json.loads(line) for line in open(jsonl)]
    assert len(want) == 3 and sent == 3 and len(lines) == 3
    err = 0.0
    for rec, ref in zip(lines, want):
        assert sorted(rec) == ["blendshapes", "timestamp"] and len(rec["blendshapes"]) == 52
        err = max(err, float(np.abs(np.asarray(rec["blendshapes"]) - ref).max()))
    print(f"rt_simplified file mode: 3 frames, max |hip - float64 reference| = {err:.3e}")
    assert err < lc.BOUND
