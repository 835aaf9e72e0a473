"""The emotion logits of the 1024-point front end at d_model 256: group workgroups against the per-window rider.

By default the front-end launch of a d_model 256 engine carries ceil(B / G) extra workgroups in front of its grid, each of which
computes the logits of G = 2 consecutive windows with one read of the weights (emotion_group_d256, km_device.h).  The option
emotion_rider = 1 puts the per-window rider (emotion_window_d256) back, emotion_separate = 1 the stand-alone kernel
(emotion_kernel_d256).  The three sum in the same order, so the whole contract is bit identity of what the step returns -- the
engine does not expose the logits themselves.  The mapping from a workgroup's linear id to its role is walked on the host
(km_mel_role_table calls the function the kernel calls); that test needs no GPU.

Shapes: d_model 256, 8 heads, window 256, trained parameters; 8528 samples a window (17 frames, two workgroups a window), the
shortest audio the d_model 256 forward tests use; the replay test runs the benchmark's 136448 samples."""
import numpy as np
import pytest
import torch

from koemorph_amd import _lib, synth
from koemorph_amd.engine import Engine
from koemorph_amd.streaming import StreamEngine

G = 2                      # kMelEmoGroup (km_context.h)
L_SHORT = 16 * 533
FORMS = ({}, {"emotion_rider": 1}, {"emotion_separate": 1})


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_engines = {}


def engine(emotion_dim):
    if emotion_dim not in _engines:
        e = Engine(emotion_dim=emotion_dim)
        e.load_state_dict(synth.make_core_params(31, 256, 256, emotion_dim, "trained"))
        e.finalize()
        _engines[emotion_dim] = e
    return _engines[emotion_dim]


def with_options(e, options, fn):
    for k, v in options.items():
        e.set_option(k, v)
    try:
        return fn()
    finally:
        for k in options:
            e.set_option(k, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("emotion_dim", [256, 88, 5])
@pytest.mark.parametrize("B", sorted({1, G - 1, G, G + 1, 2 * G + 3}))
def test_three_forms_are_bit_identical(B, emotion_dim):
    e = engine(emotion_dim)
    audio, emo = dev(synth.make_audio(900 + B, B, L_SHORT)), dev(synth.normal(950 + B, (B, emotion_dim)))
    outs = [with_options(e, o, lambda: e.forward_audio(audio, emo).cpu().numpy()) for o in FORMS]
    assert np.isfinite(outs[0]).all() and outs[0].std() > 0
    assert np.array_equal(outs[0], outs[1]), "group workgroups against the per-window rider"
    assert np.array_equal(outs[0], outs[2]), "group workgroups against emotion_kernel_d256"


@pytest.mark.gpu
def test_sequence_tiles_off_the_group_size():
    """No forward path launches the front end with logits at win0 != 0, so: 2 G + 3 clips of two window positions through
    km_sequence_forward, in tiles of 2 G + 3 windows (no multiple of G).  Sequence mode takes its logits from emotion_kernel_d256;
    the option must leave it alone."""
    e, B = engine(256), 2 * G + 3
    audio, emo = dev(synth.make_audio(920, B, 256 * 533 + 533)), dev(synth.normal(921, (B, 256)))
    got = e.sequence_forward(audio, emo, stride_frames=1, max_tile=B).cpu().numpy()
    assert got.shape == (B, 2, 52)
    want = with_options(e, {"emotion_rider": 1}, lambda: e.sequence_forward(audio, emo, stride_frames=1, max_tile=B).cpu().numpy())
    assert np.array_equal(got, want)


def _tick_with_one_stream_refilling(options):
    S, late = 2 * G + 1, G + 1
    e = Engine()
    e.load_state_dict(synth.make_core_params(31, 256, 256, 256, "trained"))
    e.finalize()
    for k, v in options.items():
        e.set_option(k, v)
    se = StreamEngine(e, S)
    frames = synth.make_audio(930, S, 533 * 257)
    for t in range(256):
        se.push(dev(frames[:, 533 * t:533 * (t + 1)]))
    mask = torch.zeros(S, dtype=torch.uint8, device="cuda")
    mask[late] = 1
    assert _lib.load().km_stream_reset_streams(e._h, mask.data_ptr(), None) == _lib.KM_OK
    se.out.fill_(7.0)
    se.push(dev(frames[:, 533 * 256:]))
    out, ready = se.tick(dev(synth.normal(931, (S, 256))))
    out, ready = out.cpu().numpy(), ready.cpu().numpy()
    e.close()
    return out, ready, late


@pytest.mark.gpu
def test_stream_tick_with_a_stream_not_ready():
    """2 G + 1 full rings, one of them (inside the second group) emptied again: its logit is not stored, its row
    keeps what it held, and the others' rows are the rider's bit for bit."""
    got, ready, late = _tick_with_one_stream_refilling({})
    want, ready_r, _ = _tick_with_one_stream_refilling({"emotion_rider": 1})
    assert ready.tolist() == [int(s != late) for s in range(2 * G + 1)] and np.array_equal(ready, ready_r)
    assert np.all(got[late] == 7.0) and np.array_equal(got, want)
    assert np.isfinite(got).all() and np.all(got[ready != 0] != 7.0)


@pytest.mark.gpu
def test_graph_replay_at_the_benchmark_shape():
    """The step of the benchmark's shape at B = G + 1, captured and replayed three times: every replay gives the eager call's bits,
    so the launch leaves its chunk counters and window maxima as it found them."""
    e, B, L = engine(256), G + 1, 136448
    audio, emo = dev(synth.make_audio(940, B, L)), dev(synth.normal(941, (B, 256)))
    state = torch.zeros(B, 52, device="cuda")
    want = e.forward_audio(audio, emo, state=state, first=True).clone()
    out, gstate = torch.empty(B, 52, device="cuda"), torch.zeros(B, 52, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e.forward_audio(audio, emo, state=gstate, first=True, out=out)
    for i in range(3):
        out.fill_(-1.0)
        graph.replay()
        assert torch.equal(out, want), i
    assert torch.equal(gstate, state)


def test_role_mapping_on_the_host():
    """Every window's logit has one owner, every (window, workgroup) of the front end appears once, and the surplus ids of the
    rounded-up grid have no role: B = 1 .. 600, per_window in {1, 2, 4, 17}, group sizes 2 (the library's), 4 and 8; and without groups the mapping is the
    one the launches without logits have always had."""
    table = _lib.load().km_mel_role_table
    for group in (G, 4, 8):
        for per_window in (1, 2, 4, 17):
            for B in range(1, 601):
                E = -(-B // group)
                n = per_window * (B + -(-E // per_window)) + 3          # the launch's grid, and three ids beyond it
                out = np.full((n, 3), -1, np.int32)
                assert table(B, per_window, group, n, out.ctypes.data) == _lib.KM_OK
                kind, b, bx = out.T
                assert np.array_equal(kind[:E], np.ones(E)) and np.array_equal(b[:E], np.arange(E)), (group, per_window, B)
                owners = np.zeros(B, np.int64)                           # windows [group b, group b + group) below B
                for g in b[:E]:
                    owners[group * g:group * g + group] += 1
                assert np.all(owners == 1), (group, per_window, B)
                fe = slice(E, E + per_window * B)
                assert np.all(kind[fe] == 2), (group, per_window, B)
                seen = np.zeros((B, per_window), np.int64)
                np.add.at(seen, (b[fe], bx[fe]), 1)
                assert np.all(seen == 1), (group, per_window, B)
                assert np.all(out[E + per_window * B:] == 0), (group, per_window, B)
    out = np.full((3 * 5 + 2, 3), -1, np.int32)
    assert table(5, 3, 0, len(out), out.ctypes.data) == _lib.KM_OK
    want = [(2, i % 5, i // 5) for i in range(15)] + [(0, 0, 0)] * 2
    assert out.tolist() == [list(w) for w in want]
    assert table(0, 1, 8, 1, out.ctypes.data) == _lib.KM_ERR_INVALID_ARG
