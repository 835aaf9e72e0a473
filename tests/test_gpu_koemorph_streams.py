"""KoeMorphStreams (km_koemorph_stream_*) on the device.

The main pin is EQUAL BITS with the loop the engine replaces: per stream, ``KoeMorphModel.forward`` at B = 1 on a second model with
the same weights, frame by frame over that stream's rows since its last reset, the output fed back.  That can hold because the chain
kernel runs the decode kernel's statements (one shared ``decode_window``, the window length an argument) and the ragged encoder lays a
window of T_i rows out as a forward call at B = 1 does (tests/test_gpu_koemorph_rollout.py pins that a window's encoding does not
depend on its neighbours).  Then the float64-backed oracle, equality with ``rollout``, capture and replay, guard regions, state and
memory."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import koemorph_stream_cases as sc
import rollout_cases as rc
from koemorph_amd import _lib, synth
from koemorph_amd.streaming import KoeMorphStreams
from oracle import koemorph_model as okm

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_koemorph.py: this project's tolerance on the 52 coefficients

_models = {}


def models(emotion_dim=256, smoothing="exponential"):
    """(engine model, loop model, cfg, params): two models of one configuration and one set of weights, made once per module."""
    key = (emotion_dim, smoothing)
    if key not in _models:
        cfg = okm.KoeMorphConfig(emotion_dim=emotion_dim, smoothing_method="exponential" if smoothing == "off" else smoothing)
        params = okm.make_koemorph_params(17, cfg)
        _models[key] = (rc.build(cfg, params), rc.build(cfg, params), cfg, params)
    return _models[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, float(np.nanmax(np.abs(a - b))))


def walk(eng, steps, mel, emo, replay=False):
    """Drive ``eng`` through ``steps`` = [(counts, reset mask or None)]; stream s takes its rows from mel[s] / emo[s] in order.
    -> per stream the list of lives, a life = (first row, rows, out (rows, 52), raw) -- rows of the life's frames in order."""
    N, R = eng.n_streams, eng.max_rows
    used = [0] * N
    lives = [[[0, 0, [], []]] for _ in range(N)]
    taken = []
    for counts, mask in steps:
        if mask is not None:
            eng.reset_streams(torch.tensor(mask, dtype=torch.bool, device="cuda"))
            for s in range(N):
                if mask[s]:
                    lives[s].append([used[s], 0, [], []])
        bm = torch.zeros(N, R, mel.shape[2], device="cuda")
        be = torch.zeros(N, R, emo.shape[2], device="cuda")
        for s in range(N):
            n = counts[s]
            bm[s, :n] = mel[s, used[s]:used[s] + n]
            be[s, :n] = emo[s, used[s]:used[s] + n]
        cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
        res = (eng.replay if replay else eng.step)(bm, be, cnt)
        assert res["rendered"].tolist() == list(counts)
        taken.append((list(counts), res["blendshapes"].clone(), res["raw_blendshapes"].clone()))
        for s in range(N):
            used[s] += counts[s]
    # second pass: every step's rows go to the life they belong to
    life_of = [0] * N
    for (counts, mask), (_, out, raw) in zip(steps, taken):
        if mask is not None:
            for s in range(N):
                if mask[s]:
                    life_of[s] += 1
        for s in range(N):
            n = counts[s]
            if n:
                life = lives[s][life_of[s]]
                life[1] += n
                life[2].append(out[s, :n])
                life[3].append(raw[s, :n])
    return lives


def loop_life(ref, mel, emo, s, life, T, smoothing, constraints):
    """The per-stream loop on a life's rows: (out (rows, 52), raw, final smoother state (1, .) or None)."""
    first, rows = life[0], life[1]
    ref.reset_temporal_state()
    out, raw = rc.forward_loop(ref, mel[s:s + 1, first:first + rows].contiguous(), emo[s:s + 1, first:first + rows].contiguous(), T,
                               apply_smoothing=smoothing, apply_constraints=constraints)
    st = None if ref._smoother_state is None else ref._smoother_state.clone()
    ref.reset_temporal_state()
    return out[0], raw[0], st


@pytest.mark.parametrize("constraints", [True, False], ids=["constraints", "free"])
@pytest.mark.parametrize("smoothing", ["off", "exponential", "gaussian", "median"])
@pytest.mark.parametrize("emotion_dim", [256, 32])
@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("T", [1, 3, 9, 17, 30, 32])
def test_streams_equal_the_per_stream_forward_loop_bit_for_bit(T, R, emotion_dim, smoothing, constraints):
    """Four streams over the schedule of koemorph_stream_cases.schedule (2 T + 3 steps: every ring wraps; a late joiner, a stream
    whose count walks 0 .. R, a reset mid-way): out, raw and the final smoother state of every stream against the loop."""
    m, ref, cfg, _ = models(emotion_dim, smoothing)
    steps = sc.schedule(T, R)
    if T >= 17:
        assert sc.mixed_steps(T, R), "the schedule must hold a step with T_i <= 16, T_i > 16 and a count of 0: the schedule is wrong"
    F = (2 * T + 3) * R
    mel, emo = (dev(a) for a in rc.rows(2000 + 31 * T + R, 4, F, cfg))
    eng = KoeMorphStreams(m, 4, context_frames=T, max_rows=R, apply_smoothing=smoothing != "off", apply_constraints=constraints)
    try:
        assert eng.plan["launches"] == 4 and eng.plan["ring_rows"] == T - 1 + R
        lives = walk(eng, steps, mel, emo)
        state = eng.smoother_state()
        frames = eng.frames().tolist()
        for s in range(4):
            assert frames[s] == lives[s][-1][1], (s, frames)
            for k, life in enumerate(lives[s]):
                if life[1] == 0:
                    continue
                want_out, want_raw, want_state = loop_life(ref, mel, emo, s, life, T, smoothing != "off", constraints)
                tag = f"T {T} R {R} e{emotion_dim} {smoothing} stream {s} life {k}"
                got_out, got_raw = torch.cat(life[2]), torch.cat(life[3])
                same_bits(got_out, want_out, tag + " out")
                same_bits(got_raw, want_raw, tag + " raw")
                assert bool(torch.isfinite(got_out).all())
                if k == len(lives[s]) - 1 and smoothing != "off":
                    same_bits(state[s:s + 1], want_state, tag + " state")
        assert len(lives[3]) == 2 and lives[3][0][1] == T * R                 # the reset cut stream 3 where the schedule says
        assert state is None if smoothing == "off" else state is not None
    finally:
        eng.close()


@pytest.mark.parametrize("N,T,R", [(3, 30, 1), (2, 9, 4)])
def test_streams_against_the_float64_oracle(N, T, R):
    """Out-of-phase streams (stream s joins at step s) against a loop of oracle.koemorph_forward per stream, carrying prev and the
    smoother state; every frame finite, the warm-up frames included."""
    m, _, cfg, params = models()
    n_steps = 40 if R == 1 else 6
    steps = [([R if k >= s else 0 for s in range(N)], None) for k in range(n_steps)]
    F = n_steps * R
    mel, emo = rc.rows(51 + T, N, F, cfg)
    eng = KoeMorphStreams(m, N, context_frames=T, max_rows=R)
    try:
        lives = walk(eng, steps, dev(mel), dev(emo))
        state = eng.smoother_state().cpu().numpy()
    finally:
        eng.close()
    worst = 0.0
    for s in range(N):
        rows = lives[s][0][1]
        assert rows == (n_steps - s) * R
        want_out, want_raw, want_state = rc.oracle_loop(params, cfg, mel[s:s + 1, :rows], emo[s:s + 1, :rows], T)
        out, raw = torch.cat(lives[s][0][2]).cpu().numpy(), torch.cat(lives[s][0][3]).cpu().numpy()
        assert np.isfinite(out).all() and np.isfinite(raw).all()
        worst = max(worst, float(np.abs(out - want_out[0]).max()), float(np.abs(raw - want_raw[0]).max()),
                    float(np.abs(state[s:s + 1] - np.asarray(want_state)).max()))
    print(f"streams {(N, T, R)} against the oracle: worst |difference| {worst:.3g}")
    assert worst <= TOL


@pytest.mark.parametrize("R", [1, 4])
def test_in_phase_streams_equal_rollout_bit_for_bit(R):
    """Three streams in phase over 40 frames at T = 30: the engine's frames are ``rollout``'s, which ties the two serving paths."""
    m, ref, cfg, _ = models()
    N, F, T = 3, 40, 30
    mel, emo = (dev(a) for a in rc.rows(77, N, F, cfg))
    ref.reset_temporal_state()
    with torch.no_grad():
        want = ref.rollout(mel, emo, context_frames=T)
    want_state = ref._smoother_state.clone()
    ref.reset_temporal_state()
    eng = KoeMorphStreams(m, N, context_frames=T, max_rows=R)
    try:
        lives = walk(eng, [([R] * N, None)] * (F // R), mel, emo)
        for s in range(N):
            same_bits(torch.cat(lives[s][0][2]), want["blendshapes"][s], f"stream {s} out")
            same_bits(torch.cat(lives[s][0][3]), want["raw_blendshapes"][s], f"stream {s} raw")
        same_bits(eng.smoother_state(), want_state, "state")
    finally:
        eng.close()


def test_captured_step_replays_on_other_rows_counts_and_phases():
    """A step captured while the streams stand at one phase, replayed over a schedule with other rows, counts, a reset and a late
    joiner: the bits of a twin engine that runs the same schedule eagerly.  Creating an engine inside a capture is refused."""
    m, ref, cfg, _ = models(256, "median")
    N, T, R = 4, 9, 2
    steps = sc.schedule(T, R)
    F = (2 * T + 3) * R
    mel, emo = (dev(a) for a in rc.rows(90, N, F, cfg))
    a, b = KoeMorphStreams(m, N, context_frames=T, max_rows=R), KoeMorphStreams(ref, N, context_frames=T, max_rows=R)
    try:
        a.step(mel[:, :R].contiguous(), emo[:, :R].contiguous())             # the captured phase: every stream at frame R
        a.capture()
        x = torch.zeros(8, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            with pytest.raises(_lib.KoeMorphError, match="km_koemorph_stream_create.*stream capture") as ei:
                KoeMorphStreams(ref, N, context_frames=T, max_rows=R)
            assert ei.value.code == _lib.KM_ERR_WORKSPACE
            x.add_(1.0)
        torch.cuda.current_stream().wait_stream(side)
        a.reset()
        got = walk(a, steps, mel, emo, replay=True)
        want = walk(b, steps, mel, emo)
        for s in range(N):
            assert len(got[s]) == len(want[s])
            for lg, lw in zip(got[s], want[s]):
                assert lg[:2] == lw[:2]
                if lg[1]:
                    same_bits(torch.cat(lg[2]), torch.cat(lw[2]), f"replay stream {s} out")
                    same_bits(torch.cat(lg[3]), torch.cat(lw[3]), f"replay stream {s} raw")
        same_bits(a.smoother_state(), b.smoother_state(), "replay state")
        assert a.frames().tolist() == b.frames().tolist()
        # a replay that brings fewer rows than were captured, without counts: one row per stream
        ra = {k: v.clone() for k, v in a.replay(mel[:, 0], emo[:, 0]).items()}
        rb = b.step(mel[:, 0], emo[:, 0])
        assert ra["rendered"].tolist() == rb["rendered"].tolist() == [1] * N
        same_bits(ra["blendshapes"][:, :1], rb["blendshapes"][:, :1], "one-row replay")
    finally:
        a.close()
        b.close()


def test_guard_regions_unwritten_rows_and_paused_streams():
    """km_koemorph_stream_step on padded buffers: the floats around out / raw / rendered, rows j >= n_s and every row of a paused
    stream keep their pattern; counts are clamped to 0 .. max_rows; misaligned rows are refused."""
    m, ref, cfg, _ = models(32, "exponential")
    N, T, R, G = 4, 9, 3, 64
    mel, emo = (dev(a) for a in rc.rows(95, N, 2 * R, cfg))
    a, b = KoeMorphStreams(m, N, context_frames=T, max_rows=R), KoeMorphStreams(ref, N, context_frames=T, max_rows=R)
    try:
        lib, h = a._lib, a._h
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for turn, counts in enumerate(([R, 0, 1, 2], [7, 2, 0, -5])):
            n = [max(0, min(c, R)) for c in counts]
            bm, be = mel[:, turn * R:(turn + 1) * R].contiguous(), emo[:, turn * R:(turn + 1) * R].contiguous()
            cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
            outs = [torch.full((G + N * R * 52 + G,), -7.0, device="cuda") for _ in range(2)]
            rend = torch.full((G + N + G,), -7, dtype=torch.int32, device="cuda")
            _lib.check(lib.km_koemorph_stream_step(h, C.c_void_p(bm.data_ptr()), C.c_void_p(be.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                   C.c_void_p(outs[0].data_ptr() + 4 * G), C.c_void_p(outs[1].data_ptr() + 4 * G),
                                                   C.c_void_p(rend.data_ptr() + 4 * G), st))
            want = b.step(bm, be, cnt.clamp(0, R))
            torch.cuda.synchronize()
            assert bool((rend[:G] == -7).all()) and bool((rend[G + N:] == -7).all()) and rend[G:G + N].tolist() == n
            for t, k in zip(outs, ("blendshapes", "raw_blendshapes")):
                assert bool((t[:G] == -7.0).all()) and bool((t[G + N * R * 52:] == -7.0).all()), k
                body = t[G:G + N * R * 52].view(N, R, 52)
                for s in range(N):
                    assert bool((body[s, n[s]:] == -7.0).all()), (k, s)
                    same_bits(body[s, :n[s]], want[k][s, :n[s]], f"{k} stream {s}")
        flat = torch.zeros(N * R * 80 + 4, device="cuda")
        rcode = lib.km_koemorph_stream_step(h, C.c_void_p(flat.data_ptr() + 4), C.c_void_p(be.data_ptr()), None,
                                            C.c_void_p(outs[0].data_ptr()), None, None, st)
        assert rcode == _lib.KM_ERR_INVALID_ARG and b"km_koemorph_stream_step: mel_dev" in lib.km_last_error()
        assert b"not 16-byte aligned" in lib.km_last_error()
    finally:
        a.close()
        b.close()


def test_reset_reproduces_frames_count_and_the_model_state_is_untouched():
    m, _, cfg, _ = models(256, "gaussian")
    N, T, R = 4, 9, 4
    steps = sc.schedule(T, R)
    mel, emo = (dev(a) for a in rc.rows(97, N, (2 * T + 3) * R, cfg))
    sentinel = dev(synth.uniform(3, (1, 5 * 52 + 1), 0, 1))
    m._smoother_state = sentinel
    keep = sentinel.clone()
    eng = KoeMorphStreams(m, N, context_frames=T, max_rows=R)
    try:
        first = walk(eng, steps, mel, emo)
        state1, frames1 = eng.smoother_state(), eng.frames().tolist()
        c = [0] * N
        for counts, mask in steps:
            c = [0 if mask and mask[s] else c[s] for s in range(N)]
            c = [v + n for v, n in zip(c, counts)]
        assert frames1 == c
        eng.reset()
        assert eng.frames().tolist() == [0] * N and not bool(eng.smoother_state().any())
        second = walk(eng, steps, mel, emo)
        for s in range(N):
            for l1, l2 in zip(first[s], second[s]):
                if l1[1]:
                    same_bits(torch.cat(l2[2]), torch.cat(l1[2]), f"stream {s} after reset")
        same_bits(eng.smoother_state(), state1, "state after reset")
        assert m._smoother_state is sentinel
        same_bits(m._smoother_state, keep, "the model's own smoother state")
    finally:
        eng.close()
        m.reset_temporal_state()


def test_changed_weights_are_picked_up_and_the_streams_keep_their_state():
    """A parameter changed in place between two steps: the next step runs the new weights, and rows, counter, previous frame and
    smoother state of every stream carry over -- the loop with the same change at the same frame gives the same bits."""
    cfg = okm.KoeMorphConfig(emotion_dim=32)
    params = okm.make_koemorph_params(23, cfg)
    m, ref = rc.build(cfg, params), rc.build(cfg, params)
    N, T = 2, 5
    mel, emo = (dev(a) for a in rc.rows(99, N, 8, cfg))
    old = ref.decoder.output_proj.bias.detach().clone()
    new = old + 0.25
    eng = KoeMorphStreams(m, N, context_frames=T)
    try:
        outs = [eng.step(mel[:, i], emo[:, i])["blendshapes"][:, 0].clone() for i in range(4)]
        with torch.no_grad():
            m.decoder.output_proj.bias.copy_(new)
        outs += [eng.step(mel[:, i], emo[:, i])["blendshapes"][:, 0].clone() for i in range(4, 8)]
        assert eng.frames().tolist() == [8, 8]
        for s in range(N):
            ref.reset_temporal_state()
            prev = None
            for i in range(8):
                with torch.no_grad():
                    ref.decoder.output_proj.bias.copy_(old if i < 4 else new)
                    lo = max(0, i - T + 1)
                    prev = ref(mel[s:s + 1, lo:i + 1].contiguous(), emo[s:s + 1, lo:i + 1].contiguous(), prev_blendshapes=prev)["blendshapes"]
                same_bits(outs[i][s:s + 1], prev, f"stream {s} frame {i}")
        assert not bool(torch.equal(outs[3], outs[4]))
    finally:
        eng.close()


def test_memory_returns_to_its_baseline():
    lib = _lib.load()
    cfg = okm.KoeMorphConfig(emotion_dim=32)
    m = rc.build(cfg, okm.make_koemorph_params(19, cfg))
    m._handle()
    gc.collect()
    torch.cuda.synchronize()
    base = lib.km_live_device_bytes()
    eng = KoeMorphStreams(m, 3, context_frames=9, max_rows=2)
    want = 4 * eng.plan["device_floats"]
    assert want == 4 * sc.expected_plan(cfg, 3, 9, 2)["device_floats"]
    assert lib.km_live_device_bytes() == base + want
    second = KoeMorphStreams(m, 3, context_frames=9, max_rows=2)             # replaces the first
    assert lib.km_live_device_bytes() == base + want
    with pytest.raises(RuntimeError, match="replaced"):
        eng.step(torch.zeros(3, 80, device="cuda"), torch.zeros(3, 32, device="cuda"))
    eng.close()                                                              # a replaced engine frees nothing
    assert lib.km_live_device_bytes() == base + want
    second.step(torch.zeros(3, 80, device="cuda"), torch.zeros(3, 32, device="cuda"))
    second.close()
    assert lib.km_live_device_bytes() == base
    with pytest.raises(RuntimeError, match="closed"):
        second.frames()
    del m
    gc.collect()
