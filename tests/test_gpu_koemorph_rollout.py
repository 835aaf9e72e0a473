"""KoeMorphModel.rollout / render (km_koemorph_rollout) on the device.

The main pin is EQUAL BITS with the loop a rollout replaces: ``KoeMorphModel.forward`` per frame on the sliced window with the output
fed back.  That can hold because the rollout kernel runs the decode kernel's statements (one shared ``decode_window``) and the
encoder's rows are independent of the other windows of a launch; ``test_forward_does_not_depend_on_the_batch`` checks the second
premise on ``forward`` alone (it passes without the rollout).  Then the float64-backed oracle, route 0, continuation, capture and
replay, guards and memory, and ``render``."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import rollout_cases as rc
from koemorph_amd import _lib, synth
from oracle import koemorph_model as okm

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_gpu_koemorph.py: this project's tolerance on the 52 coefficients

_models = {}


def model(emotion_dim=256, smoothing="exponential", **kw):
    """One model per configuration for the whole module (parameters are uploaded once)."""
    key = (emotion_dim, smoothing, tuple(sorted(kw.items())))
    if key not in _models:
        cfg = okm.KoeMorphConfig(emotion_dim=emotion_dim, smoothing_method="exponential" if smoothing == "off" else smoothing, **kw)
        params = okm.make_koemorph_params(17, cfg)
        _models[key] = (rc.build(cfg, params), cfg, params)
    return _models[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, float(np.nanmax(np.abs(a - b))))


def both(m, mel, emo, T, first=0, prev0=None, smoothing=True, constraints=True, chunk=None, state0=None):
    """(loop out, raw, state), (rollout out, raw, state) from the same starting state."""
    res = []
    for roll in (False, True):
        m._smoother_state = None if state0 is None else state0.clone()
        if roll:
            with torch.no_grad():
                o = m.rollout(mel, emo, context_frames=T, first_frame=first, prev_blendshapes=prev0, apply_smoothing=smoothing,
                              apply_constraints=constraints, chunk_frames=chunk)
            out, raw = o["blendshapes"], o["raw_blendshapes"]
        else:
            out, raw = rc.forward_loop(m, mel, emo, T, first, prev0, smoothing, constraints)
        st = None if m._smoother_state is None else m._smoother_state.clone()
        res.append((out, raw, st))
    m.reset_temporal_state()
    return res


def assert_equal_runs(loop, roll, tag):
    same_bits(roll[0], loop[0], tag + " out")
    same_bits(roll[1], loop[1], tag + " raw")
    assert (loop[2] is None) == (roll[2] is None), tag
    if loop[2] is not None:
        same_bits(roll[2], loop[2], tag + " state")


@pytest.mark.parametrize("T", [3, 9, 17, 30])
def test_forward_does_not_depend_on_the_batch(T):
    """The premise of the equal-bits pin, on forward alone: N windows at B = N give the bits of N forwards at B = 1 (the encoder
    packs several short windows into one row tile; a window's rows must not see the others)."""
    m, cfg, _ = model()
    N = 5
    mel, emo = (dev(a) for a in rc.rows(300 + T, N, T, cfg))
    prev = dev(synth.uniform(9, (N, 52), 0, 1))
    with torch.no_grad():
        whole = m(mel, emo, prev_blendshapes=prev, apply_smoothing=False)
        for b in range(N):
            one = m(mel[b:b + 1].contiguous(), emo[b:b + 1].contiguous(), prev_blendshapes=prev[b:b + 1].contiguous(), apply_smoothing=False)
            same_bits(one["blendshapes"], whole["blendshapes"][b:b + 1], f"T {T} window {b}")
            same_bits(one["raw_blendshapes"], whole["raw_blendshapes"][b:b + 1], f"T {T} window {b} raw")


SHAPES = [(1, 40, 30), (3, 11, 3), (2, 20, 9), (2, 40, 17), (1, 70, 32), (5, 6, 1)]


@pytest.mark.parametrize("smoothing", ["off", "exponential", "gaussian", "median"])
@pytest.mark.parametrize("emotion_dim", [256, 32])
@pytest.mark.parametrize("B,F,T", SHAPES, ids=lambda v: str(v))
def test_rollout_equals_the_forward_loop_bit_for_bit(B, F, T, emotion_dim, smoothing):
    """Route 1 at the default width: chunk boundaries inside the clip (4) and the whole clip in one chunk (256), prev0 given and
    None, constraints on and off; out, raw and the final smoother state.  The 5-slot ring of gaussian / median wraps at least twice
    wherever F >= 12."""
    m, cfg, _ = model(emotion_dim, smoothing)
    assert m.rollout_plan(B, F, T)["route"] == 1
    mel, emo = (dev(a) for a in rc.rows(1000 + 7 * F + T, B, F, cfg))
    prev0 = dev(synth.uniform(5, (B, 52), 0, 1))
    for given in (True, False):
        for constraints in (True, False):
            loop = None
            for chunk in (4, 256):
                l, r = both(m, mel, emo, T, prev0=prev0 if given else None, smoothing=smoothing != "off", constraints=constraints, chunk=chunk)
                loop = loop or l
                assert_equal_runs(loop, r, f"{(B, F, T)} e{emotion_dim} {smoothing} prev0 {given} constraints {constraints} chunk {chunk}")
                assert bool(torch.isfinite(r[0]).all()) and bool(torch.isfinite(r[1]).all())


def test_rollout_against_the_float64_oracle_route_1():
    """(3, 40, 30) at the default width against a loop of oracle.koemorph_forward carrying prev and the smoother state.  Every frame
    finite, the T - 1 warm-up frames included: a left-padded window would leave query 0 without a key (NaN)."""
    m, cfg, params = model()
    B, F, T = 3, 40, 30
    mel, emo = rc.rows(41, B, F, cfg)
    want_out, want_raw, want_state = rc.oracle_loop(params, cfg, mel, emo, T)
    m.reset_temporal_state()
    with torch.no_grad():
        got = m.rollout(dev(mel), dev(emo), context_frames=T)
    out, raw, st = got["blendshapes"].cpu().numpy(), got["raw_blendshapes"].cpu().numpy(), m._smoother_state.cpu().numpy()
    m.reset_temporal_state()
    worst = max(float(np.abs(out - want_out).max()), float(np.abs(raw - want_raw).max()), float(np.abs(st - np.asarray(want_state)).max()))
    print(f"rollout route 1 against the oracle: worst |difference| {worst:.3g}")
    assert np.isfinite(out).all() and np.isfinite(raw).all()
    assert worst <= TOL


def test_rollout_against_the_float64_oracle_route_0():
    """(2, 12, 5) at d_model 64 / 4 heads / decoder 32 / emotion_dim 24: the launch-per-step chain per frame, inside the library."""
    m, cfg, params = model(24, "exponential", **{k: v for k, v in rc.SMALL.items() if k != "emotion_dim"})
    B, F, T = 2, 12, 5
    assert m.rollout_plan(B, F, T)["route"] == 0
    mel, emo = rc.rows(43, B, F, cfg)
    want_out, want_raw, want_state = rc.oracle_loop(params, cfg, mel, emo, T)
    m.reset_temporal_state()
    with torch.no_grad():
        got = m.rollout(dev(mel), dev(emo), context_frames=T)
    out, raw, st = got["blendshapes"].cpu().numpy(), got["raw_blendshapes"].cpu().numpy(), m._smoother_state.cpu().numpy()
    m.reset_temporal_state()
    worst = max(float(np.abs(out - want_out).max()), float(np.abs(raw - want_raw).max()), float(np.abs(st - np.asarray(want_state)).max()))
    print(f"rollout route 0 against the oracle: worst |difference| {worst:.3g}")
    assert np.isfinite(out).all() and np.isfinite(raw).all()
    assert worst <= TOL


@pytest.mark.parametrize("case", ["d64", "emotion25", "T40", "no_fuse"])
def test_route_0_equals_the_forward_loop_bit_for_bit(case):
    if case == "d64":
        m, cfg, _ = model(24, "gaussian", **{k: v for k, v in rc.SMALL.items() if k != "emotion_dim"})
        B, F, T = 2, 14, 5
    elif case == "emotion25":
        m, cfg, _ = model(25, "exponential")
        B, F, T = 2, 8, 5
    elif case == "T40":
        m, cfg, _ = model(256, "exponential")
        B, F, T = 2, 44, 40
    else:
        m, cfg, _ = model(256, "median")
        B, F, T = 3, 14, 9
    mel, emo = (dev(a) for a in rc.rows(77, B, F, cfg))
    prev0 = dev(synth.uniform(6, (B, 52), 0, 1))
    lib, h, _ = m._handle()
    if case == "no_fuse":
        _lib.check(lib.km_set_option(h, b"kmm_no_fuse", 1))
    try:
        assert m.rollout_plan(B, F, T)["route"] == 0
        for given in (True, False):
            l, r = both(m, mel, emo, T, prev0=prev0 if given else None)
            assert_equal_runs(l, r, f"{case} prev0 {given}")
    finally:
        if case == "no_fuse":
            _lib.check(lib.km_set_option(h, b"kmm_no_fuse", 0))
    if case == "no_fuse":
        assert m.rollout_plan(B, F, T)["route"] == 1


def test_misaligned_rows_take_route_0_with_the_same_bits():
    m, cfg, _ = model(32, "exponential")
    B, F, T = 2, 12, 5
    mel, emo = (dev(a) for a in rc.rows(79, B, F, cfg))
    lib, h, d = m._handle()
    with torch.no_grad():
        want = m.rollout(mel, emo, context_frames=T, apply_smoothing=False)
    flat = torch.empty(mel.numel() + 1, device="cuda")
    flat[1:] = mel.reshape(-1)                          # the same rows, 4 bytes off a 16-byte boundary
    out = torch.empty(B, F, 52, device="cuda")
    _lib.check(lib.km_koemorph_rollout(h, C.c_void_p(flat.data_ptr() + 4), C.c_void_p(emo.data_ptr()), B, F, T, 0, None, None, 1,
                                       C.c_void_p(out.data_ptr()), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    same_bits(out, want["blendshapes"], "misaligned mel rows")


@pytest.mark.parametrize("T", [9, 30])
def test_two_calls_continue_as_one(T):
    """Frames 0 .. 24, then 25 .. 49 from the last T - 1 rendered rows as context (first_frame = T - 1; at T = 30 only 25 rows exist
    before the cut, so all of them and first_frame = 25: the second call starts inside the warm-up) with prev0 and the state
    carried, equal one call of 50 frames bit for bit; and first_frame = 3 < T - 1 equals frames 3 .. of the full call's law."""
    m, cfg, _ = model(256, "gaussian")
    B, F, cut = 2, 50, 25
    mel, emo = (dev(a) for a in rc.rows(90 + T, B, F, cfg))
    m.reset_temporal_state()
    with torch.no_grad():
        whole = m.rollout(mel, emo, context_frames=T, chunk_frames=8)
        state_whole = m._smoother_state.clone()
        m.reset_temporal_state()
        a = m.rollout(mel[:, :cut].contiguous(), emo[:, :cut].contiguous(), context_frames=T, chunk_frames=8)
        lo = max(cut - (T - 1), 0)
        b = m.rollout(mel[:, lo:].contiguous(), emo[:, lo:].contiguous(), context_frames=T, first_frame=cut - lo,
                      prev_blendshapes=a["blendshapes"][:, -1].contiguous(), chunk_frames=8)
        state_two = m._smoother_state.clone()
    for k in ("blendshapes", "raw_blendshapes"):
        same_bits(torch.cat([a[k], b[k]], 1), whole[k], f"T {T} {k}")
    same_bits(state_two, state_whole, "state")
    # first_frame = 3 inside the warm-up: the law's frames 3 .. with prev0 and a fresh state, against the loop
    prev0 = dev(synth.uniform(8, (B, 52), 0, 1))
    l, r = both(m, mel[:, :20].contiguous(), emo[:, :20].contiguous(), T, first=3, prev0=prev0, chunk=8)
    assert r[0].shape == (B, 17, 52)
    assert_equal_runs(l, r, f"T {T} first_frame 3")


def test_captured_call_replays_on_other_rows():
    m, cfg, _ = model(256, "median")
    B, F, T = 2, 40, 9
    nb = 52
    mel, emo = (dev(a) for a in rc.rows(120, B, F, cfg))
    mel2, emo2 = (dev(a) for a in rc.rows(130, B, F, cfg))
    prev_a, prev_b = dev(synth.uniform(10, (B, nb), 0, 1)), dev(synth.uniform(11, (B, nb), 0, 1))
    state_b = dev(synth.uniform(12, (B, 5 * nb + 1), 0, 1))
    state_b[:, -1] = 3.0
    with torch.no_grad():
        m.reset_temporal_state()
        m.rollout(mel, emo, context_frames=T, prev_blendshapes=prev_a, chunk_frames=16)           # reserves and fills the buffers
        s_mel, s_emo, s_prev = mel.clone(), emo.clone(), prev_a.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        m.reset_temporal_state()
        m._ensure_smoother_state(B, mel.device)
        state = m._smoother_state
        with torch.cuda.graph(g, stream=side):
            cap = m.rollout(s_mel, s_emo, context_frames=T, prev_blendshapes=s_prev, chunk_frames=16)
        s_mel.copy_(mel2); s_emo.copy_(emo2); s_prev.copy_(prev_b); state.copy_(state_b)
        g.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in cap.items()}
        got_state = state.clone()
        m._smoother_state = state_b.clone()
        want = m.rollout(mel2, emo2, context_frames=T, prev_blendshapes=prev_b, chunk_frames=16)
        for k in want:
            same_bits(got[k], want[k], "replay " + k)
        same_bits(got_state, m._smoother_state, "replay state")
        m.reset_temporal_state()


def test_reserve_growth_inside_a_capture_is_refused():
    m, cfg, _ = model(32, "off")
    B, F, T = 2, 12, 5
    mel, emo = (dev(a) for a in rc.rows(140, B, F, cfg))
    big_mel, big_emo = (dev(a) for a in rc.rows(141, B + 9, F, cfg))
    with torch.no_grad():
        m.rollout(mel, emo, context_frames=T, apply_smoothing=False)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(_lib.KoeMorphError, match="km_koemorph_rollout_reserve.*stream capture") as ei:
                m.rollout(big_mel, big_emo, context_frames=T, apply_smoothing=False)
            assert ei.value.code == _lib.KM_ERR_WORKSPACE
            cap = m.rollout(mel, emo, context_frames=T, apply_smoothing=False)        # the reserved size still captures
        g.replay()
        torch.cuda.synchronize()
        same_bits(cap["blendshapes"], m.rollout(mel, emo, context_frames=T, apply_smoothing=False)["blendshapes"], "after the refusal")


def test_not_reserved_and_reserved_smaller_are_refused():
    cfg2 = okm.KoeMorphConfig(**rc.SMALL)
    fresh = rc.build(cfg2, okm.make_koemorph_params(3, cfg2))
    lib, h, _ = fresh._handle()
    mel, emo = (dev(a) for a in rc.rows(150, 3, 12, cfg2))
    out = torch.empty(3, 12, 52, device="cuda")
    call = lambda B, T: lib.km_koemorph_rollout(h, C.c_void_p(mel.data_ptr()), C.c_void_p(emo.data_ptr()), B, 12, T, 0, None, None, 1,
                                                C.c_void_p(out.data_ptr()), None, None)
    assert call(2, 5) == _lib.KM_ERR_WORKSPACE and b"km_koemorph_rollout: no workspace" in lib.km_last_error()
    _lib.check(lib.km_koemorph_rollout_reserve(h, 2, 5, 4))
    assert call(3, 5) == _lib.KM_ERR_WORKSPACE and b"3 clips x 5 context frames, reserved 2 x 5" in lib.km_last_error()
    assert call(2, 6) == _lib.KM_ERR_WORKSPACE and b"2 clips x 6 context frames, reserved 2 x 5" in lib.km_last_error()
    assert call(2, 5) == _lib.KM_OK
    torch.cuda.synchronize()
    del fresh


def test_guards_rows_beyond_the_call_and_memory():
    lib = _lib.load()
    cfg = okm.KoeMorphConfig(emotion_dim=32)
    for case in ("route1", "route0"):
        gc.collect()
        torch.cuda.synchronize()
        base = lib.km_live_device_bytes()
        m = rc.build(cfg, okm.make_koemorph_params(19, cfg))
        B, F, T, first = 3, 21, 9 if case == "route1" else 40, 2
        mel, emo = (dev(a) for a in rc.rows(160, B, F, cfg))
        _, h, _ = m._handle()
        with torch.no_grad():
            want = m.rollout(mel, emo, context_frames=T, first_frame=first, apply_smoothing=False, chunk_frames=5)
        rows = F - first
        G = 64                                           # guard floats on either side, and one row beyond the call's rows
        bufs = []
        for _ in range(2):
            t = torch.full((G + B * rows * 52 + 52 + G,), -7.0, device="cuda")
            bufs.append(t)
        _lib.check(lib.km_koemorph_rollout(h, C.c_void_p(mel.data_ptr()), C.c_void_p(emo.data_ptr()), B, F, T, first, None, None, 1,
                                           C.c_void_p(bufs[0].data_ptr() + 4 * G), C.c_void_p(bufs[1].data_ptr() + 4 * G),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        for t, k in zip(bufs, ("blendshapes", "raw_blendshapes")):
            assert bool((t[:G] == -7.0).all()) and bool((t[G + B * rows * 52:] == -7.0).all()), (case, k)
            same_bits(t[G:G + B * rows * 52].view(B, rows, 52), want[k], f"{case} {k}")
        assert m.rollout_plan(B, F, T, first)["route"] == (1 if case == "route1" else 0)
        assert lib.km_live_device_bytes() > base
        del m, h
        gc.collect()
        torch.cuda.synchronize()
        assert lib.km_live_device_bytes() == base, case


@pytest.mark.parametrize("emotion_dim,route", [(32, 1), (25, 0)])
def test_render_equals_rollout_on_the_extracted_rows(emotion_dim, route):
    import egemaps_cases
    from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine
    from koemorph_amd.features.stft import MelSpectrogramExtractor
    m, cfg, _ = model(emotion_dim, "exponential")
    x = dev(egemaps_cases.speechlike(5, 1.2)[None, :])
    with torch.no_grad():
        mel = MelSpectrogramExtractor(target_fps=30)(x)
        lld = EGeMAPSEngine("cuda").llds(x, fps=30)
        assert mel.shape[1] == lld.shape[1] == 36 and lld.shape[2] == 25
        emo = torch.nn.functional.pad(lld, (0, emotion_dim - 25))
        assert m.rollout_plan(1, 36, None)["route"] == route
        m.reset_temporal_state()
        want = m.rollout(mel, emo)
        m.reset_temporal_state()
        got = m.render(x)
        m.reset_temporal_state()
    assert got["blendshapes"].shape == (1, 36, 52) and bool(torch.isfinite(got["blendshapes"]).all())
    for k in want:
        same_bits(got[k], want[k], f"render {k}")
