"""km_koemorph_stream_* on the host alone: the stream window law (table entries and ring positions) against a brute force that walks
per-stream row lists over a schedule with pauses and resets, km_koemorph_stream_plan against the restatement in
tests/koemorph_stream_cases.py, every refusal that needs no device with its text, and the shape errors of KoeMorphStreams.step."""
import ctypes as C

import pytest
import torch

import koemorph_stream_cases as sc
import rollout_cases as rc
from koemorph_amd import _lib
from koemorph_amd.streaming import KoeMorphStreams
from oracle import koemorph_model as okm


@pytest.mark.parametrize("T,R", [(1, 1), (1, 4), (3, 1), (9, 4), (17, 1), (30, 4), (32, 8)])
def test_window_law_equals_brute_force(T, R):
    """The table entries (frame slot, T_i, first ring position) read from a ring of T - 1 + R rows give exactly the rows the law
    names, over the GPU tests' schedule (late joiner, pauses, a reset mid-way, every ring wrapping)."""
    N, cap = 4, T - 1 + R
    brute = sc.BruteStreams(N, T, R)
    c = [0] * N
    next_id = [0] * N
    for counts, mask in sc.schedule(T, R):
        if mask:
            brute.reset(mask)
            c = [0 if m else v for v, m in zip(c, mask)]
        ids = [[(s, next_id[s] + j) for j in range(R)] for s in range(N)]
        frames = brute.step(counts, ids)
        for s in range(N):
            law = sc.step_windows(c[s], counts[s], T, cap)
            assert len(law) == len(frames[s]) == counts[s]
            for (j, ti, pos0), (jb, want, got) in zip(law, frames[s]):
                assert j == jb and ti == len(want) == min(c[s] + j + 1, T) and 0 <= pos0 < cap
                assert got == want, (T, R, s, j)                       # the ring holds the law's rows at the table's positions
                assert want[-1] == ids[s][j]                            # the window ends on its own row
            next_id[s] += counts[s]
            c[s] += counts[s]
    assert c[0] == (2 * T + 3) * R and c[0] > cap                      # the ring wrapped
    if T >= 17:
        assert sc.mixed_steps(T, R), "the schedule must mix short windows, long windows and a pause in one step"


CONFIGS = {
    "default": okm.KoeMorphConfig(),
    "emotion32": okm.KoeMorphConfig(emotion_dim=32),
    "gaussian": okm.KoeMorphConfig(smoothing_method="gaussian"),
    "no_smoothing": okm.KoeMorphConfig(use_temporal_smoothing=False),
    "emotion25": okm.KoeMorphConfig(emotion_dim=25),
    "d64": okm.KoeMorphConfig(**rc.SMALL),
}


def plan(h, N, T, R):
    out = (C.c_int64 * 6)()
    _lib.check(h.lib.km_koemorph_stream_plan(h.h, N, T, R, out))
    return dict(zip(("supported", "ring_rows", "launches", "device_floats", "chain_lds_bytes", "state_floats"), (int(v) for v in out)))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_plan_equals_the_restatement(name):
    cfg = CONFIGS[name]
    h = rc.HostHandle(cfg)
    try:
        for no_fuse in (0, 1):
            h.set_option("kmm_no_fuse", no_fuse)
            for N, T, R in ((1, 1, 1), (4, 9, 1), (4, 30, 4), (3, 32, 8), (2, 33, 1)):
                assert plan(h, N, T, R) == sc.expected_plan(cfg, N, T, R, no_fuse=bool(no_fuse)), (name, no_fuse, N, T, R)
        h.set_option("kmm_no_fuse", 0)
        assert plan(h, 4, 30, 4)["supported"] == (1 if name in ("default", "emotion32", "gaussian", "no_smoothing") else 0)
    finally:
        h.close()
    assert sc.expected_plan(okm.KoeMorphConfig(), 4, 30, 4)["ring_rows"] == 33
    assert sc.expected_plan(okm.KoeMorphConfig(), 4, 30, 4)["launches"] == 4


def _refused(lib, rcode, code, *needles):
    assert rcode == code, (rcode, lib.km_last_error())
    text = lib.km_last_error().decode()
    for n in needles:
        assert n in text, text


def test_unsupported_shapes_are_refused_at_creation_without_a_device():
    """km_koemorph_stream_create judges the shape before it needs the device: KM_ERR_UNSUPPORTED with the entry point and the value."""
    uns, who = _lib.KM_ERR_UNSUPPORTED, "km_koemorph_stream_create"
    for cfg, T, option, needles in (
            (okm.KoeMorphConfig(**rc.SMALL), 5, 0, ("d_model 64",)),
            (okm.KoeMorphConfig(emotion_dim=25), 5, 0, ("emotion_dim 25", "multiple of 16")),
            (okm.KoeMorphConfig(), 33, 0, ("context_frames 33", "at most 32")),
            (okm.KoeMorphConfig(), 30, 1, ("kmm_no_fuse",))):
        h = rc.HostHandle(cfg)
        try:
            h.set_option("kmm_no_fuse", option)
            _refused(h.lib, h.lib.km_koemorph_stream_create(h.h, 4, T, 1, 1, 1), uns, who, *needles)
            assert plan(h, 4, T, 1)["supported"] == 0
        finally:
            h.close()


def test_refusals_name_the_entry_point_and_the_value():
    h = rc.HostHandle(okm.KoeMorphConfig())
    lib = h.lib
    out6 = (C.c_int64 * 6)()
    p = C.c_void_p(64)                      # never dereferenced: every call below is refused first
    inv = _lib.KM_ERR_INVALID_ARG
    try:
        create = lambda hh=h.h, N=4, T=30, R=1: lib.km_koemorph_stream_create(hh, N, T, R, 1, 1)
        _refused(lib, create(hh=None), inv, "km_koemorph_stream_create", "NULL handle")
        _refused(lib, create(N=0), inv, "km_koemorph_stream_create", "n_streams 0 < 1")
        _refused(lib, create(R=0), inv, "km_koemorph_stream_create", "max_rows 0 < 1")
        _refused(lib, create(T=0), inv, "km_koemorph_stream_create", "context_frames 0 < 1")
        # a supported shape, but nothing was uploaded: the call stops before it touches the device
        _refused(lib, create(), _lib.KM_ERR_NOT_FINALIZED, "km_finalize")
        _refused(lib, lib.km_koemorph_stream_plan(None, 4, 30, 1, out6), inv, "km_koemorph_stream_plan", "NULL handle")
        _refused(lib, lib.km_koemorph_stream_plan(h.h, 4, 30, 1, None), inv, "km_koemorph_stream_plan", "out is NULL")
        _refused(lib, lib.km_koemorph_stream_plan(h.h, 0, 30, 1, out6), inv, "km_koemorph_stream_plan", "n_streams 0 < 1")
        _refused(lib, lib.km_koemorph_stream_plan(h.h, 4, 30, -3, out6), inv, "km_koemorph_stream_plan", "max_rows -3 < 1")
        # no engine was created on this handle
        _refused(lib, lib.km_koemorph_stream_step(h.h, p, p, None, p, None, None, None), inv, "km_koemorph_stream_step", "no stream engine")
        _refused(lib, lib.km_koemorph_stream_reset(h.h, None, None), inv, "km_koemorph_stream_reset", "no stream engine")
        _refused(lib, lib.km_koemorph_stream_frames(h.h, p, None), inv, "km_koemorph_stream_frames", "no stream engine")
        _refused(lib, lib.km_koemorph_stream_step(None, p, p, None, p, None, None, None), inv, "km_koemorph_stream_step", "NULL handle")
        assert lib.km_koemorph_stream_destroy(h.h) == _lib.KM_OK           # nothing to free
        # a handle of another kind
        from koemorph_amd.engine import Engine
        e = Engine(d_model=64, num_heads=4, mel_sequence_length=32)
        try:
            _refused(lib, create(hh=e._h), inv, "km_koemorph_stream_create", "not a KoeMorphModel handle")
            _refused(lib, lib.km_koemorph_stream_plan(e._h, 4, 30, 1, out6), inv, "km_koemorph_stream_plan", "not a KoeMorphModel handle")
            _refused(lib, lib.km_koemorph_stream_step(e._h, p, p, None, p, None, None, None), inv, "km_koemorph_stream_step", "not a KoeMorphModel handle")
            _refused(lib, lib.km_koemorph_stream_reset(e._h, None, None), inv, "km_koemorph_stream_reset", "not a KoeMorphModel handle")
        finally:
            e.close()
    finally:
        h.close()


def test_plan_before_finalize_host_is_refused():
    lib = _lib.load()
    m = rc.torch_model(okm.KoeMorphConfig())
    h = C.c_void_p()
    cfg = m._c_config()
    _lib.check(lib.km_koemorph_create(C.byref(cfg), C.byref(h)))
    try:
        _refused(lib, lib.km_koemorph_stream_plan(h, 4, 30, 1, (C.c_int64 * 6)()), _lib.KM_ERR_NOT_FINALIZED, "km_koemorph_stream_plan")
    finally:
        lib.km_destroy(h)


def test_step_shape_errors_come_before_any_device_work():
    check = lambda mel, emo, counts=None: KoeMorphStreams.check_rows(4, 2, 80, 32, mel, emo, counts)
    mel, emo = check(torch.zeros(4, 80), torch.zeros(4, 25))                 # (N, dim): one row per stream; narrow emotion rows pass
    assert mel.shape == (4, 1, 80) and emo.shape == (4, 1, 25)
    mel, emo = check(torch.zeros(4, 2, 80), torch.zeros(4, 2, 32), torch.zeros(4, dtype=torch.int32))
    assert mel.shape == (4, 2, 80) and emo.shape == (4, 2, 32)
    with pytest.raises(ValueError, match="40 wide.*emotion_dim is 32"):
        check(torch.zeros(4, 1, 80), torch.zeros(4, 1, 40))
    with pytest.raises(ValueError, match="64 wide.*mel_dim is 80"):
        check(torch.zeros(4, 1, 64), torch.zeros(4, 1, 32))
    with pytest.raises(ValueError, match="rows of 4 streams, got 3"):
        check(torch.zeros(3, 1, 80), torch.zeros(3, 1, 32))
    with pytest.raises(ValueError, match="3 rows per stream.*1 .. 2"):
        check(torch.zeros(4, 3, 80), torch.zeros(4, 3, 32))
    with pytest.raises(ValueError, match=r"expected \(N, rows, mel_dim\)"):
        check(torch.zeros(4, 2, 80), torch.zeros(4, 1, 32))
    with pytest.raises(ValueError, match=r"expected \(N, rows, mel_dim\)"):
        check(torch.zeros(80), torch.zeros(32))
    with pytest.raises(ValueError, match="int32 counts"):
        check(torch.zeros(4, 80), torch.zeros(4, 32), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="int32 counts"):
        check(torch.zeros(4, 80), torch.zeros(4, 32), torch.zeros(3, dtype=torch.int32))
