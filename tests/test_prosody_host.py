"""The restatement of the `basic` prosodic features (tests/prosody_cases.py) on known answers, the precondition of the GPU
comparison, and what the C side refuses before it touches a device.  No GPU.

PARITY UNPINNED: the restatement was written from the algorithms of librosa 0.10 and has not been checked against the package.
"""
import ctypes as C

import numpy as np
import pytest

import prosody_cases as pc
from koemorph_amd import _lib

EXPORTS = ("km_prosody_plan_create", "km_prosody_plan_destroy", "km_prosody_num_frames", "km_prosody_workspace_floats",
           "km_prosody_features", "km_prosody_windows", "km_emotion_stream_create_basic")


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_silence():
    out = pc.analyse(np.zeros(3000, np.float32))["out"]
    assert out.tolist() == [0, 0, 0, 400, 0, 0, 0, 0, 0]
    assert pc.analyse(np.zeros(3000, np.float32), np.float32)["out"].tolist() == [0, 0, 0, 400, 0, 0, 0, 0, 0]


def test_sine_200_hz():
    t = np.arange(16000) / pc.SR
    r = pc.analyse((0.5 * np.sin(2.0 * np.pi * 200.0 * t)).astype(np.float32))
    interior = slice(3, -3)                       # frames that hold no padding: 3 .. F - 4
    assert len(r["f0"]) == 32
    print("f0", r["f0"][interior].min(), r["f0"][interior].max(), "centroid", r["C"][interior].min(), r["C"][interior].max())
    assert np.abs(r["f0"][interior] - 200.0).max() < 0.05
    assert np.abs(r["C"][interior] - 200.0).max() < 0.5
    # a sine crosses zero twice a period: 2 * 200 / 16000 of the positions, one crossing more or less per frame
    assert np.abs(r["Z"][interior] - 400.0 / pc.SR).max() <= 1.0 / pc.NFFT
    assert abs(r["out"][0] - 0.125) < 1e-4 and abs(r["out"][7] - 0.5) < 1e-6 and abs(r["out"][8] + 0.5) < 1e-6


def test_num_frames():
    lib = _lib.load()
    for L, want in ((1, 1), (511, 1), (512, 2), (513, 2), (2048, 5)):
        assert pc.num_frames(L) == want and lib.km_prosody_num_frames(L) == want
        assert len(pc.analyse(np.ones(L, np.float32))["Z"]) == want
        assert lib.km_prosody_workspace_floats(3, L) == 3 * want * 4
    assert lib.km_prosody_num_frames(0) == 0 and lib.km_prosody_workspace_floats(0, 5) == -1 and lib.km_prosody_workspace_floats(2, 0) == -1


def test_trough_rules_on_hand_made_rows():
    base = np.full(pc.NC, 0.5)
    # the last index is a trough when it lies below its only neighbour
    c = base.copy(); c[-1] = 0.05
    assert pc.choose(c) == pc.NC - 1 and pc.shift_of(c, pc.NC - 1) == 0
    c = base.copy(); c[-2] = 0.02; c[-1] = 0.05          # ... and is not when the neighbour is lower still
    assert pc.choose(c) == pc.NC - 2
    # the first index against c[1] alone
    c = base.copy(); c[0] = 0.01
    assert pc.choose(c) == 0 and pc.shift_of(c, 0) == 0
    # a plateau: c[i] < c[i-1] and c[i] <= c[i+1] takes the plateau's FIRST index
    c = base.copy(); c[100:103] = 0.03
    assert pc.choose(c) == 100
    # the first trough below the threshold wins over a deeper one later
    c = base.copy(); c[50] = 0.09; c[200] = 0.001
    assert pc.choose(c) == 50
    # no trough below the threshold: the first index of the minimum, whatever the threshold says
    c = base.copy(); c[70] = 0.3; c[150] = 0.3
    assert pc.choose(c) == 70
    c = base.copy()
    assert pc.choose(c) == 0 and pc.decision_margin(c, 0) == float("inf")
    # interpolation: |b| < |a| moves the period, otherwise it stays
    c = base.copy(); c[99:102] = (0.30, 0.05, 0.20)       # a = 0.40, b = -0.05
    assert pc.choose(c) == 100 and pc.shift_of(c, 100) == pytest.approx(0.125, abs=1e-12)
    c = base.copy(); c[99:102] = (0.5, 0.05, 0.05)        # a = 0.45, b = -0.225: still |b| < |a|
    assert pc.shift_of(c, 100) == pytest.approx(0.5, abs=1e-12)
    row = np.array([0.9, 0.5, 0.1])                       # a = 0, b = -0.4: |b| < |a| is false, no shift (and no division by 0)
    assert pc.shift_of(row, 1) == 0
    row = np.array([0.2, 0.1, 0.6, 0.0])                  # around a peak the rule is the same: a = -1.1, b = -0.05
    assert pc.shift_of(row, 2) == pytest.approx(-0.05 / 1.1, abs=1e-12)
    row = np.array([0.0, 1.0, 2.1])                       # a = 0.1, b = 1.05: |b| >= |a|, no shift
    assert pc.shift_of(row, 1) == 0


# ---- the precondition of the GPU comparison -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", pc.LENGTHS)
@pytest.mark.parametrize("kind", pc.KINDS)
def test_every_decision_behind_i_star_has_a_margin(kind, L):
    """tests/test_gpu_prosody.py asks for the oracle's i* on EVERY frame of every input, which is only fair where no comparison that
    decides i* is within rounding of flipping: each needs a float64 margin of 1e-4 (``decision_margin``), three orders of magnitude
    above the float32 evaluation's error in c, asserted here as well.  The one exception is structural and exact: at L = 1 every
    entry of c is the same number, so i* = 0 by the first-index rule in float64 and float32 alike (``signal``, ``exact_tie``)."""
    o, y = pc.oracle(kind, L), pc.yardstick(kind, L)
    margins = [pc.decision_margin(c, i) for c, i in zip(o["c"], o["istar"])]
    c_err = float(np.abs(y["c"].astype(np.float64) - o["c"]).max())
    print(f"{kind} L={L}: smallest margin {min(margins):.3e}, float32 evaluation off by {c_err:.2e} in c")
    if L == 1:
        assert pc.exact_tie(pc.signal(kind, L)) and o["istar"].tolist() == [0]
    else:
        assert np.isfinite(margins).all()
    assert min(margins) >= pc.MIN_MARGIN
    assert c_err < 1e-5
    assert np.array_equal(o["istar"], y["istar"])


def test_inputs_cover_both_ways_to_an_index():
    found = [bool(((o["c"][np.arange(len(o["istar"])), o["istar"]]) < pc.THRESHOLD).any()) for o in (pc.oracle(k, 16000) for k in pc.KINDS)]
    none = [bool(((o["c"][np.arange(len(o["istar"])), o["istar"]]) >= pc.THRESHOLD).any()) for o in (pc.oracle(k, 16000) for k in pc.KINDS)]
    assert any(found) and any(none)
    assert np.concatenate([pc.oracle(k, 16000)["period"] % 1 != 0 for k in pc.KINDS]).any()          # the interpolation is exercised


# ---- the C side ---------------------------------------------------------------------------------------------------------------
def test_exports_and_prototypes():
    lib = _lib.load()
    for name in EXPORTS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_refusals_before_any_device_call():
    lib = _lib.load()
    dummy = C.create_string_buffer(64)                    # stands for a plan and for device buffers: a refused call reads none of them
    p = C.cast(dummy, C.c_void_p)
    feats = lambda B, L, stride, work, nwork, frames=None: lib.km_prosody_features(p, p, B, L, stride, work, nwork, p, frames, None)
    assert feats(0, 100, 100, p, 1 << 30) == _lib.KM_ERR_INVALID_ARG
    assert feats(1, 0, 0, p, 1 << 30) == _lib.KM_ERR_INVALID_ARG
    assert feats(65536, 100, 100, p, 1 << 30) == _lib.KM_ERR_UNSUPPORTED
    assert feats(1, (1 << 20) + 1, (1 << 20) + 1, p, 1 << 30) == _lib.KM_ERR_UNSUPPORTED
    assert feats(2, 100, 99, p, 1 << 30) == _lib.KM_ERR_INVALID_ARG                 # rows would overlap
    assert feats(2, 1000, 1000, p, 2 * 2 * 4 - 1) == _lib.KM_ERR_WORKSPACE
    assert feats(2, 1000, 1000, None, 0) == _lib.KM_ERR_INVALID_ARG                 # neither a workspace nor frames
    assert lib.km_prosody_features(None, p, 1, 100, 100, p, 64, p, None, None) == _lib.KM_ERR_INVALID_ARG
    wins = lambda clip_len, W, L, nwork: lib.km_prosody_windows(p, p, clip_len, p, W, L, p, nwork, p, None)
    assert wins(1000, 0, 100, 1 << 30) == _lib.KM_ERR_INVALID_ARG
    assert wins(0, 1, 100, 1 << 30) == _lib.KM_ERR_INVALID_ARG
    assert wins(1 << 31, 1, 100, 1 << 30) == _lib.KM_ERR_INVALID_ARG
    assert wins(1000, 65536, 100, 1 << 30) == _lib.KM_ERR_UNSUPPORTED
    assert wins(1000, 1, (1 << 20) + 1, 1 << 30) == _lib.KM_ERR_UNSUPPORTED
    assert wins(1000, 3, 600, 3 * 2 * 4 - 1) == _lib.KM_ERR_WORKSPACE
    assert lib.km_prosody_plan_create(None) == _lib.KM_ERR_INVALID_ARG and lib.km_prosody_plan_destroy(None) == 0
    h = C.c_void_p()
    for args in ((3, 1.0, 0.3, 0), (3, 1.0, 0.3, 4), (3, 1.0, 0.05, 1), (3, 0.5, 0.3, 1), (3, 1.0, 1.5, 1), (0, 1.0, 0.3, 1), (4097, 1.0, 0.3, 1)):
        assert lib.km_emotion_stream_create_basic(C.byref(h), *args) == _lib.KM_ERR_INVALID_ARG and not h.value, args
    assert lib.km_emotion_stream_create_basic(C.byref(h), 3, 66.0, 0.3, 1) == _lib.KM_ERR_UNSUPPORTED and not h.value     # 1 056 000 samples
    assert b"2^20" in lib.km_last_error() or b"1048576" in lib.km_last_error()


def test_stream_shape_of_the_basic_back_end():
    from koemorph_amd.streaming import emotion_stream_shape
    assert emotion_stream_shape(1.0, 0.3, backend="basic") == dict(ring_len=48000, window_len=16000, update_samples=4800, min_samples=8000,
                                                                  max_frames=32)
    assert emotion_stream_shape(8.5, 0.3, backend="basic")["max_frames"] == 266
    assert emotion_stream_shape(60.0, 0.3, backend="basic")["max_frames"] == 1876          # beyond the eGeMAPS back end's 20.5 s
    with pytest.raises(ValueError, match="at most"):
        emotion_stream_shape(66.0, 0.3, backend="basic")
    with pytest.raises(ValueError, match="backend"):
        emotion_stream_shape(1.0, 0.3, backend="emotion2vec")
    assert emotion_stream_shape(1.0, 0.3)["max_frames"] == 95                              # the default is the eGeMAPS arithmetic
