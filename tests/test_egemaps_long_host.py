"""Host half of the long eGeMAPS windows (tests/test_gpu_egemaps_long.py and test_gpu_emotion_long.py run the kernels): the shape
arithmetic with ``long_windows=True``, the refusals of the two ``_long`` create entry points -- the table of
tests/test_emotion_create_host.py with the window limit in the place of the frame limit --, and, with the oracle alone, the
conditions the GPU comparison relies on at every long frame count it uses.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import egemaps_cases as ec
import egemaps_long_cases as lc
import test_egemaps_stages_host as stages
import test_emotion_create_host as create
from koemorph_amd import _lib
from koemorph_amd.streaming import emotion_stream_shape
from oracle import egemaps as eg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = _lib.KM_ERR_INVALID_ARG, _lib.KM_ERR_UNSUPPORTED
NEW_EXPORTS = ("km_egemaps_functionals_long", "km_egemaps_track_from_records_long", "km_egemaps_functionals_from_records_long",
               "km_emotion_stream_create_long", "km_emotion_clip_create_long")


def test_shape_arithmetic_with_long_windows():
    assert emotion_stream_shape(30.0, 0.2, long_windows=True) == dict(ring_len=512000, window_len=480000, update_samples=3200,
                                                                      min_samples=8000, max_frames=2995)
    cap = (1 << 20) / 16000.0                                          # 65.536 s: a window of exactly 2^20 samples
    assert emotion_stream_shape(cap, 0.2, long_windows=True)["window_len"] == 1 << 20
    assert emotion_stream_shape(cap, 0.2, long_windows=True)["max_frames"] == lc.MAXF_LONG == 6548
    with pytest.raises(ValueError, match=re.escape("a window of 1064576 samples, at most 1048576 (65.5 s)")):
        emotion_stream_shape(cap + 1.0, 0.2, long_windows=True)
    # a short window is the same shape either way, and with the flag off nothing changed
    assert emotion_stream_shape(20.0, 0.3, long_windows=True) == emotion_stream_shape(20.0, 0.3)
    with pytest.raises(ValueError, match=re.escape("2055 frames per window, at most 2048 (20.5 s)")):
        emotion_stream_shape(20.6, 0.3)
    with pytest.raises(ValueError, match=re.escape("2995 frames per window, at most 2048 (20.5 s)")):
        emotion_stream_shape(30.0, 0.2, long_windows=False)
    with pytest.raises(ValueError, match="Context window"):
        emotion_stream_shape(0.9, 0.3, long_windows=True)
    with pytest.raises(ValueError, match="larger than context"):
        emotion_stream_shape(1.0, 1.5, long_windows=True)
    with pytest.raises(ValueError, match="eGeMAPS back end's switch"):
        emotion_stream_shape(30.0, 0.2, backend="basic", long_windows=True)


# entry point -> (the name its texts carry, is it a clip object): each says its own name
LONG_ENTRY_POINTS = {"km_emotion_stream_create_long": ("km_emotion_stream_create_long", False),
                     "km_emotion_clip_create_long": ("km_emotion_clip_create_long", True)}


@pytest.mark.parametrize("entry", list(LONG_ENTRY_POINTS))
def test_long_create_refuses_the_table_before_any_device_call(entry):
    lib = _lib.load()
    name, clip = LONG_ENTRY_POINTS[entry]
    good = (4,) if clip else (4, 2)
    fn = getattr(lib, entry)
    assert (fn(None, 1.0, 0.1, 4) if clip else fn(None, 4, 1.0, 0.1, 2)) == INVALID
    assert lib.km_last_error().decode() == f"{name}: NULL argument"
    cases = [(a, good, rc, text) for a, rc, text in create.TIMING]
    # the window limit takes the place of the frame limit: 66 s is refused with the basic back end's text, 20.6 s is not refused
    # at all (and so not called here: it would reach the device)
    cases += [(a, good, UNSUPPORTED, b) for a, _, b in create.FRAMES if b is not None]
    assert len(cases) == len(create.TIMING) + 1
    cases.append((((1 << 20) / 16000.0 + 1.0, 0.2), good, UNSUPPORTED, "a window of 1064576 samples, at most 1048576 (65.5 s)"))
    if clip:
        cases += [((1.0, 0.1), (0,), INVALID, "max_slots 0, 1 .. 65535"), ((1.0, 0.1), (65536,), INVALID, "max_slots 65536, 1 .. 65535"),
                  ((0.5, 0.3), (0,), INVALID, "Context window must be at least 1.0 seconds"),
                  ((1.0, 1.5), (0,), INVALID, "Update interval cannot be larger than context window"),
                  ((3601.0, 0.3), (0,), INVALID, "max_slots 0, 1 .. 65535"), ((66.0, 0.3), (65536,), INVALID, "max_slots 65536, 1 .. 65535")]
    else:
        cases += [((1.0, 0.1), (0, 1), INVALID, "n_streams 0, 1 .. 4096"), ((1.0, 0.1), (4097, 1), INVALID, "n_streams 4097, 1 .. 4096"),
                  ((1.0, 0.1), (4, 0), INVALID, "max_updates 0, 1 .. n_streams (4)"), ((1.0, 0.1), (4, 5), INVALID, "max_updates 5, 1 .. n_streams (4)"),
                  ((0.5, 0.3), (0, 1), INVALID, "n_streams 0, 1 .. 4096"),
                  ((0.5, 0.3), (4, 5), INVALID, "Context window must be at least 1.0 seconds"),
                  ((1.0, 1.5), (4, 0), INVALID, "Update interval cannot be larger than context window"),
                  ((3601.0, 0.3), (4, 5), INVALID, "max_updates 5, 1 .. n_streams (4)"), ((66.0, 0.3), (4, 0), INVALID, "max_updates 0, 1 .. n_streams (4)")]
    for (ctx, itv), counts, rc, text in cases:
        got = create._call(lib, entry, clip, ctx, itv, counts)
        assert got == (rc, None, f"{name}: {text}"), (entry, ctx, itv, counts, got)


def test_record_hooks_refuse_on_the_host():
    """Frame counts and batch sizes are checked before anything touches a device: these run without one."""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for call in (lambda B, nf: lib.km_egemaps_track_from_records_long(p, B, nf, None),
                 lambda B, nf: lib.km_egemaps_functionals_from_records_long(p, B, nf, p, None)):
        assert call(1, 0) == INVALID and call(1, -1) == INVALID and call(0, 8) == INVALID
        assert call(1, 6549) == UNSUPPORTED and "6549 frames per window, at most 6548 (65.5 s)" in lib.km_last_error().decode()
        assert call(65536, 1) == UNSUPPORTED
    assert lib.km_egemaps_functionals_long(p, p, 1, (1 << 20) + 1, 1, p, 1 << 40, p, None) == UNSUPPORTED
    assert lib.km_last_error().decode() == "km_egemaps_functionals_long: a window of 1048577 samples, at most 1048576 (65.5 s)"
    assert lib.km_egemaps_num_frames(1 << 20) == 6548 and lib.km_egemaps_num_frames((1 << 20) + 1) == 6548
    assert lib.km_egemaps_num_frames((1 << 20) + 160) == 6549


def test_header_signatures_and_sources_name_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "koemorph.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in _lib.SIGNATURES and hasattr(lib, name), name
    # the constants the frame counts of these tests are chosen around
    hdr = open(os.path.join(ROOT, "koemorph_amd", "csrc", "km_egemaps_window.h")).read()
    long_tier = re.search(r"struct LongTier \{(.*?)\};", hdr, re.S).group(1)
    assert re.search(r"\bCHUNK = %d;" % lc.TRACK_CHUNK, long_tier) and re.search(r"\bSORT_MAX = 8192;", long_tier)
    assert '"km_egemaps_window.hip"' in open(os.path.join(ROOT, "koemorph_amd", "build.py")).read()


@pytest.mark.parametrize("nf", lc.LONG_NF)
def test_crafted_records_meet_their_conditions_at_long_frame_counts(nf):
    stages.test_crafted_records_meet_their_conditions(nf)          # every condition of the short set, at this frame count
    names, rec, want, scale = ec.functional_batch(nf)
    assert len(names) == 9
    for cls in ec.TOL:                                             # the tolerances grow with nf and stop at the cap
        assert ec.TOL[cls] < lc.tol(cls, nf) <= ec.TOL_CAP or ec.TOL[cls] == ec.TOL_CAP == lc.tol(cls, nf)
    p = ec.power_of_two_count(nf)                                  # the sort's padding: n2 = 4096 and 8192 are both reached
    voiced = (rec[:, :, ec.R["f0"]] != 0).sum(axis=1)
    assert p in voiced and p + 1 in voiced and nf in voiced
    assert (p == 4096) == (nf > 4096) and (p == 2048) == (nf <= 4096)


@pytest.mark.parametrize("nf", lc.LONG_NF)
def test_crafted_candidates_meet_their_conditions_at_long_frame_counts(nf):
    """test_crafted_candidates_meet_their_conditions with the two figures that depend on the frame count: every C* is below 4096
    (float32 still resolves the weights: spacing 2^-12 against the smallest weight 1.25) and the decidable frames are judged by the
    bound recomputed for this set."""
    names, rec, cstar, through, states = ec.track_batch(nf)
    assert len(names) == 7
    bound = lc.track_bound(cstar)
    assert ec.TRACK_BOUND <= bound <= 4 * 2.0 ** -12 < ec.TRACK_BOUND_CAP
    if nf == lc.MAXF_LONG:
        assert bound == 4 * 2.0 ** -12 and 2048 <= max(cstar) < 4096
    for n, w, c, th, st in zip(names, rec, cstar, through, states):
        cf, cs, vo, rms = ec.track_inputs(w)
        live = cf > 0
        assert ((cf[live] >= 60.0) & (cf[live] <= 500.0)).all() and ((cs[live] >= 0.5) & (cs[live] <= 1.0)).all(), n
        for row in cf:
            assert len(set(row[row > 0])) == (row > 0).sum(), n     # distinct within a frame
        ok = (vo >= eg.VOICING_CUTOFF) & (rms >= eg.RMS_FLOOR)
        assert np.abs(vo - eg.VOICING_CUTOFF).min() > 1e-3          # no frame within float32 rounding of the cutoff
        if n == "all_ok":
            assert ok.all() and live.all()
        elif n == "none_ok":
            assert not ok.any() and live.any()
        elif n == "no_cand":
            assert not live.any() and (st == 3).all()
        else:
            per = live.sum(axis=1)
            assert (per == 0).any() and ((per > 0) & (per < 3)).any() and (per == 3 if n.count('two') else per == 2).any(), n
            assert ok.any() and (~ok).any() and (vo[~ok] >= 0.55).any() and (vo[~ok] < 0.55).any(), n
            assert len(set(st)) == 4, n                             # every state is on the optimal track somewhere
            runs = eg.segments(~ok)
            assert (runs <= 3).any(), n                             # (voiced-ok runs are long here: the events thin out with nf)
        assert eg.path_cost(cf, cs, vo, rms, eg.viterbi_f0(cf, cs, vo, rms)) == c and c < 4096.0, n
        assert np.abs(th.min(axis=1) - c).max() <= 3 * nf * np.finfo(np.float64).eps * max(c, 1.0)
        gap = ec.runner_up_gap(th, st, c)
        assert gap.min() > bound, (n, float(gap.min()), bound)      # here EVERY frame is decidable: the smallest gap is 0.05
        assert (gap > ec.TRACK_BOUND_CAP).mean() >= 0.95
