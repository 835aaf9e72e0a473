"""The long tier of the per-window eGeMAPS kernels, for windows beyond 2048 frames (koemorph_amd/csrc/km_egemaps_window.hip:
egm_viterbi_kernel and egm_functional_kernel at LongTier) on the crafted records of tests/egemaps_cases.py, no audio in the way:

1. EQUAL BITS.  At 1, 3, 257 and 2048 frames the ``_long`` hooks give, on the same records, the bits of the existing hooks: all 88
   functionals and the whole record array behind the pitch track.
2. LONG WINDOWS AGAINST FLOAT64 (oracle/egemaps.py) at 2049 frames, at 4095 / 4096 / 4097 -- where the sort's padding doubles to 8192
   and where the pitch track's staging starts its second chunk --, and at the cap, 6548.  All 88 outputs per class; the tolerance of
   a class at nf frames is egemaps_cases.TOL x nf / 2048, never above TOL_CAP (egemaps_long_cases.tol says why).  The track by
   check_track's three assertions with the bound recomputed by the harness's rule (egemaps_long_cases.track_bound).
3. A batched call equals B = 1 calls bit for bit; the records are read only; guard values around ``out`` survive.
4. FROM AUDIO.  ``functionals(x, long_windows=True)`` on a speech-like window of 30 s equals the functionals of its own records
   bit for bit and is held to the oracle as test_functionals_from_real_records holds the short window; on a 10 s window it equals
   ``functionals(x)`` bit for bit (the route is unchanged).
5. 6549 frames are refused and nothing is launched; with the flag off the old limit still raises.
tests/test_egemaps_long_host.py shows with the oracle alone that the crafted inputs meet the conditions relied on here.

FIGURES (MI355X; 45 crafted windows for the functionals, 35 for the track).  Worst error as a fraction of the tolerance at its frame
count (egemaps_long_cases.tol), per class, with the error / scale itself and where:
    means, percentiles, range    0.208   1.29e-7   nf=2049 all_voiced, loudness pctlrange0-2
    slope mean / std             0.003   3.40e-7   nf=6548 mixed_half, loudness meanFallingSlope
    stddevNorm                   0.148   2.81e-8   nf=2049 mixed_mostly_unvoiced, F2 amplitude
    equivalent sound level       0.183   1.68e-6 dB  nf=2049 only_first
    rates and segment lengths    0.205   4.10e-7   nf=4095 mixed_mostly_voiced, StddevUnvoicedSegmentLength
  The errors grow far less than linearly in the frame count (the worst at 6548 frames is 1.21e-7 for the means and 2.38e-6 dB for
  the level; the level's worst anywhere is 2.68e-6 dB at 4096), so the fractions fall as the tolerances grow.
  Real records (two speech-like windows of 30 s, 2995 frames; slopes and peak rate excluded): stat 0.076 (6.92e-8), stddevNorm 0.102
  (2.84e-8), level 0.078 (1.05e-6 dB), rates 0.039 (5.70e-8).  Before the percentile position became an exact quotient beyond 2048
  frames the stat class stood at 4.68 of its tolerance there (4.25e-6, loudness percentile80.0): float32 numbers near 0.8 x 2994 are
  2.4e-4 apart, the product landed 4.9e-5 off, and the two sorted neighbours it interpolates between are 7.0 loudness units apart
  (the clusters of the signal's two voices).  Up to 2048 frames the float32 product is kept: the equal-bits law.
  Pitch track: the cost excess over C* is 0 on all 35 crafted windows (C* up to 2102.66 at nf = 6548) and every frame's state is the
  oracle's (every frame is decidable: the smallest runner-up gap is 0.05); bound 4 float32 spacings at the set's largest C*, 2.4e-4
  to 9.8e-4, cap 0.125.
"""
import numpy as np
import pytest
import torch

import egemaps_cases as ec
import egemaps_long_cases as lc
from koemorph_amd import _lib
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine
from oracle import egemaps as eg

pytestmark = pytest.mark.gpu

F0 = ec.R["f0"]


@pytest.fixture(scope="module")
def engine():
    return EGeMAPSEngine("cuda")


# ---- 1. equal bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", lc.EQUAL_NF)
def test_long_kernels_give_the_bits_of_the_existing_ones(engine, nf):
    _, rec, _, _ = ec.functional_batch(nf)
    dev = torch.tensor(rec).cuda()
    assert torch.equal(engine.functionals_from_records(dev, long_windows=True).view(torch.int32),
                       engine.functionals_from_records(dev).view(torch.int32))
    _, rec, _, _, _ = ec.track_batch(nf)
    dev = torch.tensor(rec).cuda()
    old = engine.track_from_records(dev)
    new = engine.track_from_records(dev, long_windows=True)
    assert torch.equal(new.view(torch.int32), old.view(torch.int32))
    assert bool((new[:, :, F0] != -1.0).all())                     # ... and both wrote every frame's F0


# ---- 2. long windows against float64 ----------------------------------------------------------------------------------
def check_functionals(got, want, scale, nf, what, skip=()):
    assert np.isfinite(got).all(), what
    worst = ec.class_errors(got, want, scale, skip)
    print(f"{what}: " + "  ".join(f"{c} {e:.2e} ({e / lc.tol(c, nf):.3f} of tol) [{eg.FEATURE_NAMES[i]}]" for c, (e, i) in sorted(worst.items())))
    for c, (e, i) in worst.items():
        assert e <= lc.tol(c, nf), (what, c, eg.FEATURE_NAMES[i], float(got[i]), float(want[i]), float(scale[i]), e, lc.tol(c, nf))


@pytest.mark.parametrize("nf", lc.LONG_NF)
def test_functionals_from_crafted_records(engine, nf):
    names, rec, want, scale = ec.functional_batch(nf)
    dev = torch.tensor(rec).cuda()
    got = engine.functionals_from_records(dev, long_windows=True)
    if nf == lc.BATCH_CHECK_NF:                                     # 3. a window's result does not depend on its neighbours
        guarded = torch.full((len(names) + 2, 88), -7.0, device="cuda")
        lib = _lib.load()
        _lib.check(lib.km_egemaps_functionals_from_records_long(dev.data_ptr(), len(names), nf, guarded[1:-1].data_ptr(), None))
        assert torch.equal(guarded[1:-1], got) and bool((guarded[0] == -7.0).all()) and bool((guarded[-1] == -7.0).all())
        for b in range(len(names)):
            assert torch.equal(engine.functionals_from_records(dev[b:b + 1], long_windows=True)[0], got[b]), names[b]
    got = got.cpu().numpy()
    assert np.array_equal(dev.cpu().numpy(), rec)                  # the records are read only
    for b, name in enumerate(names):
        check_functionals(got[b], want[b], scale[b], nf, f"functionals nf={nf} {name}")


def check_track(rec, out, bound, what):
    """check_track of tests/test_gpu_egemaps_stages.py with the bound of this frame count's set."""
    keep = np.ones(ec.REC, bool); keep[F0] = False
    assert np.array_equal(out[:, keep].view(np.uint32), rec[:, keep].view(np.uint32)), what    # only the F0 column is written
    st = ec.track_states(rec, out[:, F0])
    assert (st >= 0).all(), (what, np.flatnonzero(st < 0)[:8])
    assert (out[(rec[:, ec.R["cf"]:ec.R["cf"] + 3] <= 0).all(axis=1), F0] == 0).all(), what
    args = ec.track_inputs(rec)
    cstar, _ = eg.viterbi_tables(*args)
    excess = eg.path_cost(*args, out[:, F0]) - cstar
    print(f"{what}: C* {cstar:.4f} excess {excess:.3e} bound {bound:.3e}")
    assert 0.0 <= excess <= bound, (what, cstar, excess, bound)
    return st


@pytest.mark.parametrize("nf", lc.LONG_NF)
def test_track_from_crafted_candidates(engine, nf):
    names, rec, cstars, throughs, states = ec.track_batch(nf)
    bound = lc.track_bound(cstars)
    dev = torch.tensor(rec).cuda()
    got = engine.track_from_records(dev, long_windows=True)
    if nf == lc.BATCH_CHECK_NF:
        for b in range(len(names)):
            assert torch.equal(engine.track_from_records(dev[b:b + 1], long_windows=True)[0], got[b]), names[b]
    out = got.cpu().numpy()
    assert np.array_equal(dev.cpu().numpy(), rec)                  # the engine works on a copy
    for b, name in enumerate(names):
        st = check_track(rec[b], out[b], bound, f"track nf={nf} {name}")
        decidable = ec.runner_up_gap(throughs[b], states[b], cstars[b]) > bound
        wrong = np.flatnonzero(decidable & (st != states[b]))
        print(f"track nf={nf} {name}: decidable {decidable.mean():.3f} states equal {(st == states[b]).mean():.4f}")
        assert len(wrong) == 0, (name, wrong[:8], st[wrong[:8]], states[b][wrong[:8]])


# ---- 4. from audio ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_audio(engine):
    """Two speech-like windows of 30 s (2995 frames), their functionals at B = 2 and the records of that call."""
    x = np.stack([ec.speechlike(21, 30.0), ec.speechlike(31, 30.0)])
    assert x.shape == (2, 480000)
    dev = torch.from_numpy(x).cuda()
    feats = engine.functionals(dev, long_windows=True).clone()
    rec = engine.records()
    assert rec.shape == (2, 2995, 36)
    return dev, feats, rec


def test_functionals_of_long_audio_run_the_long_kernels(engine, long_audio):
    dev, feats, rec = long_audio
    assert torch.equal(engine.functionals_from_records(rec, long_windows=True), feats)
    one = engine.functionals(dev[:1], long_windows=True)            # B = 1: the same bits
    assert torch.equal(one[0], feats[0])
    assert np.array_equal(engine.records()[0][:, :33].view(np.uint32), rec[0][:, :33].view(np.uint32))   # columns 33-35 are never written
    again = engine.track_from_records(rec, long_windows=True).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), rec.view(np.uint32))     # the F0 column the records already carry


def test_functionals_of_long_audio_against_the_oracle(long_audio):
    """As test_functionals_from_real_records: the sign tests behind the slopes and the loudness peak count may fall differently in
    float32 and float64 on full-precision contours (the only permitted exclusion)."""
    _, feats, rec = long_audio
    for b in range(2):
        want, scale = ec.reference_and_scales(rec[b])
        assert (rec[b][:, F0] > 0).sum() > 500 and (rec[b][:, F0] == 0).sum() > 200
        check_functionals(feats[b].cpu().numpy(), want, scale, 2995, f"functionals real nf=2995 window {b}", skip=ec.SLOPE_IDX + (ec.PEAK_IDX,))


def test_short_audio_takes_the_unchanged_route(engine):
    x = torch.from_numpy(ec.speechlike(11, 10.0)[None]).cuda()
    plain = engine.functionals(x).clone()
    assert torch.equal(engine.functionals(x, long_windows=True).view(torch.int32), plain.view(torch.int32))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_error_paths(engine):
    lib = _lib.load()
    rec = torch.full((1, 6549, 36), -3.0, device="cuda")
    out = torch.full((1, 88), -7.0, device="cuda")
    for rc in (lib.km_egemaps_track_from_records_long(rec.data_ptr(), 1, 6549, None),
               lib.km_egemaps_functionals_from_records_long(rec.data_ptr(), 1, 6549, out.data_ptr(), None)):
        assert rc == _lib.KM_ERR_UNSUPPORTED and "6549 frames per window, at most 6548 (65.5 s)" in lib.km_last_error().decode()
    L = 960 + 160 * 6548                                             # 6549 frames
    audio = torch.zeros(1, L, device="cuda")
    work = torch.full((int(lib.km_egemaps_workspace_floats(1, L)),), -5.0, device="cuda")
    rc = lib.km_egemaps_functionals_long(engine._plan, audio.data_ptr(), 1, L, 1, work.data_ptr(), work.numel(), out.data_ptr(), None)
    assert rc == _lib.KM_ERR_UNSUPPORTED
    assert lib.km_last_error().decode() == f"km_egemaps_functionals_long: a window of {L} samples, at most 1048576 (65.5 s)"
    torch.cuda.synchronize()
    assert bool((rec == -3.0).all()) and bool((out == -7.0).all()) and bool((work == -5.0).all())     # nothing was launched
    # the flag left off still raises as before
    with pytest.raises(_lib.KoeMorphError, match=r"2049 frames per window, at most 2048 \(20\.5 s\)") as e:
        engine.track_from_records(np.zeros((1, 2049, 36), np.float32))
    assert e.value.code == _lib.KM_ERR_UNSUPPORTED
    with pytest.raises(_lib.KoeMorphError, match=r"2049 frames per window, at most 2048 \(20\.5 s\)"):
        engine.functionals_from_records(np.zeros((1, 2049, 36), np.float32))
    with pytest.raises(_lib.KoeMorphError, match=r"2995 frames per window, at most 2048 \(20\.5 s\)"):
        engine.functionals(torch.zeros(1, 480000, device="cuda"))
    # the limit itself is accepted
    ok = engine.functionals_from_records(np.zeros((1, 6548, 36), np.float32), long_windows=True)
    assert ok.shape == (1, 88) and bool(torch.isfinite(ok).all())
