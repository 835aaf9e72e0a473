"""The GeMAPS feature set of the eGeMAPS kernels (KM_FEATURE_SET_GEMAPS: km_egemaps_functionals_set,
km_egemaps_functionals_from_records_set; koemorph_amd/csrc/km_egemaps.hip and km_egemaps_window.hip).

What is pinned is the 88-value path (tests/test_gpu_egemaps*.py, float64).  Here: value j of a GeMAPS call IS, bit for bit, value
``GEMAPS_COLUMNS[j]`` of the eGeMAPS call on the same samples or records --

1. FROM AUDIO at 1, 2, 3 and 257 frames (the flux's ``t > 0`` branch makes 1 and 2 the edges), B 1 and 3, normalised or not; at 2048
   frames; at 2049 through ``long_windows``.  The frame records of the GeMAPS call equal the eGeMAPS call's in every field but 5-9
   (flux, MFCC 1-4), which are 0.
2. FROM RECORDS (egemaps_cases.craft_records) on both tiers, up to 4097 frames on the long one.
3. Not zeros against zeros: at least 56 of the 62 values of a speech-like window are non-zero.
4. One case against float64 directly: the crafted windows of 257 frames, per class with egemaps_cases.TOL, restricted to the columns.
5. Guards around ``out`` at stride 62, a second run, the refusals under the new names.
6. km_linear at K = 186 (no multiple of 4), the product of the GeMAPS compression layer, with the bound of tests/test_gpu_linear.py.
"""
import numpy as np
import pytest
import torch

import egemaps_cases as ec
import gemaps_cases as gc
from koemorph_amd import _lib
from koemorph_amd.egemaps_names import GEMAPS_COLUMNS, GEMAPS_FEATURE_NAMES
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine

pytestmark = pytest.mark.gpu

COLS = torch.tensor(GEMAPS_COLUMNS)
GM = "GeMAPS"


@pytest.fixture(scope="module")
def engine():
    return EGeMAPSEngine("cuda")


def samples_for(nf):
    return 960 + 160 * (nf - 1)


def audio(B, nf):
    """B speech-like windows of exactly nf frames, each from another voice and another place of its signal."""
    L = samples_for(nf)
    rows = []
    for b in range(B):
        x = ec.speechlike(40 + b, max(2.0, L / 16000.0 + 0.5))
        at = 1600 * b
        rows.append(x[at:at + L])
    x = np.stack(rows)
    assert x.shape == (B, L)
    return torch.from_numpy(x).cuda()


def both_from_audio(engine, x, normalize, long_windows=False):
    out88 = engine.functionals(x, normalize, long_windows=long_windows).clone()
    rec88 = engine.records()
    out62 = engine.functionals(x, normalize, long_windows=long_windows, feature_set=GM).clone()
    rec62 = engine.records()
    return out88, rec88, out62, rec62


def check_against_the_88(out88, rec88, out62, rec62, what):
    assert out62.shape == (out88.shape[0], 62)
    assert gc.same_bits(out62, out88[:, COLS.cuda()]), (what, (out62 != out88[:, COLS.cuda()]).nonzero()[:8].tolist())
    keep = np.ones(33, bool)                                          # columns 33-35 of a record are never written
    keep[gc.FLUX_MFCC_FIELDS] = False
    assert np.array_equal(rec62[:, :, :33][:, :, keep].view(np.uint32), rec88[:, :, :33][:, :, keep].view(np.uint32)), what
    assert not rec62[:, :, gc.FLUX_MFCC_FIELDS].view(np.uint32).any(), what      # +0.0, all five


# ---- 1. from audio ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nf", [1, 2, 3, 257])
def test_from_audio_equals_the_columns_of_the_88(engine, nf, B, normalize):
    x = audio(B, nf)
    out88, rec88, out62, rec62 = both_from_audio(engine, x, normalize)
    assert rec88.shape == (B, nf, 36)
    check_against_the_88(out88, rec88, out62, rec62, (nf, B, normalize))
    if nf >= 2:
        assert rec88[:, 1:, gc.FLUX_MFCC_FIELDS].any()               # the eGeMAPS call did write a flux and MFCCs there


def test_from_audio_at_the_short_tiers_limit_and_beyond(engine):
    x = audio(1, 2048)
    check_against_the_88(*both_from_audio(engine, x, True), "nf 2048")
    x = audio(1, 2049)
    check_against_the_88(*both_from_audio(engine, x, True, long_windows=True), "nf 2049 long")


def test_a_second_run_gives_equal_bits(engine):
    x = audio(3, 257)
    a = engine.functionals(x, feature_set=GM).clone()
    engine.functionals(audio(1, 3), feature_set=GM)
    assert gc.same_bits(engine.functionals(x, feature_set=GM), a)


# ---- 2. from records --------------------------------------------------------------------------------------------------
def crafted(nf):
    return torch.from_numpy(np.stack([ec.craft_records(7000 + nf, nf, 0.5), ec.craft_records(7001 + nf, nf, 0.8),
                                      ec.craft_records(7002 + nf, nf, 0.0)])).cuda()


@pytest.mark.parametrize("nf", [1, 2, 3, 255, 256, 257, 2048])
def test_from_records_on_the_short_tier(engine, nf):
    rec = crafted(nf)
    out88 = engine.functionals_from_records(rec)
    out62 = engine.functionals_from_records(rec, feature_set=GM)
    assert out62.shape == (3, 62) and gc.same_bits(out62, out88[:, COLS.cuda()])


@pytest.mark.parametrize("nf", [1, 2, 3, 255, 256, 257, 2048, 2049, 4097])
def test_from_records_on_the_long_tier(engine, nf):
    rec = crafted(nf)
    out88 = engine.functionals_from_records(rec, long_windows=True)
    out62 = engine.functionals_from_records(rec, long_windows=True, feature_set=GM)
    assert out62.shape == (3, 62) and gc.same_bits(out62, out88[:, COLS.cuda()])
    if nf <= 2048:                                                     # ... with the short tier's bits up to 2048 frames
        assert gc.same_bits(out62, engine.functionals_from_records(rec, feature_set=GM))


# ---- 3. not zeros against zeros ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_most_values_of_a_speechlike_window_are_non_zero(engine, seed):
    x = torch.from_numpy(ec.speechlike(seed, 2.0)[None]).cuda()
    out62 = engine.functionals(x, feature_set=GM)[0].cpu().numpy()
    assert np.isfinite(out62).all()
    zero = [GEMAPS_FEATURE_NAMES[j] for j in np.flatnonzero(out62 == 0)]
    print(f"seed {seed}: {62 - len(zero)} of 62 non-zero; zero: {zero}")
    assert 62 - len(zero) >= 56, zero


# ---- 4. against float64 directly --------------------------------------------------------------------------------------
def test_crafted_records_against_the_float64_oracle(engine):
    names, rec, want, scale = ec.functional_batch(257)
    got = engine.functionals_from_records(torch.tensor(rec).cuda(), feature_set=GM).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - want[:, GEMAPS_COLUMNS]) / scale[:, GEMAPS_COLUMNS]
    worst = {}
    for j, col in enumerate(GEMAPS_COLUMNS):
        c = ec.CLASS[col]
        e = float(err[:, j].max())
        if e >= worst.get(c, (-1.0, 0))[0]:
            worst[c] = (e, j)
    print("GeMAPS nf=257: " + "  ".join(f"{c} {e:.2e} ({e / ec.TOL[c]:.3f} of tol) [{GEMAPS_FEATURE_NAMES[j]}]" for c, (e, j) in sorted(worst.items())))
    assert set(worst) == {"stat", "slope", "sn", "count"}             # the one "db" value is the sound level, which GeMAPS has not
    for c, (e, j) in worst.items():
        assert e <= ec.TOL[c], (c, GEMAPS_FEATURE_NAMES[j], e, ec.TOL[c])


# ---- 5. guards and refusals -------------------------------------------------------------------------------------------
def test_guards_around_out_at_stride_62(engine):
    lib = _lib.load()
    B, nf = 3, 257
    x = audio(B, nf)
    L = x.shape[1]
    want = engine.functionals(x, feature_set=GM).clone()
    work = torch.zeros(int(lib.km_egemaps_workspace_floats(B, L)), device="cuda")
    guarded = torch.full((B + 2, 62), -7.0, device="cuda")
    _lib.check(lib.km_egemaps_functionals_set(engine._plan, 1, 0, x.data_ptr(), B, L, 1, work.data_ptr(), work.numel(), guarded[1:-1].data_ptr(), None))
    torch.cuda.synchronize()
    assert gc.same_bits(guarded[1:-1], want) and bool((guarded[0] == -7.0).all()) and bool((guarded[-1] == -7.0).all())
    rec = crafted(nf)
    guarded.fill_(-7.0)
    _lib.check(lib.km_egemaps_functionals_from_records_set(1, 1, rec.data_ptr(), B, nf, guarded[1:-1].data_ptr(), None))
    torch.cuda.synchronize()
    assert gc.same_bits(guarded[1:-1], engine.functionals_from_records(rec, feature_set=GM))
    assert bool((guarded[0] == -7.0).all()) and bool((guarded[-1] == -7.0).all())
    # set 0 through the new entry points: the existing calls' bits at width 88
    out = torch.empty(B, 88, device="cuda")
    _lib.check(lib.km_egemaps_functionals_set(engine._plan, 0, 0, x.data_ptr(), B, L, 1, work.data_ptr(), work.numel(), out.data_ptr(), None))
    assert gc.same_bits(out, engine.functionals(x))
    _lib.check(lib.km_egemaps_functionals_from_records_set(0, 0, rec.data_ptr(), B, nf, out.data_ptr(), None))
    assert gc.same_bits(out, engine.functionals_from_records(rec))


def test_refusals_carry_the_new_names(engine):
    lib = _lib.load()
    err = lambda: lib.km_last_error().decode()
    assert [lib.km_feature_set_width(s) for s in (0, 1, 2, -1)] == [88, 62, -1, -1]
    L = samples_for(2049)
    x = torch.zeros(1, L, device="cuda")
    work = torch.full((int(lib.km_egemaps_workspace_floats(1, L)),), -5.0, device="cuda")
    out = torch.full((1, 88), -7.0, device="cuda")
    rec = torch.full((1, 2049, 36), -3.0, device="cuda")
    call = lambda s, lw, Lx=L, wf=None: lib.km_egemaps_functionals_set(engine._plan, s, lw, x.data_ptr(), 1, Lx, 1, work.data_ptr(),
                                                                       work.numel() if wf is None else wf, out.data_ptr(), None)
    assert call(2, 0) == _lib.KM_ERR_INVALID_ARG and err() == "km_egemaps_functionals_set: feature set 2, 0 (eGeMAPS) or 1 (GeMAPS)"
    for s in (0, 1):
        assert call(s, 0) == _lib.KM_ERR_UNSUPPORTED and err() == "km_egemaps_functionals_set: 2049 frames per window, at most 2048 (20.5 s)"
        assert call(s, 0, 959) == _lib.KM_ERR_INVALID_ARG
        assert err() == "km_egemaps_functionals_set: the window is shorter than one 60 ms frame (959 samples)"
        assert call(s, 1, L, 8) == _lib.KM_ERR_WORKSPACE and err() == "km_egemaps_functionals_set: workspace too small"
        assert call(s, 1, (1 << 20) + 1) == _lib.KM_ERR_UNSUPPORTED
        assert err() == f"km_egemaps_functionals_set: a window of {(1 << 20) + 1} samples, at most 1048576 (65.5 s)"
    rcall = lambda s, lw, nf: lib.km_egemaps_functionals_from_records_set(s, lw, rec.data_ptr(), 1, nf, out.data_ptr(), None)
    assert rcall(7, 0, 8) == _lib.KM_ERR_INVALID_ARG and err() == "km_egemaps_functionals_from_records_set: feature set 7, 0 (eGeMAPS) or 1 (GeMAPS)"
    assert rcall(1, 0, 2049) == _lib.KM_ERR_UNSUPPORTED
    assert err() == "km_egemaps_functionals_from_records_set: 2049 frames per window, at most 2048 (20.5 s)"
    assert rcall(1, 1, 6549) == _lib.KM_ERR_UNSUPPORTED
    assert err() == "km_egemaps_functionals_from_records_set: 6549 frames per window, at most 6548 (65.5 s)"
    assert rcall(1, 0, 0) == _lib.KM_ERR_INVALID_ARG and err() == "km_egemaps_functionals_from_records_set: 0 frames per window, at least 1"
    h = _lib.C.c_void_p()
    assert lib.km_emotion_stream_create_set(_lib.C.byref(h), 2, 10.0, 0.5, 2, 5, 0) == _lib.KM_ERR_INVALID_ARG and not h.value
    assert err() == "km_emotion_stream_create_set: feature set 5, 0 (eGeMAPS) or 1 (GeMAPS)"
    assert lib.km_emotion_clip_create_set(_lib.C.byref(h), 10.0, 0.5, 4, 5, 0) == _lib.KM_ERR_INVALID_ARG and not h.value
    assert err() == "km_emotion_clip_create_set: feature set 5, 0 (eGeMAPS) or 1 (GeMAPS)"
    assert lib.km_emotion_stream_create_set(_lib.C.byref(h), 2, 21.0, 0.3, 2, 1, 0) == _lib.KM_ERR_UNSUPPORTED and not h.value
    assert err() == "km_emotion_stream_create_set: 2095 frames per window, at most 2048 (20.5 s)"
    with pytest.raises(ValueError, match=r"^Unsupported feature set: eGeMAPS$"):
        engine.functionals(x, feature_set="eGeMAPS")
    with pytest.raises(ValueError, match=r"^Unsupported feature set: eGeMAPS$"):
        engine.functionals_from_records(np.zeros((1, 8, 36), np.float32), feature_set="eGeMAPS")
    torch.cuda.synchronize()
    assert bool((rec == -3.0).all()) and bool((out == -7.0).all()) and bool((work == -5.0).all())     # nothing was launched


# ---- 6. the compression product at K = 186 ----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64])
def test_km_linear_at_k_186(B):
    lib = _lib.load()
    K, N, U = 186, 256, 2.0 ** -24
    assert lib.km_gemm_kernel_choice(B, N, K, 1) == 0                 # gemm_kernel: K is no multiple of 16
    gen = torch.Generator().manual_seed(186 + B)
    x, w, b = (torch.randn(*s, generator=gen).cuda() for s in ((B, K), (N, K), (N,)))
    out = torch.full((B + 2, N), float("nan"), device="cuda")
    _lib.check(lib.km_linear(x.data_ptr(), w.data_ptr(), b.data_ptr(), B, K, N, out[1:-1].data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[-1]).all()) and not bool(torch.isnan(out[1:-1]).any())
    x64, w64, b64 = x.cpu().double(), w.cpu().double(), b.cpu().double()
    bound = (K + 2) * U * (x64.abs() @ w64.abs().T + b64.abs())       # tests/test_gpu_linear.py: a float32 sum of K products in any order
    ratio = float(((out[1:-1].cpu().double() - (x64 @ w64.T + b64)).abs() / bound).max())
    print(f"LINEAR|0 gemm_kernel|{B} x {N} x {K}|bias|{ratio:.4f}")
    assert ratio <= 1.0
