"""The eGeMAPS low-level descriptors per frame on the device (km_egemaps_llds, km_egemaps_llds_from_records;
koemorph_amd/csrc/km_egemaps_lld.hip) against the float64 restatement of tests/lld_cases.py.

1. FROM RECORDS at the native rate: every window of egemaps_cases.functional_windows(nf), nf in 1, 2, 3, 255, 256, 257, 2048, 2049
   and 6548, both feature sets.  Every column but 10 within 2^-23 |want|: on the grid of those records a three-frame sum is exact in
   float32 and the one division is correctly rounded, while an index or mask slip moves a value by a grid step, 2^-12 relative at
   the least.  Column 10 (through log2f) within lld_cases.SEMITONE_TOL of the window's largest |semitone|: four times the worst
   measured on the MI355X over this set, 1.347e-7 (at 256 frames; profiles/llds_pin.txt), so 5.39e-7, under the cap of 1e-4.
   GeMAPS column j has the bits of eGeMAPS column GEMAPS_LLD_COLUMNS[j].
2. RESAMPLED at 100, 30, 60, 29.97 and 120 rows per second: 100 gives the native bits and repeats the last row; the others are held
   to the bound of the row's endpoints -- a blend is a convex combination of them, so the larger of the two -- plus
   2^-22 (|a| + |b|) for the difference and the fused multiply-add.  Across a voiced / unvoiced edge a row has the BITS of the
   nearer frame's value; a grid of 0 rows.
3. FROM AUDIO: llds(audio) is llds_from_records(records()) bit for bit, the records are those `functionals` leaves, and the float64
   means of columns 0 and 10 are outputs 10 and 0 of `functionals` within TOL["stat"]: the tie to the pinned route.
4. Guards around `out`, a captured call replayed on other samples, the refusals under the new names, device memory, the extractor's
   descriptor level, and KoeMorphModel(emotion_dim=25) on mel and descriptor rows of the same second of audio.
"""
import numpy as np
import pytest
import torch

import egemaps_cases as ec
import lld_cases as lc
from gemaps_cases import bits, same_bits
from koemorph_amd import _lib
from koemorph_amd.egemaps_names import GEMAPS_LLD_COLUMNS, GEMAPS_LLD_NAMES, LLD_NAMES
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine, OpenSMILEeGeMAPSExtractor

pytestmark = pytest.mark.gpu

GM = "GeMAPS"
COLS = np.array(GEMAPS_LLD_COLUMNS)
NOT10 = np.array([c for c in range(25) if c != lc.SEMITONE])
REL = 2.0 ** -23


@pytest.fixture(scope="module")
def engine():
    return EGeMAPSEngine("cuda")


def audio(B, nf, extra=0):
    """B speech-like windows of exactly nf frames (plus `extra` samples, fewer than a hop), each from another voice and place."""
    L = lc.samples_for(nf) + extra
    rows = []
    for b in range(B):
        x = ec.speechlike(40 + b, max(2.0, L / 16000.0 + 0.5))
        rows.append(x[1600 * b:1600 * b + L])
    x = np.stack(rows)
    assert x.shape == (B, L) and ec.eg.frame_count(L) == nf
    return torch.from_numpy(x).cuda()


def semitone_scale(want):
    """(B, 1): the largest |semitone| of each window, 1 where it has none."""
    top = np.abs(want[:, :, lc.SEMITONE]).max(axis=1, keepdims=True)
    return np.where(top > 0, top, 1.0)


# ---- 1. from records, native rate ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", lc.RECORD_NF)
def test_from_records_at_the_native_rate(engine, nf):
    names, rec, want, voiced = lc.record_batch(nf)
    dev = torch.tensor(rec).cuda()
    got32 = engine.llds_from_records(dev)
    assert got32.shape == (len(names), nf, 25) and got32.dtype == torch.float32
    got = got32.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    bad = np.argwhere(err[:, :, NOT10] > REL * np.abs(want[:, :, NOT10]))
    assert len(bad) == 0, [(names[b], t, LLD_NAMES[NOT10[c]], got[b, t, NOT10[c]], want[b, t, NOT10[c]]) for b, t, c in bad[:5]]
    assert np.array_equal(got[:, :, lc.FIRST_NZ:] != 0, want[:, :, lc.FIRST_NZ:] != 0) and not got[:, :, lc.FIRST_NZ:][~voiced].any()
    e10 = err[:, :, lc.SEMITONE] / semitone_scale(want)
    b, t = np.unravel_index(np.argmax(e10), e10.shape)
    print(f"LLD10|nf {nf}|worst {e10.max():.3e} of the largest |semitone| ({names[b]}, frame {t})|{e10.max() / lc.SEMITONE_TOL:.3f} of tol")
    assert e10.max() <= lc.SEMITONE_TOL
    got18 = engine.llds_from_records(dev, feature_set=GM)
    assert got18.shape == (len(names), nf, 18) and same_bits(got18, got32.cpu().numpy()[:, :, COLS])


# ---- 2. resampled ----------------------------------------------------------------------------------------------------------
def grid_length(nf):
    """A window of nf frames with samples to spare: the grid then has rows past the last frame."""
    return min(lc.samples_for(nf) + 500, 1 << 20)


@pytest.mark.parametrize("nf", [1, 3, 257, 6548])
def test_a_hundred_rows_per_second_are_the_native_rows(engine, nf):
    names, rec, want, voiced = lc.record_batch(nf)
    dev = torch.tensor(rec).cuda()
    L = grid_length(nf)
    T = lc.output_frames(L, 100)
    assert T > nf
    for fs, native in ((None, engine.llds_from_records(dev)), (GM, engine.llds_from_records(dev, feature_set=GM))):
        got = engine.llds_from_records(dev, fps=100, length=L, **({"feature_set": fs} if fs else {}))
        assert got.shape == (len(names), T, native.shape[2])
        assert same_bits(got[:, :nf], native) and same_bits(got[:, nf:], native[:, -1:].expand(-1, T - nf, -1))


@pytest.mark.parametrize("fps", [30, 60, 29.97, 120])
@pytest.mark.parametrize("nf", [1, 3, 257, 6548])
def test_resampled_rows(engine, nf, fps):
    names, rec, want, voiced = lc.record_batch(nf)
    dev = torch.tensor(rec).cuda()
    L = grid_length(nf)
    T = lc.output_frames(L, fps)
    got32 = engine.llds_from_records(dev, fps=fps, length=L).cpu().numpy()
    native = engine.llds_from_records(dev).cpu().numpy()
    assert got32.shape == (len(names), T, 25) and np.isfinite(got32).all()
    got18 = engine.llds_from_records(dev, fps=fps, length=L, feature_set=GM)
    assert same_bits(got18, got32[:, :, COLS])
    j, w, exact = lc.grid(nf, T, fps)
    for b, name in enumerate(names):
        rows, a, bb, blend = lc.resample(want[b], T, fps)
        # the bound of a frame's value: 2^-23 of it, the semitone's tolerance in column 10.  A row that is no blend is the frame `one`
        one = np.where(exact[:, None] | (w <= 0.5)[:, None], a, bb)
        end_one, end_both = REL * np.abs(one), REL * np.maximum(np.abs(a), np.abs(bb))
        end_one[:, lc.SEMITONE] = end_both[:, lc.SEMITONE] = lc.SEMITONE_TOL * semitone_scale(want[b:b + 1])[0, 0]
        bound = np.where(blend, end_both + 2.0 ** -22 * (np.abs(a) + np.abs(bb)), end_one)
        assert np.array_equal(rows[~blend], one[~blend])
        err = np.abs(got32[b].astype(np.float64) - rows)
        bad = np.argwhere(err > bound)
        assert len(bad) == 0, [(name, fps, k, LLD_NAMES[c], got32[b, k, c], rows[k, c], bound[k, c]) for k, c in bad[:5]]
        # rows that are a frame, or the nearer frame across an edge, have that frame's bits; a descriptor never leaks towards a 0
        na, nb = native[b][j], native[b][np.minimum(j + 1, nf - 1)]
        picked = np.where(exact[:, None] | (w <= 0.5)[:, None], na, nb)
        assert np.array_equal(bits(got32[b])[~blend], bits(picked)[~blend]), (name, fps)
        edge = ~exact[:, None] & ((na != 0) != (nb != 0))
        edge[:, :lc.FIRST_NZ] = False
        assert not (blend & edge).any()
        smaller = np.where(na != 0, np.abs(na), np.abs(nb))
        assert not (edge & (np.abs(got32[b]) > 0) & (np.abs(got32[b]) < smaller)).any(), (name, fps)
    if nf == 257:
        assert blend.any() and (~blend & ~exact[:, None]).any()          # both kinds of row were seen


def test_a_grid_of_no_rows(engine):
    rec = torch.tensor(lc.record_batch(3)[1]).cuda()
    for fs, W in (("eGeMAPSv02", 25), (GM, 18)):
        out = engine.llds_from_records(rec, feature_set=fs, fps=30, length=533)
        assert out.shape == (rec.shape[0], 0, W) and out.is_cuda
    lib = _lib.load()
    x = audio(2, 1)                                                       # 960 samples: a frame, but no row at 16 per second
    assert lib.km_egemaps_lld_frames(960, 16.0) == 0 and lib.km_egemaps_lld_frames(960, 17.0) == 1
    work = torch.full((int(lib.km_egemaps_workspace_floats(2, 960)),), -5.0, device="cuda")
    out = torch.full((64,), -7.0, device="cuda")
    assert lib.km_egemaps_llds(engine._plan, 0, 0, x.data_ptr(), 2, 960, 1, work.data_ptr(), work.numel(), 16.0, out.data_ptr(), None) == _lib.KM_OK
    assert lib.km_egemaps_llds_from_records(0, rec.data_ptr(), 2, 3, 960, 16.0, out.data_ptr(), None) == _lib.KM_OK
    torch.cuda.synchronize()
    assert bool((work == -5.0).all()) and bool((out == -7.0).all())      # nothing was launched
    got = engine.llds(x, fps=16)
    assert got.shape == (2, 0, 25) and engine.llds(x, fps=17).shape == (2, 1, 25)


# ---- 3. from audio -----------------------------------------------------------------------------------------------------------
def check_from_audio(engine, x, normalize, long_windows=False):
    B, L = x.shape
    for fs in ("eGeMAPSv02", GM):
        engine.functionals(x, normalize, long_windows=long_windows, feature_set=fs)
        rec_f = engine.records()
        got = engine.llds(x, normalize, feature_set=fs, long_windows=long_windows).clone()
        rec = engine.records()
        assert rec.shape == (B, ec.eg.frame_count(L), 36) and got.shape[:2] == rec.shape[:2]
        assert np.array_equal(rec[:, :, :33].view(np.uint32), rec_f[:, :, :33].view(np.uint32)), fs     # columns 33-35 are never written
        assert same_bits(got, engine.llds_from_records(rec, feature_set=fs)), fs
        got30 = engine.llds(x, normalize, feature_set=fs, long_windows=long_windows, fps=30)
        assert got30.shape[1] == int(L / 16000 * 30)
        assert same_bits(got30, engine.llds_from_records(rec, feature_set=fs, fps=30, length=L)), fs


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nf", [1, 3, 257])
def test_from_audio_is_the_kernel_on_the_calls_records(engine, nf, B, normalize):
    check_from_audio(engine, audio(B, nf, extra=100), normalize)


def test_from_audio_beyond_2048_frames(engine):
    check_from_audio(engine, audio(1, 2049), True, long_windows=True)


@pytest.mark.parametrize("seed", [0, 1])
def test_column_means_are_the_pinned_functionals(engine, seed):
    x = torch.from_numpy(ec.speechlike(seed, 2.0)[None]).cuda()
    func = engine.functionals(x)[0].cpu().numpy().astype(np.float64)
    lld = engine.llds(x)[0].cpu().numpy().astype(np.float64)
    loud, semi = lld[:, 0], lld[:, lc.SEMITONE]
    semi = semi[semi != 0]
    assert len(semi) >= 20 and len(semi) < len(loud)
    e_loud = abs(loud.mean() - func[10]) / np.abs(loud).max()
    e_semi = abs(semi.mean() - func[0]) / np.abs(semi).max()
    print(f"LLDTIE|seed {seed}|loudness mean {e_loud:.2e}|semitone mean {e_semi:.2e}|tol {ec.TOL['stat']:.1e}")
    assert e_loud <= ec.TOL["stat"] and e_semi <= ec.TOL["stat"]
    assert np.isfinite(lld).all() and (lld[:, lc.FIRST_NZ + 1:] != 0).any(axis=0).sum() >= 10       # not zeros against zeros


# ---- 4. guards, capture, refusals, memory, the layers above --------------------------------------------------------------
@pytest.mark.parametrize("fps", [None, 30])
def test_guards_around_out(engine, fps):
    lib = _lib.load()
    B, nf = 3, 257
    x = audio(B, nf)
    L = x.shape[1]
    rate = 0.0 if fps is None else float(fps)
    for code, fs, W in ((0, "eGeMAPSv02", 25), (1, GM, 18)):
        want = engine.llds(x, feature_set=fs, fps=fps).clone()
        rec = torch.from_numpy(engine.records()).cuda()
        T = want.shape[1]
        n = B * T * W
        work = torch.zeros(int(lib.km_egemaps_workspace_floats(B, L)), device="cuda")
        guarded = torch.full((3 * n,), -7.0, device="cuda")
        _lib.check(lib.km_egemaps_llds(engine._plan, code, 0, x.data_ptr(), B, L, 1, work.data_ptr(), work.numel(), rate, guarded[n:2 * n].data_ptr(), None))
        torch.cuda.synchronize()
        assert same_bits(guarded[n:2 * n].view(B, T, W), want) and bool((guarded[:n] == -7.0).all()) and bool((guarded[2 * n:] == -7.0).all())
        guarded.fill_(-7.0)
        _lib.check(lib.km_egemaps_llds_from_records(code, rec.data_ptr(), B, nf, L, rate, guarded[n:2 * n].data_ptr(), None))
        torch.cuda.synchronize()
        assert same_bits(guarded[n:2 * n].view(B, T, W), want) and bool((guarded[:n] == -7.0).all()) and bool((guarded[2 * n:] == -7.0).all())


def test_a_captured_call_replayed_on_other_samples(engine):
    lib = _lib.load()
    B, nf = 2, 257
    sets = [audio(B, nf), audio(B, nf).flip(0).contiguous(), (0.5 * audio(B, nf)).roll(777, 1).contiguous()]
    eager = [engine.llds(x, fps=30).clone() for x in sets]
    L = sets[0].shape[1]
    x = torch.zeros(B, L, device="cuda")
    work = torch.zeros(int(lib.km_egemaps_workspace_floats(B, L)), device="cuda")
    out = torch.zeros_like(eager[0])
    call = lambda: _lib.check(lib.km_egemaps_llds(engine._plan, 0, 0, x.data_ptr(), B, L, 1, work.data_ptr(), work.numel(), 30.0, out.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                           # warm up on the side stream, as torch asks
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # one linear chain of five launches
        call()
    for src, want in zip(sets, eager):
        x.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want)
    del g


def test_refusals_carry_the_new_names(engine):
    lib = _lib.load()
    err = lambda: lib.km_last_error().decode()
    L = lc.samples_for(2049)
    x = torch.zeros(1, L, device="cuda")
    work = torch.full((int(lib.km_egemaps_workspace_floats(1, L)),), -5.0, device="cuda")
    out = torch.full((1, 2049 * 4, 25), -7.0, device="cuda")
    rec = torch.full((1, 2049, 36), -3.0, device="cuda")
    call = lambda s, lw, Lx=L, wf=None, fps=0.0: lib.km_egemaps_llds(engine._plan, s, lw, x.data_ptr(), 1, Lx, 1, work.data_ptr(),
                                                                    work.numel() if wf is None else wf, fps, out.data_ptr(), None)
    assert call(2, 0) == _lib.KM_ERR_INVALID_ARG and err() == "km_egemaps_llds: feature set 2, 0 (eGeMAPS) or 1 (GeMAPS)"
    for s in (0, 1):
        for fps in (0.5, 401.0, -1.0, float("nan"), float("inf")):
            assert call(s, 1, fps=fps) == _lib.KM_ERR_INVALID_ARG and err().startswith("km_egemaps_llds: fps ")
            assert err().endswith("finite and within 1 .. 400 (0: the native 100 Hz)")
        assert call(s, 0) == _lib.KM_ERR_UNSUPPORTED and err() == "km_egemaps_llds: 2049 frames per window, at most 2048 (20.5 s)"
        assert call(s, 0, 959) == _lib.KM_ERR_INVALID_ARG and err() == "km_egemaps_llds: the window is shorter than one 60 ms frame (959 samples)"
        assert call(s, 0, 959, fps=30.0) == _lib.KM_ERR_INVALID_ARG and err() == "km_egemaps_llds: the window is shorter than one 60 ms frame (959 samples)"
        assert call(s, 1, L, 8) == _lib.KM_ERR_WORKSPACE and err() == "km_egemaps_llds: workspace too small"
        assert call(s, 1, (1 << 20) + 1) == _lib.KM_ERR_UNSUPPORTED
        assert err() == f"km_egemaps_llds: a window of {(1 << 20) + 1} samples, at most 1048576 (65.5 s)"
    rcall = lambda s, nf, fps=0.0, Lg=0: lib.km_egemaps_llds_from_records(s, rec.data_ptr(), 1, nf, Lg, fps, out.data_ptr(), None)
    assert rcall(7, 8) == _lib.KM_ERR_INVALID_ARG and err() == "km_egemaps_llds_from_records: feature set 7, 0 (eGeMAPS) or 1 (GeMAPS)"
    assert rcall(1, 6549) == _lib.KM_ERR_UNSUPPORTED and err() == "km_egemaps_llds_from_records: 6549 frames per window, at most 6548 (65.5 s)"
    assert rcall(1, 0) == _lib.KM_ERR_INVALID_ARG and err() == "km_egemaps_llds_from_records: 0 frames per window, at least 1"
    assert rcall(0, 8, 500.0, 16000) == _lib.KM_ERR_INVALID_ARG
    assert err() == "km_egemaps_llds_from_records: fps 500, finite and within 1 .. 400 (0: the native 100 Hz)"
    assert rcall(0, 8, 30.0, (1 << 20) + 1) == _lib.KM_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match=r"^Unsupported feature set: eGeMAPS$"):
        engine.llds(x, feature_set="eGeMAPS")
    with pytest.raises(ValueError, match="fps must be finite and within 1 .. 400"):
        engine.llds(x, fps=0.5)
    with pytest.raises(ValueError, match="`length`"):
        engine.llds_from_records(np.zeros((1, 8, 36), np.float32), fps=30)
    with pytest.raises(_lib.KoeMorphError, match="at most 2048"):
        engine.llds(x)
    torch.cuda.synchronize()
    assert bool((rec == -3.0).all()) and bool((out == -7.0).all()) and bool((work == -5.0).all())     # nothing was launched


def test_the_calls_hold_no_device_memory():
    lib = _lib.load()
    eng = EGeMAPSEngine("cuda")
    x = audio(2, 257)
    rec = torch.tensor(lc.record_batch(257)[1]).cuda()
    eng.llds(x)                                                           # the first call: whatever is set up once
    torch.cuda.synchronize()
    live = lib.km_live_device_bytes()
    for fps in (None, 30, 120):
        eng.llds(x, fps=fps); eng.llds(x, fps=fps, feature_set=GM); eng.llds_from_records(rec, fps=fps, length=x.shape[1])
    torch.cuda.synchronize()
    assert lib.km_live_device_bytes() == live
    eng.close()


def test_the_extractors_descriptor_level():
    ext = OpenSMILEeGeMAPSExtractor(feature_level="LowLevelDescriptors", device="cuda")
    gm = OpenSMILEeGeMAPSExtractor(feature_level="LowLevelDescriptors", feature_set=GM, device="cuda")
    assert ext.feature_dim == 25 and gm.feature_dim == 18
    assert ext.get_feature_names() == LLD_NAMES and gm.get_feature_names() == GEMAPS_LLD_NAMES
    x = audio(2, 257)
    rows = ext.extract_batch(x)
    assert rows.shape == (2, 257, 25) and same_bits(rows, ext.engine.llds(x))
    assert same_bits(gm.extract_batch(x.cpu().numpy(), fps=30), gm.engine.llds(x, feature_set=GM, fps=30))
    flat = ext._extract_features_from_audio(x[0].cpu().numpy())
    assert flat.dtype == np.float32 and flat.shape == (257 * 25,) and same_bits(flat.reshape(257, 25), rows[0])
    func = OpenSMILEeGeMAPSExtractor(device="cuda")                       # the functionals level is what it was
    assert func.feature_dim == 88 and func.extract_batch(x).shape == (2, 88) and func._extract_features_from_audio(x[0].cpu().numpy()).shape == (88,)
    with pytest.raises(ValueError, match="fps applies to"):
        func.extract_batch(x, fps=30)


def test_koemorph_model_on_mel_and_descriptor_rows(engine):
    from koemorph_amd.features.stft import MelSpectrogramExtractor
    from koemorph_amd.model.gaussian_face import KoeMorphModel
    x = torch.from_numpy(ec.speechlike(5, 1.2)[None, :16000]).cuda()
    assert x.shape == (1, 16000)
    mel = MelSpectrogramExtractor(target_fps=30)(x)
    emo = engine.llds(x, fps=30)
    assert mel.shape == (1, 30, 80) and emo.shape == (1, 30, 25)
    torch.manual_seed(0)
    model = KoeMorphModel(d_model=64, d_query=64, num_heads=4, num_encoder_layers=1, num_attention_layers=1, decoder_hidden_dim=32,
                          emotion_dim=25).cuda().eval()
    with torch.no_grad():
        out = model(mel, emo)["blendshapes"]
        other = model(mel, torch.zeros_like(emo), apply_smoothing=False)["raw_blendshapes"]
        mine = model(mel, emo, apply_smoothing=False)["raw_blendshapes"]
    assert out.shape == (1, 52) and bool(torch.isfinite(out).all())
    assert not torch.equal(mine, other)                                  # the descriptors reach the output
