"""The eGeMAPS low-level descriptors per frame, everything that needs no GPU: names and widths, the float64 restatement
(tests/lld_cases.py) against the pinned oracle, the frame-grid law, and what the extractor refuses.

The grid law is the frame count of ``MelSpectrogramExtractor.forward`` -- ``int(L / sample_rate * target_fps)``, reference
src/features/stft.py:130 -- so that mel rows and descriptor rows of the same audio pair up.  ``get_output_length`` of that class
is the STFT's own count before ``forward`` truncates it, ``L // hop + 1``: never fewer rows than the grid has, which is the
relation held here.
"""
import numpy as np
import pytest

import egemaps_cases as ec
import lld_cases as lc
from koemorph_amd import _lib
from koemorph_amd import egemaps_names as names
from oracle import egemaps as eg


def test_names_widths_and_the_gemaps_columns():
    assert len(names.LLD_NAMES) == lc.W_EGEMAPS == 25 and len(set(names.LLD_NAMES)) == 25
    assert names.LLD_NAMES[:6] == ["Loudness_sma3", "alphaRatio_sma3", "hammarbergIndex_sma3", "slope0-500_sma3", "slope500-1500_sma3",
                                   "spectralFlux_sma3"]
    assert names.LLD_NAMES[6:10] == [f"mfcc{i}_sma3" for i in (1, 2, 3, 4)]
    assert names.LLD_NAMES[10:16] == ["F0semitoneFrom27.5Hz_sma3nz", "jitterLocal_sma3nz", "shimmerLocaldB_sma3nz", "HNRdBACF_sma3nz",
                                      "logRelF0-H1-H2_sma3nz", "logRelF0-H1-A3_sma3nz"]
    assert names.LLD_NAMES[16:] == [f"F{i}{n}_sma3nz" for i in (1, 2, 3) for n in ("frequency", "bandwidth", "amplitudeLogRelF0")]
    assert all(n.endswith("_sma3") for n in names.LLD_NAMES[:10]) and all(n.endswith("_sma3nz") for n in names.LLD_NAMES[10:])
    assert names.GEMAPS_LLD_COLUMNS == [0, 1, 2, 3, 4] + list(range(10, 20)) + [21, 22, 24]
    assert names.GEMAPS_LLD_NAMES == [names.LLD_NAMES[i] for i in names.GEMAPS_LLD_COLUMNS] and len(names.GEMAPS_LLD_NAMES) == lc.W_GEMAPS == 18
    assert names.LLD_DIMS == {"eGeMAPSv02": 25, "GeMAPS": 18}
    # every functional's contour is one of the descriptors: the name before the statistic, V / UV being selections of frames
    stems = {n.rsplit("_", 1)[0].replace("loudness", "Loudness") for n in names.FEATURE_NAMES[:58]}
    assert stems == set(names.LLD_NAMES[:1] + names.LLD_NAMES[5:]), stems ^ set(names.LLD_NAMES)


def test_the_library_knows_the_widths_and_the_grid():
    lib = _lib.load()
    assert [lib.km_egemaps_lld_width(s) for s in (0, 1, 2, -1)] == [25, 18, -1, -1]
    for L in (0, 959, 960, 1119, 1120, 16000, 320000, 1 << 20):
        assert lib.km_egemaps_lld_frames(L, 0.0) == lib.km_egemaps_num_frames(L) == eg.frame_count(L)
    for fps in (0.5, 400.5, -30.0, float("nan"), float("inf")):
        assert lib.km_egemaps_lld_frames(16000, fps) == -1
        with pytest.raises(ValueError, match="fps must be finite and within 1 .. 400"):
            names.lld_fps_value(fps)
    assert names.lld_fps_value(None) == 0.0 and names.lld_fps_value(30) == 30.0


# ---- the restatement against the pinned oracle ---------------------------------------------------------------------------
# index of the first output a contour feeds (the key of `contours`), the column it is, the frames it is taken over
def contour_map():
    m = [(0, lc.SEMITONE, "voiced"), (10, 0, "all"), (20, 5, "all")]
    m += [(22 + 2 * i, 6 + i, "all") for i in range(4)]
    m += [(30 + 2 * i, 11 + i, "voiced") for i in range(14)]
    m += [(58 + 2 * i, c, "voiced") for i, c in enumerate((1, 2, 3, 4, 5, 6, 7, 8, 9))]
    m += [(76 + i, c, "unvoiced") for i, c in enumerate((1, 2, 3, 4, 5))]
    return m


@pytest.mark.parametrize("nf", [1, 3, 257])
def test_restated_columns_are_the_contours_of_the_pinned_functionals(nf):
    m = contour_map()
    assert {c for _, c, _ in m} == set(range(25))
    for name, rec in ec.functional_windows(nf):
        contours = {}
        eg.functionals_from_llds(ec.records_to_llds(rec), dtype=np.float64, contours=contours)
        lld, voiced = lc.reference(rec)
        assert lld.shape == (nf, 25) and lld.dtype == np.float64
        assert sorted(contours) == sorted(k for k, _, _ in m if k < 76 or (~voiced).any()), name
        for key, col, sel in m:
            if key not in contours:
                continue
            frames = {"all": np.ones(nf, bool), "voiced": voiced, "unvoiced": ~voiced}[sel]
            assert np.array_equal(lld[frames, col], contours[key]), (nf, name, key, names.LLD_NAMES[col])
        assert not lld[~voiced, lc.FIRST_NZ:].any(), name                                # 0 in unvoiced frames, full length
        fast, voiced_fast = lc.reference_fast(rec)
        assert np.array_equal(fast, lld) and np.array_equal(voiced_fast, voiced), (nf, name)


# ---- the frame grid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps", [30, 60, 29.97])
def test_grid_rows_are_the_mel_extractors_frame_count(fps):
    from koemorph_amd.features.stft import MelSpectrogramExtractor
    lib = _lib.load()
    mel = MelSpectrogramExtractor(target_fps=fps)
    for L in (0, 1, 532, 533, 534, 960, 15999, 16000, 16001, 16017, 48000, 160000, 320000, 479999, 480000, 1 << 20):
        expected = int(L / mel.sample_rate * mel.target_fps)                             # MelSpectrogramExtractor.forward
        assert lib.km_egemaps_lld_frames(L, float(fps)) == expected == lc.output_frames(L, fps) == names.lld_output_frames(L, fps), (L, fps)
        assert expected <= mel.get_output_length(L)                                      # ... which truncates the STFT's own count


def test_rows_past_the_last_frame_repeat_it():
    nf, L = 5, lc.samples_for(5)                                                         # 1600 samples: 10 rows at 100 fps, 5 frames
    T = lc.output_frames(L, 100)
    assert T == 10
    j, w, exact = lc.grid(nf, T, 100)
    assert j.tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 4, 4] and not w.any() and exact.all()
    lld = np.arange(nf * 25, dtype=np.float64).reshape(nf, 25) + 1.0
    rows, _, _, blend = lc.resample(lld, T, 100)
    assert np.array_equal(rows[:nf], lld) and np.array_equal(rows[nf:], np.repeat(lld[-1:], T - nf, 0)) and not blend.any()
    rows, _, _, _ = lc.resample(lld, 3, 30)                                              # coordinates 0, 3.33, 6.67: the last two beyond frame 4
    assert np.array_equal(rows[1], lld[3] + np.float64(np.float32(100.0 / 30 - 3)) * (lld[4] - lld[3])) and np.array_equal(rows[2], lld[4])


def test_whole_and_half_coordinates_on_hand_made_columns():
    # fps 200: coordinates 0, 0.5, 1, 1.5, ...  Two columns with the same numbers, one plain (0) and one non-zero-smoothed (10)
    v = np.array([4.0, 8.0, 0.0, 0.0, 6.0, 2.0, 0.0, 5.0])
    lld = np.zeros((8, 25))
    lld[:, 0] = v; lld[:, 10] = v
    T = 15
    j, w, exact = lc.grid(8, T, 200)
    assert j.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7] and w.tolist() == [0.0, 0.5] * 7 + [0.0] and exact.tolist() == [True, False] * 7 + [True]
    rows, _, _, blend = lc.resample(lld, T, 200)
    assert rows[::2, 0].tolist() == v.tolist() and rows[::2, 10].tolist() == v.tolist()  # w == 0: frame j exactly
    assert rows[1::2, 0].tolist() == [6.0, 4.0, 0.0, 3.0, 4.0, 1.0, 2.5]                 # plain: always the mean of the two
    assert rows[1::2, 10].tolist() == [6.0, 8.0, 0.0, 0.0, 4.0, 2.0, 0.0]                # nz: the mean only between two non-zero frames,
    assert blend[1::2, 10].tolist() == [True, False, False, False, True, False, False]   # else the EARLIER frame at w == 0.5
    # off the half: fps 400 has w 0.25 and 0.75 -> the nearer frame across an edge
    rows, _, _, _ = lc.resample(lld, 12, 400)
    assert rows[4:8, 10].tolist() == [8.0, 8.0, 8.0, 0.0] and rows[4:8, 0].tolist() == [8.0, 6.0, 4.0, 2.0]
    # a blended nz value is never strictly between 0 and the smaller neighbour
    assert not ((rows[:, 10] > 0) & (rows[:, 10] < 2.0)).any()


# ---- the extractor's refusals (all before the device is touched) ---------------------------------------------------------
def test_extractor_refusals():
    from koemorph_amd.features.opensmile_extractor import OpenSMILEeGeMAPSExtractor, create_opensmile_extractor
    with pytest.raises(ValueError, match=r"^Unsupported feature level: LowLevelDescriptors_Deltas$"):
        OpenSMILEeGeMAPSExtractor(feature_level="LowLevelDescriptors_Deltas")
    with pytest.raises(ValueError, match=r"^Unsupported feature level: functionals$"):
        OpenSMILEeGeMAPSExtractor(feature_level="functionals")
    with pytest.raises(ValueError, match="cannot be combined with use_concatenation"):
        OpenSMILEeGeMAPSExtractor(feature_level="LowLevelDescriptors", use_concatenation=True)
    with pytest.raises(ValueError, match="cannot be combined with use_concatenation"):
        create_opensmile_extractor({"feature_level": "LowLevelDescriptors", "use_concatenation": True, "feature_set": "GeMAPS"})
    with pytest.raises(ValueError, match=r"^Unsupported feature set: eGeMAPS$"):          # the set is still checked first
        OpenSMILEeGeMAPSExtractor(feature_set="eGeMAPS", feature_level="LowLevelDescriptors")
