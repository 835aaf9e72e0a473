"""Host half of the eGeMAPS stage tests (tests/test_gpu_egemaps_stages.py runs the kernels): the oracle's split at the record
seams is exact, and the crafted records of tests/egemaps_cases.py meet the conditions the GPU comparison relies on -- shown
with oracle/egemaps.py alone, no kernel involved."""
import numpy as np
import pytest

import egemaps_cases as ec
from koemorph_amd import synth
from oracle import egemaps as eg

SIGNALS = {"vowel": lambda: synth.make_vowel(3, 110.0, 1.2), "speechlike": lambda: ec.speechlike(11),
           "noise": lambda: 0.3 * synth.normal(9, (16000,))}


@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_oracle_split_is_exact(name):
    x = eg.normalise(SIGNALS[name]())
    d = eg.llds(x)
    whole, split = eg.functionals(x), eg.functionals_from_llds(d)
    assert whole.dtype == split.dtype == np.float32 and whole.tobytes() == split.tobytes()
    # float64 output and the contour hook change nothing that is computed
    contours = {}
    assert eg.functionals_from_llds(d, dtype=np.float64, contours=contours).astype(np.float32).tobytes() == whole.tobytes()
    assert set(contours) >= {0, 10} | set(range(20, 76, 2))        # one contour behind every ten / mean-stddevNorm group
    # the descriptors survive the 36-column layout (float32 rounding aside) and the layout is its own inverse
    rec = ec.llds_to_records(d)
    back = ec.records_to_llds(rec)
    for k, v in back.items():
        assert np.array_equal(v.astype(np.float32), np.asarray(d[k], np.float32)), k
    assert np.array_equal(ec.llds_to_records(back), rec)
    # pitch track: the forward / backward tables and the cost of a given track agree with viterbi_f0
    args = (d["cand_f"], d["cand_s"], d["voicing"], d["rms"])
    cstar, through = eg.viterbi_tables(*args)
    f0 = eg.viterbi_f0(*args)
    assert np.array_equal(f0, d["f0"])
    assert eg.path_cost(*args, f0) == cstar                        # same additions in the same order: to the bit
    # alpha + beta adds the same terms as C* in another order: equal up to float64 rounding of at most 3 nf additions
    assert np.abs(through.min(axis=1) - cstar).max() <= 3 * len(f0) * np.finfo(np.float64).eps * max(cstar, 1.0)
    worse = f0.copy()
    worse[len(f0) // 2] = 0.0 if f0[len(f0) // 2] > 0 else d["cand_f"][len(f0) // 2, 0]
    assert eg.path_cost(*args, worse) > cstar or worse[len(f0) // 2] == f0[len(f0) // 2]
    assert eg.path_cost(*args, np.full(len(f0), 12345.0)) == np.inf  # not a candidate


def test_path_cost_takes_the_cheaper_of_two_equal_candidates():
    cf = np.array([[100.0, 100.0, 200.0]] * 3); cs = np.array([[0.5, 0.9, 0.7]] * 3)
    vo, rms = np.full(3, 0.9), np.full(3, 0.1)
    assert eg.path_cost(cf, cs, vo, rms, np.full(3, 100.0)) == pytest.approx(3 * 2.0 * 0.1)
    assert eg.path_cost(cf, cs, vo, rms, np.array([100.0, 0.0, 100.0])) == pytest.approx(2 * 0.2 + 4.0 + 2 * 1.25)
    cstar, through = eg.viterbi_tables(cf, cs, vo, rms)
    assert cstar == pytest.approx(0.6) and np.allclose(through[:, 1], 0.6) and (through[:, 3] >= 0.4 + 4.0 + 1.25).all()


@pytest.mark.parametrize("nf", ec.FUNC_NF)
def test_crafted_records_meet_their_conditions(nf):
    names, rec, want, scale = ec.functional_batch(nf)
    assert len(names) >= 5 and rec.shape == (len(names), nf, 36) and rec.dtype == np.float32
    voiced = rec[:, :, ec.R["f0"]] != 0
    count = dict(zip(names, voiced.sum(axis=1)))
    p = ec.power_of_two_count(nf)
    assert p & (p - 1) == 0 and (nf == 1 or p < nf <= 2 * p)
    assert count["none_voiced"] == 0 and count["all_voiced"] == nf and count["count_pow2"] == p
    assert (nf == 1) == ("count_pow2_plus1" not in count) and count.get("count_pow2_plus1", p + 1) == p + 1
    first, last = voiced[names.index("only_first")], voiced[names.index("only_last")]
    assert first.sum() == 1 and first[0] and last.sum() == 1 and last[-1]
    if nf >= 63:                                                   # mixed voicing: runs of 1 to 12 frames, both kinds, short and long
        for n in ("mixed_half", "mixed_mostly_voiced", "mixed_mostly_unvoiced"):
            m = voiced[names.index(n)]
            runs = np.concatenate([eg.segments(m), eg.segments(~m)])
            assert 1 <= runs.min() and runs.max() <= 24 and eg.segments(m).max() <= 12 and len(runs) >= 6, n
        assert count["mixed_mostly_unvoiced"] < count["mixed_half"] < count["mixed_mostly_voiced"]
    for w in rec:                                                  # the grid: at most 12 significant bits, zeros where frames are invalid
        for col, (_, _, lg) in ec._FIELDS.items():
            k = w[:, col].astype(np.float64) / 2.0 ** lg
            assert np.array_equal(k, np.round(k)) and np.abs(k).max() < 4096
    if nf >= 255:
        v = rec[names.index("all_voiced")]
        for c in ("jit", "shim", "F", "BW", "famp"):
            assert 0.03 < (v[:, ec.R[c]] == 0).mean() < 0.2, c
    # every stddevNorm entry is a well conditioned quotient: |mean| >= std / 4, i.e. sn <= 4 (sn = 0 where nothing is selected)
    assert np.isfinite(want).all() and np.isfinite(scale).all() and (scale > 0).all()
    for i in range(88):
        if ec.CLASS[i] == "sn":
            assert (want[:, i] <= 4.0).all() and (want[:, i] >= 0.0).all(), eg.FEATURE_NAMES[i]
            some = want[:, i] > 0
            assert (np.abs(want[some, i - 1]) > 0).all()
    if nf >= 63:                                                   # and the comparison is not vacuous: every output moves
        assert (np.abs(want).max(axis=0) > 0).all()


def test_reference_scales_are_what_the_classes_say():
    names, rec, want, scale = ec.functional_batch(65)
    w = names.index("mixed_half")
    d = ec.records_to_llds(rec[w])
    f0 = eg.sma3(d["f0"], True)
    semi = 12.0 * np.log2(f0[f0 > 0] / 27.5)
    assert scale[w, 0] == scale[w, 2] == scale[w, 5] == np.abs(semi).max()
    rise, fall = eg.part_slopes(semi)
    assert scale[w, 6] == scale[w, 7] == max(rise) and scale[w, 8] == scale[w, 9] == -min(fall)
    assert scale[w, 1] == np.abs(semi).max() / abs(want[w, 0]) * (1 + want[w, 1])
    loud = eg.sma3(d["loudness"], False)
    assert scale[w, 10] == loud.max() and scale[w, 87] == 1.0 and scale[w, 82] == want[w, 82]
    assert scale[w, 76] == np.abs(eg.sma3(d["alphaRatio"], False)[f0 == 0]).max()


@pytest.mark.parametrize("nf", ec.TRACK_NF)
def test_crafted_candidates_meet_their_conditions(nf):
    names, rec, cstar, through, states = ec.track_batch(nf)
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
        elif nf >= 255:
            per = live.sum(axis=1)
            assert (per == 0).any() and ((per > 0) & (per < 3)).any() and (per == 3 if n.count('two') else per == 2).any(), n
            assert ok.any() and (~ok).any() and (vo[~ok] >= 0.55).any() and (vo[~ok] < 0.55).any(), n   # RMS floor and voicing both used
            assert len(set(st)) == 4, n                             # every state is on the optimal track somewhere
            runs = eg.segments(~ok)
            assert (runs <= 3).any() and (eg.segments(ok) <= 3).any(), n
        # the oracle's own track costs C*, and C* stays small enough for float32 to resolve the weights
        assert eg.path_cost(cf, cs, vo, rms, eg.viterbi_f0(cf, cs, vo, rms)) == c and c < 1000.0, n
        assert np.abs(th.min(axis=1) - c).max() <= 3 * nf * np.finfo(np.float64).eps * max(c, 1.0)
        # frame identity is decidable almost everywhere: the runner-up state costs more than the bound on >= 95 % of the frames
        gap = ec.runner_up_gap(th, st, c)
        assert (gap > ec.TRACK_BOUND).mean() >= 0.95, (n, float((gap > ec.TRACK_BOUND).mean()))
        assert (gap > ec.TRACK_BOUND_CAP).mean() >= 0.95            # ... even at the largest bound the comparison may ever use
