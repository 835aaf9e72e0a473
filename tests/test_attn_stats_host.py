"""The attention-map statistics on the host: the float64 restatement of tests/attn_stats_cases.py against brute-force loops on
crafted maps, the band reductions of ``koemorph_amd.metrics`` against the reference's formulas written out, and the layout of
km_attn_stats_compute's vector.  No GPU."""
import math
import os
import re

import numpy as np

import attn_stats_cases as ac
from koemorph_amd import _lib, metrics, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["km_attn_stats_create", "km_attn_stats_destroy", "km_attn_stats_shape", "km_attn_stats_reset", "km_attn_stats_update",
           "km_attn_stats_compute", "km_forward_audio_attn", "km_forward_clip_attn", "km_sequence_forward_attn"]


def one_map(row, q=ac.Q):
    return np.broadcast_to(np.asarray(row, np.float32), (1, q, row.shape[0])).copy()


def test_crafted_rows_have_the_values_they_were_made_for():
    rows = ac.crafted_rows()
    st = ac.stats_f64(one_map(rows["one_hot"]))
    assert np.array_equal(st["entropy"], np.zeros(ac.Q)) and (st["peak_hist"][:, ac.K - 3] == 1).all() and st["peak_hist"].sum() == ac.Q
    st = ac.stats_f64(one_map(rows["uniform"]))
    # 1 / 80 is not a float32: the entropy of the stored row is ln 80 to the float32 rounding of its entries
    assert np.abs(st["entropy"] - math.log(ac.K)).max() < 1e-6 and (st["peak_hist"][:, 0] == 1).all()
    st = ac.stats_f64(one_map(rows["tie"]))
    assert rows["tie"][17] == rows["tie"][ac.K - 1] == rows["tie"].max()
    assert (st["peak_hist"][:, 17] == 1).all() and st["peak_hist"].sum() == ac.Q                # the lowest key wins
    st = ac.stats_f64(one_map(rows["zeros"]))
    want = -(2 * 0.125 * math.log(0.125) + 0.5 * math.log(0.5) + 0.25 * math.log(0.25))
    assert np.isfinite(st["entropy"]).all() and np.abs(st["entropy"] - want).max() < 1e-15 and (st["peak_hist"][:, 6] == 1).all()


def test_restatement_matches_brute_force_loops():
    for rows, q, k in ((1, 3, 8), (7, 5, 12), (4, ac.Q, ac.K)):
        maps = ac.make_maps(20 + rows, rows, q, k) if k == ac.K else ac.softmax_maps(20 + rows, rows, q, k)
        a, b = ac.stats_f64(maps), ac.brute_force(maps)
        assert a["rows"] == b["rows"] == rows
        assert np.array_equal(a["peak_hist"], b["peak_hist"]) and a["peak_hist"].sum() == rows * q
        assert np.abs(a["mean_map"] - b["mean_map"]).max() <= 1e-15
        assert np.abs(a["entropy"] - b["entropy"]).max() <= 1e-13
    empty = ac.stats_f64(np.zeros((0, 2, 4), np.float32))
    assert empty["rows"] == 0 and not empty["mean_map"].any() and not empty["entropy"].any() and not empty["peak_hist"].any()


def test_band_reductions_are_the_reference_formulas():
    """attention_viz.py:96-98: ``attention_weights[:, indices].mean(axis=1)`` per band; :329-331: ``mel_attention[:, indices].mean()``."""
    bands = metrics.frequency_bands()
    assert bands == {"low": list(range(0, 20)), "mid_low": list(range(20, 40)), "mid_high": list(range(40, 60)), "high": list(range(60, 80))}
    m = synth.uniform(5, (ac.Q, ac.K), 0.0, 1.0).astype(np.float64)
    band_mean, band_share = metrics.band_reductions(m)
    for band, idx in bands.items():
        want = np.array([sum(m[q, j] for j in idx) / len(idx) for q in range(ac.Q)])
        assert np.abs(band_mean[band] - want).max() < 1e-15
        assert abs(band_share[band] - sum(m[q, j] for q in range(ac.Q) for j in idx) / (ac.Q * len(idx))) < 1e-15
    assert abs(sum(band_share.values()) - 4 * m.mean()) < 1e-12


def test_vector_layout_and_unpacking():
    text = open(os.path.join(ROOT, "include", "koemorph.h")).read()
    macro = re.search(r"#define KM_ATTN_STATS_COUNT\(Q, K\) \((.*)\)\n", text).group(1)
    for q, k in ((28, 80), (3, 8), (1, 4)):
        assert eval(macro, {"Q": q, "K": k}) == _lib.km_attn_stats_count(q, k) == ac.count(q, k) == 1 + 2 * q * k + q
    maps = ac.make_maps(9, 3)
    st = ac.stats_f64(maps)
    vec = ac.pack(st)
    assert vec.shape == (ac.count(),) and vec[0] == 3.0
    assert np.array_equal(vec[1:1 + ac.Q * ac.K].reshape(ac.Q, ac.K), st["mean_map"])
    assert np.array_equal(vec[1 + ac.Q * ac.K:1 + ac.Q * ac.K + ac.Q], st["entropy"])
    got = metrics.unpack_attention_stats(vec, ac.Q, ac.K)
    assert set(got) == {"rows", "mean_map", "entropy", "peak_hist", "band_mean", "band_share"}
    assert got["rows"] == 3 and got["peak_hist"].dtype == np.int64 and np.array_equal(got["peak_hist"], st["peak_hist"])
    assert np.array_equal(got["mean_map"], st["mean_map"]) and np.array_equal(got["entropy"], st["entropy"])
    assert got["band_mean"]["mid_low"].shape == (ac.Q,)
    zero = metrics.AttentionStats().compute()                       # before any update: all zero, no device touched
    assert zero["rows"] == 0 and not zero["mean_map"].any() and sum(zero["band_share"].values()) == 0.0


def test_bounds_accept_the_restatement_and_refuse_a_miscount():
    maps = ac.make_maps(11, 7)
    ac.assert_within_bounds(ac.brute_force(maps), maps)
    wrong = ac.stats_f64(maps)
    wrong["mean_map"] = wrong["mean_map"] * (1 + 1e-12)
    try:
        ac.assert_within_bounds(wrong, maps)
    except AssertionError:
        pass
    else:
        raise AssertionError("a mean map off by 1e-12 relative passed the bound")


def test_library_exports_the_attention_entry_points():
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
