"""Evaluation metrics on the host: the float64 restatement against the reference's own output, the CPU path of the
class, the activity threshold, and the C-ABI surface (no GPU).

The fixtures tests/golden/metrics_*.npz hold what the reference's BlendshapeMetrics.compute() and
compute_lip_sync_metrics() returned (tools/gen_metrics_golden.py).  Bound: |f64 - golden| <= 1e-6 * max(|golden|, 1e-3)
per key, the reference's own float32 summation error with a margin of 5 over the worst seen when the bound was set
(1.9e-7).  Worst per case when the fixtures were generated: n8 1.6e-7, n256 1.0e-7, n4096_pieces 1.0e-7, n1 0, n2 1.4e-7,
closed_cols 1.2e-7, all_closed 1.3e-7, threshold 1.1e-7, inactive 6.7e-8, lip_2d 1.3e-7, lip_3d 2.9e-7,
lip_const_energy 2.3e-7.
"""
import os
import re

import numpy as np
import pytest

from metrics_cases import METRICS_CASES, assert_close_to_golden, metrics_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["km_metrics_create", "km_metrics_destroy", "km_metrics_reset", "km_metrics_update", "km_metrics_compute"]


@pytest.mark.parametrize("name", METRICS_CASES)
def test_f64_restatement_matches_the_reference(name):
    from koemorph_amd.metrics import DIAGNOSTIC_KEYS, _energy_host, metrics_f64
    c, pred, target, feats, golden = metrics_case(name)
    got = metrics_f64(pred, target, None if feats is None else _energy_host(feats))
    assert set(got) - set(DIAGNOSTIC_KEYS) == set(golden)
    assert got["rows"] == c["N"]
    assert_close_to_golden(got, golden, name)


def test_fixture_cases_cover_the_edges():
    g = {n: metrics_case(n)[4] for n in METRICS_CASES}
    assert "temporal_consistency" not in g["n1"] and "temporal_consistency" in g["n2"]
    assert g["n1"]["mean_correlation"] == 0.0                                  # std() of one row is NaN: every gate closed
    assert g["all_closed"]["mean_correlation"] == 0.0 and g["all_closed"]["min_correlation"] == 0.0
    assert g["all_closed"]["mouth_correlation"] == 0.0
    assert g["inactive"]["precision"] == 0.0 and g["inactive"]["recall"] == 0.0 and g["inactive"]["f1_score"] == 0.0
    assert g["lip_const_energy"]["audiovisual_sync"] == 0.0
    assert abs(g["lip_2d"]["audiovisual_sync"]) > 0.1 and abs(g["lip_3d"]["audiovisual_sync"]) > 0.1
    assert "audiovisual_sync" not in g["n256"]


def test_closed_columns_are_left_out_of_the_correlation():
    from koemorph_amd.metrics import metrics_f64
    _, pred, target, _, _ = metrics_case("closed_cols")
    assert metrics_f64(pred, target)["valid_correlations"] == 50.0
    _, pred, target, _, _ = metrics_case("all_closed")
    assert metrics_f64(pred, target)["valid_correlations"] == 0.0


@pytest.mark.parametrize("name", METRICS_CASES)
def test_cpu_class_equals_f64_and_pieces_equal_one_update(name):
    import torch
    from koemorph_amd.metrics import BlendshapeMetrics, _energy_host, compute_lip_sync_metrics, metrics_f64
    c, pred, target, feats, golden = metrics_case(name)
    want = metrics_f64(pred, target, None if feats is None else _energy_host(feats))
    one, pieces = BlendshapeMetrics(), BlendshapeMetrics()
    assert one.compute() == {}
    one.update(torch.from_numpy(pred), torch.from_numpy(target), None if feats is None else torch.from_numpy(feats))
    r = 0
    for k in c["split"]:
        pieces.update(pred[r:r + k], target[r:r + k], None if feats is None else feats[r:r + k])     # arrays work too
        r += k
    a, b = one.compute(), pieces.compute()
    assert a == b                                                               # the cross-batch difference is counted
    assert list(a) == [k for k in golden if k in a] and all(a[k] == want[k] for k in a)
    assert set(a) == {k for k in golden if not k.startswith("mouth") and k != "audiovisual_sync"}
    lip = compute_lip_sync_metrics(torch.from_numpy(pred), torch.from_numpy(target),
                                   None if feats is None else torch.from_numpy(feats))
    assert set(lip) == {k for k in golden if k.startswith("mouth") or k == "audiovisual_sync"}
    assert all(lip[k] == want[k] for k in lip)
    one.reset()
    assert one.compute() == {}


def test_activity_threshold_is_float32_point_one():
    from koemorph_amd.metrics import metrics_f64
    at, above = np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(1.0))
    assert float(at) > 0.1                      # float32(0.1) lies ABOVE the double 0.1: a float64 compare would call it active
    p = np.zeros((4, 52), np.float32)
    t = np.zeros((4, 52), np.float32)
    p[:, 0], p[:, 1] = at, above
    t[:, 1], t[:, 2] = above, at
    m = metrics_f64(p, t)
    assert m["pred_activity"] == 4 / 208 and m["target_activity"] == 4 / 208
    assert abs(m["precision"] - 1.0) < 1e-8 and abs(m["recall"] - 1.0) < 1e-8


def test_wrong_shapes_raise():
    from koemorph_amd.metrics import BlendshapeMetrics
    m = BlendshapeMetrics()
    with pytest.raises(ValueError):
        m.update(np.zeros((4, 51), np.float32), np.zeros((4, 51), np.float32))
    with pytest.raises(ValueError):
        m.update(np.zeros((4, 52), np.float32), np.zeros((5, 52), np.float32))
    with pytest.raises(ValueError):
        m.update(np.zeros((4, 52), np.float32), np.zeros((4, 52), np.float32), np.zeros((3, 80), np.float32))


def test_header_declares_and_library_exports_the_metrics_symbols():
    from koemorph_amd import _lib
    text = open(os.path.join(ROOT, "include", "koemorph.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} is not declared in koemorph.h"
        assert s in _lib.SIGNATURES and hasattr(lib, s), f"{s} is not exported"
    n = int(re.search(r"#define\s+KM_METRICS_COUNT\s+(\d+)", code).group(1))
    assert n == _lib.KM_METRICS_COUNT == len(_lib.KM_METRICS_NAMES)
    for i, k in enumerate(_lib.KM_METRICS_NAMES):                               # the header documents every index
        assert re.search(r"\b%d %s\b" % (i, k), text), f"index {i} ({k}) is not documented in koemorph.h"
    assert lib.km_abi_version() == 2
