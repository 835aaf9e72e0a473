"""Shared by tests/test_metrics_host.py and tests/test_gpu_metrics.py: the metrics fixtures and their inputs."""
import numpy as np

from conftest import load_golden

METRICS_CASES = ["n8", "n256", "n4096_pieces", "n1", "n2", "closed_cols", "all_closed", "threshold", "inactive",
                 "lip_2d", "lip_3d", "lip_const_energy"]
GOLDEN_RTOL, GOLDEN_FLOOR = 1e-6, 1e-3          # |x - golden| <= 1e-6 * max(|golden|, 1e-3)


def metrics_case(name):
    """(config, pred, target, features or None, {key: golden float32}) regenerated from the fixture's seeds."""
    from koemorph_amd import synth
    g = load_golden("metrics_" + name)
    c = g["config"]
    pred, target = synth.make_metrics_inputs(c["seed"], c["N"], c["style"])
    feats = synth.make_metrics_features(c["seed"], c["N"], c["features"], pred) if c["features"] else None
    cs = synth.metrics_inputs_checksum(pred, target, feats)
    assert abs(cs - float(g["input_checksum"])) <= 1e-9 * abs(cs), "synthetic input generator drifted from the fixtures"
    return c, pred, target, feats, {k[len("metric/"):]: float(v) for k, v in g.items() if k.startswith("metric/")}


def assert_close_to_golden(got, golden, what):
    for k, ref in golden.items():
        print(f"{what} {k}: got {got[k]!r} golden {ref!r} rel {abs(got[k] - ref) / max(abs(ref), GOLDEN_FLOOR):.3e}")
    for k, ref in golden.items():
        assert abs(got[k] - ref) <= GOLDEN_RTOL * max(abs(ref), GOLDEN_FLOOR), (what, k, got[k], ref)
