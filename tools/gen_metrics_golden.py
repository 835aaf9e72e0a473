"""Fixtures tests/golden/metrics_<case>.npz from the reference's own BlendshapeMetrics / compute_lip_sync_metrics.

Development machine only: needs a checkout of the reference (atsuki-ichikawa/KoeMorph) and torch on the CPU.

    python tools/gen_metrics_golden.py --reference /path/to/KoeMorph [--out tests/golden]

Each file holds a JSON `config` (seed, N, split, style, features), `input_checksum` of the inputs regenerated from the
seeds (koemorph_amd.synth.make_metrics_inputs / make_metrics_features) and one float32 per key the reference returned,
stored as `metric/<key>`: BlendshapeMetrics fed in the uneven pieces of `split`, compute_lip_sync_metrics on the whole
input.  The script also prints, per case, the worst relative difference between the reference and
koemorph_amd.metrics.metrics_f64 -- the number tests/test_metrics_host.py quotes -- and refuses inputs whose gated standard
deviations are neither exactly constant nor >= 1e-4 (the reference evaluates its 1e-6 gate in float32).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from koemorph_amd import synth  # noqa: E402
from koemorph_amd.metrics import DIAGNOSTIC_KEYS, _energy_host, metrics_f64  # noqa: E402

CASES = {
    "n8": dict(seed=11, N=8, split=[8], style="plain", features=None),
    "n256": dict(seed=12, N=256, split=[256], style="plain", features=None),
    "n4096_pieces": dict(seed=13, N=4096, split=[1, 700, 63, 3000, 332], style="plain", features=None),
    "n1": dict(seed=14, N=1, split=[1], style="plain", features=None),
    "n2": dict(seed=15, N=2, split=[1, 1], style="plain", features=None),
    "closed_cols": dict(seed=16, N=300, split=[100, 200], style="closed_cols", features=None),
    "all_closed": dict(seed=17, N=120, split=[120], style="all_closed", features=None),
    "threshold": dict(seed=18, N=512, split=[5, 507], style="threshold", features=None),
    "inactive": dict(seed=19, N=64, split=[64], style="inactive", features=None),
    "lip_2d": dict(seed=20, N=200, split=[50, 150], style="plain", features="2d"),
    "lip_3d": dict(seed=21, N=200, split=[200], style="plain", features="3d"),
    "lip_const_energy": dict(seed=22, N=96, split=[96], style="plain", features="const"),
}


def assert_margin(name, what, x):
    """A gated standard deviation is exactly 0 (constant input) or >= 1e-4: never near the float32 gate at 1e-6."""
    x = np.asarray(x, np.float64)
    if x.shape[0] < 2 or np.all(x == x[0]):
        return
    s = x.std(ddof=1)
    assert s >= 1e-4, f"{name}: std of {what} is {s:.3e}, inside the margin around the 1e-6 gate"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("KOEMORPH_REFERENCE"), help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or KOEMORPH_REFERENCE) is required")
    sys.path.insert(0, args.reference)
    import torch
    from src.model.losses import BlendshapeMetrics, compute_lip_sync_metrics

    for name, cfg in CASES.items():
        pred, target = synth.make_metrics_inputs(cfg["seed"], cfg["N"], cfg["style"])
        feats = synth.make_metrics_features(cfg["seed"], cfg["N"], cfg["features"], pred) if cfg["features"] else None
        assert sum(cfg["split"]) == cfg["N"]
        for c in range(52):
            assert_margin(name, f"pred column {c}", pred[:, c])
            assert_margin(name, f"target column {c}", target[:, c])
        assert_margin(name, "pred mouth activity", pred[:, 12:32].astype(np.float64).sum(1))
        assert_margin(name, "target mouth activity", target[:, 12:32].astype(np.float64).sum(1))
        energy = None if feats is None else _energy_host(feats)
        if energy is not None:
            assert_margin(name, "audio energy", energy)

        bm = BlendshapeMetrics()
        r = 0
        for k in cfg["split"]:
            bm.update(torch.from_numpy(pred[r:r + k]), torch.from_numpy(target[r:r + k]),
                      None if feats is None else torch.from_numpy(feats[r:r + k]))
            r += k
        ref = dict(bm.compute())
        ref.update(compute_lip_sync_metrics(torch.from_numpy(pred), torch.from_numpy(target),
                                            None if feats is None else torch.from_numpy(feats)))
        ours = metrics_f64(pred, target, energy)
        assert set(ours) - set(DIAGNOSTIC_KEYS) == set(ref), (name, sorted(set(ours) ^ set(ref)))
        worst, worst_key = 0.0, ""
        for k, v in ref.items():
            rel = abs(ours[k] - np.float32(v)) / max(abs(float(np.float32(v))), 1e-3)
            if rel > worst:
                worst, worst_key = rel, k
        print(f"{name:18s} N={cfg['N']:5d} keys={len(ref):2d} worst |f64 - reference| / max(|reference|, 1e-3) = {worst:.2e} ({worst_key})")
        rec = {"config": np.array(json.dumps(cfg)),
               "input_checksum": np.float64(synth.metrics_inputs_checksum(pred, target, feats))}
        for k, v in ref.items():
            rec["metric/" + k] = np.float32(v)
        np.savez(os.path.join(args.out, f"metrics_{name}.npz"), **rec)


if __name__ == "__main__":
    main()
