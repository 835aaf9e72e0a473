"""Host half of the loss-by-component tests (km_loss_terms_* / koemorph_amd.metrics.LossTerms): the case table, the
float64 restatement and the fixtures' inputs, shared with tests/test_gpu_loss_terms.py.  Nothing here needs a GPU.

The restatement is ``oracle.core.koemorph_loss`` (and ``dual_stream_loss``) evaluated TERM BY TERM on float64 tensors: one
call per term with that term's weight 1 and every other weight 0.

Golden gap.  ``tests/golden/core_*_fullloss*.npz`` hold the reference ``KoeMorphLoss``'s own ``metrics`` dict, reduced in
float32 by torch on the CPU.  ``golden_gap`` measures, per term, |float64 restatement - golden| / max(|golden|, 1e-3) on the
fixture's own prediction; the GPU test allows that measured gap + 2^-22.  Observed (printed by
test_float64_restatement_against_the_reference_terms): at most 1.21e-7 for a single term over the four fixtures (sparsity
of core_d64_T32_H4_fullloss; landmark of core_d256_T256_H8_fullloss 1.13e-7) and 1.26e-7 for the total (core_d256_T256_H8_fullloss),
i.e. about one float32 ulp; the worst-case bound asserted here is n * 2^-24 for the longest reduction, n = 8 * 136
landmark products.
"""
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, full_loss_inputs, load_golden
from koemorph_amd import synth
from koemorph_amd._lib import KM_LOSS_TERM_NAMES, KM_LOSS_TERMS
from koemorph_amd.metrics import LOSS_TERM_DEFAULT_WEIGHTS
from oracle import core as ocore

FULLLOSS_FIXTURES = ["core_d64_T32_H4_fullloss", "core_d256_T256_H8_fullloss", "core_d64_T32_H4_fullloss_av",
                     "core_d256_T256_H8_train_fullloss_av"]
KOEMORPH_TERMS = ("mse", "l1", "perceptual", "temporal", "velocity", "sparsity", "smoothness", "landmark")
FLOOR = 1e-3                     # the floor convention of tests/metrics_cases.py: |x - ref| <= rtol * max(|ref|, 1e-3)
F64_RTOL = 2.0 ** -23            # GPU float64 sums rounded once to float32, against the float64 restatement
OUT_RTOL = 2.0 ** -22            # the float32 output rounding on top of the measured golden gap

# (name, N, which optional inputs are present, extra_terms): the float64-restatement cases of the GPU test
F64_CASES = [
    ("n1", 1, ("prev", "landmark"), True),
    ("n2", 2, ("prev", "landmark"), True),
    ("n5", 5, ("prev", "landmark", "energy"), True),
    ("n8", 8, ("prev", "landmark"), True),
    ("n256", 256, ("prev", "landmark", "energy"), True),
    ("n5_no_prev", 5, ("landmark",), True),
    ("n5_no_landmark", 5, ("prev",), True),
    ("n5_cfg_null", 5, (), False),
    ("n5_dual_stream", 5, ("ds_prev",), True),
    ("n8_dual_stream_no_prev", 8, (), True),
]
DS_WEIGHTS = dict(mse_weight=0.1, l1_weight=1.0, perceptual_weight=0.0, temporal_weight=0.0, sparsity_weight=0.0, smoothness_weight=0.0,
                  landmark_weight=0.0, velocity_weight=0.0, ds_velocity_weight=0.05, ds_separation_weight=0.01)


def case_inputs(name):
    """Seeded (N, 52) rows in [0, 1] and the optional inputs the case names."""
    _, n, have, extra = next(c for c in F64_CASES if c[0] == name)
    seed = 9000 + 13 * [c[0] for c in F64_CASES].index(name)
    d = {"pred": synth.uniform(seed, (n, 52), 0.0, 1.0), "target": synth.uniform(seed + 1, (n, 52), 0.0, 1.0)}
    if "prev" in have:
        d["prev_pred"], d["prev_target"] = synth.uniform(seed + 2, (n, 52), 0.0, 1.0), synth.uniform(seed + 3, (n, 52), 0.0, 1.0)
    if "landmark" in have:
        d["landmark_w"] = (0.01 * synth.normal(seed + 4, (136, 52))).astype(np.float32)
    if "energy" in have:
        d["audio_energy"] = synth.uniform(seed + 5, (n,), 0.2, 2.0).astype(np.float32)
    if "ds_prev" in have:
        d["ds_prev_pred"] = synth.uniform(seed + 6, (n, 52), 0.0, 1.0)
    weights = dict(DS_WEIGHTS) if "dual_stream" in name else dict(LOSS_TERM_DEFAULT_WEIGHTS)
    return d, weights, extra


def energy_of(features):
    """Per-row energy of (B, T, D) audio features, float64 -> float32 (losses.py:352-358)."""
    f = np.asarray(features, np.float64)
    return np.sqrt((f * f).sum(-1)).mean(-1).astype(np.float32)


def fixture_inputs(name):
    """The fixture's own prediction and the other inputs rebuilt from its seed; the reference's terms and loss."""
    g = load_golden(name)
    c = g["config"]
    target, prev_pred, prev_target, lw = full_loss_inputs(c["seed"], c["B"])
    d = {"pred": g["train_blendshapes"] if "train_blendshapes" in g else g["blendshapes"], "target": target, "prev_pred": prev_pred,
         "prev_target": prev_target, "landmark_w": lw}
    if name.endswith("_av"):
        d["audio_energy"] = energy_of(synth.make_av_features(c["seed"], c["B"]))
    golden = {k: float(g["metric/" + k]) for k in KOEMORPH_TERMS}
    golden["total"] = float(g["loss"])
    return d, golden


def terms_f64(pred, target, prev_pred=None, prev_target=None, landmark_w=None, audio_energy=None, ds_prev_pred=None, weights=None,
              extra_terms=True):
    """{term: float64 value} for every KM_LOSS_TERM_NAMES entry + "row_smoothness": oracle.core.koemorph_loss with one weight
    at 1 and the others at 0, per term; a term whose input is missing is 0.  ``audio_energy`` (N) enters as (N, 1) features,
    whose norm over the last axis is the energy itself."""
    w = {**LOSS_TERM_DEFAULT_WEIGHTS, **(weights or {})}
    t64 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float32)).double()
    p, t = t64(pred), t64(target)
    kw = dict(prev_pred=t64(prev_pred), prev_target=t64(prev_target), landmark_w=t64(landmark_w),
              audio_features=None if audio_energy is None else t64(audio_energy).reshape(-1, 1))
    zero = {k + "_weight": 0.0 for k in KOEMORPH_TERMS}
    out = {k: 0.0 for k in KM_LOSS_TERM_NAMES}
    have_prev = prev_pred is not None and prev_target is not None
    for k in KOEMORPH_TERMS:
        if k not in ("mse", "l1") and not extra_terms:
            continue
        if (k in ("temporal", "velocity") and not have_prev) or (k == "landmark" and landmark_w is None):
            continue
        out[k] = float(ocore.koemorph_loss(p, t, **{**zero, k + "_weight": 1.0}, **kw))
    if extra_terms:
        ds0 = dict(l1_weight=0.0, l2_weight=0.0, velocity_weight=0.0, stream_separation_weight=0.0)
        if ds_prev_pred is not None:
            out["ds_velocity"] = float(ocore.dual_stream_loss(p, t, **{**ds0, "velocity_weight": 1.0}, prev_predictions=t64(ds_prev_pred)))
        if w["ds_separation_weight"] > 0:
            out["ds_separation"] = float(ocore.dual_stream_loss(p, t, **{**ds0, "stream_separation_weight": 1.0}))
    out["total"] = sum(float(np.float32(w[k + "_weight"])) * out[k] for k in KM_LOSS_TERM_NAMES if k != "total")
    out["row_smoothness"] = float(torch.diff(p, dim=1).abs().mean(dim=1).mean())
    return out


def rel(x, ref):
    return abs(x - ref) / max(abs(ref), FLOOR)


def golden_gap(name):
    """{term: |float64 restatement - reference| / max(|reference|, FLOOR)} on the fixture's own prediction."""
    d, golden = fixture_inputs(name)
    f64 = terms_f64(**d)
    return {k: rel(f64[k], ref) for k, ref in golden.items()}


def assert_terms_close(got, ref, rtol, what, keys=None):
    keys = list(keys if keys is not None else ref)
    for k in keys:
        tol = rtol[k] if isinstance(rtol, dict) else rtol
        print(f"{what} {k}: got {got[k]!r} ref {ref[k]!r} rel {rel(got[k], ref[k]):.3e} allowed {tol:.3e}")
    for k in keys:
        tol = rtol[k] if isinstance(rtol, dict) else rtol
        assert rel(got[k], ref[k]) <= tol, (what, k, got[k], ref[k])


# ---- host tests ------------------------------------------------------------------------------------------------------------
def test_term_order_is_published_in_the_header_and_mirrored_in_python():
    text = open(ROOT + "/include/koemorph.h").read()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"KM_LOSS_TERM_([A-Z0-9_]+) = (\d+)", text)}
    assert enum == {k: i for i, k in enumerate(KM_LOSS_TERM_NAMES)}
    assert int(re.search(r"#define KM_LOSS_TERMS (\d+)", text).group(1)) == KM_LOSS_TERMS == len(KM_LOSS_TERM_NAMES)
    assert KM_LOSS_TERM_NAMES[:8] == KOEMORPH_TERMS and KM_LOSS_TERM_NAMES[-1] == "total"
    assert set(LOSS_TERM_DEFAULT_WEIGHTS) == {k + "_weight" for k in KM_LOSS_TERM_NAMES if k != "total"}


@pytest.mark.parametrize("name", FULLLOSS_FIXTURES)
def test_float64_restatement_against_the_reference_terms(name):
    """The measured gap the GPU test builds its tolerance from, printed; bounded here by the worst case of a float32
    reduction of the longest term (8 * 136 landmark products): n * 2^-24.  The weighted total of the restated terms is
    koemorph_loss with the default weights."""
    gap = golden_gap(name)
    for k, v in gap.items():
        print(f"{name} {k}: float64 restatement vs reference, relative gap {v:.3e}")
    assert max(gap.values()) <= 8 * 136 * 2.0 ** -24
    d, _ = fixture_inputs(name)
    f64 = terms_f64(**d)
    t64 = lambda a: torch.from_numpy(a).double()
    whole = float(ocore.koemorph_loss(t64(d["pred"]), t64(d["target"]), prev_pred=t64(d["prev_pred"]), prev_target=t64(d["prev_target"]),
                                      landmark_w=t64(d["landmark_w"]),
                                      audio_features=t64(d["audio_energy"]).reshape(-1, 1) if "audio_energy" in d else None))
    assert abs(f64["total"] - whole) <= 1e-7 * abs(whole)        # the weights are float32(0.1) ... on one side, doubles on the other


@pytest.mark.parametrize("name", [c[0] for c in F64_CASES])
def test_case_table_skips(name):
    d, weights, extra = case_inputs(name)
    f64 = terms_f64(**d, weights=weights, extra_terms=extra)
    assert (f64["temporal"] != 0.0) == ("prev_pred" in d) == (f64["velocity"] != 0.0)
    assert (f64["landmark"] != 0.0) == ("landmark_w" in d)
    assert (f64["ds_velocity"] != 0.0) == ("ds_prev_pred" in d)
    assert (f64["ds_separation"] != 0.0) == ("dual_stream" in name)
    assert (f64["perceptual"] != 0.0) == extra and f64["mse"] > 0 and f64["l1"] > 0
