"""The loss by component on the device (km_loss_terms_* / koemorph_amd.metrics.LossTerms) against the reference's own
per-term output, the float64 restatement, itself (accumulation, determinism, graph replay) and the training tail.

Tolerances.  Against the float64 restatement (tests/test_loss_terms_host.py: oracle.core.koemorph_loss term by term):
2^-23 relative with the floor of tests/metrics_cases.py -- the kernels sum in float64 and round each term once to float32.
Against the reference's float32 ``metrics`` in the fullloss fixtures: the gap between that restatement and the fixture,
measured on the CPU in this test, + 2^-22.  The CPU-measured gap is at most 1.21e-7 for a term and 1.26e-7 for the total
(tests/test_loss_terms_host.py lists them); every test prints the figures it compares before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_loss_terms_host as lh
from conftest import golden_case, full_loss_inputs
from koemorph_amd import synth
from koemorph_amd._lib import KM_ABI_VERSION, KM_ERR_INVALID_ARG, KM_LOSS_TERM_NAMES, KM_LOSS_TERMS, KMLossConfig, load
from koemorph_amd.engine import Engine
from koemorph_amd.metrics import LossTerms
from koemorph_amd.training import Trainer

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def one_update(d, weights=None, extra_terms=True):
    """One update on a fresh accumulator: ({term: float32 value of the batch}, compute())."""
    lt = LossTerms(**(weights or {}))
    terms = lt.update(**{k: dev(v) for k, v in d.items()}, extra_terms=extra_terms)
    m = lt.compute()
    lt.close()
    return {k: float(v) for k, v in zip(KM_LOSS_TERM_NAMES, terms.cpu().numpy())}, m


@pytest.mark.parametrize("name", lh.FULLLOSS_FIXTURES)
def test_terms_match_the_reference_koemorph_loss(name):
    """The fixture's own prediction, KoeMorphLoss's default weights: every term against metric/<term>, the weighted total
    against loss, within the CPU-measured gap of the float64 restatement + 2^-22."""
    d, golden = lh.fixture_inputs(name)
    gap = lh.golden_gap(name)
    got, m = one_update(d)
    lh.assert_terms_close(got, golden, {k: gap[k] + lh.OUT_RTOL for k in golden}, name)
    assert m["updates"] == 1.0 and all(m[k] == got[k] for k in KM_LOSS_TERM_NAMES)      # one update: its mean is itself


@pytest.mark.parametrize("name", [c[0] for c in lh.F64_CASES])
def test_terms_match_the_float64_restatement(name):
    """N = 1, 2, 5, 8, 256 (one wave, several workgroups), the missing-input skips (no prev_*, no landmark_w, cfg = NULL) and
    DualStreamLoss's two terms against oracle.core.dual_stream_loss; a skipped term reports exactly 0."""
    d, weights, extra = lh.case_inputs(name)
    ref = lh.terms_f64(**d, weights=weights, extra_terms=extra)
    got, m = one_update(d, weights, extra)
    got["row_smoothness"] = m["row_smoothness"]
    lh.assert_terms_close(got, ref, lh.F64_RTOL, name)
    for k in KM_LOSS_TERM_NAMES:
        if ref[k] == 0.0:
            assert got[k] == 0.0 and m[k] == 0.0, k


def test_three_updates_then_compute_and_reset():
    """compute = the mean over updates of the per-batch values (a skipped term's update does not count in its mean), the row
    smoothness a mean over ROWS; reset clears the accumulator."""
    lt = LossTerms()
    per, rows = [], []
    for name in ("n5", "n8", "n5_no_prev"):
        d, _, _ = lh.case_inputs(name)
        per.append(lt.update(**{k: dev(v) for k, v in d.items()}).cpu().numpy().astype(np.float64))
        rows.append(d["pred"])
    m = lt.compute()
    assert m["updates"] == 3.0
    for i, k in enumerate(KM_LOSS_TERM_NAMES):
        counted = [p[i] for j, p in enumerate(per) if not (k in ("temporal", "velocity") and j == 2)]
        want = float(np.mean(counted)) if k not in ("ds_velocity", "ds_separation") else 0.0
        assert lh.rel(m[k], want) <= lh.OUT_RTOL, (k, m[k], want)        # float32 per-batch values averaged in float64 here
    allrows = np.concatenate(rows).astype(np.float64)
    assert lh.rel(m["row_smoothness"], float(np.abs(np.diff(allrows, axis=1)).mean(axis=1).mean())) <= lh.F64_RTOL
    lt.reset()
    assert lt.compute() == {}
    d, _, _ = lh.case_inputs("n2")
    t = lt.update(**{k: dev(v) for k, v in d.items()}).cpu().numpy()
    m = lt.compute()
    assert m["updates"] == 1.0 and all(m[k] == float(t[i]) for i, k in enumerate(KM_LOSS_TERM_NAMES))
    lt.close()


def test_two_identical_runs_are_bit_equal():
    outs = []
    for _ in range(2):
        lt = LossTerms()
        ts = []
        for name in ("n256", "n5", "n1"):
            d, _, _ = lh.case_inputs(name)
            ts.append(lt.update(**{k: dev(v) for k, v in d.items()}).cpu().numpy())
        lib, out = load(), torch.empty(KM_LOSS_TERMS + 2, device="cuda")
        assert lib.km_loss_terms_compute(lt._acc, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        outs.append(np.concatenate(ts + [out.cpu().numpy()]))
        lt.close()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_captured_update_equals_eager():
    d, _, _ = lh.case_inputs("n8")
    t = {k: dev(v) for k, v in d.items()}
    eager, graphed = LossTerms(), LossTerms()
    want = eager.update(**t).clone()
    graphed.update(**t)                                      # opens the accumulator outside the capture
    graphed.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = graphed.update(**t)
    g.replay(); g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    m = graphed.compute()
    assert m["updates"] == 2.0 and m["total"] == float(want[KM_LOSS_TERM_NAMES.index("total")])
    eager.close(); graphed.close()


def test_total_agrees_with_the_training_tail():
    """One Trainer.forward_backward_mel step, dropout 0, all eight KoeMorphLoss terms on: the step's own prediction fed to
    update gives the step's loss within 2^-22 relative (the tail sums in float32)."""
    c, params, (mel, short, emo), g = golden_case("core_d256_T256_H8_fullloss")
    target, prev_pred, prev_target, lw = full_loss_inputs(c["seed"], c["B"])
    e = Engine(d_model=c["d"], num_heads=c["H"], mel_sequence_length=c["T"])
    e.load_state_dict(params)
    e.finalize()
    tr = Trainer(e, max_windows=c["B"], use_smoothing=False, mse_weight=1.0, l1_weight=0.1, dropout=0.0)
    w = dict(perceptual_weight=0.5, temporal_weight=0.2, sparsity_weight=0.01, smoothness_weight=0.1, landmark_weight=0.3, velocity_weight=0.05)
    tr.set_loss_terms(**w, prev_pred=dev(prev_pred), prev_target=dev(prev_target), landmark_weights=dev(lw))
    loss = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    lt = LossTerms(mse_weight=1.0, l1_weight=0.1, **w)
    terms = lt.update(tr.out[:c["B"]], dev(target), prev_pred=dev(prev_pred), prev_target=dev(prev_target), landmark_w=dev(lw))
    total = float(terms[KM_LOSS_TERM_NAMES.index("total")].item())
    print(f"training tail loss {loss!r}, LossTerms total {total!r}, relative {abs(total - loss) / abs(loss):.3e}")
    assert abs(total - loss) <= 2.0 ** -22 * abs(loss)
    lt.close()


def test_wrong_abi_version_and_bad_arguments_are_refused():
    lib, st = load(), torch.cuda.current_stream().cuda_stream
    acc = ctypes.c_void_p()
    assert lib.km_loss_terms_create(ctypes.byref(acc)) == 0
    p, t = dev(synth.uniform(1, (4, 52), 0, 1)), dev(synth.uniform(2, (4, 52), 0, 1))
    cfg = KMLossConfig(KM_ABI_VERSION - 1, 0.5, 0.2, 0.01, 0.1, 0.3, 0.05, None, None, None, None, 0.0, 0.0, None)
    assert lib.km_loss_terms_update(acc, ctypes.byref(cfg), 1.0, 0.1, p.data_ptr(), t.data_ptr(), 4, None, st) == KM_ERR_INVALID_ARG
    assert b"abi_version" in lib.km_last_error()
    cfg.abi_version = KM_ABI_VERSION
    assert lib.km_loss_terms_update(acc, ctypes.byref(cfg), 1.0, 0.1, p.data_ptr(), t.data_ptr(), 0, None, st) == KM_ERR_INVALID_ARG
    assert lib.km_loss_terms_update(acc, ctypes.byref(cfg), 1.0, 0.1, None, t.data_ptr(), 4, None, st) == KM_ERR_INVALID_ARG
    assert lib.km_loss_terms_update(None, ctypes.byref(cfg), 1.0, 0.1, p.data_ptr(), t.data_ptr(), 4, None, st) == KM_ERR_INVALID_ARG
    assert lib.km_loss_terms_compute(acc, None, st) == KM_ERR_INVALID_ARG
    out = torch.full((KM_LOSS_TERMS + 2,), -1.0, device="cuda")
    assert lib.km_loss_terms_compute(acc, out.data_ptr(), st) == 0          # nothing was folded in by the refused calls
    assert torch.count_nonzero(out).item() == 0
    assert lib.km_loss_terms_update(acc, ctypes.byref(cfg), 1.0, 0.1, p.data_ptr(), t.data_ptr(), 4, None, st) == 0   # terms_dev = NULL
    assert lib.km_loss_terms_compute(acc, out.data_ptr(), st) == 0
    assert out[KM_LOSS_TERMS].item() == 1.0 and out[0].item() > 0
    torch.cuda.synchronize()
    assert lib.km_loss_terms_destroy(acc) == 0
    with pytest.raises(TypeError):
        LossTerms(mse=1.0)
