"""km_metrics_* on the MI355X, through the C-ABI, against koemorph_amd.metrics.metrics_f64 on the same inputs.

Bound: |dev - f64| <= 2^-23 * max(|f64|, 2^-20) per key.  Derived, not measured: every sum is float64 over float32 inputs
(relative error about N * 2^-53, negligible up to 10^6 rows), the finalisation is float64 and the single rounding to
float32 costs 2^-24; a factor 2 allows a different but equally valid order of the last few float64 operations.  Counts
(rows, valid_correlations, activity x rows x 52) are exact.  Against the fixtures of the reference's own output the bound
is the host test's: 1e-6 * max(|golden|, 1e-3).
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from koemorph_amd import synth
from koemorph_amd._lib import KM_METRICS_COUNT, KM_METRICS_NAMES, check, load
from koemorph_amd.metrics import (DIAGNOSTIC_KEYS, LIP_SYNC_KEYS, REFERENCE_KEYS, TEMPORAL_KEYS, BlendshapeMetrics,
                                  compute_lip_sync_metrics, metrics_f64)
from metrics_cases import METRICS_CASES, assert_close_to_golden, metrics_case

pytestmark = pytest.mark.gpu

RTOL, FLOOR = 2.0 ** -23, 2.0 ** -20


class Acc:
    """One accumulator driven through the C-ABI on the current stream."""

    def __init__(self):
        self.lib, self.h = load(), C.c_void_p()
        check(self.lib.km_metrics_create(C.byref(self.h)))
        self.keep = []

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def update(self, pred, target, energy=None):
        self.keep += [pred, target, energy]
        check(self.lib.km_metrics_update(self.h, pred.data_ptr(), target.data_ptr(), 0 if energy is None else energy.data_ptr(),
                                         pred.shape[0], self.stream()))

    def compute_dev(self, out=None):
        out = torch.empty(KM_METRICS_COUNT, device="cuda") if out is None else out
        check(self.lib.km_metrics_compute(self.h, out.data_ptr(), self.stream()))
        return out

    def compute(self):
        v = self.compute_dev().cpu().numpy()
        return dict(zip(KM_METRICS_NAMES, (float(x) for x in v))), v

    def reset(self):
        check(self.lib.km_metrics_reset(self.h, self.stream()))

    def close(self):
        torch.cuda.synchronize()
        check(self.lib.km_metrics_destroy(self.h))


@pytest.fixture
def acc():
    a = Acc()
    yield a
    a.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def energy_dev(feats):
    """km_audio_energy of (N, D) or (N, T, D) features: the float32 values the accumulator is fed, on the device."""
    f = dev(feats if feats.ndim == 3 else feats[:, None, :])
    e = torch.empty(f.shape[0], device="cuda")
    check(load().km_audio_energy(f.data_ptr(), f.shape[0], f.shape[1], f.shape[2], e.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return e


def assert_matches_f64(got, want, what, n):
    """Device vector (as a dict) against metrics_f64: prints every figure, then asserts the derived bound."""
    lines = []
    for k, w in want.items():
        lines.append(f"{what} {k}: dev {got[k]!r} f64 {w!r} err/bound {abs(got[k] - w) / (RTOL * max(abs(w), FLOOR)):.3f}")
    print("\n".join(lines))
    assert got["rows"] == n and got["valid_correlations"] == want["valid_correlations"]
    for k, w in want.items():
        assert abs(got[k] - w) <= RTOL * max(abs(w), FLOOR), (what, k, got[k], w)
    if n < 2:
        assert all(got[k] == 0.0 for k in TEMPORAL_KEYS)
    if "audiovisual_sync" not in want:
        assert got["audiovisual_sync"] == 0.0 and got["has_energy"] == 0.0
    else:
        assert got["has_energy"] == 1.0


def run_pieces(acc, pred, target, pieces, energy=None):
    p, t = dev(pred), dev(target)
    r = 0
    for k in pieces:
        acc.update(p[r:r + k], t[r:r + k], None if energy is None else energy[r:r + k])
        r += k
    assert r == pred.shape[0]
    return acc.compute()


@pytest.mark.parametrize("name", METRICS_CASES)
def test_golden_cases_on_the_device(name, acc):
    c, pred, target, feats, golden = metrics_case(name)
    e = None if feats is None else energy_dev(feats)
    got, _ = run_pieces(acc, pred, target, c["split"], e)
    want = metrics_f64(pred, target, None if e is None else e.cpu().numpy())
    assert_matches_f64(got, want, name, c["N"])
    cells = c["N"] * 52
    p32, t32 = pred > np.float32(0.1), target > np.float32(0.1)
    assert round(got["pred_activity"] * cells) == int(p32.sum()) and round(got["target_activity"] * cells) == int(t32.sum())
    assert_close_to_golden(got, golden, name)


def test_near_constant_column_needs_centred_sums(acc):
    """A column at 0.7 +- 3e-6: std about 2e-6, so the gate is open, and mean^2 / var is 5e10 -- raw float64 moments keep
    about five digits of its correlation."""
    N = 65536
    pred, target = synth.make_metrics_inputs(31, N, "plain")
    wiggle = 3e-6 * (2.0 * synth.uniform01(32, N) - 1.0)
    noise = 1.5e-6 * (2.0 * synth.uniform01(33, N) - 1.0)
    pred[:, 7] = (0.7 + wiggle).astype(np.float32)
    target[:, 7] = (0.7 + wiggle + noise).astype(np.float32)
    assert pred[:, 7].astype(np.float64).std(ddof=1) > 1.5e-6 and target[:, 7].astype(np.float64).std(ddof=1) > 1.5e-6
    # isolate the column's correlation: every other column constant (gate closed), so mean = min = that correlation
    for c in range(52):
        if c != 7:
            pred[:, c] = np.float32(0.01 * c)
    got, _ = run_pieces(acc, pred, target, [N])
    want = metrics_f64(pred, target)
    print("near-constant column: dev", got["mean_correlation"], "f64", want["mean_correlation"])
    assert want["valid_correlations"] == 1.0 and got["valid_correlations"] == 1.0 and abs(want["mean_correlation"]) > 0.1
    assert abs(got["mean_correlation"] - want["mean_correlation"]) <= 1e-6
    assert abs(got["min_correlation"] - want["min_correlation"]) <= 1e-6


def test_chunking_and_the_carried_row(acc):
    N = 10000
    pred, target = synth.make_metrics_inputs(41, N, "plain")
    want = metrics_f64(pred, target)
    uneven = [1, 7, 64, 4097, 2, 513, 1000, 4316]
    assert sum(uneven) == N
    for what, pieces in (("one call", [N]), ("uneven", uneven), ("rows one by one", [1] * N)):
        acc.reset()
        got, _ = run_pieces(acc, pred, target, pieces)
        assert_matches_f64(got, want, what, N)
    # resetting between pieces loses the differences across the boundaries: the carried row is what closes them
    p, t = dev(pred), dev(target)
    sums, r = np.zeros(3), 0
    for k in [2500] * 4:
        acc.reset()
        acc.update(p[r:r + k], t[r:r + k])
        m, _ = acc.compute()
        sums += np.array([m[key] for key in TEMPORAL_KEYS]) * (k - 1) * 52
        r += k
    for i, key in enumerate(TEMPORAL_KEYS):
        with_carry, without = want[key] * (N - 1) * 52, sums[i]
        assert with_carry - without > 0.5 * 3 * 52 * want[key], (key, with_carry, without)     # 3 boundaries x 52 columns


def test_run_to_run_bits():
    pred, target = synth.make_metrics_inputs(42, 100000, "plain")
    p, t = dev(pred), dev(target)
    outs = []
    for _ in range(2):
        a = Acc()
        a.update(p, t)
        outs.append(a.compute()[1])
        a.close()
    assert outs[0].tobytes() == outs[1].tobytes()


def test_reset_reuse_and_compute_leaves_the_state(acc):
    pred, target = synth.make_metrics_inputs(43, 300, "plain")
    p, t = dev(pred), dev(target)
    empty = acc.compute()[1]
    assert not empty.any()                                           # before any row: all zero (the reference returns {})
    check(acc.lib.km_metrics_update(acc.h, 0, 0, 0, 0, acc.stream()))   # N = 0 is a no-op, even without rows
    assert not acc.compute()[1].any()
    acc.update(p[:100], t[:100])
    first = acc.compute()[0]
    assert_matches_f64(first, metrics_f64(pred[:100], target[:100]), "first 100", 100)
    again = acc.compute()[1]
    acc.update(p[100:], t[100:])                                     # compute, update, compute
    assert_matches_f64(acc.compute()[0], metrics_f64(pred, target), "all 300", 300)
    acc.reset()
    assert not acc.compute()[1].any()
    acc.update(p[:100], t[:100])
    assert acc.compute()[1].tobytes() == again.tobytes()             # reusable after reset, same bits


def test_one_million_rows_in_one_call(acc):
    """The values a (B, N, 52) sequence-mode output holds once flattened."""
    N = 1 << 20
    pred, target = synth.make_metrics_inputs(44, N, "plain")
    got, _ = run_pieces(acc, pred, target, [N])
    assert_matches_f64(got, metrics_f64(pred, target), "2^20 rows", N)
    seq = BlendshapeMetrics()
    seq.update(dev(pred).view(64, N // 64, 52), dev(target).view(64, N // 64, 52))
    m = seq.compute(lip_sync=True)
    seq.close()
    assert all(np.float32(m[k]) == np.float32(got[k]) for k in m)


def test_update_and_compute_replay_in_a_graph():
    N = 777
    sets = [synth.make_metrics_inputs(50 + i, N, "plain") for i in range(3)]
    eager = []
    for pred, target in sets:
        a = Acc()
        a.update(dev(pred), dev(target))
        eager.append(a.compute()[1])
        a.close()
    a = Acc()
    p, t, out = torch.zeros(N, 52, device="cuda"), torch.zeros(N, 52, device="cuda"), torch.zeros(KM_METRICS_COUNT, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                       # warm up on the side stream, as torch asks
        a.reset(); a.update(p, t); a.compute_dev(out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # one linear chain: reset, update, compute
        a.reset(); a.update(p, t); a.compute_dev(out)
    for (pred, target), want in zip(sets, eager):
        p.copy_(dev(pred)); t.copy_(dev(target))
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        print("graph replay:", got.tolist(), "eager:", want.tolist())
        assert got.tobytes() == want.tobytes()
    del g
    a.close()


def test_python_layer_views_shapes_and_lip_sync():
    c, pred, target, feats, golden = metrics_case("lip_3d")
    wide = torch.zeros(c["N"], 104, device="cuda")
    wide[:, ::2] = dev(pred)
    view = wide[:, ::2]                                              # non-contiguous pred
    assert not view.is_contiguous()
    a, b = BlendshapeMetrics(), BlendshapeMetrics()
    a.update(view, dev(target)); b.update(dev(pred), dev(target))
    ma, mb = a.compute(), b.compute()
    assert ma == mb and tuple(ma) == REFERENCE_KEYS
    assert_close_to_golden(ma, {k: v for k, v in golden.items() if k in REFERENCE_KEYS}, "class lip_3d")
    with pytest.raises(ValueError):
        a.update(torch.zeros(4, 51, device="cuda"), torch.zeros(4, 51, device="cuda"))
    with pytest.raises(ValueError):
        a.update(torch.zeros(4, 52, device="cuda"), torch.zeros(5, 52, device="cuda"))
    assert a.compute() == ma                                         # the refused calls launched nothing
    a.reset()
    assert a.compute() == {}
    one = BlendshapeMetrics()
    one.update(dev(pred[:1]), dev(target[:1]))
    assert not set(TEMPORAL_KEYS) & set(one.compute()) and one.compute()["mae"] > 0
    for x in (a, b, one):
        x.close()
    for name in ("lip_2d", "lip_3d", "lip_const_energy", "n256", "all_closed"):
        c, pred, target, feats, golden = metrics_case(name)
        lip = compute_lip_sync_metrics(dev(pred), dev(target), None if feats is None else dev(feats))
        assert set(lip) == set(golden) & set(LIP_SYNC_KEYS)
        assert_close_to_golden(lip, {k: golden[k] for k in lip}, "lip sync " + name)


def test_trainer_hooks(tmp_path):
    from test_gpu_dataset import write_pair
    from koemorph_amd.data import SequentialKoeMorphDataset
    from koemorph_amd.engine import Engine
    from koemorph_amd.scripts import train_sequential as ts
    for name, seed in (("a", 40), ("b", 50)):
        write_pair(tmp_path, name, 8.9, 30, seed)
    kw = dict(stride_frames=4, shuffle_files=False, loop_dataset=False, batch_size=4)

    def make():
        eng = Engine(); eng.load_state_dict(synth.make_core_params(0)); eng.finalize()
        return eng, ts.SequentialTrainer(eng, SequentialKoeMorphDataset(tmp_path, **kw), SequentialKoeMorphDataset(tmp_path, **kw),
                                         learning_rate=1e-3, dropout=0.0)
    eng, st = make()
    plain = st.validate()
    full = st.validate(metrics=True)
    assert set(plain) == {"total", "batches"} and full["total"] == plain["total"] and full["batches"] == plain["batches"]
    # the same pass by hand: forward_audio over the validation windows with validate()'s state handling
    preds, targets, state, current = [], [], None, None
    for batch in st.val_data:
        fi, B = int(batch["file_indices"][0]), batch["audio"].shape[0]
        first = current != fi or state is None or state.shape[0] != B
        if first:
            current, state = fi, torch.zeros(B, 52, device="cuda")
        preds.append(eng.forward_audio(batch["audio"], st._emotion(batch), state=state, first=first).cpu().numpy())
        targets.append(batch["target"].cpu().numpy())
    want = metrics_f64(np.concatenate(preds), np.concatenate(targets))
    assert set(full) == {"total", "batches"} | set(REFERENCE_KEYS)
    for k in REFERENCE_KEYS:
        print(f"validate {k}: dev {full[k]!r} f64 {want[k]!r}")
        assert abs(full[k] - want[k]) <= RTOL * max(abs(want[k]), FLOOR), (k, full[k], want[k])
    _, st2 = make()
    e1, e2 = st.train_epoch(), st2.train_epoch(metrics=True)
    assert e1["total"] == e2["total"] and e1["batches"] == e2["batches"]
    assert set(REFERENCE_KEYS) <= set(e2) and not set(REFERENCE_KEYS) & set(e1)
    assert 0.0 < e2["mae"] < 1.0 and abs(e2["rmse"] ** 2 - e2["mse"]) < 1e-6
