"""Times the device-side evaluation metrics (km_metrics_update / km_metrics_compute) against the reference's method moved
to the GPU as it stands: torch.cat of the batches on the device followed by the torch operations of BlendshapeMetrics.compute
(src/model/losses.py:463-519) on device tensors, .item() calls included.

    python tools/bench_metrics.py [--out profiles/metrics_bench.txt]

Both run in one process after a spin-up; times are HIP events around `reps` back-to-back calls (the torch formulation
synchronises by itself, so its figure is a host clock around work that ends in a device read).  For the two large shapes
the achieved bytes/s of update alone (416 B of input per row) is printed against the 6.29 TB/s float4-copy figure.
"""
import argparse
import ctypes as C
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from koemorph_amd._lib import KM_METRICS_COUNT, check, load  # noqa: E402

HBM_MEASURED = 6.29e12


def torch_formulation(preds, targets):
    """BlendshapeMetrics.compute() with the epoch kept on the device: the same operations in the same order."""
    all_preds, all_targets = torch.cat(preds, dim=0), torch.cat(targets, dim=0)
    m = {}
    m["mae"] = F.l1_loss(all_preds, all_targets).item()
    m["mse"] = F.mse_loss(all_preds, all_targets).item()
    m["rmse"] = torch.sqrt(F.mse_loss(all_preds, all_targets)).item()
    per = F.l1_loss(all_preds, all_targets, reduction="none").mean(dim=0)
    m["max_bs_mae"], m["min_bs_mae"], m["std_bs_mae"] = per.max().item(), per.min().item(), per.std().item()
    corrs = []
    for i in range(52):
        a, b = all_preds[:, i], all_targets[:, i]
        if a.std() > 1e-6 and b.std() > 1e-6:
            c = torch.corrcoef(torch.stack([a, b]))[0, 1]
            if not torch.isnan(c):
                corrs.append(c.item())
    m["mean_correlation"] = sum(corrs) / len(corrs) if corrs else 0.0
    m["min_correlation"] = min(corrs) if corrs else 0.0
    if all_preds.shape[0] > 1:
        dp, dt = torch.diff(all_preds, dim=0), torch.diff(all_targets, dim=0)
        m["temporal_consistency"] = F.l1_loss(dp, dt).item()
        m["pred_smoothness"], m["target_smoothness"] = dp.abs().mean().item(), dt.abs().mean().item()
    pa, ta = (all_preds > 0.1).float(), (all_targets > 0.1).float()
    m["pred_activity"], m["target_activity"] = pa.mean().item(), ta.mean().item()
    tp, fp, fn = (pa * ta).sum(), (pa * (1 - ta)).sum(), ((1 - pa) * ta).sum()
    precision, recall = tp / (tp + fp + 1e-8), tp / (tp + fn + 1e-8)
    m["precision"], m["recall"] = precision.item(), recall.item()
    m["f1_score"] = (2 * precision * recall / (precision + recall + 1e-8)).item()
    return m


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", type=int, nargs="*", default=[8, 256, 65536, 1048576])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs the GPU (no fallback)")
    lib, h = load(), C.c_void_p()
    check(lib.km_metrics_create(C.byref(h)))
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(KM_METRICS_COUNT, device="cuda")
    x = torch.randn(4096, 4096, device="cuda")
    t0 = time.time()
    while time.time() - t0 < 2.0:                      # spin-up: clocks and code objects
        x @ x
    torch.cuda.synchronize()
    lines = [f"{'rows':>9} {'update us':>10} {'compute us':>10} {'upd+cmp us':>10} {'torch us':>10} {'speed-up':>8} {'update GB/s':>11} {'of 6.29 TB/s':>12}"]
    for n in args.shapes:
        g = torch.Generator(device="cuda").manual_seed(n)
        t = torch.rand(n, 52, device="cuda", generator=g)
        p = (t + 0.1 * torch.randn(n, 52, device="cuda", generator=g)).clamp_(0, 1)
        reps = 2000 if n <= 256 else (400 if n <= 65536 else 100)
        upd = lambda: check(lib.km_metrics_update(h, p.data_ptr(), t.data_ptr(), 0, n, st))
        cmp_ = lambda: check(lib.km_metrics_compute(h, out.data_ptr(), st))

        def both():
            check(lib.km_metrics_reset(h, st)); upd(); cmp_()
        for _ in range(10):
            both()
        torch_formulation([p], [t])
        torch.cuda.synchronize()
        rows = []
        for _ in range(3):                              # alternate the two, three rounds: the spread shows in the min / max
            u, c, b = events_ms(upd, reps), events_ms(cmp_, reps), events_ms(both, reps)
            torch.cuda.synchronize()
            treps = 20 if n <= 65536 else 5
            t1 = time.perf_counter()
            for _ in range(treps):
                torch_formulation([p], [t])
            torch.cuda.synchronize()
            rows.append((u, c, b, (time.perf_counter() - t1) / treps * 1e3))
        u, c, b, tt = (sorted(r[i] for r in rows)[1] for i in range(4))      # medians
        bw = n * 416 / (u * 1e-3)
        lines.append(f"{n:>9} {u * 1e3:>10.2f} {c * 1e3:>10.2f} {b * 1e3:>10.2f} {tt * 1e3:>10.1f} {tt / b:>8.0f} "
                     + (f"{bw / 1e9:>11.0f} {bw / HBM_MEASURED:>12.1%}" if n >= 65536 else f"{'':>11} {'':>12}"))
        lines.append(f"{'':>9} update min/max {min(r[0] for r in rows) * 1e3:.2f}/{max(r[0] for r in rows) * 1e3:.2f} us, "
                     f"reset+update+compute min/max {min(r[2] for r in rows) * 1e3:.2f}/{max(r[2] for r in rows) * 1e3:.2f} us, "
                     f"torch min/max {min(r[3] for r in rows) * 1e3:.1f}/{max(r[3] for r in rows) * 1e3:.1f} us")
    torch.cuda.synchronize()
    check(lib.km_metrics_destroy(h))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
