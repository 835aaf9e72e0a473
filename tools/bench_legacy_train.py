"""Same-run A/B of one full training step of SimplifiedKoeMorphModel (forward, loss, backward, clip, AdamW):
A = LegacyTrainer.step (km_legacy_train_*), B = the reference's own formulation kept on the same device: the torch containers
(nn.Sequential / nn.MultiheadAttention, dropout 0.1) behind this library's mel front end, KoeMorphLoss restated in torch,
clip_grad_norm_, torch.optim.AdamW.  Spin-up, warm-up, rotating inputs, HIP events, A and B interleaved round by round.

After the A/B, per shape, a run of its own under a plain kernel trace (a child process: rocprofv3 --kernel-trace around this
file with --trace-steps) gives the launches per step and each kernel's time; the matrix products' executed FLOP (from the
step's GEMM shapes, and the MFMA instructions the two attention kernels issue, padding included) over that time is set against
the fp32-MFMA peak.  Times under the trace are per kernel; the step's wall time is the A/B's.

    python tools/bench_legacy_train.py --out profiles/legacy_train_bench.txt
"""
import argparse
import collections
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                                    # noqa: E402
from koemorph_amd.model.simplified_model import SimplifiedKoeMorphModel          # noqa: E402
from koemorph_amd.training import LegacyTrainer                                   # noqa: E402

PEAK_FP32_MFMA = 157.3e12      # MI355X, v_mfma_f32_16x16x4_f32 / 32x32x2_f32 on 256 CUs (AMD's figure)
SHAPES = ((16, 160000), (8, 136448))
GROUPS = ((range(12, 32), 2.0), (range(0, 12), 1.0), (range(32, 44), 1.0), (range(44, 52), 1.5))


class TorchModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.audio_encoder = nn.Sequential(nn.Linear(80, 256), nn.ReLU(), nn.Dropout(0.1), nn.Linear(256, 256), nn.ReLU(), nn.Dropout(0.1))
        self.attention = nn.MultiheadAttention(256, 8, dropout=0.1, batch_first=True)
        self.decoder = nn.Sequential(nn.Linear(256, 128), nn.ReLU(), nn.Dropout(0.1), nn.Linear(128, 128), nn.ReLU(), nn.Dropout(0.1),
                                     nn.Linear(128, 52), nn.Sigmoid())
        self.blendshape_queries = nn.Parameter(torch.randn(52, 256) * 0.1)

    def forward(self, mel):
        e = self.audio_encoder(mel)
        q = self.blendshape_queries.unsqueeze(0).repeat(mel.shape[0], 1, 1)
        a, _ = self.attention(query=q, key=e, value=e)
        return self.decoder(a).mean(dim=1)


def torch_loss(pred, target):
    loss = nn.functional.mse_loss(pred, target) + 0.1 * nn.functional.l1_loss(pred, target)
    per = sum(w * nn.functional.mse_loss(pred[:, list(i)], target[:, list(i)]) for i, w in GROUPS)
    return loss + 0.5 * per


def events(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i, (a, b) in enumerate(ev):
        a.record(); fn(i); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def step_flop(B, T):
    """Executed FLOP of one step's matrix products: {"gemm": ..., "ltr_attn_fwd_kernel": ..., "ltr_attn_bwd_kernel": ...}.
    Every linear layer is a product in the forward pass, one for its weight gradient and one for its input gradient (the mel
    input has none); the attention kernels issue 64 (forward) and 224 (backward) 16x16x4 MFMAs of 2048 FLOP per (window, head)
    and tile of 16 keys, whatever part of the 64 query rows and of the last key tile is padding."""
    R, R2 = B * T, B * 52
    layers = [R * 256 * 80, R * 256 * 256, R * 512 * 256, 52 * 256 * 256, R2 * 256 * 256, R2 * 128 * 256, R2 * 128 * 128, R2 * 52 * 128]
    tiles = B * 8 * ((T + 15) // 16)
    return {"gemm": 2.0 * (3 * sum(layers) - layers[0]), "ltr_attn_fwd_kernel": tiles * 64 * 2048.0, "ltr_attn_bwd_kernel": tiles * 224 * 2048.0}


def short(name):
    return name.split("(")[0].split("<")[0].replace("void ", "").replace("km::", "").strip()[:48]


def trace_child(B, Ln, steps):
    """What runs under the kernel trace: `steps` eager steps at one shape and nothing else."""
    model = SimplifiedKoeMorphModel().cuda()
    tr = LegacyTrainer(model, max_windows=B, max_frames=1 + Ln // 533, dropout=0.1)
    tr.set_loss_terms(perceptual_weight=0.5)
    audio = torch.from_numpy(synth.make_audio(10, B, Ln)).cuda()
    target = torch.from_numpy(synth.uniform(20, (B, 52), 0, 1)).cuda()
    for _ in range(steps):
        tr.step(audio, target)
    torch.cuda.synchronize()


def kernel_table(B, Ln, steps=30):
    """Lines of the per-kernel record of one shape, from a kernel trace of a child process."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return ["    per-kernel record not taken: rocprofv3 is not on the PATH"]
    tmp = tempfile.mkdtemp(prefix="ltr_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--trace-steps", str(steps), "--trace-shape", str(B), str(Ln)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if res.returncode != 0 or not files:
            return [f"    per-kernel record not taken: the traced run ended with status {res.returncode}", "    " + res.stderr.strip()[-300:]]
        rows = []
        for f in files:
            rows += list(csv.DictReader(open(f)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [short(r["Kernel_Name"]) for r in rows]
    marks = [i for i, n in enumerate(names) if n == "ltr_loss_kernel"]          # once per step
    if len(marks) < 12:
        return [f"    per-kernel record not taken: {len(marks)} steps in the trace"]
    first, last = marks[-11], marks[-1]                                           # the last 10 steps (a period, whatever its phase)
    per_step = (last - first) / 10.0
    acc = collections.OrderedDict()
    for i in range(first, last):
        acc.setdefault(names[i], []).append((int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1e3)
    T = 1 + Ln // 533
    flop = step_flop(B, T)
    gemm_us = sum(sum(v) for n, v in acc.items() if "gemm" in n) / 10.0
    total_us = sum(sum(v) for v in acc.values()) / 10.0
    out = [f"    launches per step: {per_step:g} (front end, forward, loss, backward, clip and AdamW)",
           f"    kernel time per step {total_us:.1f} us under the trace; per kernel: launches per step, us per launch (mean), us per step, executed FLOP / time over the {PEAK_FP32_MFMA / 1e12:.1f} TFLOP/s fp32-MFMA peak"]
    for n, v in acc.items():
        us = sum(v) / 10.0
        if n in flop:
            frac = f"{flop[n] / (us * 1e-6) / PEAK_FP32_MFMA * 100:6.2f} %"
        elif "gemm" in n:
            frac = "  (gemm)"
        else:
            frac = "       -"
        out.append(f"      {n:48s} {len(v) / 10.0:5.1f} x {sum(v) / len(v):8.1f} = {us:8.1f} us  {frac}")
    if gemm_us > 0:
        out.append(f"      all GEMM launches together: {flop['gemm'] / 1e9:.2f} GFLOP in {gemm_us:.1f} us = "
                   f"{flop['gemm'] / (gemm_us * 1e-6) / PEAK_FP32_MFMA * 100:.2f} % of the peak")
    out.append("      (-: no matrix product of the model: masks, dropout, ReLU, fixed-order sums, loss, optimizer; the mel front end's products are not counted)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-kernel record (the traced child run)")
    ap.add_argument("--trace-steps", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--trace-shape", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_steps:
        return trace_child(a.trace_shape[0], a.trace_shape[1], a.trace_steps)
    lines = []
    for B, Ln in SHAPES:
        model = SimplifiedKoeMorphModel().cuda()
        tr = LegacyTrainer(model, max_windows=B, max_frames=1 + Ln // 533, dropout=0.1)
        tr.set_loss_terms(perceptual_weight=0.5)
        ref = TorchModel().cuda().train()
        ref.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
        opt = torch.optim.AdamW(ref.parameters(), lr=1e-4, weight_decay=1e-5)
        audio = [torch.from_numpy(synth.make_audio(10 + i, B, Ln)).cuda() for i in range(4)]
        target = [torch.from_numpy(synth.uniform(20 + i, (B, 52), 0, 1)).cuda() for i in range(4)]

        def step_hip(i):
            tr.step(audio[i % 4], target[i % 4])

        def step_torch(i):
            mel = model.extract_mel_features(audio[i % 4])
            opt.zero_grad(set_to_none=True)
            torch_loss(ref(mel), target[i % 4]).backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
            opt.step()

        tr.step(audio[0], target[0])
        tr.capture(B, Ln)

        def step_graph(i):
            tr.step_graph(audio[i % 4], target[i % 4])

        for f in (step_hip, step_torch, step_graph):      # spin-up and warm-up
            events(f, 30)
        res = {"hip": [], "graph": [], "torch": []}
        for _ in range(a.rounds):
            res["hip"] += events(step_hip, a.steps)
            res["torch"] += events(step_torch, a.steps)
            res["graph"] += events(step_graph, a.steps)
        med = {k: float(np.median(v)) for k, v in res.items()}
        p10 = {k: float(np.percentile(v, 10)) for k, v in res.items()}
        p90 = {k: float(np.percentile(v, 90)) for k, v in res.items()}
        lines.append(f"{B} x {Ln} samples ({1 + Ln // 533} frames), full step, ms median [p10, p90] over {a.rounds * a.steps} steps:")
        for k, name in (("hip", "km_legacy_train_* eager"), ("graph", "km_legacy_train_* hipGraph + AdamW"), ("torch", "torch containers + AdamW")):
            lines.append(f"    {name:36s} {med[k]:8.3f} [{p10[k]:.3f}, {p90[k]:.3f}]")
        lines.append(f"    torch / hip eager {med['torch'] / med['hip']:.2f}x, torch / hip graph {med['torch'] / med['graph']:.2f}x")
        del tr, ref, opt, model, audio, target
        torch.cuda.synchronize()
        if not a.no_kernels:
            lines += kernel_table(B, Ln)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
