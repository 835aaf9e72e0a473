"""Train SimplifiedKoeMorphModel on the GPU: the loop of the reference's src/train.py (:165-330) without hydra.

Defaults are those of configs/training/default.yaml and configs/data/default.yaml: AdamW lr 1e-4, weight decay 1e-5,
CosineAnnealingLR(T_max 100, eta_min 1e-6) stepped per epoch, KoeMorphLoss weights mse 1.0 / l1 0.1 / perceptual 0.5, gradient
clipping 1.0, batch 16, audio cropped to 10 s.  Data: ``<name>.wav`` + ``<name>.jsonl`` pairs in ``--data-dir`` (the loaders of
koemorph_amd.data.sequential_dataset); a batch is cropped to ``--audio-max-length`` seconds and zero-padded to its longest clip,
the target is the first label frame of each clip (train.py:178-182).  Checkpoints hold a ``model_state_dict`` the reference
module loads (train.py:262-283).

    python -m koemorph_amd.scripts.train --data-dir data/train --epochs 100 --checkpoint-dir checkpoints
"""
from __future__ import annotations

import argparse
import os
from pathlib import Path

import numpy as np
import torch

from ..data.sequential_dataset import _load_wav, load_jsonl_labels
from ..metrics import BlendshapeMetrics
from ..model.simplified_model import SimplifiedKoeMorphModel
from ..training import LegacyTrainer


def load_pairs(data_dir, sample_rate: int, max_samples: int):
    """[(audio (<= max_samples,) float32, first label frame (52,))] for every wav + jsonl pair, sorted by name."""
    out = []
    for wav in sorted(Path(data_dir).glob("*.wav")):
        js = wav.with_suffix(".jsonl")
        if not js.exists():
            continue
        labels, _ = load_jsonl_labels(js)
        if labels.shape[0] == 0:
            continue
        out.append((_load_wav(wav, sample_rate)[:max_samples], labels[0, :52].astype(np.float32)))
    if not out:
        raise FileNotFoundError(f"no <name>.wav + <name>.jsonl pairs in {data_dir}")
    return out


def batches(pairs, batch_size: int, order):
    for i in range(0, len(order), batch_size):
        idx = order[i:i + batch_size]
        L = max(pairs[j][0].shape[0] for j in idx)
        audio = np.zeros((len(idx), L), np.float32)
        for r, j in enumerate(idx):
            audio[r, :pairs[j][0].shape[0]] = pairs[j][0]
        yield audio, np.stack([pairs[j][1] for j in idx])


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--val-dir", default=None)
    ap.add_argument("--checkpoint-dir", default="checkpoints")
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--weight-decay", type=float, default=1e-5)
    ap.add_argument("--t-max", type=int, default=100)
    ap.add_argument("--eta-min", type=float, default=1e-6)
    ap.add_argument("--mse-weight", type=float, default=1.0)
    ap.add_argument("--l1-weight", type=float, default=0.1)
    ap.add_argument("--perceptual-weight", type=float, default=0.5)
    ap.add_argument("--grad-clip", type=float, default=1.0)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--audio-max-length", type=float, default=10.0)
    ap.add_argument("--sample-rate", type=int, default=16000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--save-every", type=int, default=10)
    ap.add_argument("--resume", default=None)
    a = ap.parse_args(argv)

    torch.manual_seed(a.seed)
    rng = np.random.RandomState(a.seed)
    max_samples = int(a.audio_max_length * a.sample_rate)
    train = load_pairs(a.data_dir, a.sample_rate, max_samples)
    val = load_pairs(a.val_dir, a.sample_rate, max_samples) if a.val_dir else None
    model = SimplifiedKoeMorphModel(sample_rate=a.sample_rate).cuda()
    if a.resume:
        ck = torch.load(a.resume, map_location="cpu")
        model.load_state_dict(ck["model_state_dict"])
    max_frames = 1 + max_samples // model.hop_length
    tr = LegacyTrainer(model, max_windows=a.batch_size, max_frames=max_frames, lr=a.lr, weight_decay=a.weight_decay,
                       grad_clip=a.grad_clip, mse_weight=a.mse_weight, l1_weight=a.l1_weight, dropout=a.dropout, seed=a.seed)
    tr.set_loss_terms(perceptual_weight=a.perceptual_weight)
    start = 0
    if a.resume and "optimizer_state_dict" in ck and ck["optimizer_state_dict"].get("layout") == "per-key-v1":
        tr.load_optimizer_state(ck["optimizer_state_dict"])
        start = tr.epoch
        tr.lr = a.eta_min + (a.lr - a.eta_min) * (1 + np.cos(np.pi * start / a.t_max)) / 2
    os.makedirs(a.checkpoint_dir, exist_ok=True)

    def save(name, epoch, losses):
        tr.sync_inference_weights()
        torch.save({"epoch": epoch, "model_state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                    "optimizer_state_dict": tr.optimizer_state(), "train_loss": losses[-1], "args": vars(a)},
                   os.path.join(a.checkpoint_dir, name))

    def evaluate(pairs):
        tr.sync_inference_weights()
        model.eval()
        m = BlendshapeMetrics()
        for audio, target in batches(pairs, a.batch_size, list(range(len(pairs)))):
            with torch.no_grad():
                pred = model(torch.from_numpy(audio).cuda())
            m.update(pred, torch.from_numpy(target).cuda())
        return m.compute()

    epoch_losses, best = [], float("inf")
    for epoch in range(start, a.epochs):
        total, n = torch.zeros(1, device="cuda"), 0
        for audio, target in batches(train, a.batch_size, list(rng.permutation(len(train)))):
            total += tr.step(torch.from_numpy(audio).cuda(), torch.from_numpy(target).cuda())
            n += 1
        epoch_losses.append(float(total.item()) / n)
        line = f"epoch {epoch + 1}/{a.epochs}  train loss {epoch_losses[-1]:.6f}  lr {tr.lr:.3e}"
        vm = evaluate(val) if val is not None else None
        if vm is not None:
            line += f"  val mae {vm['mae']:.5f}  val correlation {vm['mean_correlation']:.4f}"
        print(line, flush=True)
        tr.end_epoch(a.t_max, a.eta_min)      # before any checkpoint of this epoch: a resumed run starts at the next epoch and its rate
        if vm is not None and vm["mae"] < best:
            best = vm["mae"]
            save("best_model.pth", epoch + 1, epoch_losses)
        if (epoch + 1) % a.save_every == 0:
            save(f"checkpoint_epoch_{epoch + 1}.pth", epoch + 1, epoch_losses)
    save("final_model.pth", a.epochs, epoch_losses)
    metrics = evaluate(val if val is not None else train)
    print("final metrics: " + "  ".join(f"{k} {metrics[k]:.5f}" for k in ("mae", "rmse", "mean_correlation")), flush=True)
    return {"epoch_losses": epoch_losses, "metrics": metrics, "checkpoint": os.path.join(a.checkpoint_dir, "final_model.pth")}


if __name__ == "__main__":
    main()
