"""Same-run A/B of the validation pass: ``SequentialTrainer.validate()`` as it is (gather every batch, per-window front end,
torch MSE + ``.item()`` per batch) against ``validate(components=True)`` from the resident clip (``Engine.forward_clip`` +
``LossTerms`` on the device, one readback per file).

One synthetic clip (seeded noise + seeded labels, written to a temporary directory: the data set reads files), stride-1
windows, at 8 and at 64 windows per batch.  Both calls run on ONE trainer and one engine, alternating, ``--rounds`` times
after a warm-up of each; the time is the host clock around a call that ends in a device synchronise (validate() reads its
result back).  Reports the median, the spread and the per-batch time of each, and checks on the way that both give the
same ``total`` up to the float32 rounding of the default path's torch reduction.

    python tools/bench_validate.py --seconds 30 --rounds 7 --out profiles/validate_bench.txt
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_clip(d: Path, seconds: float, seed: int):
    from scipy.io import wavfile
    from koemorph_amd import synth
    n = int(seconds * 16000)
    wavfile.write(d / "clip.wav", 16000, synth.uniform(seed, (n,), -0.5, 0.5).astype(np.float32))
    frames = int(seconds * 30)
    labels = synth.uniform(seed + 1, (frames, 52), 0, 1).astype(np.float32)
    with open(d / "clip.jsonl", "w") as f:
        for i in range(frames):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seconds", type=float, default=30.0, help="length of the synthetic clip")
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64], help="windows per batch")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", help="also write the record to this file")
    args = ap.parse_args(argv)

    import torch
    from koemorph_amd import synth
    from koemorph_amd.data import SequentialKoeMorphDataset
    from koemorph_amd.engine import Engine
    from koemorph_amd.scripts.train_sequential import SequentialTrainer

    sync = torch.cuda.synchronize
    lines = [f"tools/bench_validate.py on one {torch.cuda.get_device_name(0)}: one synthetic clip of {args.seconds:g} s, stride-1 windows of 256 frames,",
             f"validate() [A: gather + per-window front end + torch MSE and .item() per batch] against validate(components=True) [B: forward_clip",
             f"from the resident clip + LossTerms on the device, one readback per file], same trainer, alternating, {args.rounds} rounds after one",
             "warm-up each; host clock around the call (it ends in a readback).  ms per pass, median (min .. max); us per batch from the median.",
             "",
             f"{'windows/batch':>13} {'batches':>8} {'A ms':>24} {'B ms':>24} {'A us/batch':>11} {'B us/batch':>11} {'B / A':>7}"]
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        write_clip(tmp, args.seconds, args.seed)
        for B in args.batches:
            eng = Engine()
            eng.load_state_dict(synth.make_core_params(0, style="trained"))
            eng.finalize()
            data = SequentialKoeMorphDataset(tmp, resident_windows=True, shuffle_files=False, loop_dataset=False, batch_size=B)
            st = SequentialTrainer(eng, data, data, from_clip=True, dropout=0.0)
            assert eng.forward_clip_supported()
            a = lambda: st.validate()
            b = lambda: st.validate(components=True)
            _, va = timed(a, sync)
            _, vb = timed(b, sync)
            n = va["batches"]
            assert vb["batches"] == n and abs(va["total"] - vb["total"]) <= (B * 52 + 4) * 2.0 ** -24 * va["total"], (va["total"], vb["total"])
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(timed(a, sync)[0])
                tb.append(timed(b, sync)[0])
            ma, mb = statistics.median(ta), statistics.median(tb)
            fa = f"{ma:8.2f} ({min(ta):.2f} .. {max(ta):.2f})"
            fb = f"{mb:8.2f} ({min(tb):.2f} .. {max(tb):.2f})"
            lines.append(f"{B:>13} {n:>8} {fa:>24} {fb:>24} {ma * 1e3 / n:>11.1f} {mb * 1e3 / n:>11.1f} {mb / ma:>7.2f}")
            lines.append(f"{'':>13} total A {va['total']!r}  B {vb['total']!r}  (relative {abs(va['total'] - vb['total']) / va['total']:.1e})")
            del st, data, eng
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
