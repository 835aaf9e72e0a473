"""What the eGeMAPS low-level descriptors per frame (EGeMAPSEngine.llds, km_egemaps_llds) cost next to the functionals of the same
audio (EGeMAPSEngine.functionals): both calls launch the same peak, frame, pitch-track and voiced kernels, and then the tiled
descriptor kernel where the other has the functionals kernel, one workgroup per window.  Context, not thresholds; the method of
tools/bench_gemaps.py: medians of --rounds rounds with minimum and maximum, the calls interleaved round by round in one process, a
host clock around work that ends in a device synchronise.  The yardstick is the `functionals` call of the same run, whose launches
this feature does not touch; the ratio is reported, not fixed in advance.

  1  64 windows of 20 s (1995 frames): functionals, llds at the native rate, llds at 30 rows per second
  2  8 clips of 60 s (5995 frames) with long_windows: the same three
  3  the last kernel alone on the records of those calls (km_egemaps_functionals_from_records_set, km_egemaps_llds_from_records),
     and the bytes the descriptor kernel moves -- records read once plus rows written -- per its time, next to 8 TB/s.  That time is
     a host clock around one launch here; the kernel's own time comes from a kernel trace of --kernel-only, which runs the
     descriptor launches alone

    python tools/bench_llds.py --out profiles/llds_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gemaps import speech, stats                                                       # noqa: E402
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine                         # noqa: E402

SR = 16000
HBM_PEAK = 8.0e12
CASES = ((64, 20.0, False), (8, 60.0, True))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out")
    ap.add_argument("--kernel-only", action="store_true", help="launch the descriptor kernel alone, 20 times per case (for a kernel trace)")
    args = ap.parse_args()
    eng = EGeMAPSEngine("cuda")
    lines = [f"medians of {args.rounds} rounds (minimum .. maximum), the calls interleaved; ms, host clock around a device synchronise",
             "from audio: peak, frame, pitch-track and voiced kernels, then the functionals kernel or the descriptor kernel",
             "last kernel alone: on the records those calls left"]
    for B, seconds, long_windows in CASES:
        audio = torch.from_numpy(speech(seconds, B)).cuda()
        L = audio.shape[1]
        eng.functionals(audio, long_windows=long_windows)
        rec = torch.from_numpy(eng.records()).cuda()
        nf = rec.shape[1]
        if args.kernel_only:
            for fps in (None, 30):
                for _ in range(20):
                    eng.llds_from_records(rec, fps=fps, length=L)
            torch.cuda.synchronize()
            continue
        calls = {
            "functionals": lambda: eng.functionals(audio, long_windows=long_windows),
            "llds native": lambda: eng.llds(audio, long_windows=long_windows),
            "llds 30 fps": lambda: eng.llds(audio, long_windows=long_windows, fps=30),
            "functionals kernel alone": lambda: eng.functionals_from_records(rec, long_windows=long_windows),
            "llds kernel alone, native": lambda: eng.llds_from_records(rec),
            "llds kernel alone, 30 fps": lambda: eng.llds_from_records(rec, fps=30, length=L),
        }
        for fn in calls.values():
            fn()
        t = {n: [] for n in calls}
        for _ in range(args.rounds):
            for n, fn in calls.items():
                t[n].append(timed(fn))
        lines.append(f"  {B} windows of {seconds:g} s ({nf} frames){', long_windows' if long_windows else ''}")
        base = np.median(t["functionals"])
        for n in ("functionals", "llds native", "llds 30 fps"):
            lines.append(f"    {n:28s} {stats(t[n])}   / functionals {np.median(t[n]) / base:.3f}")
        rows = {"llds kernel alone, native": nf, "llds kernel alone, 30 fps": int(L / SR * 30)}
        for n in ("functionals kernel alone", "llds kernel alone, native", "llds kernel alone, 30 fps"):
            line = f"    {n:28s} {stats(t[n])}"
            if n in rows:
                moved = 4.0 * B * (nf * 36 + rows[n] * 25)
                line += f"   {moved / 1e6:7.2f} MB moved, {moved / (np.median(t[n]) * 1e-3) / 1e9:7.1f} GB/s by this clock ({100 * moved / (np.median(t[n]) * 1e-3) / HBM_PEAK:.2f} % of 8 TB/s)"
            lines.append(line)
        del audio, rec
        torch.cuda.empty_cache()
    if args.kernel_only:
        return
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
