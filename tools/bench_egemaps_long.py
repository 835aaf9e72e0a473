"""One emotion-stream update at the reference's long_context timing (30 s context, 0.2 s interval: 2995 frames per window,
StreamEmotion(long_windows=True)) next to the default timing (20 s / 0.3 s: 1995 frames, the plain object).  Context, not thresholds.
Medians of --rounds rounds with minimum and maximum, the two objects interleaved round by round in one process; every time is a host
clock around work that ends in a device synchronise.

  1  one StreamEmotion.update call on 128 streams with full windows that selects 1, 8 and 128 of them (eager launches)
  2  the two per-window kernels alone -- pitch track and functionals, whose walks, compaction, slope scan and segment scan are serial
     in the frame count -- on the records of as many windows, and their share of the call above

    python tools/bench_egemaps_long.py --out profiles/egemaps_long_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                                              # noqa: E402
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine                         # noqa: E402
from koemorph_amd.streaming import StreamEmotion                                            # noqa: E402

SR, S = 16000, 128
ROUTES = (("long 30 s / 0.2 s", 30.0, 0.2, True), ("plain 20 s / 0.3 s", 20.0, 0.3, False))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def layer():
    torch.manual_seed(0)
    return torch.nn.Linear(264, 256)


def phrase(seed, seconds):
    """Voiced - silence - noise - voiced, as the tests' speech-like signal: the serial sections see voiced and unvoiced runs."""
    a = synth.make_vowel(seed, 120.0 + 10 * (seed % 7), seconds * 0.35, vibrato=0.03)
    b = np.zeros(int(seconds * 0.1 * SR), np.float32)
    c = (0.2 * synth.normal(seed + 2, (int(seconds * 0.2 * SR),))).astype(np.float32)
    d = 0.6 * synth.make_vowel(seed + 3, 190.0, seconds * 0.35, vibrato=0.02)
    return np.concatenate([a, b, c, d]).astype(np.float32)


def speech(seconds):
    """(S, seconds * SR): eight phrases' worth of distinct audio, rotated per stream."""
    base = np.concatenate([phrase(11 * k, 2.5) * (0.3 + 0.1 * (k % 5)) for k in range(int(seconds / 2.5) + 1)])[:int(seconds * SR)]
    return np.stack([np.roll(base, 4001 * s) for s in range(S)]).astype(np.float32)


def stats(xs):
    return f"{np.median(xs):8.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = [f"medians of {args.rounds} rounds (minimum .. maximum), the two objects interleaved; ms, host clock around a device synchronise",
             f"one update call on {S} streams with full windows, all due; the per-window kernels (pitch track + functionals) alone on",
             "the records of as many windows, and their share of the call:"]
    eng = EGeMAPSEngine("cuda")
    for k in (1, 8, S):
        calls = {}
        for name, ctx, itv, long_windows in ROUTES:
            audio = torch.from_numpy(speech(ctx + 2.0)).cuda()
            se = StreamEmotion(S, ctx, itv, max_updates=k, compression_layer=layer(), long_windows=long_windows)
            for at in range(0, audio.shape[1], 4 * SR):
                se.push(audio[:, at:at + 4 * SR].contiguous())
            se.update()
            fresh = audio[:, :int(itv * SR)].contiguous()
            # the records of k full windows, for the per-window kernels alone
            eng.functionals(audio[:k, :int(ctx * SR)].contiguous(), long_windows=long_windows)
            rec = torch.from_numpy(eng.records()).cuda()
            assert rec.shape[1] == se.shape["max_frames"]

            def call(se=se, fresh=fresh):
                se.push(fresh)
                torch.cuda.synchronize()
                ms = timed(se.update)
                assert int(se.updated.sum()) == k
                return ms

            def per_window(rec=rec, long_windows=long_windows):
                work = rec.clone()                                   # track_from_records clones as well: keep the copy outside the clock
                lib, st = eng._lib, torch.cuda.current_stream().cuda_stream
                out = torch.empty(rec.shape[0], 88, device="cuda")
                track = lib.km_egemaps_track_from_records_long if long_windows else lib.km_egemaps_track_from_records
                func = lib.km_egemaps_functionals_from_records_long if long_windows else lib.km_egemaps_functionals_from_records

                def both():
                    assert track(work.data_ptr(), rec.shape[0], rec.shape[1], st) == 0
                    assert func(work.data_ptr(), rec.shape[0], rec.shape[1], out.data_ptr(), st) == 0
                return timed(both)
            calls[name] = (call, per_window, se)
            del audio
        for c, p, _ in calls.values():                               # warm-up
            c(); p()
        t = {n: ([], []) for n in calls}
        for _ in range(args.rounds):
            for n, (c, p, _) in calls.items():
                t[n][0].append(c())
                t[n][1].append(p())
        for n, (upd, win) in t.items():
            frames = calls[n][2].shape["max_frames"]
            lines.append(f"  selects {k:4d} windows of {frames} frames, {n:18s}: update {stats(upd)}   per-window kernels {stats(win)}"
                         f"   share {100 * np.median(win) / np.median(upd):5.1f} %")
        for _, _, se in calls.values():
            se.close()
        del calls
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
