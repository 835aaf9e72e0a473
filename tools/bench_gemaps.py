"""What the GeMAPS feature set (62 functionals, StreamEmotion(feature_set="GeMAPS")) costs next to eGeMAPS (88) on the same audio:
the GeMAPS frame kernel leaves out the previous frame's 1024-point transform, the flux sum and the four DCT sums, the functionals
kernel seven contours and the RMS sum.  Context, not thresholds; the method of tools/bench_egemaps_long.py: medians of --rounds rounds
with minimum and maximum, the two objects interleaved round by round in one process, a host clock around work that ends in a device
synchronise.  The yardstick is the eGeMAPS object of the same run.

  1  one StreamEmotion.update call on 128 streams with full windows that selects 1, 8 and 128 of them, at 10 s / 0.5 s (995 frames,
     the reference's `fast` variant) and at 20 s / 0.3 s (1995 frames)
  2  next to it the five kernels alone on as many dense windows (km_egemaps_functionals_set) and the two per-window kernels alone on
     their records (pitch track + functionals); the per-frame kernels (peak, frame, voiced) are the difference of those medians, and
     their share of the update call is reported
  3  ClipEmotion.build of a 60 s clip at 10 s / 0.5 s, both sets

    python tools/bench_gemaps.py --out profiles/gemaps_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                                              # noqa: E402
from koemorph_amd.features import ClipEmotion                                               # noqa: E402
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine                         # noqa: E402
from koemorph_amd.streaming import StreamEmotion                                            # noqa: E402

SR, S = 16000, 128
SETS = (("GeMAPS", 62, 1), ("eGeMAPSv02", 88, 0))
TIMINGS = ((10.0, 0.5), (20.0, 0.3))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def layer(n_feat):
    torch.manual_seed(0)
    return torch.nn.Linear(3 * n_feat, 256)


def phrase(seed, seconds):
    """Voiced - silence - noise - voiced, as the tests' speech-like signal."""
    a = synth.make_vowel(seed, 120.0 + 10 * (seed % 7), seconds * 0.35, vibrato=0.03)
    b = np.zeros(int(seconds * 0.1 * SR), np.float32)
    c = (0.2 * synth.normal(seed + 2, (int(seconds * 0.2 * SR),))).astype(np.float32)
    d = 0.6 * synth.make_vowel(seed + 3, 190.0, seconds * 0.35, vibrato=0.02)
    return np.concatenate([a, b, c, d]).astype(np.float32)


def speech(seconds, streams=S):
    """(streams, seconds * SR): phrases of distinct voices, rotated per stream."""
    base = np.concatenate([phrase(11 * k, 2.5) * (0.3 + 0.1 * (k % 5)) for k in range(int(seconds / 2.5) + 1)])[:int(seconds * SR)]
    return np.stack([np.roll(base, 4001 * s) for s in range(streams)]).astype(np.float32)


def stats(xs):
    return f"{np.median(xs):8.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = [f"medians of {args.rounds} rounds (minimum .. maximum), the GeMAPS and the eGeMAPS object interleaved; ms, host clock around a device synchronise",
             f"update: one StreamEmotion.update on {S} streams with full windows; five kernels: km_egemaps_functionals_set on as many dense",
             "windows; per-window: pitch track + functionals on their records; per-frame (peak, frame, voiced) = five kernels - per-window"]
    eng = EGeMAPSEngine("cuda")
    lib, st = eng._lib, torch.cuda.current_stream().cuda_stream
    findings = []
    for ctx, itv in TIMINGS:
        audio = torch.from_numpy(speech(ctx + 2.0)).cuda()
        fresh = audio[:, :int(itv * SR)].contiguous()
        for k in (1, 8, S):
            calls = {}
            dense = audio[:k, :int(ctx * SR)].contiguous()
            for name, width, code in SETS:
                se = StreamEmotion(S, ctx, itv, max_updates=k, compression_layer=layer(width), feature_set=name)
                for at in range(0, audio.shape[1], 4 * SR):
                    se.push(audio[:, at:at + 4 * SR].contiguous())
                se.update()
                eng.functionals(dense, feature_set=name)
                rec = torch.from_numpy(eng.records()).cuda()
                assert rec.shape[1] == se.shape["max_frames"]
                work = torch.empty(int(lib.km_egemaps_workspace_floats(k, dense.shape[1])), device="cuda")
                out = torch.empty(k, width, device="cuda")

                def call(se=se):
                    se.push(fresh)
                    torch.cuda.synchronize()
                    ms = timed(se.update)
                    assert int(se.updated.sum()) == k
                    return ms

                def five(code=code, work=work, out=out):
                    return timed(lambda: lib.km_egemaps_functionals_set(eng._plan, code, 0, dense.data_ptr(), k, dense.shape[1], 1, work.data_ptr(),
                                                                        work.numel(), out.data_ptr(), st))

                def per_window(code=code, rec=rec, out=out):
                    scratch = rec.clone()                             # the track rewrites the F0 column: keep the copy outside the clock

                    def both():
                        assert lib.km_egemaps_track_from_records(scratch.data_ptr(), rec.shape[0], rec.shape[1], st) == 0
                        assert lib.km_egemaps_functionals_from_records_set(code, 0, scratch.data_ptr(), rec.shape[0], rec.shape[1], out.data_ptr(), st) == 0
                    return timed(both)
                calls[name] = (call, five, per_window, se)
            for c, f, p, _ in calls.values():                        # warm-up
                c(); f(); p()
            t = {n: ([], [], []) for n in calls}
            for _ in range(args.rounds):
                for n, (c, f, p, _) in calls.items():
                    t[n][0].append(c()); t[n][1].append(f()); t[n][2].append(p())
            frames = calls["GeMAPS"][3].shape["max_frames"]
            for n, (upd, fv, win) in t.items():
                per_frame = np.median(fv) - np.median(win)
                lines.append(f"  {ctx:4.0f} s / {itv} s, selects {k:4d} windows of {frames} frames, {n:10s}: update {stats(upd)}   five kernels {stats(fv)}"
                             f"   per-window {stats(win)}   per-frame {per_frame:8.3f}   share of update {100 * per_frame / np.median(upd):5.1f} %")
            g, e = t["GeMAPS"][0], t["eGeMAPSv02"][0]
            lines.append(f"        GeMAPS / eGeMAPS update medians: {np.median(g) / np.median(e):.3f}")
            if np.median(g) > max(e):
                findings.append(f"{ctx:g} s / {itv} s, {k} windows: the GeMAPS median {np.median(g):.3f} is above the eGeMAPS maximum {max(e):.3f}")
            for _, _, _, se in calls.values():
                se.close()
            del calls
        del audio, fresh
        torch.cuda.empty_cache()
    # 3. a 60 s clip's track at the `fast` timing
    clip = torch.from_numpy(speech(60.0, 1)[0]).cuda()
    ces = {n: ClipEmotion(10.0, 0.5, compression_layer=layer(w), feature_set=n) for n, w, _ in SETS}
    for ce in ces.values():
        ce.build(clip)
    tb = {n: [] for n in ces}
    for _ in range(args.rounds):
        for n, ce in ces.items():
            tb[n].append(timed(lambda: ce.build(clip)))
    rows = ces["GeMAPS"].num_rows(clip.shape[0])
    for n, xs in tb.items():
        lines.append(f"  ClipEmotion.build, 60 s clip at 10 s / 0.5 s ({rows} rows, max_slots 64), {n:10s}: {stats(xs)}")
    lines.append(f"        GeMAPS / eGeMAPS build medians: {np.median(tb['GeMAPS']) / np.median(tb['eGeMAPSv02']):.3f}")
    if np.median(tb["GeMAPS"]) > max(tb["eGeMAPSv02"]):
        findings.append("ClipEmotion.build: the GeMAPS median is above the eGeMAPS maximum")
    for ce in ces.values():
        ce.close()
    lines.append("FINDINGS (a GeMAPS median above the eGeMAPS maximum of the same run): " + ("none" if not findings else "; ".join(findings)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
