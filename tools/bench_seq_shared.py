#!/usr/bin/env python3
"""Sequence mode on ONE GPU with and without option seq_assemble, at the four shapes that have a one-launch core: the 60 fps recipe
(d_model 256 / window 512 / hop 266), long_context (d_model 512 / 8 heads / window 512 / hop 266) and `fast` / `basic` (d_model 128,
windows 128 / 256, hop 533, option core128 on both engines).  4 clips of 20 s at stride 1 per call.

Two engines with the same weights, one per route (km_sequence_plan route 0: every window's STFT, the staged log-mel image and
launch_core_generic -- the launches of the default; route 2: the clip's STFT once, the edge frames, seq_assemble_kernel and the core
behind the power-mel workspace), interleaved in rounds of one run.  The figure of a round is the host clock around `calls` calls
ending in one synchronisation, divided by their number; reported: the median, minimum and maximum of 15 rounds after a warm-up round,
the STFT frames either route computes and the largest difference between the two routes' outputs.  One JSON line per shape, also
appended to --out (profiles/seq_shared_bench.txt)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koemorph_amd import synth
from koemorph_amd.engine import Engine, MelConfig

# name: (d_model, heads, window, emotion_dim, front-end fps, core128)
SHAPES = {"60fps": (256, 8, 512, 256, 60, 0), "long_context": (512, 8, 512, 256, 60, 0), "fast": (128, 4, 128, 256, 30, 1),
          "basic": (128, 4, 256, 9, 30, 1)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--clips", type=int, default=4)
ap.add_argument("--seconds", type=float, default=20.0)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--calls", type=int, default=3, help="calls per round and route")
ap.add_argument("--tile", type=int, default=256, help="windows per tile (the workspace the engines reserve)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, L = args.clips, int(args.seconds * 16000)

for shape in args.shapes.split(","):
    d, H, T, ED, fps, core128 = SHAPES[shape]
    params = synth.make_core_params(0, d, T, ED, "trained")
    eng = {}
    for name, on in (("per_window", 0), ("assembled", 1)):
        e = Engine(d_model=d, num_heads=H, mel_sequence_length=T, emotion_dim=ED, mel=MelConfig.model_batch(target_fps=fps))
        e.load_state_dict(params)
        e.finalize()
        e.set_option("core128", core128)
        e.set_option("seq_assemble", on)
        eng[name] = e
    plans = {k: e.sequence_plan(L, 1, B) for k, e in eng.items()}
    assert plans["per_window"]["route"] == 0 and plans["assembled"]["route"] == 2, plans
    audio = torch.from_numpy(synth.make_audio(1, B, L, "speech")).cuda()
    emo = torch.from_numpy(synth.normal(2, (B, ED))).cuda()
    out, ms = {}, {k: [] for k in eng}
    for r in range(args.rounds + 1):                          # round 0 warms up (and grows the images)
        for k, e in eng.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                out[k] = e.sequence_forward(audio, emo, 1, max_tile=args.tile)
            torch.cuda.synchronize()
            if r:
                ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
    N = plans["assembled"]["N"]
    rec = {"workload": f"sequence_forward: {shape} (d_model {d}, {H} heads, window {T}, hop {eng['assembled'].mel.hop_length}), {B} clips x "
                       f"{args.seconds:g} s, stride 1, {N} windows a clip in tiles of {args.tile}; {args.rounds} rounds x {args.calls} calls per "
                       "route, interleaved",
           "max_abs_difference_between_routes": float((out["assembled"] - out["per_window"]).abs().max())}
    for k in eng:
        v = np.asarray(ms[k])
        rec[k] = {"ms_per_call_median_of_rounds": round(float(np.median(v)), 3), "ms_min": round(float(v.min()), 3),
                  "ms_max": round(float(v.max()), 3), "windows_per_s": round(B * N / float(np.median(v)) * 1e3, 1),
                  "stft_frames": plans[k]["stft_frames"]}
    rec["assembled_over_per_window"] = round(rec["assembled"]["ms_per_call_median_of_rounds"] / rec["per_window"]["ms_per_call_median_of_rounds"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    for e in eng.values():
        e.close()
