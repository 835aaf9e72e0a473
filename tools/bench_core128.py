#!/usr/bin/env python3
"""The reference's `fast` / `basic` variants on ONE GPU -- d_model 128, 4 heads, window 128 / 256, front end at hop 533 -- with
core128_kernel (one launch, option core128) and with the launch-per-product chain (the default of the forward calls), in ONE run:
two engines with the same weights, interleaved in rounds, on 256 windows of (window + 1) x 533 samples.
Timed: km_forward_audio (front end + core) and km_core_forward from caller-provided log-mel (core alone behind the row packing).
The figure of a round is the host clock around `calls` calls ending in one synchronisation, divided by their number; reported: the
median, minimum and maximum of 15 rounds after a warm-up round, and whether the two routes' outputs agree to 1e-6."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koemorph_amd import synth
from koemorph_amd.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="fast", choices=("fast", "basic"))
ap.add_argument("--windows", type=int, default=256)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--calls", type=int, default=20, help="calls per round and route")
args = ap.parse_args()
T, ED = {"fast": (128, 256), "basic": (256, 9)}[args.shape]
B, L = args.windows, (T + 1) * 533

params = synth.make_core_params(0, 128, T, ED, "trained")
eng = {}
for name, core128 in (("core128", 1), ("chain", 0)):
    e = Engine(d_model=128, num_heads=4, mel_sequence_length=T, emotion_dim=ED)
    e.load_state_dict(params)
    e.finalize()
    e.set_option("core128", core128)
    e.reserve(B, L)
    eng[name] = e
assert eng["core128"].core_route() == 4 and eng["chain"].core_route() == 3
audio = torch.from_numpy(synth.make_audio(1, B, L, "uniform")).cuda()
emo = torch.from_numpy(synth.normal(2, (B, ED))).cuda()
mel, short = eng["chain"].mel_batch(audio)
out = {k: torch.empty(B, 52, device="cuda") for k in eng}

calls = {
    "forward_audio": lambda k: eng[k].forward_audio(audio, emo, out=out[k]),
    "core_forward": lambda k: eng[k].core_forward(mel, short, emo),
}
for what, call in calls.items():
    ms = {k: [] for k in eng}
    for r in range(args.rounds + 1):                          # round 0 warms up
        for k in eng:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                res = call(k)
            torch.cuda.synchronize()
            if r:
                ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
            if what == "core_forward":
                out[k] = res["blendshapes"]
    rec = {"workload": f"{what}: `{args.shape}` (d_model 128, 4 heads, window {T}, emotion_dim {ED}), hop 533, {B} windows" +
                       (f" x {L} samples" if what == "forward_audio" else f" of {mel.shape[1]} log-mel frames") +
                       f"; {args.rounds} rounds x {args.calls} calls per route, interleaved",
           "routes_agree_to_1e-6": bool((out["core128"] - out["chain"]).abs().max() < 1e-6)}
    for k in eng:
        v = np.asarray(ms[k])
        rec[k] = {"ms_per_call_median_of_rounds": round(float(np.median(v)), 4), "ms_min": round(float(v.min()), 4),
                  "ms_max": round(float(v.max()), 4), "windows_per_s": round(B / float(np.median(v)) * 1e3, 1)}
    rec["core128_over_chain"] = round(rec["core128"]["ms_per_call_median_of_rounds"] / rec["chain"]["ms_per_call_median_of_rounds"], 4)
    print(json.dumps(rec), flush=True)
