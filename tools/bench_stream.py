#!/usr/bin/env python3
"""BASELINE config 5 on ONE GPU: 128 concurrent speaker streams, per-tick decode under a hipGraph.
Prints ticks/s and p50/p99 tick latency (host wall clock around replay + the 26 KB result readback).

Default: the 30 fps shape (d_model 256, 8 heads, window 256, 533-sample frames).  ``--d-model 512 --heads 8|16 --fps 60``: the 60 fps
long-context shape (window 512, 8.5 s ring of hop 266, 267-sample frames).  ``--baseline`` adds what a caller had to do at that shape
before the stream path covered it: rings kept outside the library, unrolled into 128 chronological windows per tick, km_forward_audio
on them with the EMA state (km_smooth behind the generic core), and the same readback -- timed the same way."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koemorph_amd import synth
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.streaming import StreamEngine

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--ticks", type=int, default=1000)
ap.add_argument("--d-model", type=int, default=256, choices=(256, 512))
ap.add_argument("--heads", type=int, default=8, choices=(8, 16))
ap.add_argument("--fps", type=int, default=30, choices=(30, 60))
ap.add_argument("--baseline", action="store_true", help="also time host-side rings + forward_audio + EMA per tick")
args = ap.parse_args()
S = args.streams
if args.d_model == 256:
    eng = Engine(); eng.load_state_dict(synth.make_core_params(0)); eng.finalize()
else:
    eng = Engine(d_model=512, num_heads=args.heads, mel_sequence_length=512, mel=MelConfig.model_batch(target_fps=args.fps))
    eng.load_state_dict(synth.make_core_params(0, 512, 512)); eng.finalize()
se = StreamEngine(eng, S) if args.fps == 30 else StreamEngine(eng, S, update_interval=1.0 / args.fps)
n = se.ring_hop + 1                                    # 533 / 267 samples per stream and tick
fill = se.shape["ring_len"] // se.ring_hop + 3
frames = torch.from_numpy(synth.make_audio(1, S, n * 8, "uniform")).cuda()
emo = torch.from_numpy(synth.normal(2, (S, 256))).cuda()
for t in range(fill):                                  # fill the rings (eager)
    se.push(frames[:, (t % 8) * n:(t % 8 + 1) * n]); se.tick(emo)
host_out = torch.empty(S, 52, pin_memory=True)
se.capture(n, host_out=host_out)


def timed(step):
    lat = []
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for t in range(args.ticks):
        t0 = time.perf_counter()
        step(t)
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    return time.perf_counter() - t_all, np.array(lat) * 1e3


t_all, lat = timed(lambda t: se.replay(frames[:, (t % 8) * n:(t % 8 + 1) * n], emo))
shape = f"d_model {args.d_model}, {args.heads} heads, {args.fps} fps"
res = {"workload": f"C5: {S} streams/GPU ({shape}), one {n}-sample frame per stream per tick, hipGraph replay + D2H of {S}x52 floats",
       "ticks_per_s": round(args.ticks / t_all, 1), "frames_per_s": round(args.ticks * S / t_all, 1),
       "tick_ms_mean": round(t_all / args.ticks * 1e3, 4),
       "tick_latency_ms_p50": round(float(np.percentile(lat, 50)), 4),
       "tick_latency_ms_p99": round(float(np.percentile(lat, 99)), 4),
       "realtime_budget_ms": round(1000.0 / args.fps, 1), "all_ready": bool(se.ready.cpu().all())}
if args.baseline:
    L, hop = se.shape["ring_len"], se.ring_hop
    ring = torch.zeros(S, L, device="cuda")
    win = torch.empty(S, L, device="cuda")
    state = torch.zeros(S, 52, device="cuda")
    out = torch.empty(S, 52, device="cuda")
    eng.reserve(S, L)
    wptr, calls = 0, 0

    def host_rings(t):
        global wptr, calls
        f = frames[:, (t % 8) * n:(t % 8 + 1) * n]     # the same n-sample frame the stream path is handed; the ring keeps hop of them
        k = min(hop, L - wptr)
        ring[:, wptr:wptr + k] = f[:, :k]
        if k < hop:
            ring[:, :hop - k] = f[:, k:hop]
        wptr = (wptr + hop) % L
        win[:, :L - wptr] = ring[:, wptr:]             # chronological order
        win[:, L - wptr:] = ring[:, :wptr]
        eng.forward_audio(win, emo, state=state, first=(calls == 0), out=out)
        calls += 1
        host_out.copy_(out, non_blocking=True)

    for t in range(20):
        host_rings(t)
    b_all, b_lat = timed(host_rings)
    res["baseline_forward_audio_tick_ms_mean"] = round(b_all / args.ticks * 1e3, 4)
    res["baseline_forward_audio_tick_ms_p50"] = round(float(np.percentile(b_lat, 50)), 4)
    res["baseline_note"] = "per tick: 2-4 torch slice copies (ring write, unroll into chronological windows), km_forward_audio with EMA state, D2H"
print(json.dumps(res))
