#!/usr/bin/env python3
"""What the attention maps cost in sequence mode (km_sequence_forward_attn), in ONE run, the routes alternating round by round,
medians over the rounds, at bench_seq.py's workload (CLIPS=4 clips of SECONDS=20 s, stride 1, tiles of MAX_TILE=2048 windows):

  plain        Engine.sequence_forward: blendshapes only (the ATTN = false instantiation of the fused core)
  maps         the same call with return_attention=True: raw (B, N, 52) and the maps (B, N, 28, 80) written as well
  stats_only   the same call with stats=AttentionStats(): the maps of one tile at a time, reduced on the device, never whole
  loop         what SequentialDualStreamModel.forward(audio, return_attention=True) did before: one
               SimplifiedDualStreamModel.forward(window, True, emotion) per window position (a fresh log-mel, the staged core,
               a stand-alone smoothing launch), timed on the first LOOP_WINDOWS=64 positions and scaled to all of them

(maps - plain) / windows is the cost of the ATTN block per window: eight barrier-separated rounds of LDS read-modify-write and a
9 KB store.  A round times REPS calls of one route between two device synchronisations.  Needs a GPU; prints one JSON line and,
with an argument, writes the same record to that path (profiles/seq_attention_bench.txt).
"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from koemorph_amd import synth
from koemorph_amd.metrics import AttentionStats
from koemorph_amd.model import SequentialDualStreamModel, SimplifiedDualStreamModel

assert torch.cuda.is_available(), "bench_seq_attention.py measures on a GPU"
clips, seconds, stride = int(os.environ.get("CLIPS", 4)), float(os.environ.get("SECONDS", 20)), int(os.environ.get("STRIDE", 1))
rounds, reps, max_tile = int(os.environ.get("ROUNDS", 15)), int(os.environ.get("REPS", 5)), int(os.environ.get("MAX_TILE", 2048))
loop_windows = int(os.environ.get("LOOP_WINDOWS", 64))


def alternate(routes, rounds):
    """{name: median ms per call}: every round times each route once, in turn, after one warm-up round."""
    ms = {name: [] for name in routes}
    for r in range(rounds + 1):
        for name, (fn, n) in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            if r:
                ms[name].append((time.perf_counter() - t0) / n * 1e3)
    return {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for name, v in ms.items()}


torch.manual_seed(0)
L = int(seconds * 16000)
model = SequentialDualStreamModel(stride_frames=stride).cuda().eval()
sd = {"dual_stream_attention." + k: torch.from_numpy(v) for k, v in synth.make_core_params(0).items()}
sd["smoothing_alpha"] = torch.tensor(0.8)
model.load_state_dict(sd)
eng = model.dual_stream_attention.engine()
audio = torch.from_numpy(synth.make_audio(1, clips, L, "uniform")).cuda()
emo = torch.from_numpy(synth.normal(2, (clips, 256))).cuda()
N = eng.sequence_num_outputs(L, stride)
acc = AttentionStats()


def loop():
    """The per-window route on the first `loop_windows` positions (the route this replaces walked all N)."""
    model.reset_temporal_state()
    for i in range(min(loop_windows, N)):
        s = i * model.stride_samples
        SimplifiedDualStreamModel.forward(model, audio[:, s:s + model.window_samples].contiguous(), True, emo)


def stats_only():
    acc.reset()
    eng.sequence_forward(audio, emo, stride, True, max_tile=max_tile, stats=acc)


res = {"rounds": rounds, "reps": reps, "device": torch.cuda.get_device_name(), "clips": clips, "seconds": seconds, "stride": stride,
       "windows": clips * N, "max_tile": max_tile}
t = alternate({"plain": (lambda: eng.sequence_forward(audio, emo, stride, True, max_tile=max_tile), reps),
               "maps": (lambda: eng.sequence_forward(audio, emo, stride, True, max_tile=max_tile, return_attention=True), reps),
               "stats_only": (stats_only, reps),
               "loop": (loop, 1)}, rounds)
res.update(t)
n_loop = min(loop_windows, N)
res["loop"]["positions_timed"] = n_loop
res["loop"]["scaled_to_all_positions_ms"] = round(t["loop"]["median_ms"] * N / n_loop, 2)
res["attn_block_ns_per_window"] = round((t["maps"]["median_ms"] - t["plain"]["median_ms"]) * 1e6 / (clips * N), 1)
res["stats_minus_plain_us"] = round((t["stats_only"]["median_ms"] - t["plain"]["median_ms"]) * 1e3, 2)
res["loop_over_maps"] = round(res["loop"]["scaled_to_all_positions_ms"] / t["maps"]["median_ms"], 1)
a = eng.sequence_forward(audio, emo, stride, True, max_tile=max_tile)
b = eng.sequence_forward(audio, emo, stride, True, max_tile=max_tile, return_attention=True)
res["blendshapes_bit_identical"] = bool(torch.equal(a, b["blendshapes"]))
res["stats_rows"] = acc.compute()["rows"]
line = json.dumps(res)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")
