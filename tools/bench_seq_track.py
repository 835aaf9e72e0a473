#!/usr/bin/env python3
"""Sequence mode with an emotion track (km_sequence_forward_track) and the batched track build (km_emotion_clip_build_batch),
each against the route it stands beside, in ONE run, the two routes of a pair alternating round by round, medians over the rounds:

  sequence   one vector per clip (km_sequence_forward) | a (clips, K, 256) track (km_sequence_forward_track), at bench_seq.py's
             workload (CLIPS=4 clips of SECONDS=20 s, stride 1, tiles of 256 windows); the track route adds the per-window
             logit kernel as one dependent launch and runs the emotion branch on clips * K rows instead of clips
  build      a loop of ClipEmotion.build over BUILD_CLIPS=8 clips of BUILD_SECONDS=10 s | one ClipEmotion.build_batch of them, at
             the default 20 s / 0.3 s shape and 64 slots per pass; the outputs are compared bit for bit

A round times REPS calls of one route between two device synchronisations.  Needs a GPU; prints one JSON line and, with an
argument, writes the same record to that path (profiles/seq_track_bench.txt).
"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from koemorph_amd import synth
from koemorph_amd.engine import Engine
from koemorph_amd.features import ClipEmotion

assert torch.cuda.is_available(), "bench_seq_track.py measures on a GPU"
clips, seconds, stride = int(os.environ.get("CLIPS", 4)), float(os.environ.get("SECONDS", 20)), int(os.environ.get("STRIDE", 1))
bclips, bseconds = int(os.environ.get("BUILD_CLIPS", 8)), float(os.environ.get("BUILD_SECONDS", 10))
rounds, reps = int(os.environ.get("ROUNDS", 15)), int(os.environ.get("REPS", 5))


def alternate(routes, rounds, reps):
    """{name: median ms per call}: every round times each route once, in turn, after one warm-up round."""
    ms = {name: [] for name in routes}
    for r in range(rounds + 1):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            if r:
                ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    return {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for name, v in ms.items()}


torch.manual_seed(0)
ce = ClipEmotion()
res = {"rounds": rounds, "reps": reps, "device": torch.cuda.get_device_name()}

# ---- sequence: one vector per clip | a track ----
L = int(seconds * 16000)
eng = Engine(); eng.load_state_dict(synth.make_core_params(0)); eng.finalize()
audio = torch.from_numpy(synth.make_audio(1, clips, L, "uniform")).cuda()
emo = torch.from_numpy(synth.normal(2, (clips, 256))).cuda()
K = ce.num_rows(L)
track = emo[:, None, :].expand(clips, K, 256).contiguous()        # constant rows: the two routes must give the same bytes
first, interval = ce.shape["min_samples"], ce.shape["update_samples"]
seq = alternate({"vector_per_clip": lambda: eng.sequence_forward(audio, emo, stride, True, max_tile=256),
                 "track": lambda: eng.sequence_forward_track(audio, track, first, interval, stride, True, max_tile=256)}, rounds, reps)
a = eng.sequence_forward(audio, emo, stride, True, max_tile=256)
b = eng.sequence_forward_track(audio, track, first, interval, stride, True, max_tile=256)
res["sequence"] = dict(seq, clips=clips, seconds=seconds, stride=stride, windows=int(a.shape[0] * a.shape[1]), track_rows=K,
                       bit_identical=bool(torch.equal(a, b)),
                       track_minus_vector_us=round((seq["track"]["median_ms"] - seq["vector_per_clip"]["median_ms"]) * 1e3, 2))

# ---- build: a loop of build | build_batch ----
Lb = int(bseconds * 16000)
batch = torch.from_numpy(synth.make_audio(3, bclips, Lb)).cuda()
Kb = ce.num_rows(Lb)
bld = alternate({"build_loop": lambda: [ce.build(batch[c]) for c in range(bclips)], "build_batch": lambda: ce.build_batch(batch)}, rounds, reps)
loop = torch.stack([ce.build(batch[c])[0] for c in range(bclips)])
one, _ = ce.build_batch(batch)
res["build"] = dict(bld, clips=bclips, seconds=bseconds, rows_per_clip=Kb, max_slots=ce.max_slots,
                    passes_loop=bclips * -(-Kb // ce.max_slots), passes_batch=-(-bclips * Kb // ce.max_slots),
                    bit_identical=bool(torch.equal(loop, one)),
                    loop_over_batch=round(bld["build_loop"]["median_ms"] / bld["build_batch"]["median_ms"], 3))
line = json.dumps(res)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")
