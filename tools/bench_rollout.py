#!/usr/bin/env python3
"""KoeMorphModel.rollout against the loop it replaces (one ``forward`` per frame, the output fed back), default width, T = 30.

Both run interleaved in one process, a host clock around synchronised calls; medians of ROUNDS (15) rounds with minimum and maximum.
Cells: B in {1, 16, 128} clips of 300 frames and one clip of 1800 frames, chunk_frames in {64, 256, 1024}.  ``ONLY=rollout`` runs one
rollout per cell and nothing else (the form to put behind a kernel trace); CELLS="1x300,16x300" picks cells."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koemorph_amd import synth
from koemorph_amd.model import KoeMorphModel

T = 30
ROUNDS = int(os.environ.get("ROUNDS", 15))
CHUNKS = [int(c) for c in os.environ.get("CHUNKS", "64,256,1024").split(",")]
CELLS = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("CELLS", "1x300,16x300,128x300,1x1800").split(",")]
ONLY = os.environ.get("ONLY", "")

cfg = synth.KoeMorphConfig()
params = synth.make_koemorph_params(5, cfg)
m = KoeMorphModel(d_query=cfg.d_model)
sd = m.state_dict(); sd.update({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}); m.load_state_dict(sd)
m = m.cuda().eval()


def loop(mel, emo):
    prev = None
    for i in range(mel.shape[1]):
        s = max(0, i - T + 1)
        prev = m(mel[:, s:i + 1].contiguous(), emo[:, s:i + 1].contiguous(), prev_blendshapes=prev)["blendshapes"]
    return prev


def timed(fn):
    m.reset_temporal_state()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


with torch.no_grad():
    for B, F in CELLS:
        mel = torch.from_numpy(synth.normal(1, (B, F, cfg.mel_dim))).cuda()
        emo = torch.from_numpy(synth.normal(2, (B, F, cfg.emotion_dim))).cuda()
        if ONLY == "rollout":
            for chunk in CHUNKS:
                timed(lambda: m.rollout(mel, emo, context_frames=T, chunk_frames=chunk))
            continue
        rounds = max(3, ROUNDS // 3) if B * F >= 128 * 300 else ROUNDS      # the loop of the largest cell takes seconds per round
        times = {"loop": []}
        for chunk in CHUNKS:                                                 # warm-up: reserves, first launches
            m.reset_temporal_state()
            m.rollout(mel, emo, context_frames=T, chunk_frames=chunk)
            times[chunk] = []
        for _ in range(rounds):
            times["loop"].append(timed(lambda: loop(mel, emo)))
            for chunk in CHUNKS:
                times[chunk].append(timed(lambda: m.rollout(mel, emo, context_frames=T, chunk_frames=chunk)))
        base = statistics.median(times["loop"])
        row = {"clips": B, "frames": F, "rounds": rounds, "loop": stats(times["loop"])}
        for chunk in CHUNKS:
            row[f"rollout_chunk{chunk}"] = dict(stats(times[chunk]), loop_over_rollout=round(base / statistics.median(times[chunk]), 2),
                                                us_per_frame=round(statistics.median(times[chunk]) * 1e3 / F, 1))
        print(json.dumps(row), flush=True)
