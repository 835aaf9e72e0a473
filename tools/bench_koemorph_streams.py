"""Same-run A/B of one tick of KoeMorphModel streams, three paths interleaved in ONE process:

  step    KoeMorphStreams.step, eager: the rings on the device, one ragged four-launch step per tick (km_koemorph_stream_step).
  replay  the same step as a hipGraph replay (capture / replay).
  roll    the yardstick, whose launches are the parent's: ``forward`` at B = N on a device-resident (N, T, .) window that the host
          rolls by one row per tick (torch.roll + a row copy), prev fed back.  What a user could do before the engine, and only for
          streams in phase.  A cell with max_rows = R renders R frames per stream and is set against R yardstick ticks.

Every stream stands past its warm-up (full windows of T rows), the heaviest steady state.  Times are a host clock around work that ends
in a device synchronise; per round each path runs --ticks ticks and the round's figure is the mean tick; the file holds the median,
minimum and maximum over --rounds rounds (15) after a warm-up.  No ratio is fixed in advance: every cell is reported.

    python tools/bench_koemorph_streams.py --out profiles/koemorph_streams_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                    # noqa: E402
from koemorph_amd.model import KoeMorphModel                      # noqa: E402
from koemorph_amd.streaming import KoeMorphStreams                # noqa: E402

CELLS = [(1, 30, 1), (16, 30, 1), (128, 30, 1), (16, 30, 2), (16, 30, 8)]


def make_model(seed=7):
    torch.manual_seed(seed)
    return KoeMorphModel(d_query=256).cuda().eval()


class Engine:
    def __init__(self, N, T, R, replay):
        self.eng = KoeMorphStreams(make_model(), N, context_frames=T, max_rows=R)
        self.replay = replay
        if replay:
            self.eng.capture()

    def warm(self, mel, emo, T):
        for i in range(-(-T // self.eng.max_rows) + 1):          # past the warm-up frames: every window is full
            self.tick(mel, emo)

    def tick(self, mel, emo):
        (self.eng.replay if self.replay else self.eng.step)(mel, emo)


class Rolled:
    """forward at B = N on a (N, T, .) window rolled by one row per tick; R ticks per call of ``tick``."""

    def __init__(self, N, T, R):
        self.m, self.R = make_model(), R
        self.mel = torch.zeros(N, T, 80, device="cuda")
        self.emo = torch.zeros(N, T, 256, device="cuda")
        self.prev = None

    def warm(self, mel, emo, T):
        for i in range(3):
            self.tick(mel, emo)

    def tick(self, mel, emo):
        with torch.no_grad():
            for j in range(self.R):
                self.mel = torch.roll(self.mel, -1, 1); self.mel[:, -1] = mel[:, j]
                self.emo = torch.roll(self.emo, -1, 1); self.emo[:, -1] = emo[:, j]
                self.prev = self.m(self.mel, self.emo, prev_blendshapes=self.prev)["blendshapes"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    lines = [f"KoeMorphModel streams, default width; ms per tick of max_rows frames per stream: median [min, max] over {a.rounds} rounds of "
             f"{a.ticks} ticks, the three paths interleaved round by round in one process"]
    for N, T, R in CELLS:
        mel = torch.from_numpy(synth.normal(3, (N, R, 80))).cuda()
        emo = torch.from_numpy(synth.normal(4, (N, R, 256))).cuda()
        paths = {"step": Engine(N, T, R, False), "replay": Engine(N, T, R, True), "roll": Rolled(N, T, R)}
        for p in paths.values():
            p.warm(mel, emo, T)
        torch.cuda.synchronize()
        res = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, p in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.ticks):
                    p.tick(mel, emo)
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3 / a.ticks)
        lines.append(f"  N {N:4d}  T {T}  max_rows {R}  ({N * R} frames per tick; yardstick: {R} forward calls at B = {N})")
        names = {"step": "KoeMorphStreams.step, eager (4 launches)", "replay": "KoeMorphStreams.replay (hipGraph)",
                 "roll": f"yardstick: roll + forward at B = N, x{R}"}
        for k, v in res.items():
            lines.append(f"    {names[k]:44s} {np.median(v):8.3f} [{min(v):.3f}, {max(v):.3f}]")
        y = np.median(res["roll"])
        lines.append(f"    yardstick / step {y / np.median(res['step']):.2f}x, yardstick / replay {y / np.median(res['replay']):.2f}x")
        for p in paths.values():
            if isinstance(p, Engine):
                p.eng.close()
        del paths
        torch.cuda.synchronize()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
