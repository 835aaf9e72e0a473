"""Same-run A/B of one tick of KoeMorphModel streams FROM AUDIO, three paths interleaved in ONE process.  A tick is one push of
``hop`` samples per stream (one frame per stream), every stream past its warm-up (a full emotion window, full model windows):

  push    KoeMorphAudioStreams.push, eager: seven launches for the rows (km_koemorph_audio_rows), four for the step.
  replay  the same push as a hipGraph replay (capture / replay).
  dense   the yardstick, whose launches are the parent's: each stream's last ``emotion_window`` seconds kept on the device as a
          (N, W) tensor the host rolls by ``hop`` per tick, the dense ``MelSpectrogramExtractor`` and ``EGeMAPSEngine.llds(fps=fps)`` on
          it, the newest row of each picked, ``KoeMorphStreams.step``.  What a user could do before the engine.

Times are a host clock around work that ends in a device synchronise; per round each path runs --ticks ticks and the round's figure is
the mean tick; the file holds the median, minimum and maximum over --rounds rounds (15) after a warm-up, and the margin of the median
against the frame period 1 / fps.  No ratio is fixed in advance: every cell is reported.

    python tools/bench_koemorph_audio.py --out profiles/koemorph_audio_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                                    # noqa: E402
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine               # noqa: E402
from koemorph_amd.features.stft import MelSpectrogramExtractor                    # noqa: E402
from koemorph_amd.model import KoeMorphModel                                      # noqa: E402
from koemorph_amd.streaming import KoeMorphAudioStreams, KoeMorphStreams          # noqa: E402

STREAMS = (1, 16, 128)


def make_model(seed=7):
    torch.manual_seed(seed)
    return KoeMorphModel(d_query=256).cuda().eval()


class Pushed:
    def __init__(self, N, fps, window, T, replay):
        self.eng = KoeMorphAudioStreams(make_model(), N, fps=fps, context_frames=T, emotion_window=window, max_samples=int(16000 / fps))
        self.replay = replay
        if replay:
            self.eng.push(torch.zeros(N, self.eng.hop, device="cuda"))
            self.eng.capture(self.eng.hop)

    def tick(self, x):
        (self.eng.replay if self.replay else self.eng.push)(x)

    def close(self):
        self.eng.close()


class Dense:
    def __init__(self, N, fps, window, T):
        self.hop, self.fps = int(16000 / fps), fps
        self.win = torch.zeros(N, int(window * 16000), device="cuda")
        self.mel = MelSpectrogramExtractor(target_fps=fps)
        self.egm = EGeMAPSEngine("cuda")
        self.eng = KoeMorphStreams(make_model(), N, context_frames=T, max_rows=1)
        self.row = self.win.shape[1] // self.hop - 1

    def tick(self, x):
        self.win = torch.roll(self.win, -self.hop, 1)
        self.win[:, -self.hop:] = x
        mel = self.mel(self.win)[:, self.row]
        emo = self.egm.llds(self.win, fps=self.fps)[:, self.row]
        self.eng.step(mel, emo)

    def close(self):
        self.eng.close()
        self.egm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--context", type=int, default=30)
    ap.add_argument("--streams", type=int, nargs="*", default=list(STREAMS))
    ap.add_argument("--only", default=None, help="run one path alone, without timing it (for a kernel trace): push | replay | dense")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    hop, period = int(16000 / a.fps), 1e3 / a.fps
    lines = [f"KoeMorphModel streams from audio, default width, {a.fps:g} fps (hop {hop}), emotion window {a.window:g} s, context {a.context}; ms per "
             f"tick (one push of {hop} samples = one frame per stream): median [min, max] over {a.rounds} rounds of {a.ticks} ticks, the three "
             f"paths interleaved round by round in one process; frame period {period:.2f} ms"]
    warm = int(a.window * 16000) // hop + a.context + 2
    for N in a.streams:
        x = torch.from_numpy(0.1 * synth.normal(5, (N, hop))).cuda()
        paths = {"push": lambda: Pushed(N, a.fps, a.window, a.context, False), "replay": lambda: Pushed(N, a.fps, a.window, a.context, True),
                 "dense": lambda: Dense(N, a.fps, a.window, a.context)}
        if a.only:
            paths = {a.only: paths[a.only]}
        paths = {k: make() for k, make in paths.items()}
        for p in paths.values():
            for _ in range(warm):
                p.tick(x)
        torch.cuda.synchronize()
        res = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, p in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.ticks):
                    p.tick(x)
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e3 / a.ticks)
        lines.append(f"  N {N:4d}")
        names = {"push": "KoeMorphAudioStreams.push, eager (7 + 4 launches)", "replay": "KoeMorphAudioStreams.replay (hipGraph)",
                 "dense": "yardstick: rolled windows, dense mel + llds, step"}
        for k, v in res.items():
            med = float(np.median(v))
            lines.append(f"    {names[k]:52s} {med:8.3f} [{min(v):.3f}, {max(v):.3f}]   {period / med:6.1f}x inside the frame period")
        if "dense" in res and "push" in res:
            y = np.median(res["dense"])
            lines.append(f"    yardstick / push {y / np.median(res['push']):.2f}x, yardstick / replay {y / np.median(res['replay']):.2f}x")
        for p in paths.values():
            p.close()
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
