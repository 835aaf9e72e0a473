"""Same-run timing of the device resampler (km_resampler_* / km_resample_clip) against the routes there were before it.

  (a) a live tick of many streams at 48 kHz: every stream brings 1600 samples (1/30 s) per tick
        16k    the tick on 16 kHz input: upload of (streams, 534) + replayed feed + step            (no conversion at all)
        dev    upload of (streams, 1600) + replayed StreamResampler.push + feed + step             (dev - 16k = the added cost)
        host   scipy.signal.resample_poly per stream on the host (stateless: every chunk's edges are zero-padded), upload of
               (streams, 534) + replayed feed + step                                               (the route before)
      The rings are filled first, so every step fires every stream.
  (b) a 60 s clip at 48 000 and at 44 100 Hz, from float32 samples in host memory to a resident 16 kHz clip
        dev    upload at the native rate + Resampler.clip
        host   the conversion of data/sequential_dataset.py's _load_wav (resample_poly, float32) + upload

Times are a host clock around work that ends in a device synchronise; the routes are interleaved round by round after a warm-up and
each figure is the median of --rounds rounds (a round of (a) is the mean over --ticks ticks).

    python tools/bench_resample.py --out profiles/resample_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                                              # noqa: E402
from koemorph_amd.engine import Engine                                                      # noqa: E402
from koemorph_amd.features import Resampler                                                 # noqa: E402
from koemorph_amd.streaming import ChunkedStreamEngine, StreamResampler                     # noqa: E402

RATE_IN, CHUNK_IN, CHUNK_OUT = 48000, 1600, 534
PREFILL_TICKS = 262                       # 256 frames fill the 8.5 s ring
SRC_TICKS = 64                            # the audio source holds this many ticks and is read round and round


def resample_poly():
    try:
        from scipy.signal import resample_poly as f
        return f
    except ImportError:
        return None


class Tick:
    """One ChunkedStreamEngine with a captured tick; kind: '16k', 'dev' or 'host'."""

    def __init__(self, kind, S, audio48, audio16):
        self.kind, self.S = kind, S
        e = Engine()
        e.load_state_dict(synth.make_core_params(61, style="trained"))
        e.finalize()
        self.se = ChunkedStreamEngine(e, S)
        self.emotion = torch.from_numpy(synth.normal(7, (S, 256))).cuda()
        self.rs = StreamResampler(S, RATE_IN) if kind == "dev" else None
        n = CHUNK_IN if kind == "dev" else CHUNK_OUT
        self.x_static = torch.zeros(S, n, device="cuda")
        self.c_static = torch.full((S,), 533, dtype=torch.int32, device="cuda")
        self.pinned = torch.zeros(S, n).pin_memory()
        for t in range(PREFILL_TICKS):                       # eager: fills the rings, creates every buffer
            self._load(t, audio48, audio16)
            self.x_static.copy_(self.pinned)
            self._chain()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._chain()

    def _chain(self):
        if self.rs is not None:
            out, counts = self.rs.push(self.x_static)
            self.se.feed(out, counts)
        else:
            self.se.feed(self.x_static, self.c_static)
        self.se.step(self.emotion)

    def _load(self, t, audio48, audio16):
        t %= SRC_TICKS
        if self.kind == "dev":
            self.pinned.copy_(torch.from_numpy(audio48[:, t * CHUNK_IN:(t + 1) * CHUNK_IN]))
        elif self.kind == "16k":
            self.pinned[:, :533].copy_(torch.from_numpy(audio16[:, t * 533:(t + 1) * 533]))
        else:
            chunk = audio48[:, t * CHUNK_IN:(t + 1) * CHUNK_IN]
            poly = resample_poly()
            for s in range(self.S):
                self.pinned[s].copy_(torch.from_numpy(poly(chunk[s], 1, 3).astype(np.float32)))

    def tick(self, t, audio48, audio16):
        self._load(t, audio48, audio16)
        self.x_static.copy_(self.pinned, non_blocking=True)
        self.graph.replay()
        torch.cuda.synchronize()
        return self.se.fired


def bench_ticks(S, rounds, ticks, lines):
    audio48 = synth.make_audio(41, S, SRC_TICKS * CHUNK_IN)
    audio16 = synth.make_audio(42, S, SRC_TICKS * 533)
    kinds = ["16k", "dev"] + (["host"] if resample_poly() is not None else [])
    routes = {k: Tick(k, S, audio48, audio16) for k in kinds}
    per = {k: [] for k in kinds}
    t = PREFILL_TICKS
    for r in range(rounds + 2):                              # two warm-up rounds
        for k in kinds:
            t0 = time.perf_counter()
            for i in range(ticks):
                fired = routes[k].tick(t + i, audio48, audio16)
            dt = (time.perf_counter() - t0) / ticks * 1e3
            assert bool(fired.all()), k
            if r >= 2:
                per[k].append(dt)
        t += ticks
    med = {k: float(np.median(v)) for k, v in per.items()}
    lines.append(f"(a) {S} streams, {CHUNK_IN} samples at {RATE_IN} Hz per stream and tick, every stream fires; ms per tick,")
    lines.append(f"    median of {rounds} rounds of {ticks} ticks, routes interleaved round by round")
    lines.append(f"  16 kHz input: upload + replayed feed + step                        {med['16k']:9.3f}")
    lines.append(f"  48 kHz input: upload + replayed push + feed + step                 {med['dev']:9.3f}   "
                 f"(added by the resampler: {med['dev'] - med['16k']:+.3f})")
    if "host" in med:
        lines.append(f"  48 kHz input: resample_poly per stream on the host, upload, replay {med['host']:9.3f}")
    else:
        lines.append("  48 kHz input: resample_poly per stream on the host, upload, replay  not measured (no scipy)")


def bench_clips(rounds, lines):
    poly = resample_poly()
    lines.append(f"(b) a 60 s clip, float32 samples in host memory -> resident 16 kHz clip; ms, median of {rounds} rounds, routes interleaved")
    for rate, (up, down) in ((48000, (1, 3)), (44100, (160, 441))):
        x = synth.make_audio(43, 1, rate * 60)[0].astype(np.float32)
        r = Resampler(rate)
        per = {"dev": [], "host": []}
        for i in range(rounds + 2):
            t0 = time.perf_counter()
            y = r.clip(torch.from_numpy(x).cuda())
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert y.shape[0] == 16000 * 60
            if i >= 2:
                per["dev"].append(dt)
            if poly is not None:
                t0 = time.perf_counter()
                z = torch.from_numpy(poly(x, up, down).astype(np.float32)).cuda()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                assert z.shape == y.shape
                if i >= 2:
                    per["host"].append(dt)
        host = f"{np.median(per['host']):9.3f}" if per["host"] else "not measured (no scipy)"
        lines.append(f"  {rate} Hz: upload + Resampler.clip {np.median(per['dev']):9.3f}     host resample_poly + upload {host}")
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    bench_ticks(args.streams, args.rounds, args.ticks, lines)
    bench_clips(args.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
