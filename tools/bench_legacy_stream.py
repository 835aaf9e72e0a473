"""Same-run A/B of one real-time tick of SimplifiedKoeMorphModel for many streams (scripts/rt_simplified.py's loop, per stream:
RingBuffer.write(chunk), RingBuffer.read(audio_length), model(audio)):

  A  LegacyStreamEngine: FIFOs on the device, push + tick replayed as one hipGraph whose last node is the result readback; per tick
     the host uploads the chunks, replays and synchronises once.
  B  (--baseline) the route without km_legacy_stream_*: one numpy RingBuffer per stream on the host, the popped windows uploaded as
     one (n_ready, audio_length) batch, km_legacy_forward on it, the result read back.

Two schedules: chunks of audio_length samples (every stream pops a window on every tick: the heaviest tick) and chunks of
--chunk samples (the reference's default 1024: a stream pops on one tick in about 16).  Times are a host clock around work that
ends in a device synchronise, A and B interleaved round by round after a warm-up; the median and the 10th / 90th percentile over
all timed ticks (with chunks of 1024 the median tick is one on which no stream pops).  Launches per tick come from a kernel trace of a child process (rocprofv3 --kernel-trace), a run of its own.

    python tools/bench_legacy_stream.py --streams 128 --baseline --out profiles/legacy_stream_bench.txt
"""
import argparse
import collections
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                                    # noqa: E402
from koemorph_amd.model.simplified_model import SimplifiedKoeMorphModel          # noqa: E402
from koemorph_amd.scripts.rt import RingBuffer                                    # noqa: E402
from koemorph_amd.streaming import LegacyStreamEngine                             # noqa: E402
from oracle import legacy                                                         # noqa: E402


def make_model():
    m = SimplifiedKoeMorphModel().cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in legacy.make_legacy_params(7).items()})
    return m


class StreamRoute:
    def __init__(self, S, L, chunk):
        self.eng = LegacyStreamEngine(make_model(), S, audio_length=L)
        self.host_out = torch.zeros(S, 52).pin_memory()
        self.eng.capture(chunk, host_out=self.host_out)
        self.pinned = torch.zeros(S, chunk).pin_memory()

    def tick(self, chunks):
        self.pinned.copy_(torch.from_numpy(chunks))
        self.eng.replay(self.pinned)
        torch.cuda.synchronize()
        return self.host_out


class HostRoute:
    def __init__(self, S, L, chunk):
        self.model, self.L = make_model(), L
        self.rings = [RingBuffer(32000) for _ in range(S)]
        self.model(torch.zeros(S, L, device="cuda"))          # reserves the workspace for the largest batch

    def tick(self, chunks):
        wins = []
        for ring, c in zip(self.rings, chunks):
            ring.write(c)
            w = ring.read(self.L)
            if w is not None:
                wins.append(w)
        if not wins:
            return None
        out = self.model(torch.from_numpy(np.stack(wins)).cuda()).cpu()
        return out


def timed(route, data, lo, hi):
    ts = []
    for i in range(lo, hi):
        t0 = time.perf_counter()
        route.tick(data[i % len(data)])
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def trace_child(S, L, chunk, ticks, route):
    r = (StreamRoute if route == "stream" else HostRoute)(S, L, chunk)
    data = synth.make_audio(11, S, chunk)
    for _ in range(ticks):
        r.tick(data)
    torch.cuda.synchronize()


def launches(S, L, chunk, route, ticks=64):
    prof = shutil.which("rocprofv3")
    if prof is None:
        return "launches per tick not taken: rocprofv3 is not on the PATH"
    tmp = tempfile.mkdtemp(prefix="lstream_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--trace-route", route,
               "--trace-ticks", str(ticks), "--streams", str(S), "--audio-length", str(L), "--chunk", str(chunk)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if res.returncode != 0 or not files:
            return f"launches per tick not taken: the traced run ended with status {res.returncode}"
        names = collections.Counter()
        for f in files:
            for row in csv.DictReader(open(f)):
                names[row["Kernel_Name"].split("(")[0].replace("void ", "").replace("km::", "").replace("kf::", "").strip()[:40]] += 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    per = {n: c / ticks for n, c in names.items() if c >= ticks // 32}
    return f"kernels per tick over {ticks} ticks: " + ", ".join(f"{n} {v:.2f}" for n, v in sorted(per.items())) + f"; total {sum(per.values()):.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--audio-length", type=int, default=16000)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--baseline", action="store_true", help="also time the host-ring + km_legacy_forward route, interleaved")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-route", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--trace-ticks", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    S, L = a.streams, a.audio_length
    if a.trace_route:
        return trace_child(S, L, a.chunk, a.trace_ticks, a.trace_route)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    lines = [f"{S} streams, windows of {L} samples ({1 + L // 533} frames), FIFO of 32000; ms per tick, median [p10, p90]"]
    for chunk, what in ((L, "every stream pops on every tick"), (a.chunk, f"chunks of {a.chunk}: a stream pops on one tick in about {L / a.chunk:.0f}")):
        data = [synth.make_audio(20 + i, S, chunk) for i in range(4)]
        routes = {"stream": StreamRoute(S, L, chunk)}
        if a.baseline:
            routes["host"] = HostRoute(S, L, chunk)
        for r in routes.values():
            timed(r, data, 0, 48)                            # warm-up
        res = {k: [] for k in routes}
        for rnd in range(a.rounds):
            for k, r in routes.items():
                res[k] += timed(r, data, rnd * a.ticks, (rnd + 1) * a.ticks)
        lines.append(f"  chunk {chunk} ({what}), {a.rounds * a.ticks} ticks per route:")
        names = {"stream": "LegacyStreamEngine: graph replay, one sync", "host": "host rings + upload + km_legacy_forward"}
        for k, v in res.items():
            lines.append(f"    {names[k]:44s} {np.median(v):8.3f} [{np.percentile(v, 10):.3f}, {np.percentile(v, 90):.3f}]")
        if a.baseline:
            lines.append(f"    host route / stream route: {np.median(res['host']) / np.median(res['stream']):.2f}x")
        del routes
        torch.cuda.synchronize()
        if not a.no_trace:
            for k in (("stream", "host") if a.baseline else ("stream",)):
                lines.append(f"    {k}: " + launches(S, L, chunk, k))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
