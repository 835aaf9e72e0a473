"""Same-run A/B of the emotion half of a real-time tick for many streams in lockstep (every stream receives one chunk per tick and
is due on every ninth tick):

  A  StreamEmotion: rings, update rule, slots and Linear(264, 256) on the device; push + update replayed as one hipGraph; per tick
     the host uploads the chunks, replays and synchronises once.  With --max-updates below the stream count the due streams are
     served over several ticks, longest waiting first.
  B  the route without km_emotion_stream_*: one mirror OpenSMILEeGeMAPSExtractor per stream (host AudioBuffer, upload of the 20 s
     window, km_egemaps_functionals with B = 1, 88 floats back, km_linear with B = 1) driven by process_audio_frame with an
     audio-time clock.

The rings are filled with 22.5 s of audio first, so every window is a full 20 s one (1 995 frames).  Times are a host clock around
work that ends in a device synchronise, A and B interleaved cycle by cycle after a warm-up; per route the median and the worst tick
and the mean over all ticks.  Then the time of one update call that selects 1, 8 and all streams' windows (eager launches, one
synchronise), median of --calls calls.

    python tools/bench_stream_emotion.py --streams 128 --max-updates 8 128 --out profiles/stream_emotion_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                                              # noqa: E402
from koemorph_amd.features.opensmile_extractor import OpenSMILEeGeMAPSExtractor             # noqa: E402
from koemorph_amd.streaming import StreamEmotion                                            # noqa: E402

SR, CHUNK, CYCLE = 16000, 534, 9          # 9 x 534 = 4806 >= 4800: due on every ninth tick
PREFILL = 80000


def layer():
    torch.manual_seed(0)
    return torch.nn.Linear(264, 256)


class DeviceRoute:
    def __init__(self, S, max_updates, prefill):
        self.se = StreamEmotion(S, max_updates=max_updates, compression_layer=layer())
        for x in prefill:
            self.se.push(torch.from_numpy(x).cuda())
        self.se.update()                                     # first launches outside the capture
        torch.cuda.synchronize()
        self.se.capture(CHUNK)
        self.pinned = torch.zeros(S, CHUNK).pin_memory()
        self.updates = 0

    def tick(self, chunks):
        self.pinned.copy_(torch.from_numpy(chunks))
        _, upd = self.se.replay(self.pinned)
        torch.cuda.synchronize()
        return upd


class HostRoute:
    def __init__(self, S, prefill):
        self.now = [0.0]
        lin = layer()
        self.ex = [OpenSMILEeGeMAPSExtractor(use_concatenation=True, device="cuda", clock=lambda: self.now[0]) for _ in range(S)]
        for e in self.ex:
            e.compression_layer = lin
        for x in prefill:
            for e, row in zip(self.ex, x):
                e.audio_buffer.append(row)
            self.now[0] += x.shape[1] / SR
        self.out = np.zeros((S, 256), np.float32)

    def tick(self, chunks):
        self.now[0] += CHUNK / SR
        for s, (e, row) in enumerate(zip(self.ex, chunks)):
            before = e.total_updates
            e.process_audio_frame(row)
            if e.total_updates != before:
                self.out[s] = e.get_concatenated_features()
        return self.out


def stats(ts):
    return f"median {np.median(ts):9.3f}   worst {np.max(ts):9.3f}   mean {np.mean(ts):9.3f}"


def update_call(S, k, prefill, calls):
    se = StreamEmotion(S, max_updates=k, compression_layer=layer())
    for x in prefill:
        se.push(torch.from_numpy(x).cuda())
    fresh = torch.from_numpy(synth.make_audio(5, S, 4800)).cuda()
    ts = []
    for i in range(calls + 3):
        se.push(fresh)                                       # everybody is due again
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, upd = se.update()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
        assert int(upd.sum()) == k
    se.close()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--max-updates", type=int, nargs="+", default=[8, 128])
    ap.add_argument("--cycles", type=int, default=12, help="timed cycles of nine ticks per route")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    S = a.streams
    caps = [min(k, S) for k in a.max_updates]
    prefill = [synth.make_audio(30 + i, S, PREFILL) for i in range(5)]
    data = [synth.make_audio(50 + i, S, CHUNK) for i in range(CYCLE)]
    routes = {f"StreamEmotion, max_updates {k}": DeviceRoute(S, k, prefill) for k in caps}
    if not a.no_baseline:
        routes["one mirror extractor per stream"] = HostRoute(S, prefill)
    res = {k: [] for k in routes}
    for cyc in range(a.cycles + 2):
        for name, r in routes.items():
            for i in range(CYCLE):
                t0 = time.perf_counter()
                r.tick(data[i])
                if cyc >= 2:                                 # two cycles of warm-up
                    res[name].append((time.perf_counter() - t0) * 1e3)
    lines = [f"{S} streams in lockstep, 20 s windows (1995 frames), chunks of {CHUNK} samples, every stream due on every ninth tick;",
             f"ms per tick over {a.cycles * CYCLE} ticks per route, routes interleaved cycle by cycle"]
    for name, ts in res.items():
        lines.append(f"  {name:36s} {stats(ts)}")
    del routes
    torch.cuda.synchronize()
    lines.append(f"one update call (eager, synchronised), all {S} streams due, median of {a.calls} calls:")
    for k in sorted({1, min(8, S), S}):
        ms = update_call(S, k, prefill, a.calls)
        lines.append(f"  selects {k:4d} windows: {ms:9.3f} ms   ({ms / k:.3f} ms per window)")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
