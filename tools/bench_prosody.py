"""The `basic` prosodic emotion features next to what already runs (context, not thresholds).  Medians of --rounds rounds, the routes
of a section interleaved round by round; every time is a host clock around work that ends in a device synchronise.

  1  one StreamEmotion.update call that selects 1, 8 and 128 windows of 8.5 s (eager launches), basic back end next to the eGeMAPS
     back end for the same selection in the same run
  2  one replayed tick at the `basic` shape (d_model 128, 4 heads, window 256, emotion_dim 9): ChunkedStreamEngine.feed + step in one
     graph, with and without StreamEmotion(backend="basic").push + update in front of it in the same graph; three times as many
     ticks, median and worst (in lockstep every stream is due on the same tick, one in nine)
  3  BasicEmotion on 256 dense windows of 8.5 s

    python tools/bench_prosody.py --out profiles/prosody_bench.txt
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
from koemorph_amd.features import BasicEmotion                                              # noqa: E402
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEmotion                       # noqa: E402

SR, CONTEXT, WINDOW, FRAME = 16000, 8.5, 136000, 533


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def layer():
    torch.manual_seed(0)
    return torch.nn.Linear(264, 256)


def update_routes(S, k):
    """Two emotion-stream objects with full 8.5 s windows; a call makes every stream due again and times one update of k windows."""
    out = {}
    fill = [torch.from_numpy(synth.make_audio(30 + i, S, 42000)).cuda() for i in range(4)]        # 10.5 s: the ring, once
    fresh = torch.from_numpy(synth.make_audio(5, S, 4800)).cuda()
    for name, kw in (("basic", dict(backend="basic")), ("eGeMAPS", dict(compression_layer=layer()))):
        se = StreamEmotion(S, CONTEXT, 0.3, max_updates=k, **kw)
        for x in fill:
            se.push(x)
        se.update()

        def call(se=se):
            se.push(fresh)
            torch.cuda.synchronize()
            ms = timed(se.update)
            assert int(se.updated.sum()) == k
            return ms
        out[name] = (call, se)
    return out


def engine_basic():
    from koemorph_amd.synth import make_core_params
    e = Engine(d_model=128, num_heads=4, mel_sequence_length=256, emotion_dim=9)
    e.load_state_dict(make_core_params(93, 128, 256, 9, "trained"))
    e.finalize()
    return e


def tick_routes(S):
    """feed + step replayed as one graph, the emotion matrix a constant (A) or produced by the basic streams in the same graph (B)."""
    audio = synth.make_audio(77, S, FRAME * 300)
    out = {}
    for name in ("tick alone", "tick + basic emotion stream"):
        ce = ChunkedStreamEngine(engine_basic(), S, context_window=CONTEXT)
        se = StreamEmotion(S, CONTEXT, 0.3, backend="basic") if "emotion" in name else None
        emo = se.emotion if se is not None else torch.from_numpy(synth.normal(3, (S, 9))).cuda()
        x_static = torch.zeros(S, FRAME, device="cuda")
        for t in range(270):                                                     # 8.99 s: rings full, streams firing
            x = torch.from_numpy(audio[:, t * FRAME:(t + 1) * FRAME].copy()).cuda()
            if se is not None:
                se.push(x)
                se.update()
            ce.feed(x)
            ce.step(emo)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            if se is not None:
                se.push(x_static)
                se.update()
            ce.feed(x_static)
            ce.step(emo)
        state = dict(t=270)

        def call(g=g, x_static=x_static, state=state, ce=ce):
            t = 270 + state["t"] % 30
            state["t"] += 1
            x_static.copy_(torch.from_numpy(audio[:, t * FRAME:(t + 1) * FRAME].copy()))
            ms = timed(g.replay)
            assert bool(ce.fired.all())
            return ms
        out[name] = (call, (ce, se, g))
    return out


def interleaved(routes, rounds, warm=3):
    res = {k: [] for k in routes}
    for r in range(rounds + warm):
        for name, (call, _) in routes.items():
            ms = call()
            if r >= warm:
                res[name].append(ms)
    return {k: (float(np.median(v)), float(np.max(v))) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--dense", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    S = a.streams
    lines = [f"medians of {a.rounds} rounds, routes interleaved; ms, host clock around a device synchronise",
             f"one update call on {S} streams with full 8.5 s windows (basic: 266 frames of 32 ms; eGeMAPS: 845 frames of 10 ms), all due:"]
    for k in sorted({1, min(8, S), S}):
        routes = update_routes(S, k)
        med = interleaved(routes, a.rounds)
        lines.append(f"  selects {k:4d} windows:   basic {med['basic'][0]:8.3f}   eGeMAPS {med['eGeMAPS'][0]:8.3f}")
        for _, (se) in routes.values():
            se.close()
        del routes
    routes = tick_routes(S)
    med = interleaved(routes, 3 * a.rounds)
    lines.append(f"one replayed tick of {S} streams at the basic shape (d_model 128, window 256, emotion_dim 9), chunk upload included,")
    lines.append(f"{3 * a.rounds} ticks per route; the streams are in lockstep, so one tick in nine updates all {S} windows (the worst tick):")
    for name, (ms, worst) in med.items():
        lines.append(f"  {name:30s} median {ms:8.3f}   worst {worst:8.3f}")
    del routes
    be = BasicEmotion()
    x = torch.from_numpy(synth.make_audio(9, a.dense, WINDOW)).cuda()
    be(x)
    ts = [timed(lambda: be(x)) for _ in range(a.rounds + 3)][3:]
    lines.append(f"BasicEmotion on {a.dense} dense windows of 8.5 s: {np.median(ts):8.3f}   ({np.median(ts) / a.dense * 1e3:.1f} us per window)")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
