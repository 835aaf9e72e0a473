#!/usr/bin/env python3
"""BASELINE config 5 on ONE GPU: 128 concurrent speaker streams, per-tick decode under a hipGraph.
Prints ticks/s and p50/p99 tick latency (host wall clock around replay + the 26 KB result readback).

Default: the 30 fps shape (d_model 256, 8 heads, window 256, 533-sample frames).  ``--d-model 512 --heads 8|16 --fps 60``: the 60 fps
long-context shape (window 512, 8.5 s ring of hop 266, 267-sample frames); ``--d-model 256 --heads 8 --fps 60``: the shape of the
reference's frame_rate=60 recipe (window 512, same ring), with ``--chunked`` / ``--attention`` that shape alone;
``--d-model 128 --heads 4 --window 128|256``: the reference's `fast` / `basic` variants at 30 fps (core128_stream_kernel), again with
``--chunked`` / ``--attention`` that shape alone, and with ``--baseline`` the two routes interleaved in 15 rounds of one run (medians
of the rounds, minimum and maximum).  ``--baseline`` adds what a caller had to do at that shape
before the stream path covered it: rings kept outside the library, unrolled into 128 chronological windows per tick, km_forward_audio
on them with the EMA state (km_smooth behind the generic core), and the same readback -- timed the same way.

``--chunked``: streams out of phase.  In ONE run, at d_model 256 / 30 fps and d_model 512 / 8 heads / 60 fps, interleaved in rounds:
(a) a replayed km_stream_feed + km_stream_step with every stream firing, (b) the lockstep replayed km_stream_push + km_stream_tick,
(c) a replayed feed + step on which one stream in four brings a frame; then the route there was before for streams that do not move
together: one SimplifiedDualStreamModel(real_time_mode=True) per stream driven frame by frame (8 streams, the d_model 256 shape),
reported per stream-frame.  Host wall clock around one synchronised tick, as above.

``--attention``: what the attention outputs cost.  In ONE run, at both shapes, a replayed chunked tick (feed + step, every stream
firing) on three engines, interleaved in rounds: (plain) km_stream_step, (maps) km_stream_step_attn writing `raw` and the
head-averaged maps, (maps_stats) the same with km_attn_stats_update_masked gated on `fired` in the graph.  The figure of a round is
the host clock around its synchronised ticks divided by their number; reported: the median of 15 rounds, and the spread."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koemorph_amd import synth
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEngine

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--ticks", type=int, default=1000)
ap.add_argument("--d-model", type=int, default=256, choices=(128, 256, 512))
ap.add_argument("--heads", type=int, default=8, choices=(4, 8, 16))
ap.add_argument("--window", type=int, default=None, choices=(128, 256), help="mel_sequence_length at d_model 128 (default 128)")
ap.add_argument("--fps", type=int, default=30, choices=(30, 60))
ap.add_argument("--baseline", action="store_true", help="also time host-side rings + forward_audio + EMA per tick")
ap.add_argument("--attention", action="store_true", help="a replayed chunked tick without maps, with maps, with maps + the masked statistics update")
ap.add_argument("--chunked", action="store_true", help="feed + step (all fire / one in four) against push + tick at both shapes, and one model per stream")
args = ap.parse_args()
S = args.streams


def make_engine(d_model, heads, fps):
    if d_model == 128:         # `fast` (window 128) / `basic` (window 256); emotion_dim 256 at both, as every shape here
        e = Engine(d_model=128, num_heads=4, mel_sequence_length=args.window)
        e.load_state_dict(synth.make_core_params(0, 128, args.window)); e.finalize()
    elif d_model == 256 and fps == 30:
        e = Engine(); e.load_state_dict(synth.make_core_params(0)); e.finalize()
    else:      # window 512 at hop 266: d_model 512 (long context) or d_model 256 / 8 heads (the frame_rate=60 recipe)
        e = Engine(d_model=d_model, num_heads=heads, mel_sequence_length=512, mel=MelConfig.model_batch(target_fps=fps))
        e.load_state_dict(synth.make_core_params(0, d_model, 512)); e.finalize()
    return e


def stats(lat):
    lat = np.asarray(lat) * 1e3
    return {"ms_mean": round(float(lat.mean()), 4), "ms_p10": round(float(np.percentile(lat, 10)), 4),
            "ms_p50": round(float(np.percentile(lat, 50)), 4), "ms_p90": round(float(np.percentile(lat, 90)), 4)}


def chunked_shape(d_model, heads, fps, rounds=8):
    ui = 0.0333 if fps == 30 else 1.0 / fps
    lock = StreamEngine(make_engine(d_model, heads, fps), S, update_interval=ui)
    chk = ChunkedStreamEngine(make_engine(d_model, heads, fps), S, update_interval=ui)
    n, frame = lock.ring_hop + 1, chk.frame_samples          # both routes upload n samples per stream and tick
    frames = torch.from_numpy(synth.make_audio(1, S, n * 8, "uniform")).cuda()
    emo = torch.from_numpy(synth.normal(2, (S, 256))).cuda()
    every = torch.full((S,), frame, dtype=torch.int32, device="cuda")
    quarter = [torch.where((torch.arange(S, device="cuda") + p) % 4 == 0, every, torch.zeros_like(every)) for p in range(4)]
    chunk = lambda t: frames[:, (t % 8) * n:(t % 8 + 1) * n]
    for t in range(lock.shape["ring_len"] // lock.ring_hop + 3):      # fill the rings (eager)
        lock.push(chunk(t)); lock.tick(emo)
        chk.feed(chunk(t), every); chk.step(emo)
    h_lock, h_chk = torch.empty(S, 52, pin_memory=True), torch.empty(S, 52, pin_memory=True)
    lock.capture(n, host_out=h_lock)
    chk.capture(n, host_out=h_chk)
    routes = {"a_feed_step_all_fire": lambda t: chk.replay(chunk(t), every, emo),
              "b_push_tick": lambda t: lock.replay(chunk(t), emo),
              "c_feed_step_one_in_four": lambda t: chk.replay(chunk(t), quarter[t % 4], emo)}
    lat = {k: [] for k in routes}
    fired = {}
    per_round = max(1, args.ticks // rounds)
    for r in range(rounds + 1):                               # round 0 warms up
        for name, step in routes.items():
            torch.cuda.synchronize()
            for t in range(per_round):
                t0 = time.perf_counter()
                step(t)
                torch.cuda.synchronize()
                if r:
                    lat[name].append(time.perf_counter() - t0)
            fired[name] = int(chk.fired.sum()) if name != "b_push_tick" else int(lock.ready.sum())
    res = {"workload": f"{S} streams/GPU (d_model {d_model}, {heads} heads, {fps} fps), replayed graph + D2H of {S}x52 floats, one "
                       f"synchronisation per tick, {rounds} rounds x {per_round} ticks per route, interleaved",
           "samples_uploaded_per_stream": n, "frame_samples": frame, "streams_computed_on_last_tick": fired}
    for name in routes:
        res[name] = stats(lat[name])
    return res


def attention_shape(d_model, heads, fps, rounds=15):
    from koemorph_amd.metrics import AttentionStats
    ui = 0.0333 if fps == 30 else 1.0 / fps
    eng = {k: ChunkedStreamEngine(make_engine(d_model, heads, fps), S, update_interval=ui) for k in ("plain", "maps", "maps_stats")}
    n, frame = eng["plain"].ring_hop + 1, eng["plain"].frame_samples
    frames = torch.from_numpy(synth.make_audio(1, S, n * 8, "uniform")).cuda()
    emo = torch.from_numpy(synth.normal(2, (S, 256))).cuda()
    every = torch.full((S,), frame, dtype=torch.int32, device="cuda")
    chunk = lambda t: frames[:, (t % 8) * n:(t % 8 + 1) * n]
    for t in range(eng["plain"].shape["ring_len"] // eng["plain"].ring_hop + 3):      # fill the rings (eager)
        for k, se in eng.items():
            se.feed(chunk(t), every); se.step(emo, return_attention=(k != "plain"))
    acc = AttentionStats()
    host = {k: torch.empty(S, 52, pin_memory=True) for k in eng}
    eng["plain"].capture(n, host_out=host["plain"])
    eng["maps"].capture(n, host_out=host["maps"], return_attention=True)
    eng["maps_stats"].capture(n, host_out=host["maps_stats"], return_attention=True, stats=acc)
    per_round = max(1, args.ticks // rounds)
    ms = {k: [] for k in eng}
    for r in range(rounds + 1):                               # round 0 warms up
        for k, se in eng.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(per_round):
                se.replay(chunk(t), every, emo)
                torch.cuda.synchronize()
            if r:
                ms[k].append((time.perf_counter() - t0) / per_round * 1e3)
    same = all(torch.equal(eng["plain"].out, eng[k].out) for k in ("maps", "maps_stats"))
    res = {"workload": f"{S} streams/GPU (d_model {d_model}, {heads} heads, {fps} fps), replayed feed + step with every stream firing + D2H of "
                       f"{S}x52 floats, one synchronisation per tick, {rounds} rounds x {per_round} ticks per route, interleaved",
           "out_identical_across_routes": bool(same), "stats_rows": int(acc.compute()["rows"]),
           "all_fired": bool(all(int(se.fired.sum()) == S for se in eng.values()))}
    for k in eng:
        v = np.asarray(ms[k])
        res[k] = {"tick_ms_median_of_rounds": round(float(np.median(v)), 4), "tick_ms_min": round(float(v.min()), 4),
                  "tick_ms_max": round(float(v.max()), 4)}
    for k in ("maps", "maps_stats"):
        res[k]["over_plain_ms"] = round(res[k]["tick_ms_median_of_rounds"] - res["plain"]["tick_ms_median_of_rounds"], 4)
    return res


def per_model_route(n_models=8, ticks=60):
    """One SimplifiedDualStreamModel(real_time_mode=True) per stream, each driven frame by frame (its ring on the host, the 8.5 s
    window uploaded per frame, front end + core + EMA launches per stream).  Steps are one audio hop apart: a stepped clock."""
    from koemorph_amd.model import SimplifiedDualStreamModel
    sd = {"dual_stream_attention." + k: torch.from_numpy(v) for k, v in synth.make_core_params(0).items()}
    sd["smoothing_alpha"] = torch.tensor(0.8)
    models, clock = [], [0.0]
    for _ in range(n_models):
        m = SimplifiedDualStreamModel(real_time_mode=True).cuda().eval()
        m.load_state_dict(sd)
        m.mel_extractor._clock = lambda: clock[0]
        models.append(m)
    audio = synth.make_audio(1, n_models, 533 * 8, "uniform")
    emo = torch.from_numpy(synth.normal(2, (n_models, 256))).cuda()
    fill = 136000 // 532 + 3
    lat = []
    for t in range(fill + ticks):
        clock[0] += 0.0333
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = [m.process_audio_frame_realtime(audio[i, (t % 8) * 533:(t % 8 + 1) * 533], emotion_features=emo[i:i + 1])
                for i, m in enumerate(models)]
        torch.cuda.synchronize()
        if t >= fill:
            assert all(o is not None for o in outs)
            lat.append((time.perf_counter() - t0) / n_models)
    return {"workload": f"{n_models} x SimplifiedDualStreamModel(real_time_mode=True) (d_model 256, 30 fps), one 533-sample frame per model "
                        f"per tick, one synchronisation per tick, {ticks} ticks; figures are per stream-frame",
            "per_stream_frame": stats(lat)}


if args.d_model == 256 and args.fps == 60 and args.heads != 8:
    ap.error("d_model 256 at 60 fps streams with 8 heads only")
d128 = args.d_model == 128
if d128:
    args.window = args.window or 128
    if args.heads != 4 or args.fps != 30:
        ap.error("d_model 128 streams with --heads 4 at 30 fps")
elif args.window is not None or args.heads == 4:
    ap.error("--window and --heads 4 go with --d-model 128")
recipe60 = args.d_model == 256 and args.fps == 60         # the shape of the frame_rate=60 recipe: that shape alone
one_shape = ((128, 4, 30),) if d128 else ((256, 8, 60),) if recipe60 else None
if args.attention:
    for shape in (one_shape or ((256, 8, 30), (512, 8, 60))):
        print(json.dumps(attention_shape(*shape)), flush=True)
    sys.exit(0)
if args.chunked:
    for shape in (one_shape or ((256, 8, 30), (512, 8, 60))):
        print(json.dumps(chunked_shape(*shape)), flush=True)
    if not one_shape:
        print(json.dumps(per_model_route()), flush=True)
    sys.exit(0)
eng = make_engine(args.d_model, args.heads, args.fps)
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
shape = f"d_model {args.d_model}, {args.heads} heads, {args.fps} fps" + (f", window {args.window}" if d128 else "")
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
    if d128:       # the two routes interleaved in rounds of one run: the figure of a round is its mean synchronised tick
        rounds, per_round = 15, max(1, args.ticks // 15)
        routes = {"stream_replay": lambda t: se.replay(frames[:, (t % 8) * n:(t % 8 + 1) * n], emo), "baseline_forward_audio": host_rings}
        ms = {k: [] for k in routes}
        for r in range(rounds + 1):                           # round 0 warms up
            for k, step in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(per_round):
                    step(t)
                    torch.cuda.synchronize()
                if r:
                    ms[k].append((time.perf_counter() - t0) / per_round * 1e3)
        for k, v in ms.items():
            v = np.asarray(v)
            res[k + "_interleaved"] = {"tick_ms_median_of_rounds": round(float(np.median(v)), 4), "tick_ms_min": round(float(v.min()), 4),
                                       "tick_ms_max": round(float(v.max()), 4), "rounds": rounds, "ticks_per_round": per_round}
        res["stream_not_above_baseline"] = bool(res["stream_replay_interleaved"]["tick_ms_median_of_rounds"] <=
                                                res["baseline_forward_audio_interleaved"]["tick_ms_median_of_rounds"])
    b_all, b_lat = timed(host_rings)
    res["baseline_forward_audio_tick_ms_mean"] = round(b_all / args.ticks * 1e3, 4)
    res["baseline_forward_audio_tick_ms_p50"] = round(float(np.percentile(b_lat, 50)), 4)
    res["baseline_note"] = "per tick: 2-4 torch slice copies (ring write, unroll into chronological windows), km_forward_audio with EMA state, D2H"
print(json.dumps(res))
