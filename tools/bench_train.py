#!/usr/bin/env python3
"""BASELINE config 3: train_sequential-style dense stride-1 step, window 256, 8 windows per GPU, data parallel.

    python tools/bench_train.py                                   # 1 GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 tools/bench_train.py

Per step and per rank: log-mel front end of 8 x 136448 samples -> forward -> MSE loss -> backward -> ONE all-reduce
of the flat fp32 gradient bucket over RCCL/xGMI -> global-norm clip -> AdamW.  Prints one JSON line on rank 0.

    python tools/bench_train.py --clip [--stride 1] [--batches 8,16,64]

One resident synthetic clip, dense windows: (a) km_gather_windows + Trainer.step, the step on gathered windows, against
(b) Trainer.step_clip, the step from the clip with shared STFT frames, in ONE process, alternating blocks of >= 0.5 s after
warming both, three alternations; ms per step (host clock around steps that end in a synchronise) with the spread over the
blocks, and the STFT frames the front end computes per step on each path (from the shapes).  One JSON line per batch size."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
from koemorph_amd import parallel, synth
from koemorph_amd.engine import Engine
from koemorph_amd.training import Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--graph", action="store_true", help="replay forward+backward from a hipGraph")
ap.add_argument("--clip", action="store_true", help="A/B: gathered windows + step against step_clip on one resident clip")
ap.add_argument("--stride", type=int, default=1, help="--clip: start frames of consecutive windows are this far apart")
ap.add_argument("--batches", default="8,16,64", help="--clip: batch sizes")
ap.add_argument("--block-seconds", type=float, default=0.5, help="--clip: least duration of a timed block")
args = ap.parse_args()


def bench_clip():
    """Same process, same trainer, same weights trajectory on both paths (the steps are bit-identical), blocks alternate."""
    from koemorph_amd import clip_span
    from koemorph_amd._lib import check, load
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = load()
    T, hop = 256, 533
    W = T * hop
    for B in [int(v) for v in args.batches.split(",")]:
        eng = Engine(); eng.load_state_dict(synth.make_core_params(0)); eng.finalize(dev)
        tr = Trainer(eng, max_windows=B)
        n_pos = 32                                                   # the batch walks along the clip like a training epoch
        n_frames = (n_pos + B) * args.stride + T + 1
        clip = torch.from_numpy(synth.make_audio(10, 1, n_frames * hop, "uniform")[0]).to(dev)
        emo = torch.from_numpy(synth.normal(20, (B, 256))).to(dev)
        target = torch.from_numpy(synth.uniform(30, (B, 52), 0, 1)).to(dev)
        host_starts = [[(p + i) * args.stride for i in range(B)] for p in range(n_pos)]
        dev_starts = [torch.tensor(h, dtype=torch.int32, device=dev) for h in host_starts]
        audio = torch.empty(B, W, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def step_gather(p):
            check(lib.km_gather_windows(clip.data_ptr(), clip.shape[0], dev_starts[p].data_ptr(), B, hop, W, audio.data_ptr(), None, 0,
                                        0, 0, None, None, stream))
            tr.step(audio, emo, target)

        def step_clip(p):
            tr.step_clip(clip, dev_starts[p], emo, target, extremes=(host_starts[p][0], host_starts[p][-1]))

        def block(fn, n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(n):
                fn(i % n_pos)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / n * 1e3

        for fn in (step_gather, step_clip):
            block(fn, args.warmup)
        n = max(args.steps, int(args.block_seconds / (block(step_gather, args.steps) * 1e-3)) + 1)
        ms = {"gather": [], "clip": []}
        for _ in range(3):
            ms["gather"].append(block(step_gather, n))
            ms["clip"].append(block(step_clip, n))
        rec = {"workload": f"C3 dense training step, {B} windows, stride {args.stride}, window 256, one resident clip",
               "clip_supported": tr.clip_supported(), "steps_per_block": n}
        for k, v in ms.items():
            rec[f"{k}_ms_per_step"] = [round(x, 4) for x in v]
            rec[f"{k}_ms_median"] = round(sorted(v)[1], 4)
        rec["frames_per_step"] = {"gather": clip_span.frames_computed(host_starts[0], T, False),
                                  "clip": clip_span.frames_computed(host_starts[0], T, True)}
        rec["final_loss"] = float(tr.loss.item())
        print(json.dumps(rec), flush=True)


if args.clip:
    bench_clip()
    sys.exit(0)
rank, world, local = parallel.init_from_env()
torch.cuda.set_device(local)
dev = torch.device(f"cuda:{local}")
eng = Engine(); eng.load_state_dict(synth.make_core_params(0)); eng.finalize(dev)
tr = Trainer(eng, max_windows=args.batch)
B = args.batch
audio = torch.from_numpy(synth.make_audio(10 + rank, B, 136448, "uniform")).to(dev)
emo = torch.from_numpy(synth.normal(20 + rank, (B, 256))).to(dev)
target = torch.from_numpy(synth.uniform(30 + rank, (B, 52), 0, 1)).to(dev)
for _ in range(args.warmup):
    tr.step(audio, emo, target)
if args.graph:
    tr.capture(B, 136448)
    step = lambda: tr.step_graph(audio, emo, target)
else:
    step = lambda: tr.step(audio, emo, target)
torch.cuda.synchronize(dev)
if world > 1:
    dist.barrier(); torch.cuda.synchronize(dev)
t0 = time.perf_counter()
for _ in range(args.steps):
    step()
torch.cuda.synchronize(dev)
if world > 1:
    dist.barrier(); torch.cuda.synchronize(dev)
dt = time.perf_counter() - t0
if world > 1:
    t = torch.tensor([dt], device=dev, dtype=torch.float64); dist.all_reduce(t, op=dist.ReduceOp.MAX); dt = float(t.item())
if rank == 0:
    print(json.dumps({"workload": f"C3: train step, {B} windows/GPU x 136448 samples, window 256, d_model 256, AdamW, "
                      f"flat {tr.n_params}-float gradient all-reduce", "n_gpus": world, "graph": bool(args.graph), "steps": args.steps,
                      "ms_per_step": round(dt / args.steps * 1e3, 4), "windows_per_s": round(B * world * args.steps / dt, 1),
                      "final_loss": float(tr.loss.item())}))
if world > 1:
    dist.destroy_process_group()
