#!/usr/bin/env python3
"""Training step and eval-mode forward from a resident clip on ONE GPU with and without option clip_assemble, at the shapes the
default refuses: the 60 fps recipe (d_model 256 / 8 heads / window 512 / hop 266) and long_context (d_model 512 / 8 heads / window
512 / hop 266) for training and forward, `fast` (d_model 128 / window 128 / hop 533, option core128 on both engines) for the forward.
Batches of 8, 16 and 64 stride-1 windows.

Two engines with the same weights, one per route, interleaved in rounds of one run.  gathered (option off, km_clip_plan route 0): the
launches of the default -- km_gather_windows into a buffer kept across calls, then km_train_step_audio / km_forward_audio;
assembled (option on, route 2): the span image, the two snippets per window, clip_pack_edges_kernel or clip_assemble_kernel, then
the same step / core.  The figure of a round is the host clock around `calls` calls ending in one synchronisation, divided by their
number; reported: the median, minimum and maximum of 15 rounds after a warm-up round, the STFT frames either route computes and
whether the two routes' results are equal bits.  One JSON line per shape, call and batch size, also appended to --out
(profiles/clip_assemble_bench.txt)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koemorph_amd import synth
from koemorph_amd._lib import check
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.training import Trainer

# name: (d_model, heads, window, emotion_dim, front-end fps, core128, calls measured)
SHAPES = {"60fps": (256, 8, 512, 256, 60, 0, ("train", "forward")), "long_context": (512, 8, 512, 256, 60, 0, ("train", "forward")),
          "fast": (128, 4, 128, 256, 30, 1, ("forward",))}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--batches", default="8,16,64")
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--calls", type=int, default=5, help="calls per round and route")
ap.add_argument("--out", default=None)
args = ap.parse_args()
batches = [int(b) for b in args.batches.split(",")]
BM = max(batches)

for shape in args.shapes.split(","):
    d, H, T, ED, fps, core128, kinds = SHAPES[shape]
    params = synth.make_core_params(0, d, T, ED, "trained")
    eng, trn = {}, {}
    for name, on in (("gathered", 0), ("assembled", 1)):
        e = Engine(d_model=d, num_heads=H, mel_sequence_length=T, emotion_dim=ED, mel=MelConfig.model_batch(target_fps=fps))
        e.load_state_dict(params)
        e.finalize()
        e.set_option("core128", core128)
        e.set_option("clip_assemble", on)
        eng[name] = e
        if "train" in kinds:
            trn[name] = Trainer(e, max_windows=BM, use_smoothing=False)
    hop = eng["assembled"].mel.hop_length
    W = T * hop
    clip = torch.from_numpy(synth.make_audio(1, 1, (T + BM + 40) * hop, "speech")[0]).cuda()
    windows = torch.empty(BM, W, device="cuda")
    lib = eng["gathered"]._lib

    def gather(starts, B):
        check(lib.km_gather_windows(clip.data_ptr(), clip.shape[0], starts.data_ptr(), B, hop, W, windows.data_ptr(), None, 0, 0, 0, None, None,
                                    torch.cuda.current_stream().cuda_stream))
        return windows[:B]

    for kind in kinds:
        for B in batches:
            starts = torch.arange(7, 7 + B, dtype=torch.int32, device="cuda")
            ext = (7, 7 + B - 1)
            emo = torch.from_numpy(synth.normal(2, (B, ED))).cuda()
            target = torch.from_numpy(synth.uniform(3, (B, 52), 0, 1)).cuda()
            state = {k: torch.zeros(B, 52, device="cuda") for k in eng}
            plans = {k: e.clip_plan(B, *ext, training=kind == "train") for k, e in eng.items()}
            assert plans["gathered"]["route"] == 0 and plans["assembled"]["route"] == 2, plans

            def call(k):
                if kind == "train":
                    if k == "assembled":
                        trn[k].forward_backward_clip(clip, starts, emo, target, extremes=ext)
                    else:
                        trn[k].forward_backward(gather(starts, B), emo, target)
                    return trn[k].flat_grad
                if k == "assembled":
                    return eng[k].forward_clip(clip, starts, emo, state=state[k], first=True, extremes=ext)
                return eng[k].forward_audio(gather(starts, B), emo, state=state[k], first=True)

            out, ms = {}, {k: [] for k in eng}
            for r in range(args.rounds + 1):                      # round 0 warms up (and grows the images)
                for k in eng:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        out[k] = call(k)
                    torch.cuda.synchronize()
                    if r:
                        ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
            rec = {"workload": f"{kind} from a resident clip: {shape} (d_model {d}, {H} heads, window {T}, hop {hop}), {B} stride-1 windows; "
                               f"{args.rounds} rounds x {args.calls} calls per route, interleaved",
                   "equal_bits_between_routes": bool(torch.equal(out["assembled"], out["gathered"]))}
            for k in eng:
                v = np.asarray(ms[k])
                rec[k] = {"ms_per_call_median_of_rounds": round(float(np.median(v)), 4), "ms_min": round(float(v.min()), 4),
                          "ms_max": round(float(v.max()), 4), "stft_frames": plans[k]["stft_frames"]}
            rec["assembled_over_gathered"] = round(rec["assembled"]["ms_per_call_median_of_rounds"] / rec["gathered"]["ms_per_call_median_of_rounds"], 4)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    trn.clear()
    for e in eng.values():
        e.close()
