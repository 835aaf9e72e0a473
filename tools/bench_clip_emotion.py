"""Same-run A/B of the offline emotion producer on one clip at the default shape (20 s context, 0.3 s interval):

  A  ClipEmotion.build: the clip's whole emotion track on the device (plan, the ragged eGeMAPS kernels over the clip in place, the
     scrub + Linear(264, 256) epilogue), ceil(K / max_slots) passes, one synchronise at the end.
  B  the route that existed before: one host OpenSMILEeGeMAPSExtractor mirror stepped through the clip in chunks of gcd(MIN, U)
     samples and updated at the same audio times (host AudioBuffer, upload of the window, km_egemaps_functionals with B = 1, 88
     floats back, km_linear with B = 1, 256 floats back per update).

A and B are interleaved repeat by repeat after a warm-up; times are a host clock around work that ends in a device synchronise.
Then ``rows`` for 64 windows (eager, synchronised), and a ``SequentialTrainer.train_epoch`` over the clip from the resident clip with
``clip_emotion`` (track cached: built in the warm-up epoch) against the seeded-noise rows, epochs interleaved.

    python tools/bench_clip_emotion.py --seconds 60 --out profiles/clip_emotion_bench.txt

``--backend basic``: the same three measurements for the track of nine prosodic values (``ClipEmotion(backend="basic")``) at the
`basic` model shape (d_model 128, 4 heads, window 256, emotion_dim 9): ``build``, ``rows`` for 64 windows, and ``train_epoch`` three
ways, interleaved round by round -- the track, the seeded noise, and the route that existed before the track, an
``emotion_provider`` that runs ``BasicEmotion.windows`` on every gathered batch.  Medians of ``--rounds`` rounds with best and worst.

    python tools/bench_clip_emotion.py --backend basic --seconds 60 --out profiles/clip_emotion_basic_bench.txt
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from koemorph_amd import synth                                                              # noqa: E402
from koemorph_amd.data import SequentialKoeMorphDataset                                     # noqa: E402
from koemorph_amd.engine import Engine                                                      # noqa: E402
from koemorph_amd.features import ClipEmotion                                               # noqa: E402
from koemorph_amd.features.opensmile_extractor import OpenSMILEeGeMAPSExtractor             # noqa: E402
from koemorph_amd.scripts.train_sequential import SequentialTrainer                         # noqa: E402

SR = 16000


def layer():
    torch.manual_seed(0)
    return torch.nn.Linear(264, 256)


def speech(seconds: float) -> np.ndarray:
    """Vowels, silence and noise in turn, 2.5 s a segment."""
    parts, k = [], 0
    while sum(len(p) for p in parts) < int(seconds * SR):
        v = synth.make_vowel(40 + k, 110.0 + 15 * (k % 5), 1.5, vibrato=0.03)
        parts += [v, np.zeros(SR // 4, np.float32), (0.2 * synth.normal(90 + k, (3 * SR // 4,))).astype(np.float32)]
        k += 1
    return (0.5 * np.concatenate(parts)[:int(seconds * SR)]).astype(np.float32)


def host_route(ex, audio: np.ndarray, shape: dict) -> np.ndarray:
    """One mirror extractor over the clip, updated at MIN + k U.  Its clock stands still, so only the forced updates extract."""
    ex.reset()
    g, MIN, U = math.gcd(shape["min_samples"], shape["update_samples"]), shape["min_samples"], shape["update_samples"]
    rows = []
    for at in range(0, len(audio), g):
        t = min(at + g, len(audio))
        due = t >= MIN and (t - MIN) % U == 0
        before = ex.total_updates
        ex.process_audio_frame(audio[at:t], force_update=due)
        if ex.total_updates != before:
            rows.append(ex.get_concatenated_features())
    torch.cuda.synchronize()
    return np.stack(rows) if rows else np.zeros((0, 256), np.float32)


def stats(ts):
    return f"median {np.median(ts):10.3f}   worst {np.max(ts):10.3f}   best {np.min(ts):10.3f}"


def write_pair(d, audio):
    from scipy.io import wavfile
    wavfile.write(os.path.join(d, "clip.wav"), SR, audio)
    F = len(audio) * 30 // SR
    labels = synth.uniform(7, (F, 52), 0, 1).astype(np.float32)
    with open(os.path.join(d, "clip.jsonl"), "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main_basic(a):
    from koemorph_amd.features.basic_emotion import BasicEmotion
    audio = speech(a.seconds)
    clip = torch.from_numpy(audio).cuda()
    ce = ClipEmotion(backend="basic")
    K = ce.num_rows(len(audio))
    built = {}
    ts = [timed(lambda: built.__setitem__("t", ce.build(clip)[0])) for _ in range(a.rounds + 1)][1:]
    track = built["t"]
    lines = [f"basic back end: clip of {a.seconds:g} s ({len(audio)} samples), context 20 s, interval 0.3 s: K = {K} rows of 9, max_slots "
             f"{ce.max_slots} ({-(-K // ce.max_slots)} passes); medians of {a.rounds} rounds after one warm-up round",
             f"  ClipEmotion.build, ms per whole track  {stats(ts)}   ({np.median(ts) / max(K, 1):.3f} ms per row)"]
    starts = torch.arange(64, dtype=torch.int32, device="cuda") * 20
    out = torch.empty(64, 9, device="cuda")
    ts = [timed(lambda: ce.rows(track, len(audio), starts, 533, 256, out=out)) for _ in range(a.rounds + 5)][5:]
    lines.append(f"  rows for 64 windows (eager, synchronised), ms  {stats(ts)}")
    if not a.no_train:
        be = BasicEmotion()

        def provider(windows):                               # what existed: the windows' own prosody, once per gathered batch
            B, L = windows.shape
            at = torch.arange(B, dtype=torch.int32, device=windows.device) * L
            return be.windows(windows.reshape(-1), at, L)

        with tempfile.TemporaryDirectory() as d:
            write_pair(d, audio)
            trainers = {}
            for name in ("basic", "noise", "provider"):
                eng = Engine(d_model=128, num_heads=4, mel_sequence_length=256, emotion_dim=9)
                eng.load_state_dict(synth.make_core_params(0, 128, 256, 9, "init"))
                eng.finalize()
                ds = SequentialKoeMorphDataset(d, shuffle_files=False, loop_dataset=False, batch_size=a.batch_size, resident_windows=True)
                trainers[name] = SequentialTrainer(eng, ds, from_clip=True, clip_emotion=ce if name == "basic" else None,
                                                   emotion_provider=provider if name == "provider" else None)
            ep = {k: [] for k in trainers}
            steps = 0
            for e in range(a.rounds + 1):                    # the warm-up round builds and caches the track
                for name, st in trainers.items():
                    res = {}
                    t = timed(lambda: res.update(st.train_epoch()))
                    steps = res["batches"]
                    if e:
                        ep[name].append(t)
            lines.append(f"train_epoch over the clip at d_model 128 / 4 heads / window 256 / emotion_dim 9, batch {a.batch_size}, {steps} steps, "
                         f"ms per epoch, sources interleaved round by round (track cached; {ce.builds} builds in all):")
            label = {"basic": "--emotion basic (track, resident clip)", "noise": "--emotion noise (resident clip)",
                     "provider": "emotion_provider: BasicEmotion.windows per batch (gathered)"}
            for name, ts in ep.items():
                lines.append(f"  {label[name]:62s} {stats(ts)}   ({np.median(ts) / max(steps, 1):.3f} ms per step)")
        be.close()
    ce.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=("egemaps", "basic"), default="egemaps")
    ap.add_argument("--rounds", type=int, default=15, help="--backend basic: timed rounds of every measurement")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs per emotion source")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if a.backend == "basic":
        return main_basic(a)
    audio = speech(a.seconds)
    clip = torch.from_numpy(audio).cuda()
    lin = layer()
    ce = ClipEmotion(compression_layer=lin)
    K = ce.num_rows(len(audio))
    ex = OpenSMILEeGeMAPSExtractor(use_concatenation=True, device="cuda", clock=lambda: 0.0)
    ex.compression_layer = lin
    res = {"ClipEmotion.build": [], "host mirror extractor": []}
    track = host = None
    for rep in range(a.repeats + 1):                           # one repeat of warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        track, _ = ce.build(clip)
        torch.cuda.synchronize()
        if rep:
            res["ClipEmotion.build"].append((time.perf_counter() - t0) * 1e3)
        if not a.no_baseline:
            t0 = time.perf_counter()
            host = host_route(ex, audio, ce.shape)
            if rep:
                res["host mirror extractor"].append((time.perf_counter() - t0) * 1e3)
    lines = [f"clip of {a.seconds:g} s ({len(audio)} samples), context 20 s, interval 0.3 s: K = {K} rows, max_slots {ce.max_slots} "
             f"({-(-K // ce.max_slots)} passes);",
             f"ms per whole track over {a.repeats} repeats, routes interleaved repeat by repeat"]
    for name, ts in res.items():
        if ts:
            lines.append(f"  {name:28s} {stats(ts)}   ({np.median(ts) / max(K, 1):.3f} ms per row)")
    if host is not None:
        assert host.shape == (K, 256), (host.shape, K)
        lines.append(f"  largest difference between the two tracks: {float(np.abs(track.cpu().numpy() - host).max()):.3e}")
    starts = torch.arange(64, dtype=torch.int32, device="cuda") * 20
    out = torch.empty(64, 256, device="cuda")
    ts = []
    for i in range(50 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ce.rows(track, len(audio), starts, 533, 256, out=out)
        torch.cuda.synchronize()
        if i >= 5:
            ts.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"rows for 64 windows (eager, synchronised), ms over 50 calls: {stats(ts)}")
    if not a.no_train:
        with tempfile.TemporaryDirectory() as d:
            write_pair(d, audio)
            trainers = {}
            for name in ("egemaps", "noise"):
                eng = Engine()
                eng.load_state_dict(synth.make_core_params(0, style="init"))
                eng.finalize()
                ds = SequentialKoeMorphDataset(d, shuffle_files=False, loop_dataset=False, batch_size=a.batch_size, resident_windows=True)
                trainers[name] = SequentialTrainer(eng, ds, from_clip=True, clip_emotion=ce if name == "egemaps" else None)
            ep = {k: [] for k in trainers}
            steps = 0
            for e in range(a.epochs + 1):                      # the warm-up epoch builds and caches the track
                for name, st in trainers.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m = st.train_epoch()
                    torch.cuda.synchronize()
                    steps = m["batches"]
                    if e:
                        ep[name].append((time.perf_counter() - t0) * 1e3)
            lines.append(f"train_epoch over the clip from the resident clip, batch {a.batch_size}, {steps} steps, ms per epoch over {a.epochs} "
                         f"epochs, sources interleaved (track cached; {ce.builds} builds in all):")
            for name, ts in ep.items():
                lines.append(f"  --emotion {name:8s} {stats(ts)}   ({np.median(ts) / max(steps, 1):.3f} ms per step)")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
