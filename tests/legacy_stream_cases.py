"""Cases and float64 reference of the legacy model's device-resident streams (km_legacy_stream_*, LegacyStreamEngine).

A case is a schedule of push + tick rounds over n streams: in round r stream s is offered the first counts[r][s] samples of its next
n_per_stream-sample chunk, scaled by gains[r][s], and then every stream ticks.  The reference keeps one
oracle.buffers.RingBufferOracle per stream (the reference's RingBuffer, scripts/rt_simplified.py:46-97) and, for every window a
read returns, computes oracle.mel.mel_batch(window, n_fft=1024, hop=533) and oracle.legacy.legacy_forward_mel(..., float64).

simulate() is the FIFO part alone (no model): tests/test_legacy_stream_host.py checks on the CPU that every case really has
ready and not-ready streams in one tick, a write truncated by a full FIFO and a read that runs past the end of the ring, so the
GPU tests cannot pass vacuously.  simulate() and reference() are computed once per case and shared; callers must not modify them.
"""
from __future__ import annotations

import functools
from typing import Dict

import numpy as np

from koemorph_amd import synth
from oracle import buffers, legacy, mel

BOUND = 2e-5            # the project's bound for this model from audio against the oracle (tests/test_gpu_models.py:274)
PARAM_SEED = 7
HOP = 533               # int(16000 // 30), simplified_model.py:36
BUFFER = 32000          # int(2.0 * 16000), scripts/rt_simplified.py:333


def params() -> Dict[str, np.ndarray]:
    return legacy.make_legacy_params(PARAM_SEED)


def _case(name, seed, audio_length, n_per, counts, gains=None):
    counts = np.asarray(counts, np.int32)
    rounds, n_streams = counts.shape
    gains = np.ones((rounds, n_streams), np.float32) if gains is None else np.asarray(gains, np.float32)
    return dict(name=name, seed=seed, n_streams=n_streams, buffer_samples=BUFFER, audio_length=audio_length, n_per_stream=n_per,
                rounds=rounds, counts=counts, gains=gains)


def _cases():
    out = {}
    # streams out of phase: stream 0 fills a window every second round, stream 1 every third or fourth (its write pointer moves
    # by 5000 + 37 r: writes that straddle the end of the ring), stream 2 takes 20 000 a round against 16 000 consumed, so its
    # FIFO is full from round 4 on and drops the rest.  Reads start at 0 or 16 000 and end exactly at the ring's end: the read
    # pointer wraps to 0 without a read that straddles (32 000 = 2 x 16 000); the edge cases below have straddling reads
    out["phase"] = _case("phase", 301, 16000, 20000, [[8000, 5000 + 37 * r, 20000] for r in range(12)])
    # frame-count edges: 4 frames; 32 frames (no zero row, full key tile); the smallest window of 32 frames (odd length: the
    # staging rows are not 16-byte aligned).  Stream 0 is ready in every round, stream 1 in the second only; the second read of
    # stream 0 at 17 000 / 16 523 straddles the end of the ring
    out["T4"] = _case("T4", 302, 1600, 2000, [[2000, 900]] * 3)
    out["T32"] = _case("T32", 303, 17000, 18000, [[18000, 9000]] * 3)
    out["T32min"] = _case("T32min", 304, 16523, 18000, [[18000, 9000]] * 3)
    # stale window maximum: stream 0 gets a loud window, nothing for two rounds, then a quiet one; stream 1 is ready throughout
    out["stale"] = _case("stale", 305, 16000, 16000, [[16000, 16000], [0, 16000], [0, 16000], [16000, 16000]],
                         [[100.0, 1.0], [1.0, 1.0], [1.0, 1.0], [0.01, 1.0]])
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def chunks(name: str) -> np.ndarray:
    """(rounds, n_streams, n_per_stream) float32: what round r offers stream s (gain applied)."""
    c = CASES[name]
    audio = synth.make_audio(c["seed"], c["n_streams"], c["rounds"] * c["n_per_stream"])
    x = audio.reshape(c["n_streams"], c["rounds"], c["n_per_stream"]).transpose(1, 0, 2)
    x = np.ascontiguousarray(x * c["gains"][:, :, None], dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def simulate(name: str) -> dict:
    """The FIFOs alone: ready (rounds, n_streams) bool, windows[r][s] (the popped window or None) and what happened on the way."""
    c = CASES[name]
    x = chunks(name)
    fifos = [buffers.RingBufferOracle(c["buffer_samples"]) for _ in range(c["n_streams"])]
    ready = np.zeros((c["rounds"], c["n_streams"]), bool)
    windows, truncated, write_straddles, read_wraps, read_straddles = [], 0, 0, 0, 0
    for r in range(c["rounds"]):
        row = []
        for s, f in enumerate(fifos):
            n = int(c["counts"][r, s])
            truncated += n > f.size - f.available
            write_straddles += f.write_ptr + min(n, f.size - f.available) > f.size
            f.write(x[r, s, :n])
            rp = f.read_ptr
            w = f.read(c["audio_length"])
            if w is not None:
                ready[r, s] = True
                read_wraps += rp + c["audio_length"] >= f.size
                read_straddles += rp + c["audio_length"] > f.size
            row.append(w)
        windows.append(row)
    return dict(ready=ready, windows=windows, truncated=int(truncated), write_straddles=int(write_straddles),
                read_wraps=int(read_wraps), read_straddles=int(read_straddles))


def forward_window(window: np.ndarray) -> np.ndarray:
    """model(audio) of the reference for one popped window, float64 behind the oracle's mel: (52,)."""
    long, _ = mel.mel_batch(np.asarray(window, np.float32)[None, :], n_fft=1024, hop=HOP)
    import torch
    return legacy.legacy_forward_mel(params(), long, dtype=torch.float64)[0]


@functools.lru_cache(maxsize=None)
def reference(name: str) -> np.ndarray:
    """(rounds, n_streams, 52) float64; NaN rows where the stream was not ready."""
    c, sim = CASES[name], simulate(name)
    out = np.full((c["rounds"], c["n_streams"], 52), np.nan)
    for r in range(c["rounds"]):
        for s in range(c["n_streams"]):
            if sim["windows"][r][s] is not None:
                out[r, s] = forward_window(sim["windows"][r][s])
    out.setflags(write=False)
    return out
