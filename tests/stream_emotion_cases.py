"""Schedule S and the host oracle of the device-resident emotion streams (koemorph_amd.streaming.StreamEmotion), shared by
tests/test_stream_emotion_host.py and tests/test_gpu_stream_emotion.py.

The oracle restates the update rule in integer samples, per stream, on top of oracle.buffers.AudioBufferOracle:
  eligible   total > 0, due (no features yet or total - last_update_total >= U), window of at least MIN samples
  selected   of the eligible streams the max_updates that waited longest (total - last_update_total, never updated = -1), ties to
             the lowest index
  update     features <- functionals(window); empty 300 / 600 ms slots take them too; last_update_total <- total
It does not compute features: it says who updates on which step, on which window, and which update filled the slots.
"""
from __future__ import annotations

import functools

import numpy as np

from koemorph_amd import synth
from oracle.buffers import AudioBufferOracle

SR = 16000

# ---- Schedule S ---------------------------------------------------------------------------------------------------------------
N_STREAMS, STEPS, CONTEXT, INTERVAL = 5, 52, 1.0, 0.3
SHAPE_S = dict(ring_len=48000, window_len=16000, update_samples=4800, min_samples=8000, max_frames=95)
RESETS = {30: (2,)}                      # before step 30 stream 2 is handed to the next speaker
UPDATES_UNCAPPED, UPDATES_CAP2 = 68, 66
GAINS = (0.9, 0.25, 0.6, 0.05, 0.4)      # peak normalisation has to undo these


def count(s: int, t: int) -> int:
    if s == 0:
        return 1600
    if s == 1:
        return 1024
    if s == 2:
        return 0 if t < 7 else 1600
    if s == 3:
        return 160 if t < 20 else 4000
    return 0 if 25 <= t < 31 else 1600


def counts_table() -> np.ndarray:
    return np.array([[count(s, t) for s in range(N_STREAMS)] for t in range(STEPS)], np.int32)


def speechlike(seed: int, seconds: float) -> np.ndarray:
    """voiced - silence - noise - voiced with vibrato (as in tests/test_gpu_egemaps.py)."""
    a = synth.make_vowel(seed, 130.0, seconds * 0.35, vibrato=0.03)
    b = np.zeros(int(seconds * 0.1 * SR), np.float32)
    c = (0.2 * synth.normal(seed + 2, (int(seconds * 0.2 * SR),))).astype(np.float32)
    d = 0.6 * synth.make_vowel(seed + 3, 190.0, seconds * 0.35, formants=((500.0, 80.0), (1500.0, 120.0), (2500.0, 150.0)), vibrato=0.02)
    return np.concatenate([a, b, c, d]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def audio(s: int) -> np.ndarray:
    """Everything stream s receives over the schedule, in order: 2.2 s speech-like segments one after the other, at the stream's gain."""
    need = int(counts_table()[:, s].sum())
    parts, k = [], 0
    while sum(len(p) for p in parts) < need:
        parts.append(speechlike(700 + 40 * s + 5 * k, 2.2))
        k += 1
    x = (GAINS[s] * np.concatenate(parts)[:need]).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def chunks():
    """chunks()[t][s]: the samples stream s receives on step t."""
    cnt = counts_table()
    off = np.concatenate([np.zeros((1, N_STREAMS), np.int64), np.cumsum(cnt, axis=0)])
    return [[audio(s)[off[t, s]:off[t + 1, s]] for s in range(N_STREAMS)] for t in range(STEPS)]


def padded(row, m=None):
    """One step's chunks as the (n, m) matrix + int32 counts that push takes."""
    cnt = np.array([len(c) for c in row], np.int32)
    m = max(int(cnt.max()), 1) if m is None else m
    x = np.zeros((len(row), m), np.float32)
    for s, c in enumerate(row):
        x[s, :len(c)] = c
    return x, cnt


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
class EmotionStreamOracle:
    def __init__(self, n_streams: int, context_window: float, update_interval: float, max_updates=None):
        self.n, self.context = n_streams, context_window
        self.U, self.MIN = int(update_interval * SR), int(0.5 * SR)
        self.max_updates = n_streams if max_updates is None else max_updates
        self.buf = [AudioBufferOracle(context_window + 2.0, SR) for _ in range(n_streams)]
        self.last = [-1] * n_streams
        self.has = [False] * n_streams
        self.slot_from = [None] * n_streams          # the update (step index) whose features the 300 / 600 ms slots hold
        self.step_index = -1

    def reset(self, s: int) -> None:
        self.buf[s] = AudioBufferOracle(self.context + 2.0, SR)
        self.last[s], self.has[s], self.slot_from[s] = -1, False, None

    def window(self, s: int) -> np.ndarray:
        b = self.buf[s]
        if b.total == 0:
            return np.zeros(0, np.float32)       # the reference's window of zeros from an empty buffer is not reproduced
        return b.get_window(self.context)

    def step(self, row) -> dict:
        """push one chunk per stream (an empty one leaves the stream alone), then update."""
        self.step_index += 1
        for s, c in enumerate(row):
            if len(c):
                self.buf[s].append(c)
        waits = {}
        for s in range(self.n):
            total = self.buf[s].total
            due = (not self.has[s]) or total - self.last[s] >= self.U
            if total > 0 and due and len(self.window(s)) >= self.MIN:
                waits[s] = total - self.last[s]
        chosen = sorted(waits, key=lambda s: (-waits[s], s))[:self.max_updates]
        windows = {}
        for s in chosen:
            windows[s] = self.window(s)
            if self.slot_from[s] is None:
                self.slot_from[s] = self.step_index
            self.last[s], self.has[s] = self.buf[s].total, True
        return dict(updated=sorted(chosen), order=chosen, windows=windows, valid=list(self.has), slot_from=list(self.slot_from))


@functools.lru_cache(maxsize=None)
def simulate(max_updates=None, with_reset=True):
    """Schedule S through the oracle: one record per step."""
    o = EmotionStreamOracle(N_STREAMS, CONTEXT, INTERVAL, max_updates)
    out = []
    for t, row in enumerate(chunks()):
        if with_reset:
            for s in RESETS.get(t, ()):
                o.reset(s)
        out.append(o.step(row))
    return out


def simulate_alone(s: int):
    """Stream s of schedule S as the only stream of an oracle of its own: the steps on which it updates."""
    o = EmotionStreamOracle(1, CONTEXT, INTERVAL)
    steps = []
    for t, row in enumerate(chunks()):
        if s in RESETS.get(t, ()):
            o.reset(0)
        if o.step([row[s]])["updated"]:
            steps.append(t)
    return steps
