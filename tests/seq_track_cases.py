"""Sequence mode with an emotion track, per window in float64: the oracle tests/test_gpu_sequence_track.py compares against.

``SequentialOracle`` takes one emotion vector per clip, so the sequence with a track is composed here from its parts: window i of
every clip (zero-padded past the clip end, sequential_dual_stream_model.py:101-115) goes through ``SimplifiedOracle.forward(window,
row_i, smooth=False)`` with the track row the window maps to, and ``TemporalSmootherOracle`` runs along the frame axis.  The
window's log-mel does not depend on the emotion input, so ``WindowOracle`` computes it once per window for all mappings compared.
"""
from __future__ import annotations

import functools
import hashlib

import numpy as np

from koemorph_amd import synth
from koemorph_amd.engine import sequence_track_row
from oracle import models, smoothing

HOP, T = 533, 256
FIRST, INTERVAL = 8000, 4800                    # min_samples / update_samples of the default 20 s / 0.3 s ClipEmotion
PARAM_SEED, AUDIO_SEED, TRACK_SEED, CLIPS = 52, 90, 191, 2


def clip_length(extra_hops: int) -> int:
    return 136448 + 533 * extra_hops + 100


def num_outputs(L: int, stride: int, hop: int = HOP, window: int = T) -> int:
    return max(1, (L // hop - window) // stride + 1)


def num_rows(L: int) -> int:
    return 0 if L < FIRST else (L - FIRST) // INTERVAL + 1


@functools.lru_cache(maxsize=None)
def params():
    return synth.make_core_params(PARAM_SEED, style="trained")


@functools.lru_cache(maxsize=None)
def audio(extra_hops: int) -> np.ndarray:
    a = synth.make_audio(AUDIO_SEED, CLIPS, clip_length(extra_hops))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def track(K: int, seed: int = TRACK_SEED) -> np.ndarray:
    t = synth.normal(seed, (CLIPS, K, 256))
    t.setflags(write=False)
    return t


def window_rows(L: int, stride: int, K: int, first: int, interval: int, hop: int = HOP, window: int = T):
    return [sequence_track_row(i, K, first, interval, 0, L, stride, window, hop) for i in range(num_outputs(L, stride, hop, window))]


class WindowOracle(models.SimplifiedOracle):
    """SimplifiedOracle whose log-mel of a window is computed once: the mappings compared differ in the emotion rows alone."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._mels = {}

    def extract_mel_features(self, audio):
        key = hashlib.blake2b(np.ascontiguousarray(audio).tobytes(), digest_size=16).digest()
        if key not in self._mels:
            self._mels[key] = super().extract_mel_features(audio)
        return self._mels[key]


def sequence_with_rows(orc: models.SimplifiedOracle, clips: np.ndarray, trk: np.ndarray, stride: int, rows, smooth: bool,
                       alpha: float = 0.8) -> np.ndarray:
    """(B, N, 52): window i, cut and zero-padded as SequentialOracle.forward does, with row rows[i] of every clip's track; EMA
    along the frames when ``smooth``."""
    B, L = clips.shape
    W = orc.mel_sequence_length * orc.hop
    assert len(rows) == num_outputs(L, stride, orc.hop, orc.mel_sequence_length)
    sm = smoothing.TemporalSmootherOracle(alpha)
    frames = []
    for i, k in enumerate(rows):
        s = i * stride * orc.hop
        e = min(s + W, L)
        win = np.zeros((B, W), np.float32)
        win[:, :e - s] = clips[:, s:e]
        o = orc.forward(win, np.array(trk[:, k]), smooth=False)["blendshapes"]       # a copy: the shared track stays read-only
        frames.append(sm(o) if smooth else o)
    return np.stack(frames, axis=1)


@functools.lru_cache(maxsize=None)
def production_oracle():
    return WindowOracle(params())
