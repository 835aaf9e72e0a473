"""Inputs and float64-oracle expectations shared by tests/test_gpu_streaming_d512.py and tests/test_stream_shapes_host.py:
the 60 fps long-context streaming configuration (d_model 512, window 512, 8 / 16 heads, update_interval 1/60, front end
n_fft 1024 at hop 266, reflect padding).

The reference formulas behind the shapes (src/features/mel_sliding_window.py:46-50, 112, 280-307):
    ring_len          = int(context_window * sample_rate)
    ring_hop          = int(sample_rate / (1 / update_interval))
    n_frames          = 1 + ring_len // mel_hop                      (librosa, center=True)
    stream_out_frames = int(context_window / update_interval)        (rows kept: truncate / repeat the last frame)
"""
import functools

import numpy as np
import torch

from koemorph_amd import synth
from oracle import buffers, core, mel as omel, smoothing

SR, MEL_HOP, UI60 = 16000, 266, 1.0 / 60.0
PARAMS_SEED = 21


@functools.lru_cache(maxsize=None)
def params():
    return synth.make_core_params(PARAMS_SEED, 512, 512, 256, "trained")     # as tests/test_gpu_core.py makes its d512 parameters


# ---- the short ring: 3 streams, context 1.0 s, frames of 266 / 267 samples alternately ----------------------------------------
SHORT_S, SHORT_CW, SHORT_TICKS = 3, 1.0, 71
SHORT_FIRST_READY = 60                       # 61 frames of 266 samples >= 16000: the ring is full (and its write pointer has wrapped)
SHORT_CHECKED = (60, 61, 62, 65, 68, 70)     # the first ready tick (EMA 'first' branch), the two after it, three later ones
LOUD_STREAM = 2


def frame_len(t):
    return 266 + (t & 1)


@functools.lru_cache(maxsize=None)
def short_frames():
    """[tick] -> (3, 266 | 267) float32.  Stream 2 is quiet except for one burst inside the frame pushed at every checked tick,
    each three times the amplitude of the one before: at a checked tick the newest burst sits in the last 266 samples of the
    window, i.e. under STFT frame 60 -- past the U = 60 rows the extractor keeps -- and weighs 9 times the older ones, so the
    window maximum (the dB reference) lies in a frame that truncation drops (tests/test_stream_shapes_host.py checks that it does)."""
    total = sum(frame_len(t) for t in range(SHORT_TICKS))
    audio = synth.make_audio(31, SHORT_S, total).copy()
    audio[LOUD_STREAM] *= 1e-3
    out, pos, amp = [], 0, 1e-2
    for t in range(SHORT_TICKS):
        n = frame_len(t)
        f = audio[:, pos:pos + n].copy()
        if t in SHORT_CHECKED:
            f[LOUD_STREAM, 100:260] = amp * np.sign(synth.uniform(400 + t, (160,)))
            amp *= 3.0
        out.append(np.ascontiguousarray(f, np.float32))
        pos += n
    return out


@functools.lru_cache(maxsize=None)
def short_emotion():
    return synth.normal(33, (SHORT_S, 256))


def stream_features(win, context_window):
    return omel.mel_sliding_window(win, n_fft=1024, hop=MEL_HOP, context_window=context_window, update_interval=UI60)


def oracle_blendshapes(win, emo_row, heads, context_window):
    """One stream's unsmoothed 52 coefficients for the ring content `win`: sliding-window dB mel, core in float64."""
    feats = stream_features(win, context_window)
    out = core.core_forward_np(params(), feats[None], feats[None, -3:], emo_row[None], num_heads=heads, mel_sequence_length=512,
                               dtype=torch.float64)["blendshapes"]
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def short_windows():
    """{tick: [ring content of every stream]} at the checked ticks, and the tick at which the oracle rings report full."""
    rings = [buffers.MelAudioBufferOracle(SHORT_CW, SR, UI60) for _ in range(SHORT_S)]
    wins, first = {}, None
    for t, f in enumerate(short_frames()):
        for s in range(SHORT_S):
            assert rings[s].add_audio_frame(f[s])
        if rings[0].is_full and first is None:
            first = t
        if t in SHORT_CHECKED:
            wins[t] = [rings[s].get_current_audio() for s in range(SHORT_S)]
    return wins, first


@functools.lru_cache(maxsize=None)
def short_expected(heads, t):
    """(3, 52) unsmoothed oracle outputs at checked tick t, computed once per head count and tick."""
    w = short_windows()[0][t]
    emo = short_emotion()
    return np.concatenate([oracle_blendshapes(w[s], emo[s], heads, SHORT_CW) for s in range(SHORT_S)])


def smoother():
    return smoothing.TemporalSmootherOracle(0.8)
