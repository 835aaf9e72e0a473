"""Inputs and float64-oracle expectations of tests/test_gpu_streaming_d128.py and tests/test_stream_d128_host.py: streaming at the
reference's `fast` (d_model 128, 4 heads, window 128, emotion_dim 256) and `basic` (window 256, emotion_dim 9) variants at 30 fps --
update_interval 0.0333 (ring hop 532), front end n_fft 1024 at hop 533, reflect padding.  The pipeline is that of
tests/stream_d512_cases.py: MelAudioBuffer ring -> sliding-window dB mel -> core in float64 with the last three kept rows as short
rows -> EMA.  Not a test module.

The reference formulas behind the shapes (src/features/mel_sliding_window.py:46-50, 112, 280-307):
    ring_len          = int(context_window * sample_rate)
    ring_hop          = int(sample_rate / (1 / update_interval))     532
    n_frames          = 1 + ring_len // mel_hop                      (librosa, center=True)
    stream_out_frames = int(context_window / update_interval)        (rows kept: truncate / repeat the last frame)
"""
import functools

import numpy as np
import torch

from core_logit_cases import make_params
from koemorph_amd import synth
from oracle import buffers, core, mel as omel, smoothing

SR, MEL_HOP, UI30 = 16000, 533, 0.0333
D_MODEL, HEADS = 128, 4
# name: (window T, emotion_dim, seed of the parameters) -- shapes and seeds of tests/test_gpu_generic_shapes.py
VARIANTS = {"fast": (128, 256, 91), "basic": (256, 9, 93)}


@functools.lru_cache(maxsize=None)
def params(name):
    T, ED, seed = VARIANTS[name]
    return make_params("trained", seed, D_MODEL, T, ED)


def frame_len(t):
    return 532 + (t & 1)


# ---- the short ring: 3 streams, context 1.0 s: 31 frames computed, U = 30 kept, zero rows up to T --------------------------------------
SHORT_S, SHORT_CW, SHORT_TICKS = 3, 1.0, 41
SHORT_FIRST_READY = 30                       # 15 x 532 + 15 x 533 = 15975 < 16000 <= 16507: the 31st frame fills the ring
SHORT_CHECKED = (30, 31, 32, 35, 38, 40)     # the first ready tick (EMA 'first' branch), the two after it, three later ones
LOUD_STREAM = 2


@functools.lru_cache(maxsize=None)
def short_frames():
    """[tick] -> (3, 532 | 533) float32.  The loud-burst construction of stream_d512_cases.short_frames at this hop: stream 2 is quiet
    except for one burst at the end of the frame pushed at every checked tick, each three times the amplitude of the one before.  At a
    checked tick the newest burst sits in the last 233 samples of the window, near the centre of STFT frame 30 (and mirrored by its
    reflect padding) but in the outer third of frame 29's Hann window -- so the window maximum, the dB reference, lies in frame 30,
    past the U = 30 rows the extractor keeps (tests/test_stream_d128_host.py checks that it does)."""
    total = sum(frame_len(t) for t in range(SHORT_TICKS))
    audio = synth.make_audio(31, SHORT_S, total).copy()
    audio[LOUD_STREAM] *= 1e-3
    out, pos, amp = [], 0, 1e-2
    for t in range(SHORT_TICKS):
        n = frame_len(t)
        f = audio[:, pos:pos + n].copy()
        if t in SHORT_CHECKED:
            f[LOUD_STREAM, 300:520] = amp * np.sign(synth.uniform(400 + t, (220,)))
            amp *= 3.0
        out.append(np.ascontiguousarray(f, np.float32))
        pos += n
    return out


@functools.lru_cache(maxsize=None)
def short_emotion(name):
    return synth.normal(33, (SHORT_S, VARIANTS[name][1]))


def ring(context_window):
    return buffers.MelAudioBufferOracle(context_window, SR, UI30)


def stream_features(win, context_window):
    return omel.mel_sliding_window(win, n_fft=1024, hop=MEL_HOP, context_window=context_window, update_interval=UI30)


def oracle_blendshapes(name, win, emo_row, context_window):
    """One stream's unsmoothed 52 coefficients for the ring content `win`: sliding-window dB mel, core in float64.  The features hold
    the U kept rows; the core truncates or zero-pads them to the window, the short rows are the last three kept ones."""
    feats = stream_features(win, context_window)
    out = core.core_forward_np(params(name), feats[None], feats[None, -3:], emo_row[None], num_heads=HEADS,
                               mel_sequence_length=VARIANTS[name][0], dtype=torch.float64)["blendshapes"]
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def short_windows():
    """{tick: [ring content of every stream]} at the checked ticks, and the tick at which the oracle rings report full."""
    rings = [ring(SHORT_CW) for _ in range(SHORT_S)]
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
def short_expected(name, t):
    """(3, 52) unsmoothed oracle outputs of the short ring at checked tick t, computed once per variant and tick; not to be modified."""
    w = short_windows()[0][t]
    emo = short_emotion(name)
    return np.concatenate([oracle_blendshapes(name, w[s], emo[s], SHORT_CW) for s in range(SHORT_S)])


def smoother():
    return smoothing.TemporalSmootherOracle(0.8)
