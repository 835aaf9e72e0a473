"""Float64-oracle expectations of tests/test_gpu_streaming_d256w.py: streaming at the shape of the reference's frame_rate=60
recipe (d_model 256, 8 heads, window 512, update_interval 1/60, front end n_fft 1024 at hop 266, reflect padding).  The audio, the
emotion rows, the ring oracle and the feature function are those of tests/stream_d512_cases.py; only the core's parameters differ.
Not a test module."""
import functools

import numpy as np
import torch

import stream_d512_cases as sc
from koemorph_amd import synth
from oracle import core

PARAMS_SEED = 23
HEADS, D_MODEL, WINDOW = 8, 256, 512


@functools.lru_cache(maxsize=None)
def params():
    return synth.make_core_params(PARAMS_SEED, D_MODEL, WINDOW, 256, "trained")


def oracle_blendshapes(win, emo_row, context_window):
    """One stream's unsmoothed 52 coefficients for the ring content `win`: sliding-window dB mel, core in float64."""
    feats = sc.stream_features(win, context_window)
    out = core.core_forward_np(params(), feats[None], feats[None, -3:], emo_row[None], num_heads=HEADS, mel_sequence_length=WINDOW,
                               dtype=torch.float64)["blendshapes"]
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def short_expected(t):
    """(3, 52) unsmoothed oracle outputs of the short ring at checked tick t, computed once per tick; not to be modified."""
    w = sc.short_windows()[0][t]
    emo = sc.short_emotion()
    return np.concatenate([oracle_blendshapes(w[s], emo[s], sc.SHORT_CW) for s in range(sc.SHORT_S)])
