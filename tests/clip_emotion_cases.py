"""The emotion track of a clip in closed form (km_emotion_clip_*, koemorph_amd.features.ClipEmotion), shared by
tests/test_clip_emotion_host.py and tests/test_gpu_clip_emotion.py: which windows the track's rows are extracted from, and which
row a training window takes.  Host integers only; nothing here computes features.
"""
from __future__ import annotations

import math

SR = 16000


def shape(context_window: float, update_interval: float) -> dict:
    """R, C, U, MIN as km_emotion_stream_create computes them."""
    R = int((context_window + 2.0) * SR)
    return dict(R=R, C=min(int(context_window * SR), R), U=int(update_interval * SR), MIN=int(0.5 * SR))


def chunk(context_window: float, update_interval: float) -> int:
    """The chunk size at which a stream fed the clip updates at exactly the track's times."""
    sh = shape(context_window, update_interval)
    return math.gcd(sh["MIN"], sh["U"])


def num_rows(n: int, context_window: float, update_interval: float) -> int:
    sh = shape(context_window, update_interval)
    return 0 if n < sh["MIN"] else (n - sh["MIN"]) // sh["U"] + 1


def plan(n: int, context_window: float, update_interval: float) -> list:
    """[(t_k, start, length)] for the K rows of a clip of n samples: the window AudioBuffer.get_window returns after t_k samples --
    the OLDEST C samples while the ring of R has not wrapped, the newest C from then on."""
    sh = shape(context_window, update_interval)
    out = []
    for k in range(num_rows(n, context_window, update_interval)):
        t = sh["MIN"] + k * sh["U"]
        out.append((t, 0, min(t, sh["C"])) if t < sh["R"] else (t, t - sh["C"], sh["C"]))
    return out


def window_row(start_frame: int, window_frames: int, hop: int, n: int, context_window: float, update_interval: float):
    """-> (row, valid) of the window that starts at frame start_frame: the last update made by the time it ends."""
    sh = shape(context_window, update_interval)
    K = num_rows(n, context_window, update_interval)
    if K == 0:
        return 0, 0
    e = min(n, (start_frame + window_frames) * hop)
    return max(0, min((e - sh["MIN"]) // sh["U"], K - 1)), 1
