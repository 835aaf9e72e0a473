"""The restatement of the `basic` prosodic emotion features and the inputs of their tests, shared by tests/test_prosody_host.py
and tests/test_gpu_prosody*.py.  NumPy only.

PARITY UNPINNED.  The reference's EmotionExtractor._extract_basic (src/features/emotion_extractor.py:503-545) calls
librosa.feature.zero_crossing_rate, librosa.feature.spectral_centroid and librosa.yin(fmin=50, fmax=400) and pins only
librosa>=0.10.0; the package is not part of this repository's environment.  ``analyse`` restates what those functions do at their
0.10 defaults, written from the algorithms, and has NOT been checked against the package by anyone.  One deliberate deviation:
librosa obtains yin's difference function from an FFT autocorrelation and zeroes terms below 1e-6; here it is the direct sum of
squared differences (equal wherever a frame's energy is far above 1e-6, exactly 0 on digital silence: f0 = 400, as librosa gives).

With y one window of L >= 1 samples at 16 kHz: F = 1 + L // 512 frames; frame f position n in [0, 2048) reads source index
s = 512 f + n - 1024; z_f[n] = y[s] inside [0, L) and 0 outside (zero padding), e_f[n] = y[clip(s, 0, L - 1)] (edge padding).
``analyse(y, dtype)`` evaluates everything in ``dtype``: float64 is the oracle, float32 the yardstick of the GPU comparison (the
precision librosa itself works at on float32 audio).
"""
from __future__ import annotations

import functools

import numpy as np

from koemorph_amd import synth

SR, NFFT, HOP, TMIN, TMAX = 16000, 2048, 512, 40, 320
NC = TMAX - TMIN + 1                      # 281 candidate periods 40 .. 320 (fmax = 400 Hz, fmin = 50 Hz)
THRESHOLD = 0.1
FEATURE_NAMES = ("energy", "zcr", "spectral_centroid", "f0_mean", "f0_std", "mean", "std", "max", "min")


def num_frames(L: int) -> int:
    return 1 + L // HOP if L >= 1 else 0


def frame_matrix(y: np.ndarray):
    """-> (z (F, 2048) zero padded, e (F, 2048) edge padded), in y's dtype."""
    L = len(y)
    s = HOP * np.arange(num_frames(L))[:, None] + np.arange(NFFT)[None, :] - NFFT // 2
    e = y[np.clip(s, 0, L - 1)]
    z = np.where((s >= 0) & (s < L), e, y.dtype.type(0))
    return z, e


def choose(c: np.ndarray) -> int:
    """i*: the first trough of c below the threshold, else the first index of the minimum."""
    n = len(c)
    for i in range(n):
        if i == 0:
            trough = c[0] < c[1]
        elif i == n - 1:
            trough = c[i] < c[i - 1]
        else:
            trough = c[i] < c[i - 1] and c[i] <= c[i + 1]
        if trough and c[i] < THRESHOLD:
            return i
    return int(np.argmin(c))


def shift_of(c: np.ndarray, i: int):
    """Parabolic interpolation around i: -b / a where 0 < i < n - 1 and |b| < |a|, else 0 (in c's dtype)."""
    if 0 < i < len(c) - 1:
        a = c[i + 1] + c[i - 1] - 2 * c[i]
        b = (c[i + 1] - c[i - 1]) / 2
        if abs(b) < abs(a):
            return -b / a
    return c.dtype.type(0)


def decision_margin(c: np.ndarray, i_star: int) -> float:
    """How far the comparisons that decide i* are from flipping, in units of c.  An index i < i* is passed over because one of
    (c[i] < c[i-1], c[i] <= c[i+1], c[i] < 0.1) is false: the margin of that decision is the largest distance among its false
    comparisons; at i* all are true and the margin is the smallest distance among them.  Without a qualifying trough every index
    is passed over and the gap between the minimum and the runner-up counts as well.  inf for a row that is constant: there the
    first-index rule decides alone (see ``exact_tie``)."""
    n = len(c)
    if c.max() == c.min():
        return float("inf")

    def comparisons(i):
        out = [(c[i] < THRESHOLD, abs(c[i] - THRESHOLD))]
        if i > 0:
            out.append((c[i] < c[i - 1], abs(c[i] - c[i - 1])))
        if i < n - 1:
            out.append((c[i] < c[i + 1] if i == 0 else c[i] <= c[i + 1], abs(c[i] - c[i + 1])))
        return out

    qualifies = lambda i: all(t for t, _ in comparisons(i))
    found = qualifies(i_star)
    margin = float("inf")
    for i in range(i_star + 1 if found else n):
        cmp = comparisons(i)
        if all(t for t, _ in cmp):
            margin = min(margin, min(m for _, m in cmp))
        else:
            margin = min(margin, max(m for t, m in cmp if not t))
    if not found:
        srt = np.sort(c)
        margin = min(margin, float(srt[1] - srt[0]))
    return float(margin)


def analyse(y: np.ndarray, dtype=np.float64) -> dict:
    """Everything the features are made of, evaluated in ``dtype``:
    Z, C, f0, period (F) per frame, istar (F) int, c (F, 281), out (9) in the order of FEATURE_NAMES."""
    dt = np.dtype(dtype).type
    y = np.ascontiguousarray(y, np.float32).astype(dtype)
    L = len(y)
    assert L >= 1
    F = num_frames(L)
    z, e = frame_matrix(y)
    # zero_crossing_rate: threshold 1e-10 zeroes small values, then signbit; position 0 never counts
    neg = e < dt(-1e-10)
    Z = (neg[:, 1:] != neg[:, :-1]).sum(axis=1).astype(dtype) / dt(NFFT)
    # spectral_centroid of the magnitude STFT, periodic Hann window
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)).astype(dtype)
    mag = np.abs(np.fft.rfft(z * w, axis=1))
    assert mag.dtype == np.dtype(dtype), mag.dtype            # numpy >= 2 keeps float32 through the transform
    freq = (np.arange(NFFT // 2 + 1) * (SR / NFFT)).astype(dtype)
    S = mag.sum(axis=1)
    S = np.where(S < np.finfo(np.float32).tiny, dt(1), S)
    C = (mag * freq).sum(axis=1) / S
    # yin: difference function, cumulative mean normalisation, first trough below the threshold, parabolic interpolation
    d = np.stack([((z[:, 1:1025] - z[:, 1 + t:1025 + t]) ** 2).sum(axis=1) for t in range(TMAX + 1)], axis=1)     # (F, 321)
    cum = np.cumsum(d[:, 1:], axis=1) / np.arange(1, TMAX + 1).astype(dtype)                                     # (F, 320): tau 1 ..
    c = d[:, TMIN:] / (cum[:, TMIN - 1:] + dt(np.finfo(np.float32).tiny))
    istar = np.array([choose(row) for row in c])
    period = np.array([dt(TMIN + i) + shift_of(row, i) for row, i in zip(c, istar)], dtype)
    f0 = dt(SR) / period
    out = np.array([np.mean(y * y), np.mean(Z), np.mean(C), np.mean(f0), np.std(f0), np.mean(y), np.std(y), np.max(y), np.min(y)], dtype)
    return dict(Z=Z, C=C, f0=f0, period=period, istar=istar, c=c, out=out)


def exact_tie(y: np.ndarray) -> bool:
    """The rows of c are constant in float64 AND in float32 on every frame: i* = 0 by the first-index rule in any precision."""
    return all((r["c"].max(axis=1) == r["c"].min(axis=1)).all() for r in (analyse(y, np.float64), analyse(y, np.float32)))


# ---- the inputs of the GPU comparison -----------------------------------------------------------------------------------------
KINDS = ("vibrato", "noise", "chirp")
LENGTHS = (1, 511, 512, 513, 5000, 16000)
SEEDS = {"vibrato": 4104, "noise": 4205, "chirp": 4304}      # picked for the margins test_prosody_host.py asserts
MIN_MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def _full(kind: str) -> np.ndarray:
    n = max(LENGTHS)
    t = np.arange(n) / SR
    seed = SEEDS[kind]
    if kind == "vibrato":        # a harmonic complex whose 140 Hz fundamental wobbles by 3 % five times a second, plus noise
        phase = 2.0 * np.pi * np.cumsum(140.0 * (1.0 + 0.03 * np.sin(2.0 * np.pi * 5.0 * t))) / SR
        x = 0.25 * sum(np.sin(h * phase) / h for h in range(1, 7)) + 0.01 * synth.normal(seed, (n,))
    elif kind == "noise":
        x = 0.3 * synth.normal(seed, (n,))
    else:                        # a 100 -> 400 Hz chirp gated on and off every 0.15 s, on a DC offset, plus noise
        gate = ((t // 0.15) % 2 == 0).astype(np.float64)
        x = 0.4 * gate * np.sin(2.0 * np.pi * (100.0 * t + 150.0 * t * t)) + 0.05 + 0.005 * synth.normal(seed, (n,))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def signal(kind: str, L: int) -> np.ndarray:
    """The first L samples of the kind's signal.  L = 1 is special by construction, whatever the sample v: every lag's sum is the
    same 2 v^2, so nothing but the first-index rule decides i*.  There the sample is rounded to a power of two, which makes every
    entry of c exactly 1 in float64 and in float32 alike (``exact_tie``): the rule is what is tested, not a rounding."""
    x = _full(kind)[:L].copy()
    if L == 1:
        x[0] = np.float32(2.0 ** np.round(np.log2(abs(float(x[0])))) * (1 if x[0] >= 0 else -1))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle(kind: str, L: int) -> dict:
    return analyse(signal(kind, L), np.float64)


@functools.lru_cache(maxsize=None)
def yardstick(kind: str, L: int) -> dict:
    return analyse(signal(kind, L), np.float32)


def bound(kind: str, L: int, key: str) -> np.ndarray:
    """The tolerance of the GPU comparison for one case and quantity: 8 x the float32 evaluation's largest error against float64,
    floored at 2^-22 relative to each reference value.  The factor covers a summation order and an FFT factorisation other than
    NumPy's; a wrong window, twiddle or lag offset is orders of magnitude beyond it."""
    ref, y32 = oracle(kind, L)[key], yardstick(kind, L)[key].astype(np.float64)
    err = np.abs(y32 - ref)
    if key != "out":                      # per-frame quantities: the largest error over the frames; "out" holds nine quantities
        err = err.max()
    return np.maximum(8.0 * err, 2.0 ** -22 * np.abs(ref))
