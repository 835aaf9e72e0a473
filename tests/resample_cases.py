"""Oracle, inputs, error bound and stream schedules of the device resampler (km_resampler_* / km_resample_clip), shared by
tests/test_resample_host.py (no GPU), tests/test_gpu_resample.py, tests/test_gpu_resample_stream.py and
tests/test_gpu_dataset_resample.py.  Everything is computed once and shared; callers must not modify it.

The oracle is the output law in float64, by brute force over the taps of the float64 filter:
    y[m] = sum_j x[j] h[m down - j up + half_len],   tap index in [0, 2 half_len], 0 <= j < N,   n_out = ceil(N up / down).

The error bound of one output whose sum has n terms (the float32 samples are the oracle's input, so they carry no error):
    (n + 2) 2^-24 sum_k |h_k| |x_j|.
The kernel rounds each coefficient to float32 once (relative 2^-24) and then runs one fmaf chain, one rounding per step:
n roundings of partial sums that are bounded by the sum of absolute terms, (1 + 2^-24)^(n + 1) - 1 < (n + 2) 2^-24 for n < 2^20.
Terms outside the signal are exact zeros in the kernel and absent here, so n counts the terms with 0 <= j < N.
"""
from __future__ import annotations

import functools

import numpy as np

from koemorph_amd import synth
from koemorph_amd.features import resample as rs

RATE_OUT = 16000
CLIP_RATES = (48000, 44100, 32000, 8000, 11025)           # 1/3 (61 taps), 160/441 (8821), 1/2, 2/1, 640/441 (12801, the largest table)
LAW_RATES = (48000, 44100, 32000, 22050, 8000)
CHUNK_SIZES = (0, 1, 7, 160, 1024, 1600)


@functools.lru_cache(maxsize=None)
def plan(rate_in: int):
    """(up, down, h float64 read-only, half_len)"""
    up, down = rs.resample_ratio(rate_in, RATE_OUT)
    h, half_len = rs.resample_filter(up, down)
    h.setflags(write=False)
    return up, down, h, half_len


def clip_lengths(rate_in: int):
    """1, 2, down - 1, 61, the shortest input that needs a second output tile (one tile + 1 outputs; + 2 where up = 2 makes
    every length even), and 5000 (deduplicated, in this order)."""
    up, down, _, _ = plan(rate_in)
    tile_plus_1 = (rs.CLIP_TILE * down) // up + 1
    assert rs.n_out(tile_plus_1 - 1, up, down) <= rs.CLIP_TILE < rs.n_out(tile_plus_1, up, down) <= rs.CLIP_TILE + up
    out = []
    for n in (1, 2, down - 1, 61, tile_plus_1, 5000):
        if n >= 1 and n not in out:
            out.append(n)
    return out


@functools.lru_cache(maxsize=None)
def signal(seed: int, n: int) -> np.ndarray:
    x = synth.make_audio(seed, 1, n)[0].astype(np.float32)
    x.setflags(write=False)
    return x


def oracle(x: np.ndarray, rate_in: int):
    """(y float64 (n_out), bound float64 (n_out)) of the float32 samples x."""
    up, down, h, half_len = plan(rate_in)
    N = int(x.shape[0])
    n_out = rs.n_out(N, up, down)
    xd = x.astype(np.float64)
    m = np.arange(n_out, dtype=np.int64)
    c = m * down + half_len
    q = c // up                                              # the newest sample an output reads
    K = (2 * half_len) // up + 1
    y = np.zeros(n_out)
    mag = np.zeros(n_out)
    terms = np.zeros(n_out, np.int64)
    for k in range(K):                                       # ascending k is descending j; float64 makes the order immaterial here
        j = q - k
        t = c - j * up
        ok = (t <= 2 * half_len) & (j >= 0) & (j < N)
        jj, tt = np.where(ok, j, 0), np.where(ok, t, 0)
        term = np.where(ok, xd[jj] * h[tt], 0.0)
        y += term
        mag += np.abs(term)
        terms += ok
    return y, (terms + 2) * 2.0 ** -24 * mag


@functools.lru_cache(maxsize=None)
def clip_case(rate_in: int, n: int):
    x = signal(900 + rate_in % 97, n)
    y, bound = oracle(x, rate_in)
    y.setflags(write=False)
    bound.setflags(write=False)
    return x, y, bound


def oracle_direct(x: np.ndarray, up: int, down: int, h: np.ndarray, half_len: int) -> np.ndarray:
    """The output law term by term in Python loops (small inputs): what `oracle` vectorises."""
    N = len(x)
    y = np.zeros(rs.n_out(N, up, down))
    for m in range(len(y)):
        for j in range(N):
            t = m * down - j * up + half_len
            if 0 <= t <= 2 * half_len:
                y[m] += float(x[j]) * h[t]
    return y


def emitted_brute(n: int, up: int, down: int, half_len: int) -> int:
    """The number of leading outputs whose taps touch no sample at or beyond n."""
    m = 0
    while (m * down + half_len) // up <= n - 1:              # the newest sample output m reads has arrived
        m += 1
    return m


# ---- stream schedules ------------------------------------------------------------------------------------------------
# counts[step][stream]: on every step stream s brings the next counts[step][s] samples of its own source; `resets` maps a step
# to the streams reset before that step's push.  Three streams, about 5000 samples each: stream 0 cycles through the chunk
# sizes, stream 1 joins late and pauses, stream 2 is reset mid-way and refilled.
STREAMS, STEPS, N_MAX, RESET_STEP = 3, 12, 1600, 6
_CYCLE = (160, 1, 1024, 0, 7, 1600, 1024, 160, 0, 1, 1024, 7)


def _counts(t, s):
    if s == 0:
        return _CYCLE[t]
    if s == 1:
        return 0 if t < 3 or t in (7, 8) else (1600, 7, 1024, 160, 1, 1024, 1600)[(t - 3) - (2 if t > 8 else 0)]
    return (1024, 160, 7, 1600, 1, 1024, 1600, 7, 160, 1024, 0, 1)[t]


@functools.lru_cache(maxsize=None)
def schedule():
    counts = np.array([[_counts(t, s) for s in range(STREAMS)] for t in range(STEPS)], np.int32)
    counts.setflags(write=False)
    return counts, {RESET_STEP: (2,)}


@functools.lru_cache(maxsize=None)
def stream_sources(rate_in: int) -> np.ndarray:
    counts, _ = schedule()
    x = synth.make_audio(700 + rate_in % 89, STREAMS, int(counts.sum(axis=0).max()))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def stream_chunks(rate_in: int):
    """[step] -> (STREAMS, N_MAX) float32 feed tensors (row s holds counts[step][s] samples, then a filler that must be ignored)."""
    counts, _ = schedule()
    src = stream_sources(rate_in)
    pos = np.zeros(STREAMS, np.int64)
    out = []
    for t in range(STEPS):
        x = np.full((STREAMS, N_MAX), 7.0, np.float32)
        for s in range(STREAMS):
            n = int(counts[t, s])
            x[s, :n] = src[s, pos[s]:pos[s] + n]
            pos[s] += n
        x.setflags(write=False)
        out.append(x)
    return out


def stream_lives(rate_in: int):
    """Per stream the list of lives [(first step, input of that life)]: a reset starts a new life with the samples that follow."""
    counts, resets = schedule()
    src = stream_sources(rate_in)
    lives = []
    for s in range(STREAMS):
        cuts = [0] + [int(counts[:t, s].sum()) for t in sorted(resets) if s in resets[t]] + [int(counts[:, s].sum())]
        starts = [0] + [t for t in sorted(resets) if s in resets[t]]
        lives.append([(starts[i], src[s, cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)])
    return lives
