"""Shared by tests/test_koemorph_audio_host.py and tests/test_gpu_koemorph_audio.py: the law of km_koemorph_audio_rows restated in
numpy, a brute-force walk of its clock and window table, the shifted frame grid of the emotion rows, a restatement of
km_koemorph_audio_plan and the schedules the tests walk.

THE LAW.  hop = int(16000 / fps) (float64, as MelSpectrogramExtractor computes it).  Stream s has received n_s samples since creation
or its last reset.  Frame k is due as soon as n_s >= (k + 1) * hop: after a push the stream has K = n_s // hop frames, and the push
renders frames c_s .. K - 1 in order (c_s: the count before it).  Supported: hop >= 257 and fps >= 10.

Mel row k: the row of the STFT frame centred on sample k * hop of the stream, in the configuration MelConfig.torchaudio(16000, fps,
512, mel_dim, 80.0, 8000, normalized=True, "reflect", 1e-8); reflection at the stream's first sample only (with hop >= 257 every frame
has its samples when it is due).  A function of the stream's samples alone: row k of the dense extractor on any prefix that holds
sample k * hop + 255 and one more, up to float32 rounding.

Emotion row k: a push that leaves stream s with new frames sets the window -- a0 the smallest multiple of 160 >= n_s - W (0 while
n_s <= W), len = n_s - a0, m = a0 // 160, nf = (len - 960) // 160 + 1 (0 for len < 960).  Its descriptors are the native rows of
EGeMAPSEngine.llds(audio[a0:n_s], normalize=True, fps=None).  Row k sits at p = float64(k * hop) / 160.0, j = floor(p) - m,
w = p - floor(p): frame 0 for j < 0, the last frame for j >= nf - 1, frame j for w == 0, otherwise fmaf(float32(w), b - a, a) between
frames j and j + 1 -- except that a column smoothed over non-zero values takes the nearer frame where either side is 0 (the earlier at
w == 0.5).  The row is emotion_dim wide, zeros to the right; a window without a frame gives a row of zeros.  Emotion rows depend on the
push schedule: the window ends where the push ends.

Creation: W = int(emotion_window * 16000) >= max_samples + hop + 1120 (then j >= 0 and every full window has a frame), a window of at
most 2048 frames, ring_len = W + max_samples, max_rows = max_samples // hop + 1.  Sample i of a life sits at (origin + i) mod ring_len;
a reset makes the ring's write position the next life's origin."""
import numpy as np

ENTRY = 48          # bytes of a table entry (four int64, four int32)
SLOT = 16           # bytes of an eGeMAPS slot
REC = 36            # floats of a frame record
LLD_WIDTH = {"eGeMAPSv02": 25, "GeMAPS": 18}


def hop_of(fps):
    return int(16000 / fps)


def window_samples(seconds):
    return int(seconds * 16000)


def window(n, W):
    """(a0, len, m, nf) of a push that ends at n samples."""
    a0 = 0 if n <= W else -(-(n - W) // 160) * 160
    length = n - a0
    return a0, length, a0 // 160, 0 if length < 960 else (length - 960) // 160 + 1


def entry(n0, pushed, hop, W, ring_len, origin=0, stream=0):
    """The table entry of one stream's push in closed form, in the order of km_koemorph_audio_schedule's out[10]."""
    n = n0 + pushed
    first, rows = n0 // hop, n // hop - n0 // hop
    if rows < 1:
        return [first, rows, 0, 0, 0, 0, n, -1, 0, 0]
    a0, length, m, nf = window(n, W)
    slot = [stream, (origin + a0) % ring_len, nf] if nf > 0 else [-1, 0, 0]
    return [first, rows, a0, length, nf, m, n] + slot


class BruteStream:
    """The law by walking samples: the life's samples are numbered 0, 1, ..., and a ring image of ring_len slots holds (life, number)."""

    def __init__(self, hop, W, ring_len):
        self.hop, self.W, self.ring_len = hop, W, ring_len
        self.ring = [None] * ring_len
        self.wpos = 0
        self.n = 0
        self.origin = 0
        self.life = 0

    def reset(self):
        self.n = 0
        self.life += 1
        self.origin = self.wpos                                # the ring's write position stays

    def push(self, count):
        """-> (first new frame, new frames, a0, len, nf, m, ring index of a0 or None)."""
        before = sum(1 for k in range(self.n // self.hop + 2) if (k + 1) * self.hop <= self.n)
        for _ in range(count):
            self.ring[self.wpos] = (self.life, self.n)
            self.wpos = (self.wpos + 1) % self.ring_len
            self.n += 1
        after = sum(1 for k in range(self.n // self.hop + 2) if (k + 1) * self.hop <= self.n)
        if after == before:
            return before, 0, 0, 0, 0, 0, None
        a0 = 0
        while a0 < self.n - self.W:                             # the smallest multiple of 160 that is >= n - W
            a0 += 160
        length = self.n - a0
        nf = sum(1 for t in range(length // 160 + 1) if 160 * t + 960 <= length)
        start = self.ring.index((self.life, a0)) if nf else None
        if nf:                                                  # the window lies in the ring, in order, from `start` on
            got = [self.ring[(start + i) % self.ring_len] for i in range(length)]
            assert got == [(self.life, i) for i in range(a0, self.n)]
        return before, after - before, a0, length, nf, a0 // 160, start

    def frame_samples(self, k):
        """Ring indices of the 512 samples of mel frame k, reflected at the stream's start."""
        return [(self.origin + abs(k * self.hop - 256 + i)) % self.ring_len for i in range(512)]


# ---- the shifted frame grid ----------------------------------------------------------------------------------------------
def grid(nf, ks, hop, m):
    """Per row k of ``ks``: (frame j, weight w float64, exact) -- exact where the row IS frame j."""
    p = (np.asarray(ks, np.int64) * hop).astype(np.float64) / 160.0
    fl = np.floor(p)
    j = fl.astype(np.int64) - m
    w = p - fl
    low, last = j < 0, j >= nf - 1
    j = np.where(low, 0, np.where(last, nf - 1, j))
    w = np.where(low | last, 0.0, w)
    return j, w, w == 0.0


def resample_columns(lld, ks, hop, m, nz):
    """tests/lld_cases.resample_columns on the shifted grid p = k * hop / 160 - m: (rows, a, b, blended)."""
    nf = len(lld)
    j, w, exact = grid(nf, ks, hop, m)
    a = lld[j]
    b = lld[np.minimum(j + 1, nf - 1)]
    w32 = w.astype(np.float32).astype(np.float64)[:, None]
    lin = a + w32 * (b - a)
    nearer = np.where((w <= 0.5)[:, None], a, b)
    blend = ~exact[:, None] & (~nz[None, :] | ((a != 0) & (b != 0)))
    rows = np.where(exact[:, None], a, np.where(blend, lin, nearer))
    return rows, a, b, blend


# ---- the plan ------------------------------------------------------------------------------------------------------------
def expected_plan(N, fps, seconds, max_samples):
    hop, W = hop_of(fps), window_samples(seconds)
    max_nf = (W - 960) // 160 + 1
    ring_len = W + max_samples
    return dict(supported=1, hop=hop, max_rows=max_samples // hop + 1, ring_len=ring_len, window_samples=W, window_frames=max_nf, launches=7,
                device_bytes=N * (4 * ring_len + 8 + 4 + ENTRY + SLOT + 4 + 4 * max_nf * REC))


# ---- schedules -----------------------------------------------------------------------------------------------------------
def chunks(total, M):
    """Push sizes that deliver ``total`` samples M at a time."""
    return [M] * (total // M) + ([total % M] if total % M else [])


def ragged_schedule(total, M, N=3):
    """[(counts, reset mask or None)] until stream 0 holds ``total`` samples: stream 0 takes every chunk whole, stream 1 joins at
    the fifth push, stream 2's counts walk 0 .. M in steps of M // 7 + 1."""
    steps, have, k = [], 0, 0
    while have < total:
        c0 = min(M, total - have)
        walk = (k * (M // 7 + 1)) % (M + 1)
        steps.append(([c0, c0 if k >= 4 else 0, walk][:N], None))
        have += c0
        k += 1
    return steps
