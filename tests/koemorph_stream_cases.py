"""Shared by tests/test_koemorph_stream_host.py and tests/test_gpu_koemorph_streams.py: the law of km_koemorph_stream_step restated,
a brute force of it, a restatement of km_koemorph_stream_plan and the schedule the GPU tests walk.

THE LAW.  Stream s of an engine with context T has a frame counter c_s, 0 after creation and after a reset of that stream.  A step
that gives stream s n_s new rows (0 <= n_s <= max_rows) renders n_s frames for it, in order.  Frame i = c_s + j (counted since the
stream's last reset) is ``KoeMorphModel.forward`` on that stream's rows i - T_i + 1 .. i, T_i = min(i + 1, T): a dense (1, T_i, .)
batch, no audio_mask, prev_blendshapes = the stream's previous rendered frame (frame 0 has none and runs unconditioned), the stream's
own smoother state (zeros after a reset; forward's rules for batch 1), updated by every frame.  Short windows are shorter windows,
never padded ones.  Streams share nothing; a stream with n_s = 0 keeps its ring, counter, previous frame and state, and its rows of
every output are not written.  The ring holds T - 1 + max_rows rows; row i of a life sits at position i mod that."""
import rollout_cases as rc

NB = 52
CHAIN_LDS_BYTES = 4 * ((2 * 52 * 264 + 32 * 264 + (2 * 64 * 8 + 2 * 64) + 64) + 64 + (16 * 52 + 4))   # decode images + prev + state


def step_windows(c, n, T, cap):
    """The table entries of one stream's step: [(frame slot j, T_i, ring position of the window's first row)] for j < n."""
    out = []
    for j in range(n):
        i = c + j
        ti = min(i + 1, T)
        out.append((j, ti, (i - ti + 1) % cap))
    return out


class BruteStreams:
    """The law by walking rows: every stream keeps the list of rows of its current life and a ring image of cap slots."""

    def __init__(self, N, T, R):
        self.N, self.T, self.R, self.cap = N, T, R, T - 1 + R
        self.life = [[] for _ in range(N)]                  # row ids of the current life
        self.ring = [[None] * self.cap for _ in range(N)]   # slot -> row id
        self.wpos = [0] * N

    def reset(self, mask):
        for s in range(self.N):
            if mask[s]:
                self.life[s] = []
                self.wpos[s] = 0                            # (the engine writes row i of a life at i mod cap)

    def step(self, counts, row_ids):
        """row_ids[s]: the ids of the rows stream s brings.  -> per stream [(j, the window's row ids as read from the ring)]."""
        res = []
        for s in range(self.N):
            n = max(0, min(counts[s], self.R))
            for j in range(n):                              # the engine appends all n rows first ...
                self.ring[s][self.wpos[s]] = row_ids[s][j]
                self.wpos[s] = (self.wpos[s] + 1) % self.cap
            before = len(self.life[s])
            self.life[s] += list(row_ids[s][:n])
            frames = []
            for j in range(n):                              # ... then renders frame by frame
                i = before + j
                want = [r for k, r in enumerate(self.life[s]) if k <= i and i - k < self.T]
                ti = len(want)
                pos0 = (i - ti + 1) % self.cap
                got = [self.ring[s][(pos0 + t) % self.cap] for t in range(ti)]
                frames.append((j, want, got))
            res.append(frames)
        return res


def state_floats(cfg):
    if not cfg.use_temporal_smoothing:
        return 0
    return NB if cfg.smoothing_method == "exponential" else 5 * NB + 1


def supported(cfg, T, no_fuse=False):
    return rc.fused_width(cfg) and not no_fuse and 1 <= T <= rc.FUSED_TMAX


def expected_plan(cfg, N, T, R, no_fuse=False):
    if not supported(cfg, T, no_fuse):
        return dict(supported=0, ring_rows=0, launches=0, device_floats=0, chain_lds_bytes=0, state_floats=0)
    cap = T - 1 + R
    sf = state_floats(cfg)
    floats = (N * cap * (cfg.mel_dim + cfg.emotion_dim) + 2 * N + N + N * NB + N * sf + 4 * N * R + 2 * N * R * T * 256)
    return dict(supported=1, ring_rows=cap, launches=4, device_floats=floats, chain_lds_bytes=CHAIN_LDS_BYTES, state_floats=sf)


def schedule(T, R, N=4):
    """The GPU test's 2 T + 3 steps (numbered from 1) for four streams: [(counts, reset mask or None)].  Stream 0 takes every row,
    stream 1 joins at step 5, stream 2 alternates its count through 0 .. R, stream 3 is reset ahead of step T + 1."""
    steps = []
    for k in range(1, 2 * T + 4):
        counts = [R, R if k >= 5 else 0, (k - 1) % (R + 1), R][:N]
        mask = [s == 3 for s in range(N)] if k == T + 1 else None
        steps.append((counts, mask))
    return steps


def mixed_steps(T, R):
    """Steps of ``schedule`` that hold a stream with T_i <= 16, one with T_i > 16 and one with count 0, all at once."""
    c = [0] * 4
    hits = []
    for k, (counts, mask) in enumerate(schedule(T, R)):
        if mask:
            c = [0 if m else v for v, m in zip(c, mask)]
        tis = [ti for s in range(4) for _, ti, _ in step_windows(c[s], counts[s], T, T - 1 + R)]
        if any(t <= 16 for t in tis) and any(t > 16 for t in tis) and any(n == 0 for n in counts):
            hits.append(k)
        c = [v + n for v, n in zip(c, counts)]
    return hits
