"""Shared by tests/test_lld_host.py and tests/test_gpu_llds.py: the float64 restatement of the eGeMAPS low-level descriptors per
frame (km_egemaps_llds, koemorph_amd/csrc/km_egemaps_lld.hip) and of their frame grid.

The descriptors are the smoothed contours oracle.egemaps.functionals_from_llds builds before it reduces them (its lines 529-545),
kept at full length: ``reference`` restates those lines with oracle.egemaps.sma3 itself.  ``reference_fast`` is the same arithmetic
without the loop over frames -- a three-frame sum in frame order divided by the count, which is what ``w.mean()`` of at most three
float64 numbers is -- for the windows of thousands of frames; tests/test_lld_host.py holds it EQUAL to ``reference``, bit for bit,
and the GPU tests use ``reference`` itself up to 257 frames.
"""
import functools

import numpy as np

import egemaps_cases as ec
from oracle import egemaps as eg

W_EGEMAPS, W_GEMAPS = 25, 18
FIRST_NZ = 10                                # columns 0-9 plain smoothing, 10 the semitone, 11-24 masked non-zero smoothing
SEMITONE = 10
PLAIN = ("loudness", "alphaRatio", "hammarbergIndex", "slope0-500", "slope500-1500", "spectralFlux")
U = 2.0 ** -24                               # unit roundoff of float32

# Column 10 goes through log2f.  Its worst error on the MI355X over every window of functional_windows(nf), nf in RECORD_NF, against
# the float64 restatement and relative to the window's largest |semitone| is SEMITONE_WORST (tests/test_gpu_llds.py prints it;
# profiles/llds_pin.txt has the run); the tolerance is four times that, the rule of egemaps_cases.TOL, and never above TOL_CAP.
TOL_CAP = ec.TOL_CAP
SEMITONE_WORST = 1.347e-7
SEMITONE_TOL = min(4 * SEMITONE_WORST, TOL_CAP)

RECORD_NF = (1, 2, 3, 255, 256, 257, 2048, 2049, 6548)
GRID_FPS = (100, 30, 60, 29.97, 120)


def nz_fields(d):
    """The fourteen voiced-only descriptors in column order (functionals_from_llds :540-542)."""
    nzs = [d["jitterLocal"], d["shimmerLocaldB"], d["HNRdBACF"], d["H1-H2"], d["H1-A3"]]
    for i in range(3):
        nzs += [d["F"][:, i], d["BW"][:, i], d["Famp"][:, i]]
    return nzs


def _columns(d, sma3):
    f0 = sma3(d["f0"], True)
    voiced = f0 > 0
    cols = [sma3(d[k], False) for k in PLAIN] + [sma3(d["mfcc"][:, i], False) for i in range(4)]
    cols.append(np.where(voiced, 12.0 * np.log2(np.maximum(f0, 1e-9) / 27.5), 0.0))
    cols += [sma3(np.where(voiced, v, 0.0), True) for v in nz_fields(d)]
    return np.stack(cols, axis=1), voiced


def reference(rec):
    """(nf, 36) records -> ((nf, 25) float64 descriptors, voiced mask), with oracle.egemaps.sma3."""
    return _columns(ec.records_to_llds(rec), eg.sma3)


def _sma3_fast(v, nz):
    v = np.asarray(v, np.float64)
    n = len(v)
    pad = np.concatenate([[0.0], v, [0.0]])
    has = np.concatenate([[False], np.ones(n, bool), [False]])
    use = [has[i:i + n] & ((pad[i:i + n] != 0) if nz else True) for i in range(3)]            # frames t - 1, t, t + 1
    acc = np.zeros(n)
    for i in range(3):                                                                        # in frame order, as w.mean() adds them
        acc = acc + np.where(use[i], pad[i:i + n], 0.0)
    cnt = use[0].astype(int) + use[1].astype(int) + use[2].astype(int)
    out = np.where(cnt > 0, acc / np.maximum(cnt, 1), 0.0)
    return np.where(v != 0, out, 0.0) if nz else out


def reference_fast(rec):
    """``reference`` without the loop over frames; equal bits (tests/test_lld_host.py)."""
    return _columns(ec.records_to_llds(rec), _sma3_fast)


@functools.lru_cache(maxsize=None)
def record_batch(nf):
    """(names, records (B, nf, 36), float64 descriptors (B, nf, 25), voiced (B, nf)) of functional_windows(nf); computed once."""
    wins = ec.functional_windows(nf)
    rec = np.stack([w for _, w in wins])
    ref = [(reference if nf <= 257 else reference_fast)(w) for w in rec]
    out = ([n for n, _ in wins], rec, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]))
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ---- the frame grid ------------------------------------------------------------------------------------------------------
def samples_for(nf):
    """The shortest window of nf frames."""
    return 960 + 160 * (nf - 1)


def output_frames(L, fps):
    """Rows of the grid: int(L / 16000 * fps), float64 in that order; fps None is the native grid."""
    return eg.frame_count(L) if fps is None else int(L / 16000 * fps)


def grid(nf, T, fps):
    """Per row k < T: (frame j, weight w float64, exact) -- exact where the row IS frame j (w == 0, or j the last frame)."""
    p = np.arange(T, dtype=np.float64) * 100.0 / fps
    j = np.floor(p)
    w = p - j
    last = j >= nf - 1
    j = np.where(last, nf - 1, j).astype(np.int64)
    w = np.where(last, 0.0, w)
    return j, w, w == 0.0


def resample(lld, T, fps):
    """The grid law on float64 (or float32) descriptors (nf, W) whose first FIRST_NZ columns are the plain ones when W is 25 -- pass
    ``nz`` columns explicitly otherwise.  Returns (rows (T, W), a (T, W), b (T, W), blended (T, W) bool)."""
    return resample_columns(lld, T, fps, np.arange(lld.shape[1]) >= FIRST_NZ)


def resample_columns(lld, T, fps, nz):
    nf = len(lld)
    j, w, exact = grid(nf, T, fps)
    a = lld[j]
    b = lld[np.minimum(j + 1, nf - 1)]
    w32 = w.astype(np.float32).astype(np.float64)[:, None]
    lin = a + w32 * (b - a)
    nearer = np.where((w <= 0.5)[:, None], a, b)
    blend = ~exact[:, None] & (~nz[None, :] | ((a != 0) & (b != 0)))
    rows = np.where(exact[:, None], a, np.where(blend, lin, nearer))
    return rows, a, b, blend
