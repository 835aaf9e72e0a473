"""Shared by tests/test_egemaps_long_host.py and tests/test_gpu_egemaps_long.py: the frame counts, tolerances and track bound of
the long tier of the per-window eGeMAPS kernels, windows beyond 2048 frames (koemorph_amd/csrc/km_egemaps_window.hip).  The records,
references and error classes are those of tests/egemaps_cases.py, unchanged; only the frame counts are new."""
import numpy as np

import egemaps_cases as ec

MAXF_SHORT, MAXF_LONG = 2048, 6548                 # ShortTier::MAXF; LongTier::MAXF = (2**20 - 960) // 160 + 1
TRACK_CHUNK = 4096                                 # LongTier::CHUNK: frames of pitch-track inputs staged in LDS at a time (the host test reads the header)
SORT_DOUBLES = 4096                                # the functionals' sort is padded to 4096 up to here and to 8192 beyond

# equal bits with the short tier: one frame, fewer than a wave, one past the 256-thread stride, their limit
EQUAL_NF = (1, 3, 257, 2048)
# against float64: one past the old limit; one below, at and one above the sort's doubling and every chunk boundary of the track
# kernel's staging (both 4096: the only boundary below the cap); the cap
LONG_NF = (2049, TRACK_CHUNK - 1, TRACK_CHUNK, TRACK_CHUNK + 1, MAXF_LONG)
assert SORT_DOUBLES in LONG_NF and SORT_DOUBLES + 1 in LONG_NF and all(MAXF_SHORT < n <= MAXF_LONG for n in LONG_NF)
assert [c for c in range(TRACK_CHUNK, MAXF_LONG, TRACK_CHUNK)] == [TRACK_CHUNK]
BATCH_CHECK_NF = TRACK_CHUNK + 1                   # batched results against B = 1 calls, records read only, guards around `out`


def tol(cls, nf):
    """ec.TOL is four times the worst error measured at up to 2048 frames, and the error of a fixed-order float32 sum grows at most
    linearly in its length: the tolerance of a class at nf frames is ec.TOL x nf / 2048, never above ec.TOL_CAP."""
    return min(ec.TOL[cls] * nf / MAXF_SHORT, ec.TOL_CAP)


def track_bound(cstars):
    """The rule behind ec.TRACK_BOUND for another set: four float32 spacings at the set's largest C* (4 x 2^-12 at 6548 frames,
    where C* reaches 2103), never above ec.TRACK_BOUND_CAP."""
    return min(4.0 * float(np.spacing(np.float32(max(cstars)))), ec.TRACK_BOUND_CAP)
