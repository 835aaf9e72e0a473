"""Shared by tests/test_egemaps_stages_host.py and tests/test_gpu_egemaps_stages.py: per-frame records written by hand for the
two eGeMAPS kernels that are pure functions of the record array (pitch track, functionals), their float64 references from
oracle/egemaps.py, and the scale every error is taken relative to.

Records for the functionals are random walks at realistic magnitudes on a FIXED GRID per field (a power-of-two step, at most
12 significant bits): a three-frame sum is then exact in float32, equal neighbourhoods smooth to equal values in float32 and
in float64, and unequal ones differ by far more than float32 rounding -- so every discrete decision (voiced mask, turning
points, loudness peaks, sort order) is the same on both sides and no output has to be left out of the comparison."""
import functools

import numpy as np

from oracle import egemaps as eg

REC = 36
R = dict(loud=0, alpha=1, hamm=2, sl0=3, sl1=4, flux=5, mfcc=6, rms=10, cf=11, cs=14, voi=17, F=18, BW=21, f0=24, jit=25, shim=26,
         hnr=27, h1h2=28, h1a3=29, famp=30)            # the Rec enum of koemorph_amd/csrc/km_egemaps.hip; columns 33-35 are unused

# Tolerances of tests/test_gpu_egemaps_stages.py, error / scale per class (CLASS below): four times the worst error observed on
# the MI355X over the crafted set (that module's docstring has the figures), none above TOL_CAP of its scale -- an index or
# divisor slip moves a value by about scale / nf, at least 5e-4 at nf = 2048.  "slope" sits AT the cap: four times its worst
# (4.71e-5) would be 1.9e-4.  "count" is not measured: small integers through one division, relative 1e-6.
TOL_CAP = 1e-4
TOL = {"stat": 6.2e-7, "slope": TOL_CAP, "sn": 1.9e-7, "db": 9.2e-6, "count": 1e-6}
# Largest cost by which a GPU track may exceed the optimum.  Observed: 0 on every window (the float32 recursion finds a track
# of exactly the optimal float64 cost), and four times 0 would ask for more than float32 can promise: two tracks whose costs
# differ by less than the spacing of float32 numbers at C* look alike to the kernel.  So the bound is four times that spacing
# at the largest C* of the set (2^-14 for 512 <= C* < 1024; the host test holds every C* below 1000) -- 500 times below the
# cap of a tenth of the smallest transition weight (w_vuv = 1.25), which is what a wrong weight, a skipped penalty or a
# misread back pointer costs at the least.
TRACK_BOUND_CAP = 0.125
TRACK_BOUND = 4 * 2.0 ** -14

FUNC_NF = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 300, 1024, 2048)
TRACK_NF = (1, 2, 3, 255, 256, 257, 2048)


def speechlike(seed, seconds=2.0):
    """The voiced - silence - noise - voiced signal of tests/test_gpu_egemaps.py."""
    from koemorph_amd import synth
    a = synth.make_vowel(seed, 130.0, seconds * 0.35, vibrato=0.03)
    b = np.zeros(int(seconds * 0.1 * 16000), np.float32)
    c = (0.2 * synth.normal(seed + 2, (int(seconds * 0.2 * 16000),))).astype(np.float32)
    d = 0.6 * synth.make_vowel(seed + 3, 190.0, seconds * 0.35, formants=((500.0, 80.0), (1500.0, 120.0), (2500.0, 150.0)), vibrato=0.02)
    return np.concatenate([a, b, c, d]).astype(np.float32)


# ---- records <-> the oracle's descriptor dict ---------------------------------------------------------------------------
_SCALAR = (("loudness", "loud"), ("alphaRatio", "alpha"), ("hammarbergIndex", "hamm"), ("slope0-500", "sl0"), ("slope500-1500", "sl1"),
           ("spectralFlux", "flux"), ("rms", "rms"), ("voicing", "voi"), ("f0", "f0"), ("jitterLocal", "jit"), ("shimmerLocaldB", "shim"),
           ("HNRdBACF", "hnr"), ("H1-H2", "h1h2"), ("H1-A3", "h1a3"))
_VECTOR = (("mfcc", "mfcc", 4), ("cand_f", "cf", 3), ("cand_s", "cs", 3), ("F", "F", 3), ("BW", "BW", 3), ("Famp", "famp", 3))


def records_to_llds(rec):
    """(nf, 36) records -> the dict of oracle.egemaps.llds(), float64 (exact: every float32 is a float64)."""
    rec = np.asarray(rec)
    assert rec.ndim == 2 and rec.shape[1] == REC, rec.shape
    d = {name: rec[:, R[col]].astype(np.float64) for name, col in _SCALAR}
    d.update({name: rec[:, R[col]:R[col] + n].astype(np.float64) for name, col, n in _VECTOR})
    return d


def llds_to_records(d):
    """The dict of oracle.egemaps.llds() -> (nf, 36) float32 records (rounds; the unused columns are zero)."""
    rec = np.zeros((len(d["f0"]), REC), np.float32)
    for name, col in _SCALAR:
        rec[:, R[col]] = d[name]
    for name, col, n in _VECTOR:
        rec[:, R[col]:R[col] + n] = d[name]
    return rec


# ---- crafted records for the functionals --------------------------------------------------------------------------------
# column -> (offset, amplitude, log2 of the grid step): value = offset + amplitude * w, w a bounded walk in [-1, 1].  Every
# |value| stays below 4096 steps (12 bits), and |offset| >= 1.5 amplitude keeps each mean at least half an amplitude from zero
# (the stddevNorm entries divide by it; MFCC 3 and 4 hover around zero on real speech and get an offset here).
_FIELDS = {
    R["f0"]: (200.0, 140.0, -3), R["loud"]: (1.6, 1.0, -10), R["alpha"]: (-14.0, 9.0, -6), R["hamm"]: (22.0, 14.0, -6),
    R["sl0"]: (0.05, 0.03, -15), R["sl1"]: (-0.025, 0.015, -16), R["flux"]: (0.45, 0.3, -12),
    R["mfcc"]: (24.0, 14.0, -6), R["mfcc"] + 1: (-15.0, 10.0, -6), R["mfcc"] + 2: (12.0, 8.0, -6), R["mfcc"] + 3: (-9.0, 6.0, -6),
    R["rms"]: (0.15, 0.1, -13), R["jit"]: (0.0125, 0.0075, -17), R["shim"]: (0.85, 0.55, -11), R["hnr"]: (10.0, 6.0, -7),
    R["h1h2"]: (5.0, 3.0, -8), R["h1a3"]: (20.0, 8.0, -7),
    R["F"]: (600.0, 300.0, 0), R["F"] + 1: (1500.0, 500.0, 0), R["F"] + 2: (2800.0, 600.0, 0),
    R["BW"]: (120.0, 70.0, -3), R["BW"] + 1: (180.0, 100.0, -3), R["BW"] + 2: (250.0, 140.0, -3),
    R["famp"]: (-12.0, 7.0, -7), R["famp"] + 1: (-18.0, 8.0, -7), R["famp"] + 2: (-24.0, 6.0, -7),
}


def _walk(rng, nf):
    """Random walk plus noise, reflected into [-1, 1]."""
    w = np.cumsum(rng.normal(0.0, 0.12, nf)) + rng.uniform(-1.0, 1.0) + rng.normal(0.0, 0.08, nf)
    return 1.0 - np.abs((w + 1.0) % 4.0 - 2.0)                    # triangle wave: reflect at the walls


def _runs_mask(rng, nf, voiced_share):
    """Alternating voiced / unvoiced runs of 1 to 12 frames; the longer kind has runs up to 12, the other proportionally."""
    if voiced_share <= 0.0:
        return np.zeros(nf, bool)
    if voiced_share >= 1.0:
        return np.ones(nf, bool)
    hi_v = 12 if voiced_share >= 0.5 else max(1, int(round(12 * voiced_share / (1.0 - voiced_share))))
    hi_u = 12 if voiced_share <= 0.5 else max(1, int(round(12 * (1.0 - voiced_share) / voiced_share)))
    mask = np.zeros(nf, bool)
    t, on = 0, bool(rng.randint(2))
    while t < nf:
        n = rng.randint(1, (hi_v if on else hi_u) + 1)
        mask[t:t + n] = on
        t, on = t + n, not on
    return mask


def craft_records(seed, nf, voiced_share, mask=None):
    """One window of (nf, 36) float32 records on the grid described in the module docstring.  Voiced frames (F0 != 0) come in
    runs of 1 to 12 frames filling about `voiced_share` of the window, or exactly where `mask` says.  About 10 % of the voiced
    frames carry zero jitter and shimmer, and about 10 % a zero formant (frequency, bandwidth and amplitude), as the frame
    kernels write for invalid frames.  The voiced-only descriptors are deliberately NOT zeroed in unvoiced frames: masking
    them there is the functional kernel's job."""
    rng = np.random.RandomState(seed)
    voiced = _runs_mask(rng, nf, voiced_share) if mask is None else np.asarray(mask, bool)
    assert voiced.shape == (nf,)
    rec = np.zeros((nf, REC), np.float64)
    for col, (off, amp, lg) in _FIELDS.items():
        step = 2.0 ** lg
        rec[:, col] = np.round((off + amp * _walk(rng, nf)) / step) * step
        assert np.abs(rec[:, col]).max() < 4096 * step
    rec[~voiced, R["f0"]] = 0.0
    bad = voiced & (rng.uniform(size=nf) < 0.1)
    rec[bad, R["jit"]] = 0.0; rec[bad, R["shim"]] = 0.0
    for i in range(3):
        bad = voiced & (rng.uniform(size=nf) < 0.1)
        for c in ("F", "BW", "famp"):
            rec[bad, R[c] + i] = 0.0
    rec[:, R["cf"]] = rec[:, R["f0"]]; rec[:, R["cs"]] = np.where(voiced, 0.9375, 0.0); rec[:, R["voi"]] = np.where(voiced, 0.875, 0.125)
    out = rec.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), rec)            # on the grid: nothing was rounded
    return out


def _with_count(rng, mask, count):
    """Flip random frames of `mask` until exactly `count` are voiced."""
    mask = mask.copy()
    while mask.sum() != count:
        pool = np.flatnonzero(mask if mask.sum() > count else ~mask)
        mask[pool[rng.randint(len(pool))]] = mask.sum() < count
    return mask


def power_of_two_count(nf):
    """The largest power of two below nf (so that the count plus one still fits), 1 for nf <= 2."""
    p = 1
    while 2 * p < nf:
        p *= 2
    return p


def functional_windows(nf):
    """[(name, (nf, 36) records)]: the voicing patterns the functional kernel has to survive at this frame count."""
    seed = 1000 * nf
    rng = np.random.RandomState(seed + 99)
    first = np.zeros(nf, bool); first[0] = True
    last = np.zeros(nf, bool); last[-1] = True
    p = power_of_two_count(nf)
    wins = [("mixed_half", craft_records(seed + 1, nf, 0.5)), ("mixed_mostly_voiced", craft_records(seed + 2, nf, 0.8)),
            ("mixed_mostly_unvoiced", craft_records(seed + 3, nf, 0.25)),
            ("none_voiced", craft_records(seed + 4, nf, 0.0)), ("all_voiced", craft_records(seed + 5, nf, 1.0)),
            ("only_first", craft_records(seed + 6, nf, 0.0, first)), ("only_last", craft_records(seed + 7, nf, 0.0, last)),
            ("count_pow2", craft_records(seed + 8, nf, 0.0, _with_count(rng, _runs_mask(rng, nf, 0.5), p)))]
    if p + 1 <= nf:
        wins.append(("count_pow2_plus1", craft_records(seed + 9, nf, 0.0, _with_count(rng, _runs_mask(rng, nf, 0.5), p + 1))))
    return wins


# ---- error classes and scales of the 88 outputs ------------------------------------------------------------------------
# "stat"  means, percentiles, percentile range      / max |contour| over the selected frames
# "slope" mean and std of the part slopes            / max |part slope| of that direction
# "sn"    stddevNorm                                 / (max |v| / |mean|) (1 + sn): the oracle's own conditioning of the quotient
# "db"    equivalent sound level                     absolute, in dB
# "count" peak / segment rates and segment lengths   relative (small integers through one division)
_TEN = ["stat", "sn", "stat", "stat", "stat", "stat", "slope", "slope", "slope", "slope"]
CLASS = _TEN + _TEN + ["stat", "sn"] * 28 + ["stat"] * 5 + ["count"] * 6 + ["db"]
assert len(CLASS) == 88
SLOPE_IDX = (6, 7, 8, 9, 16, 17, 18, 19)
PEAK_IDX = 81


def reference_and_scales(rec):
    """float64 functionals of one window of records and the scale of every output's error (see CLASS)."""
    contours = {}
    want = eg.functionals_from_llds(records_to_llds(rec), dtype=np.float64, contours=contours)
    scale = np.ones(88)
    amax = lambda v: float(np.abs(v).max()) if len(v) else 0.0
    for base, v in contours.items():
        top = amax(v)
        if base in (0, 10):
            idx = (base, base + 2, base + 3, base + 4, base + 5)
            rise, fall = eg.part_slopes(v)
            scale[base + 6] = scale[base + 7] = amax(np.asarray(rise)) or 1.0
            scale[base + 8] = scale[base + 9] = amax(np.asarray(fall)) or 1.0
        else:
            idx = (base,)
        for i in idx:
            scale[i] = top or 1.0
        if base + 1 < 88 and CLASS[base + 1] == "sn":
            m, sn = want[base], want[base + 1]
            scale[base + 1] = (top / abs(m)) * (1.0 + sn) if m != 0 else 1.0
    for i in range(88):
        if CLASS[i] == "count":
            scale[i] = abs(want[i]) or 1.0
    return want, scale


@functools.lru_cache(maxsize=None)
def functional_batch(nf):
    """(names, records (B, nf, 36), float64 reference (B, 88), scales (B, 88)) of functional_windows(nf); computed once."""
    wins = functional_windows(nf)
    rec = np.stack([w for _, w in wins])
    ref = [reference_and_scales(w) for w in rec]
    out = ([n for n, _ in wins], rec, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def class_errors(got, want, scale, skip=()):
    """{class: (worst |got - want| / scale, index of the worst output)} over one window's 88 outputs."""
    err = np.abs(np.asarray(got, np.float64) - want) / scale
    worst = {}
    for i in range(88):
        if i not in skip and err[i] >= worst.get(CLASS[i], (-1.0, 0))[0]:
            worst[CLASS[i]] = (float(err[i]), i)
    return worst


# ---- crafted candidates for the pitch track ----------------------------------------------------------------------------
def _log_walk(rng, nf, lo, hi):
    """Slowly moving track in log2 Hz: about a hundredth of an octave per frame, reflected into [lo, hi] Hz."""
    a, b = np.log2(lo), np.log2(hi)
    w = rng.uniform(a, b) + np.cumsum(rng.normal(0.0, 0.01, nf))
    return 2.0 ** (b - np.abs((w - a) % (2 * (b - a)) - (b - a)))


def _stretches(rng, nf, share, longest=3):
    """Boolean mask: stretches of 1 to `longest` frames covering roughly `share` of the window."""
    m = np.zeros(nf, bool)
    t = rng.randint(0, 8)
    while t < nf:
        n = rng.randint(1, longest + 1)
        m[t:t + n] = True
        t += n + rng.randint(1, max(2, int((longest + 1) / share)))
    return m


def craft_candidates(seed, nf, kind="mixed"):
    """One window of (nf, 36) records for the pitch-track kernel: candidate frequencies (distinct within a frame, 60 to
    500 Hz) and strengths (0.5 to 1, on a 1/256 grid), voicing measure (on a 1/64 grid, so never within rounding of the
    0.55 cutoff) and RMS.  An intended track with strengths near 0.9 moves slowly; its octave-error decoy and, in every
    second window, a second track 0.4 to 0.65 octaves away fill the other slots, in random slot order.  Stretches of 1 to
    3 frames lose the intended candidate, lose all candidates, make the decoy the strongest, or switch the frame's
    voiced-ok flag (by the voicing measure or by an RMS below the floor), so that both the voiced-to-voiced cost and the
    voicing-switch cost decide parts of the track.
    kind: "mixed"; "all_ok" (every frame voiced-ok, three candidates); "none_ok" (no frame voiced-ok); "no_cand" (no
    candidate anywhere)."""
    rng = np.random.RandomState(seed)
    rec = np.zeros((nf, REC), np.float64)
    main = _log_walk(rng, nf, 110.0, 240.0)
    decoy = np.where(rng.uniform(size=nf) < 0.5, 2.0 * main, 0.5 * main)
    decoy = np.where(decoy > 480.0, 0.5 * main, np.where(decoy < 62.0, 2.0 * main, decoy))
    other = 2.0 ** (np.log2(main) + rng.choice([-1.0, 1.0]) * rng.uniform(0.45, 0.6) + 0.02 * np.sin(np.arange(nf) / 17.0))
    two = seed % 2 == 0 or kind == "all_ok"
    q = lambda v: np.round(np.clip(v, 0.5, 1.0) * 256.0) / 256.0
    s_main = q(0.9 + rng.uniform(-0.02, 0.02, nf))
    s_decoy = q(rng.uniform(0.5, 0.75, nf))
    s_other = q(rng.uniform(0.5, 0.75, nf))
    ok = np.ones(nf, bool)
    has = np.ones((nf, 3), bool)                                   # main, decoy, other
    has[:, 2] = two
    dens = min(1.0, 256.0 / nf)                                    # events per frame thin out in long windows: C* stays in the hundreds
    if kind in ("mixed", "all_ok"):
        s_decoy = np.where(_stretches(rng, nf, 0.08 * dens), q(rng.uniform(0.99, 1.0, nf)), s_decoy)
    if kind == "mixed":
        has[_stretches(rng, nf, 0.08 * dens), 0] = False
        has[_stretches(rng, nf, 0.05 * dens), 1] = False
        has[_stretches(rng, nf, 0.05 * dens)] = False
        ok &= ~_stretches(rng, nf, 0.12 * dens)
        ok &= ~_stretches(rng, nf, 0.3 * dens, 5)                  # ... and not-ok runs of up to 5 frames
    elif kind == "none_ok":
        ok[:] = False
    elif kind == "no_cand":
        has[:] = False
        ok = _stretches(rng, nf, 0.5 * dens, 12)
    low_rms = ~ok & (rng.uniform(size=nf) < 0.5)                   # not voiced-ok by the RMS floor, voicing measure high
    rec[:, R["voi"]] = np.where(ok | low_rms, np.round(rng.uniform(0.6, 0.95, nf) * 64) / 64, np.round(rng.uniform(0.1, 0.5, nf) * 64) / 64)
    rec[:, R["rms"]] = np.where(low_rms, 0.0005, np.round(rng.uniform(0.01, 0.3, nf) * 1024) / 1024)
    f = np.stack([main, decoy, other], 1).astype(np.float32).astype(np.float64)
    s = np.stack([s_main, s_decoy, s_other], 1)
    for t in range(nf):
        order = rng.permutation(3)
        for slot, c in enumerate(order):
            if has[t, c]:
                rec[t, R["cf"] + slot] = f[t, c]; rec[t, R["cs"] + slot] = s[t, c]
        live = rec[t, R["cf"]:R["cf"] + 3]
        live = live[live > 0]
        assert len(set(live)) == len(live) and (len(live) == 0 or (live.min() >= 60.0 and live.max() <= 500.0))
    rec[:, R["f0"]] = -1.0                                         # the kernel has to overwrite every frame's F0
    return rec.astype(np.float32)


def track_windows(nf):
    seed = 2000 * nf
    return [("mixed_one_track", craft_candidates(seed + 1, nf)), ("mixed_two_tracks", craft_candidates(seed + 2, nf)),
            ("mixed_one_track_b", craft_candidates(seed + 3, nf)), ("mixed_two_tracks_b", craft_candidates(seed + 4, nf)),
            ("all_ok", craft_candidates(seed + 5, nf, "all_ok")), ("none_ok", craft_candidates(seed + 6, nf, "none_ok")),
            ("no_cand", craft_candidates(seed + 7, nf, "no_cand"))]


def track_inputs(rec):
    """(cf, cs, vo, rms) of one window of records, float64, as oracle.egemaps.viterbi_f0 takes them."""
    d = records_to_llds(rec)
    return d["cand_f"], d["cand_s"], d["voicing"], d["rms"]


def track_states(rec, f0):
    """Per-frame state of a track on these records: the slot whose candidate frequency equals the track value bit for bit,
    3 for an unvoiced frame (value 0), -1 for a value that is neither."""
    rec = np.asarray(rec, np.float32); f0 = np.asarray(f0, np.float32)
    st = np.full(len(f0), -1)
    for c in (2, 1, 0):
        st[(rec[:, R["cf"] + c] == f0) & (f0 > 0)] = c
    st[f0 == 0] = 3
    return st


@functools.lru_cache(maxsize=None)
def track_batch(nf):
    """(names, records (B, nf, 36), [C*], [through-cost (nf, 4)], [oracle states (nf)]) of track_windows(nf); computed once."""
    wins = track_windows(nf)
    rec = np.stack([w for _, w in wins])
    rec.setflags(write=False)
    cstar, through, states = [], [], []
    for w in rec:
        args = track_inputs(w)
        c, th = eg.viterbi_tables(*args)
        cstar.append(c); through.append(th); states.append(track_states(w, eg.viterbi_f0(*args)))
    return [n for n, _ in wins], rec, cstar, through, states


def runner_up_gap(through, states, cstar):
    """Per frame: the cheapest track through any OTHER state than the oracle's, minus C* (inf where there is no other state)."""
    th = through.copy()
    th[np.arange(len(states)), states] = np.inf
    return th.min(axis=1) - cstar
