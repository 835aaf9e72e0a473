"""Global-norm clipping + AdamW on a flat bucket (sumsq_partial_kernel + adamw_kernel, koemorph_amd/csrc/km_train.hip) from GIVEN
gradients and moments at a GIVEN step: a float64 oracle, the float32 bound it is held to, a NumPy float32 restatement of the two
kernels (with the mistakes an optimizer kernel can make as named mutations) and the table of cases shared by
tests/test_adamw_host.py and tests/test_gpu_adamw.py.

The oracle restates torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (pinned to them in test_adamw_host.py) on the float32
hyperparameters that cross the C ABI, widened to float64: that is the operation the kernel is given.

Bound, per element, with u = 2^-24 and K = 16 (s = the oracle's clip scale, bc = the bias corrections, denom = the oracle's):
    p:  3 u |p0| + K u (lr / bc1) (|b1 m0| + |(1 - b1) g s|) / denom
    m:  K u (|b1 m0| + |(1 - b1) g s|)
    v:  K u v_ref
3 u |p0|: the rounding of 1 - lr wd, of its product with p0 and of the final subtraction.  |b1 m0| + |(1 - b1) g s| and not
|m_ref| is what float32 can deliver where m0 and g cancel.  K covers the ~12 roundings of the chain, the fixed-order tree sum of
n squares and the transcendental functions of the bias corrections.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
K = 16.0
f32 = np.float32

HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, max_norm=0.05)
MUTATIONS = ("eps_before_div", "eps_in_sqrt", "step_off_by_one", "clip_without_1e-6", "wd_after_update", "alpha_common_counter",
             "powf_correction", "nan_dropped_by_clamp")


def hyper(**kw):
    """The hyperparameters as the float32 values the C ABI carries."""
    h = dict(HP)
    h.update(kw)
    return {k: f32(x) for k, x in h.items()}


def widen(hp):
    return {k: float(f32(x)) for k, x in hp.items()}


def bucket_size(d, T, emotion_dim=256):
    """Floats of the dual-stream trainer's bucket: every tensor starts at a multiple of 4 floats, smoothing_alpha included.
    So every bucket is a multiple of 4 (837 744 at d_model 256 / window 256, 66 160 at 64 / 32: more than the 65 536
    accumulators of the norm): the kernel's element path runs for smoothing_alpha's group and for a misaligned flat_grad only,
    never for a tail, and no block of the partial sums is without an element at a shape the trainers have."""
    from koemorph_amd import synth
    shapes = synth.core_param_shapes(d, T, 3, emotion_dim, 52)
    return sum((int(np.prod(s, dtype=np.int64)) + 3) // 4 * 4 for s in shapes.values()) + 4


N_LEGACY = 419124        # SimplifiedKoeMorphModel (every tensor a multiple of 4 floats)


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def clip_scale(g, max_norm):
    """clip_grad_norm_(error_if_nonfinite=False): max_norm / (norm + 1e-6) clamped to 1, a NaN kept; max_norm <= 0 = off."""
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2)))
        if not max_norm > 0.0:
            return 1.0, norm
        c = max_norm / (norm + 1e-6)
        return (1.0 if c >= 1.0 else c), norm


def oracle_step(p, m, v, g, t, t_alpha, alpha_idx, alpha_live, hp):
    """One step in float64 -> (p, m, v, info).  alpha_idx < 0: no smoothing_alpha.  Not live: the element is left wholly
    untouched (its gradient is None in torch: no decay, no moments, no step); live: it is updated with t_alpha."""
    h = widen(hp)
    p, m, v, g = (np.array(a, np.float64) for a in (p, m, v, g))
    n = p.size
    live = np.ones(n, bool)
    tt = np.full(n, float(t))
    if alpha_idx is not None and alpha_idx >= 0:
        if alpha_live:
            tt[alpha_idx] = float(t_alpha)
        else:
            live[alpha_idx] = False
    with np.errstate(all="ignore"):
        s, norm = clip_scale(g[live], h["max_norm"])
        # 1 - beta ** step on Python floats, as torch evaluates it (in float64 its cancellation is 5e-14 at step 2: nothing
        # against u, but more than the 1e-14 to which the oracle is pinned to torch)
        bc1, bc2 = np.ones(n), np.ones(n)
        for step in set(tt.tolist()):
            bc1[tt == step], bc2[tt == step] = 1.0 - h["b1"] ** step, 1.0 - h["b2"] ** step
        gs = g * s
        pn = p * (1.0 - h["lr"] * h["wd"])
        mn = h["b1"] * m + (1.0 - h["b1"]) * gs
        vn = h["b2"] * v + (1.0 - h["b2"]) * gs * gs
        denom = np.sqrt(vn) / np.sqrt(bc2) + h["eps"]
        pn = pn - h["lr"] / bc1 * mn / denom
    for new, old in ((pn, p), (mn, m), (vn, v)):
        new[~live] = old[~live]
    return pn, mn, vn, dict(scale=s, norm=norm, bc1=bc1, bc2=bc2, denom=denom, live=live)


def bound(p0, m0, g, v_ref, info, hp):
    """(bound_p, bound_m, bound_v) per element; zero where the step must leave the element alone."""
    h = widen(hp)
    p0, m0, g = (np.asarray(a, np.float64) for a in (p0, m0, g))
    with np.errstate(all="ignore"):
        msum = np.abs(h["b1"] * m0) + np.abs((1.0 - h["b1"]) * g * info["scale"])
        bp = 3 * U * np.abs(p0) + K * U * (h["lr"] / info["bc1"]) * msum / info["denom"]
        bm = K * U * msum
        bv = K * U * np.asarray(v_ref, np.float64)
    for b in (bp, bm, bv):
        b[~info["live"]] = 0.0
    return bp, bm, bv


def fraction(got, ref, bnd):
    """Largest |got - ref| / bound over the elements; a NaN must meet a NaN, a zero bound an exact result."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    err, b = np.abs(got[ok] - ref[ok]), bnd[ok]
    if np.any((b == 0) & (err != 0)) or np.any(np.isnan(b)):
        return float("inf")
    nz = b > 0
    return float((err[nz] / b[nz]).max()) if nz.any() else 0.0


def fractions(got, ref, bnds):
    return tuple(fraction(a, r, b) for a, r, b in zip(got, ref, bnds))


# ---- float32 restatement of the two kernels -------------------------------------------------------------------------------------
def sumsq_f32(g):
    """The kernels' order: 256 x 256 strided accumulators, a 256-wide tree per block, a butterfly per wave over the 256
    partials, then (s0 + s1) + (s2 + s3)."""
    g = np.asarray(g, f32)
    rows = -(-g.size // 65536)
    gp = np.zeros(rows * 65536, f32)
    gp[:g.size] = g
    acc = np.zeros(65536, f32)
    with np.errstate(all="ignore"):
        for r in gp.reshape(rows, 65536):
            acc = acc + r * r
        sh = acc.reshape(256, 256).copy()
        s = 128
        while s > 0:
            sh[:, :s] = sh[:, :s] + sh[:, s:2 * s]
            s >>= 1
        w = sh[:, 0].reshape(4, 64).copy()
        lane = np.arange(64)
        o = 32
        while o > 0:
            w = w + w[:, lane ^ o]
            o >>= 1
        return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def _fma(a, b, c):
    """fmaf: the product of two float32 is exact in float64 (the second rounding of the sum changes a result in ~2^-29 of cases)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _correction(b, t, powf):
    if powf:             # 1.0f - powf(b, t): cancels while b^t is close to 1
        return f32(1) - f32(np.power(np.float64(b), np.float64(t)))
    x = f32(t) * f32(np.log(np.float64(b)))          # -expm1f(t * logf(b))
    return f32(-np.expm1(np.float64(x)))


def emulate_f32(p, m, v, g, t, t_alpha, alpha_idx, alpha_live, hp, mutation=None):
    """(p, m, v, gnorm) as the kernels compute them: every operation rounded to float32 in the kernels' order, fused where the
    kernel spells a fused multiply-add, the bias corrections as -expm1f(t logf(beta))."""
    assert mutation is None or mutation in MUTATIONS, mutation
    h = {k: f32(x) for k, x in hp.items()}
    p, m, v, g = (np.array(a, f32) for a in (p, m, v, g))
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    one = f32(1)
    powf = mutation == "powf_correction"
    t_all = t + 1 if mutation == "step_off_by_one" else t
    with np.errstate(all="ignore"):
        gnorm = np.sqrt(sumsq_f32(g))
        scale = one
        if h["max_norm"] > 0:
            c = h["max_norm"] / (gnorm if mutation == "clip_without_1e-6" else gnorm + f32(1e-6))
            if mutation == "nan_dropped_by_clamp":
                scale = c if c < one else one
            else:
                scale = c if not c >= one else one
        bc1 = np.full(p.size, _correction(h["b1"], t_all, powf), f32)
        bc2 = np.full(p.size, _correction(h["b2"], t_all, powf), f32)
        if alpha_idx is not None and alpha_idx >= 0 and alpha_live and mutation != "alpha_common_counter":
            bc1[alpha_idx], bc2[alpha_idx] = _correction(h["b1"], t_alpha, powf), _correction(h["b2"], t_alpha, powf)
        gi = g * scale
        decay = _fma(-h["lr"], h["wd"], one)
        m = _fma(one - h["b1"], gi, h["b1"] * m)
        v = _fma(gi, (one - h["b2"]) * gi, h["b2"] * v)
        if mutation == "eps_before_div":
            denom = (np.sqrt(v) + h["eps"]) / np.sqrt(bc2)
        elif mutation == "eps_in_sqrt":
            denom = np.sqrt(v + h["eps"]) / np.sqrt(bc2)
        else:
            denom = np.sqrt(v) / np.sqrt(bc2) + h["eps"]
        step = (h["lr"] / bc1) * m / denom
        p = (p - step) * decay if mutation == "wd_after_update" else _fma(p, decay, -step)
    if alpha_idx is not None and alpha_idx >= 0 and not alpha_live:
        p[alpha_idx], m[alpha_idx], v[alpha_idx] = p0[alpha_idx], m0[alpha_idx], v0[alpha_idx]
    assert p.dtype == m.dtype == v.dtype == f32 and gnorm.dtype == f32
    return p, m, v, gnorm


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def scale_to_edge(g, max_norm, side):
    """g rescaled so that max_norm / (norm + 1e-6) = 1 + side * 5e-7: clipping barely inactive (side = +1) or barely active."""
    g = np.asarray(g, f32)
    want = float(f32(max_norm)) / (1.0 + side * 5e-7) - 1e-6
    g64 = g.astype(np.float64)
    for _ in range(4):
        g64 = g64 * (want / np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        g = g64.astype(f32)
    c = float(f32(max_norm)) / (np.sqrt(np.sum(g.astype(np.float64) ** 2)) + 1e-6)
    assert 1e-7 < side * (c - 1.0) < 1e-6, c
    return g


def make_state(n, seed, fresh=False, grad="normal", alpha_idx=-1, alpha_live=False, max_norm=0.05):
    """(p, m, v, g) float32.  p ~ N(0, 2^-10): the update has to be resolvable above ulp(p).  g ~ N(0, 1e-3) with a run of 100
    exact zeros and a run of 400 of magnitude 1e-10 .. 1e-6 whose moments are zero (where the placement of eps decides the
    result); the other moments nonzero and of mixed sign unless ``fresh``.  grad: "normal", "zero", "edge+", "edge-"."""
    rng = np.random.RandomState(seed)
    p = (rng.standard_normal(n) * 2.0 ** -10).astype(f32)
    g = (rng.standard_normal(n) * 1e-3).astype(f32)
    m = (rng.standard_normal(n) * 2e-4).astype(f32)
    v = ((rng.standard_normal(n) * 2e-4) ** 2).astype(f32)
    z0, t0 = n // 3, n // 2
    g[z0:z0 + 100] = 0.0
    g[t0:t0 + 400] = (10.0 ** rng.uniform(-10, -6, 400) * rng.choice([-1.0, 1.0], 400)).astype(f32)
    for a in (m, v):
        a[z0:z0 + 100] = 0.0
        a[t0:t0 + 400] = 0.0
    if fresh:
        m[:] = 0.0
        v[:] = 0.0
    if alpha_idx >= 0 and not alpha_live:
        g[alpha_idx] = 0.0       # a gradient torch leaves at None is a zero of the bucket
    if grad == "zero":
        g[:] = 0.0
    elif grad in ("edge+", "edge-"):
        g = scale_to_edge(g, max_norm, +1 if grad == "edge+" else -1)
    else:
        assert grad == "normal", grad
    return p, m, v, g


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _case(name, kind="d64", t=7, fresh=False, grad="normal", nonfinite=None, alpha=None, **hp):
    """kind: d64 (d_model 64, window 32, 4 heads), d256 (256 / 256 / 8) or legacy.  alpha: None = smoothing_alpha not live (or
    absent), else the t_alpha of a live one."""
    return dict(name=name, kind=kind, t=t, fresh=fresh or t == 1, grad=grad, nonfinite=nonfinite, alpha=alpha, hp=hyper(**hp))


_CLIP = dict(t=1, wd=0.0)
CASES = [
    _case("t1_fresh", t=1), _case("t2", t=2), _case("t3", t=3), _case("t7", t=7), _case("t50", t=50), _case("t1000", t=1000),
    _case("t100000", t=100000),
    _case("clip_off", max_norm=0.0, **_CLIP), _case("clip_inactive", max_norm=1.0, **_CLIP), _case("clip_active", **_CLIP),
    _case("clip_edge_inactive", grad="edge+", **_CLIP), _case("clip_edge_active", grad="edge-", **_CLIP),
    _case("zero_grad", t=1, grad="zero"),
    _case("wd_0", wd=0.0), _case("wd_0.1", wd=0.1), _case("lr_2^-7", lr=2.0 ** -7), _case("lr_1e-4", lr=1e-4),
    _case("betas_0.8_0.99", b1=0.8, b2=0.99),
    _case("bucket_d256", kind="d256"), _case("bucket_legacy", kind="legacy"),
    _case("nan_grad", nonfinite="nan"), _case("inf_grad", nonfinite="inf"),
    _case("alpha_not_live", t=1000), _case("alpha_live", t=1000, alpha=3),
]
BY_NAME = {c["name"]: c for c in CASES}
CLIP_CASES = ("clip_off", "clip_inactive", "clip_active", "clip_edge_inactive", "clip_edge_active")
# cases a test drives through one plain optimizer step (the alpha cases need forward passes first)
PLAIN = [c["name"] for c in CASES if not c["name"].startswith("alpha_")]
NONFINITE_AT = 4097       # a plain element, away from the zero and tiny runs and from every trainer's smoothing_alpha


def case_state(case, n, alpha_idx, seed=11):
    """(p, m, v, g) of a case on a bucket of n floats whose smoothing_alpha sits at alpha_idx (< 0: none)."""
    p, m, v, g = make_state(n, seed, fresh=case["fresh"], grad=case["grad"], alpha_idx=alpha_idx,
                            alpha_live=case["alpha"] is not None, max_norm=float(case["hp"]["max_norm"]))
    if case["nonfinite"]:
        assert alpha_idx != NONFINITE_AT
        g[NONFINITE_AT] = np.nan if case["nonfinite"] == "nan" else np.inf
    return p, m, v, g


def case_oracle(case, state, alpha_idx):
    """(reference (p, m, v), bounds (p, m, v), info) of a case."""
    p, m, v, g = state
    live = case["alpha"] is not None
    rp, rm, rv, info = oracle_step(p, m, v, g, case["t"], case["alpha"], alpha_idx, live, case["hp"])
    return (rp, rm, rv), bound(p, m, g, rv, info, case["hp"]), info


def applied_scale(m_new, g, hp):
    """From a fresh step without weight decay: m = (1 - b1) g s, so m / ((1 - b1) g) is the clip scale the kernel applied."""
    g = np.asarray(g, np.float64)
    nz = g != 0
    return np.asarray(m_new, np.float64)[nz] / ((1.0 - widen(hp)["b1"]) * g[nz])
