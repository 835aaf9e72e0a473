"""The float64 oracle of tests/adamw_cases.py against torch's own clip_grad_norm_ + AdamW, and the float32 restatement of the two
optimizer kernels against the bound of every case of tests/test_gpu_adamw.py: unmutated it stays inside, every mutation leaves it
in a named case.  Runs without a GPU."""
import numpy as np
import pytest
import torch

import adamw_cases as A

N = 1024
SPLIT = 600          # two tensors, so that the norm is the global one


def torch_steps(p, m, v, grads, t_first, hp):
    """clip_grad_norm_ + AdamW.step on two float64 tensors, once per gradient, the first step being number t_first."""
    h = A.widen(hp)
    P = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in (p[:SPLIT], p[SPLIT:])]
    opt = torch.optim.AdamW(P, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    for q in P:         # one throw-away step creates the state in this torch's own layout; then overwrite all of it
        q.grad = torch.zeros_like(q)
    opt.step()
    for q, sl in zip(P, (slice(0, SPLIT), slice(SPLIT, None))):
        st = opt.state[q]
        st["exp_avg"].copy_(torch.from_numpy(np.asarray(m[sl], np.float64)))
        st["exp_avg_sq"].copy_(torch.from_numpy(np.asarray(v[sl], np.float64)))
        st["step"] = torch.tensor(float(t_first - 1)) if torch.is_tensor(st["step"]) else t_first - 1
        with torch.no_grad():
            q.copy_(torch.from_numpy(np.asarray(p[sl], np.float64)))
    for g in grads:
        P[0].grad, P[1].grad = (torch.tensor(np.asarray(a, np.float64)) for a in (g[:SPLIT], g[SPLIT:]))
        if h["max_norm"] > 0:
            torch.nn.utils.clip_grad_norm_(P, h["max_norm"])
        opt.step()
    cat = lambda key: np.concatenate([opt.state[q][key].numpy() for q in P])
    return np.concatenate([q.detach().numpy() for q in P]), cat("exp_avg"), cat("exp_avg_sq")


def oracle_steps(p, m, v, grads, t_first, hp):
    for i, g in enumerate(grads):
        p, m, v, info = A.oracle_step(p, m, v, g, t_first + i, None, -1, False, hp)
    return p, m, v, info


def rel(a, b):
    """Largest difference relative to the vector's largest magnitude.  Not element by element: where the decayed parameter and
    the step, or b1 m and (1 - b1) g, cancel, two float64 evaluations differ by 7e-14 of the element (1.3e-18 on a parameter of
    1.4e-6 among parameters of 6e-3) without either being wrong."""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("clip,max_norm", [("active", 0.01), ("inactive", 1.0), ("off", 0.0)])
def test_oracle_matches_torch_clip_and_adamw(clip, max_norm):
    """3 consecutive steps from fresh moments and one step entered at t = 1000 through the optimizer's state: every element of
    p, m and v to 1e-14 relative."""
    hp = A.hyper(max_norm=max_norm)
    grads = [A.make_state(N, 20 + i)[3] for i in range(3)]
    for t_first, gs, fresh in ((1, grads, True), (1000, grads[:1], False)):
        p, m, v, _ = A.make_state(N, 7, fresh=fresh)
        want = torch_steps(p, m, v, gs, t_first, hp)
        *got, info = oracle_steps(p, m, v, gs, t_first, hp)
        assert (info["scale"] < 1.0) == (clip == "active"), info["scale"]
        worst = max(rel(a, b) for a, b in zip(got, want))
        print(f"\noracle vs torch, clip {clip}, from t = {t_first}: {worst:.2e} relative")
        assert worst <= 1e-14, (clip, t_first, worst)


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_oracle_matches_torch_on_a_non_finite_gradient(kind):
    """error_if_nonfinite=False: one NaN makes the norm, the coefficient and with them every parameter NaN; one Inf makes the
    coefficient 0, that element NaN, and moves the others by their old moments alone."""
    hp = A.hyper()
    p, m, v, g = A.make_state(N, 7)
    g[5] = np.nan if kind == "nan" else np.inf
    want = torch_steps(p, m, v, [g], 7, hp)
    *got, info = oracle_steps(p, m, v, [g], 7, hp)
    for a, b in zip(got, want):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(b)
        assert ok.sum() == (0 if kind == "nan" else N - 1)
        if ok.any():
            assert rel(a[ok], b[ok]) <= 1e-14
    if kind == "inf":
        h = A.widen(hp)
        assert info["scale"] == 0.0
        np.testing.assert_allclose(np.delete(got[1], 5), np.delete(h["b1"] * m.astype(np.float64), 5), rtol=1e-15)


def test_untouched_and_live_smoothing_alpha_in_the_oracle():
    hp = A.hyper()
    p, m, v, g = A.make_state(N, 7, alpha_idx=77)
    rp, rm, rv, _ = A.oracle_step(p, m, v, g, 1000, None, 77, False, hp)
    assert (rp[77], rm[77], rv[77]) == (p[77], m[77], v[77])
    p, m, v, g = A.make_state(N, 7, alpha_idx=77, alpha_live=True)
    lp, lm, lv, _ = A.oracle_step(p, m, v, g, 1000, 3, 77, True, hp)
    s = A.clip_scale(g, A.widen(hp)["max_norm"])[0]
    one = A.oracle_step(p[77:78], m[77:78], v[77:78], g[77:78].astype(np.float64) * s, 3, None, -1, False, A.hyper(max_norm=0.0))
    assert abs(lp[77] - one[0][0]) <= 1e-15 * abs(lp[77]) and lm[77] == one[1][0]


# ---- the float32 restatement against the bound, at the GPU test's cases ------------------------------------------------------------
ALPHA_AT = 1234        # any slot that is neither first nor last of its group of four

_cache = {}


def host_case(name):
    """(case, state, reference, bounds) on a bucket of the size the GPU test meets."""
    if name not in _cache:
        case = A.BY_NAME[name]
        n = {"d64": A.bucket_size(64, 32), "d256": A.bucket_size(256, 256), "legacy": A.N_LEGACY}[case["kind"]]
        alpha_idx = -1 if case["kind"] == "legacy" else ALPHA_AT
        state = A.case_state(case, n, alpha_idx)
        ref, bnds, _ = A.case_oracle(case, state, alpha_idx)
        _cache[name] = (case, state, ref, bnds, alpha_idx)
    return _cache[name]


def emulated_fractions(name, mutation=None):
    case, state, ref, bnds, alpha_idx = host_case(name)
    got = A.emulate_f32(*state, case["t"], case["alpha"], alpha_idx, case["alpha"] is not None, case["hp"], mutation)
    return A.fractions(got[:3], ref, bnds)


def test_bucket_sizes():
    assert A.bucket_size(256, 256) == 837744 and A.bucket_size(64, 32) > 65536


def test_restatement_stays_inside_the_bound_at_every_case():
    lines = []
    for c in A.CASES:
        fr = emulated_fractions(c["name"])
        lines.append(f"EMU|{c['name']}|p {fr[0]:.3f}|m {fr[1]:.3f}|v {fr[2]:.3f}")
    print("\n" + "\n".join(lines))
    for c, line in zip(A.CASES, lines):
        assert max(emulated_fractions(c["name"])) <= 1.0, line


def test_restatement_applies_the_oracles_clip_scale():
    """wd = 0 and fresh moments: m / ((1 - b1) g) is the scale applied.  It equals the oracle's to 8 u, which pins the norm."""
    for name in A.CLIP_CASES:
        case, state, _, _, alpha_idx = host_case(name)
        m_new = A.emulate_f32(*state, case["t"], None, alpha_idx, False, case["hp"])[1]
        s = A.clip_scale(state[3], A.widen(case["hp"])["max_norm"])[0]
        err = float(np.abs(A.applied_scale(m_new, state[3], case["hp"]) / s - 1.0).max())
        print(f"EMU|{name}|scale {s!r}|error {err / A.U:.2f} u")
        assert err <= 8 * A.U, (name, err / A.U)
    assert A.clip_scale(host_case("clip_edge_inactive")[1][3], 0.05)[0] == 1.0 > A.clip_scale(host_case("clip_edge_active")[1][3], 0.05)[0]


# the case in which each mutation has to leave the bound (others may catch it too)
CAUGHT_BY = {"eps_before_div": "t1_fresh", "eps_in_sqrt": "t7", "step_off_by_one": "t1000", "clip_without_1e-6": "clip_active",
             "wd_after_update": "wd_0.1", "alpha_common_counter": "alpha_live", "powf_correction": "t2",
             "nan_dropped_by_clamp": "nan_grad"}


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_every_mutation_leaves_the_bound(mutation):
    fr = emulated_fractions(CAUGHT_BY[mutation], mutation)
    print(f"\nMUT|{mutation}|{CAUGHT_BY[mutation]}|p {fr[0]:.3g}|m {fr[1]:.3g}|v {fr[2]:.3g}")
    assert max(fr) > 1.0, (mutation, fr)
    if mutation == "clip_without_1e-6":      # also caught by the scale itself
        case, state, _, _, alpha_idx = host_case("clip_active")
        m_new = A.emulate_f32(*state, 1, None, alpha_idx, False, case["hp"], mutation)[1]
        s = A.clip_scale(state[3], 0.05)[0]
        assert np.abs(A.applied_scale(m_new, state[3], case["hp"]) / s - 1.0).max() > 8 * A.U


def test_mutation_table_is_complete():
    assert set(CAUGHT_BY) == set(A.MUTATIONS)
