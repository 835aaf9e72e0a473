"""sumsq_partial_kernel + adamw_kernel (km_train_adamw, km_legacy_train_adamw) from GIVEN gradients, moments and step counters
against the float64 oracle of tests/adamw_cases.py (pinned to torch's clip_grad_norm_ + AdamW in tests/test_adamw_host.py), every
element of p, m and v inside the float32 bound stated there (u = 2^-24, K = 16).  Each case loads the whole flat bucket -- the
slots that pad every tensor to a multiple of four floats included: to the kernel they are elements like any other -- fills the
caller-owned flat_grad, takes ONE optimizer step, and repeats it from the same state for equal bits."""
import numpy as np
import pytest
import torch

import adamw_cases as A
from koemorph_amd import synth
from koemorph_amd.engine import Engine
from koemorph_amd.training import LegacyTrainer, Trainer

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPE = {"d64": dict(d=64, T=32, H=4), "d256": dict(d=256, T=256, H=8)}


class Bucket:
    """The flat vectors of a trainer through the C ABI."""

    def __init__(self, tr, legacy=False):
        self.tr, self.n = tr, tr.n_params
        self.pre = "km_legacy_train_" if legacy else "km_train_"
        self.alpha_idx = -1 if legacy else tr.offset("smoothing_alpha")
        self.own_grad = tr.flat_grad

    def _call(self, name, *args):
        from koemorph_amd._lib import check
        check(getattr(self.tr._lib, self.pre + name)(self.tr._h, *args))

    def load(self, p, m, v, steps):
        torch.cuda.synchronize()
        p, m, v = (np.ascontiguousarray(a, np.float32) for a in (p, m, v))
        steps = np.ascontiguousarray(steps, np.int32)
        self._call("set_params", p.ctypes.data, self.n)
        self._call("set_optimizer_state", m.ctypes.data, v.ctypes.data, self.n, steps.ctypes.data)

    def read(self):
        torch.cuda.synchronize()
        p, m, v = (np.empty(self.n, np.float32) for _ in range(3))
        steps = np.zeros(2, np.int32)
        self._call("get_params", p.ctypes.data, self.n)
        self._call("get_optimizer_state", m.ctypes.data, v.ctypes.data, self.n, steps.ctypes.data)
        return p, m, v, steps

    def step(self, state, hp, steps, grad_into=None):
        """Load (p, m, v) and the counters, put g into flat_grad (or the tensor given), one optimizer step, read back."""
        p, m, v, g = state
        tr = self.tr
        tr.lr, tr.betas, tr.eps = float(hp["lr"]), (float(hp["b1"]), float(hp["b2"])), float(hp["eps"])
        tr.weight_decay, tr.grad_clip = float(hp["wd"]), float(hp["max_norm"])
        self.load(p, m, v, steps)
        tr.flat_grad = self.own_grad if grad_into is None else grad_into
        try:
            tr.flat_grad.copy_(torch.from_numpy(np.ascontiguousarray(g, np.float32)))
            tr.optimizer_step()
            return self.read()
        finally:
            tr.flat_grad = self.own_grad


def make_trainer(kind, **kw):
    if kind == "legacy":
        from koemorph_amd.model.simplified_model import SimplifiedKoeMorphModel
        from oracle.legacy import make_legacy_params
        model = SimplifiedKoeMorphModel()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in make_legacy_params(5).items()})
        return LegacyTrainer(model.to(DEV), max_windows=2, max_frames=8)
    c = SHAPE[kind]
    e = Engine(d_model=c["d"], num_heads=c["H"], mel_sequence_length=c["T"])
    e.load_state_dict(synth.make_core_params(71, c["d"], c["T"], 256, "trained"))
    e.finalize()
    return Trainer(e, **{"max_windows": 5, **kw})


_buckets = {}


def bucket(kind):
    """One trainer per kind for the whole module.  No forward pass ever runs on these, so smoothing_alpha is never live."""
    if kind not in _buckets:
        _buckets[kind] = Bucket(make_trainer(kind), legacy=kind == "legacy")
    return _buckets[kind]


def test_bucket_sizes_are_the_ones_the_host_test_emulates():
    assert bucket("d64").n == A.bucket_size(64, 32) and bucket("d256").n == A.bucket_size(256, 256)
    assert bucket("legacy").n == A.N_LEGACY
    for kind in ("d64", "d256"):
        assert bucket(kind).alpha_idx % 4 == 0 and not A.NONFINITE_AT - 3 <= bucket(kind).alpha_idx <= A.NONFINITE_AT


def judge(tag, got, ref, bnds):
    fr = A.fractions(got[:3], ref, bnds)
    print(f"\nADAMW|{tag}|p {fr[0]:.3f}|m {fr[1]:.3f}|v {fr[2]:.3f}")
    for name, f in zip("pmv", fr):
        assert f <= 1.0, f"{tag}: {name} at {f:.3f} of its bound"
    return fr


def same_bits(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("name", A.PLAIN)
def test_one_step_from_given_state(name):
    case = A.BY_NAME[name]
    b = bucket(case["kind"])
    state = A.case_state(case, b.n, b.alpha_idx)
    ref, bnds, info = A.case_oracle(case, state, b.alpha_idx)
    steps = [case["t"] - 1, 5]
    got = b.step(state, case["hp"], steps)
    assert got[3].tolist() == [case["t"], 5]
    judge(name, got, ref, bnds)
    p0, m0, v0, g = state
    if b.alpha_idx >= 0:            # never live here: untouched, and so are its moments
        i = b.alpha_idx
        assert (got[0][i], got[1][i], got[2][i]) == (p0[i], m0[i], v0[i])
    if name in A.CLIP_CASES:
        # wd = 0, fresh moments: m / ((1 - b1) g) is the scale the kernel applied; to 8 u of the oracle's, which pins the norm
        err = float(np.abs(A.applied_scale(got[1], g, case["hp"]) / info["scale"] - 1.0).max())
        print(f"ADAMW|{name}|scale {info['scale']!r}|error {err / A.U:.2f} u")
        assert err <= 8 * A.U, (name, err / A.U)
    if name == "zero_grad":
        # the norm is 0 and nothing moves: every parameter is its product with the float32 nearest to 1 - lr wd, exactly
        h = A.widen(case["hp"])
        want = p0 * np.float32(1.0 - h["lr"] * h["wd"])
        if b.alpha_idx >= 0:
            want[b.alpha_idx] = p0[b.alpha_idx]
        assert want.dtype == np.float32 and np.array_equal(got[0], want)
        assert not got[1].any() and not got[2].any()
    if name == "nan_grad":
        others = np.arange(b.n) != b.alpha_idx
        assert np.isnan(got[0][others]).all() and np.isnan(got[1][others]).all() and np.isnan(got[2][others]).all()
    if name == "inf_grad":
        nan = np.zeros(b.n, bool)
        nan[A.NONFINITE_AT] = True
        assert info["scale"] == 0.0 and all(np.array_equal(np.isnan(a), nan) for a in got[:3])
    assert same_bits(got, b.step(state, case["hp"], steps)), "a second run from the same state gave other bits"


def test_misaligned_gradient_bucket():
    """flat_grad 4 bytes into a larger buffer: no group of four is loaded as a float4.  Same bits as the aligned run, and the
    floats on either side of the view keep theirs."""
    case = A.BY_NAME["t7"]
    b = bucket("d64")
    state = A.case_state(case, b.n, b.alpha_idx)
    steps = [6, 0]
    aligned = b.step(state, case["hp"], steps)
    big = torch.full((b.n + 2,), 12345.0, device=DEV)
    view = big[1:1 + b.n]
    assert big.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    got = b.step(state, case["hp"], steps, grad_into=view)
    assert same_bits(aligned, got)
    assert big[0].item() == 12345.0 and big[-1].item() == 12345.0
    assert np.array_equal(view.cpu().numpy().view(np.int32), np.asarray(state[3], np.float32).view(np.int32))
    ref, bnds, _ = A.case_oracle(case, state, b.alpha_idx)
    judge("misaligned", got, ref, bnds)


def mel_batch(seed, B=5, T=32):
    mel, short, emo = synth.make_core_inputs(seed, B, T + 1, style="randn")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    return to(mel), to(short), to(emo), to(synth.uniform(seed + 100, (B, 52), 0, 1))


def test_smoothing_alpha_not_live_then_live():
    """After the first forward pass at a batch size the EMA passed its input through: smoothing_alpha has no gradient, and the
    step leaves it, its moments and its counter alone while its three float4 neighbours move with the common counter.  After
    the second it is live and moves with its OWN counter."""
    b = Bucket(make_trainer("d64", use_smoothing=True))
    tr, i = b.tr, b.alpha_idx
    tr.forward_backward_mel(*mel_batch(300))
    case = A.BY_NAME["alpha_not_live"]
    state = A.case_state(case, b.n, i)
    ref, bnds, _ = A.case_oracle(case, state, i)
    got = b.step(state, case["hp"], [999, 2])
    assert got[3].tolist() == [1000, 2]
    assert all(a[i].view(np.int32) == s[i].view(np.int32) for a, s in zip(got[:3], state[:3]))
    judge("alpha_not_live", got, ref, bnds)
    near = slice(i - i % 4, i - i % 4 + 4)
    for a, s in zip(got[:3], state[:3]):       # the neighbours (padding slots of the bucket) did move
        assert (np.delete(a[near], i % 4) != np.delete(s[near], i % 4)).all()
    assert same_bits(got, b.step(state, case["hp"], [999, 2]))

    tr.forward_backward_mel(*mel_batch(301))
    case = A.BY_NAME["alpha_live"]
    state = A.case_state(case, b.n, i)
    ref, bnds, info = A.case_oracle(case, state, i)
    assert info["live"].all() and info["bc2"][i] != info["bc2"][i + 1]
    got = b.step(state, case["hp"], [999, 2])
    assert got[3].tolist() == [1000, 3]
    judge("alpha_live", got, ref, bnds)
    assert got[0][i] != state[0][i]
    assert same_bits(got, b.step(state, case["hp"], [999, 2]))


def test_padded_channel_encoder_copy_follows_the_optimizer():
    """The training program reads mel_channel_encoder.weight from a padded copy that adamw_kernel rewrites with the master
    weights.  A trainer whose copy was built from scratch from the same weights (load_params -> pad_rows_kernel) has to compute
    the same bits in the next step."""
    a, c = (Bucket(make_trainer("d64", use_smoothing=False)) for _ in range(2))
    shapes = {k: v.shape for k, v in a.tr.engine.state_dict_shapes().items()}
    before = a.tr.params(shapes)
    p0 = a.read()[0]
    case = A.BY_NAME["t1_fresh"]
    _, m, v, g = A.case_state(case, a.n, a.alpha_idx)
    a.step((p0, m, v, g), case["hp"], [0, 0])
    after = a.tr.params(shapes)
    moved = np.abs(after["mel_channel_encoder.weight"] - before["mel_channel_encoder.weight"])
    # a first step moves a weight by lr g s / (|g s| + eps): by lr wherever the gradient is not tiny
    assert np.median(moved) > 0.9 * float(case["hp"]["lr"]) and (moved > 0).mean() > 0.75
    c.tr.load_params(after)
    named = np.zeros(a.n, bool)
    for _, o, n in a.tr._param_table():
        named[o:o + n] = True
    batch = mel_batch(302)
    la, lc = a.tr.forward_backward_mel(*batch).item(), c.tr.forward_backward_mel(*batch).item()
    ga, gc = a.tr.flat_grad.cpu().numpy()[named], c.tr.flat_grad.cpu().numpy()[named]
    assert np.isfinite(la) and np.float32(la).view(np.int32) == np.float32(lc).view(np.int32)
    assert np.array_equal(ga.view(np.int32), gc.view(np.int32)) and np.abs(ga).max() > 0
