"""km_resample_clip / Resampler.clip against the float64 oracle of the output law (tests/resample_cases.py).

Every output must lie within (n + 2) 2^-24 sum_k |h_k| |x_j| of the oracle fed the same float32 samples, n being the number of
terms of that output's sum (the derivation: tests/resample_cases.py).

Largest measured fraction of that bound over all lengths of a rate, one run on an MI355X:
    48 000 -> 16 000    0.151          44 100    0.192          32 000    0.098          8 000    0.238          11 025    0.404
"""
import numpy as np
import pytest
import torch

import resample_cases as rc
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.features import Resampler
from koemorph_amd.features import resample as rs

pytestmark = pytest.mark.gpu

_RESAMPLERS = {}


def resampler(rate_in):
    if rate_in not in _RESAMPLERS:
        _RESAMPLERS[rate_in] = Resampler(rate_in, rc.RATE_OUT)
    return _RESAMPLERS[rate_in]


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the cases' arrays are read-only


@pytest.mark.parametrize("rate_in", rc.CLIP_RATES)
def test_clip_within_the_bound_of_the_oracle(rate_in):
    r = resampler(rate_in)
    up, down, h, half_len = rc.plan(rate_in)
    assert (r.up, r.down, r.half_len) == (up, down, half_len)
    worst = 0.0
    for n in rc.clip_lengths(rate_in):
        x, y, bound = rc.clip_case(rate_in, n)
        got = r.clip(dev(x)).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == y.shape == (rs.n_out(n, up, down),), n
        err = np.abs(got.astype(np.float64) - y)
        frac = float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0
        worst = max(worst, frac)
        print(f"rate {rate_in} n {n}: n_out {y.size}, max |hip - oracle| {err.max():.3e}, largest fraction of the bound {frac:.3f}")
        assert np.all(err <= bound), (rate_in, n, int(np.argmax(err - bound)), float(err.max()))
    print(f"rate {rate_in}: largest fraction of the bound {worst:.3f}")


@pytest.mark.parametrize("rate_in", rc.CLIP_RATES)
def test_silent_clip_and_impulse_read_the_table_back(rate_in):
    r = resampler(rate_in)
    up, down, h, half_len = rc.plan(rate_in)
    n = 1500
    got = r.clip(torch.zeros(n, device="cuda")).cpu().numpy()
    assert got.shape == (rs.n_out(n, up, down),) and not got.any()
    for j0 in (0, 700, n - 1):
        x = np.zeros(n, np.float32)
        x[j0] = 1.0
        got = r.clip(dev(x)).cpu().numpy()
        m = np.arange(got.size, dtype=np.int64)
        t = m * down - j0 * up + half_len
        ok = (t >= 0) & (t <= 2 * half_len)
        want = np.where(ok, h[np.where(ok, t, 0)], 0.0).astype(np.float32)
        assert ok.any() and np.array_equal(got, want), (rate_in, j0)


@pytest.mark.parametrize("rate_in", (48000, 44100))
def test_two_calls_give_the_same_bits_and_alignment_does_not_matter(rate_in):
    r = resampler(rate_in)
    x, _, _ = rc.clip_case(rate_in, 5000)
    a = r.clip(dev(x))
    b = r.clip(dev(x))
    assert torch.equal(a, b)
    shifted = torch.zeros(5003, device="cuda")
    shifted[3:] = dev(x)
    c = r.clip(shifted[3:])                               # a source that is not 16-byte aligned takes the scalar loads
    assert c.data_ptr() % 16 == 0 and shifted[3:].data_ptr() % 16 != 0
    assert torch.equal(a, c)


def test_clip_refuses_bad_arguments():
    r = resampler(48000)
    with pytest.raises(ValueError):
        r.clip(torch.zeros(0, device="cuda"))
    with pytest.raises(ValueError):
        r.clip(torch.zeros(4, 4, device="cuda"))
    x = torch.zeros(30, device="cuda")
    out = torch.zeros(11, device="cuda")
    code = r._lib.km_resample_clip(r._h, x.data_ptr(), 30, out.data_ptr(), 11, None)
    assert code != 0 and b"n_out" in r._lib.km_last_error()
    with pytest.raises(ValueError):
        Resampler(16000, 16000)
    with pytest.raises(KoeMorphError, match="LDS"):
        Resampler(16001, 16000)
