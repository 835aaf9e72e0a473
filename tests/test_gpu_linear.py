"""km_linear against a float64 matmul on each of launch_gemm's five kernels.

The products are linear_cases.TABLE; tests/test_gemm_choice.py holds, on the host, that they reach gemm_kernel and the four
gemm_nt_kernel instantiations (km_gemm_kernel_choice), with M and N off the tile for each, K = 16 (one k step) and K = 272 (past
the 256 at which the 128 x 128 tile drops its scheduling barriers).  x, w and b are unit gaussians inside NaN-guarded allocations
(1280 floats of NaN on either side: a read outside an operand meets NaN), the output starts as NaN inside guards of its own.

Checked per product, with and without the bias:
  * a few hundred rows -- the first and the last, every row of the first and of the last 128-row tile that exists, and rows spread
    over the rest -- in all N columns against float64:  |c - c64| <= (K + 2) 2^-24 (sum_k |x_k w_k| + |b|)  entry by entry.
    The bound is the standard one for a float32 sum of K products in ANY order (each product one rounding, each of the K - 1
    additions at most one rounding of a partial sum that is at most sum |x_k w_k| (1 + ...)), plus the bias addition and the
    store: (K + 2) u to first order, u = 2^-24.  It is not tuned; the MFMA accumulates in float32 without intermediate rounding
    surprises, so the kernels sit far below it (table).
  * no NaN anywhere in the output (every entry was written, none from a guard), the output's guards still all NaN, the operands'
    bits unchanged.

Every case prints `LINEAR|kernel code|M x N x K|bias|largest |c - c64| / bound|rows compared` before it asserts.

OBSERVED (MI355X): largest error / bound per kernel code, and the product that gave it (28 lines)
  0 gemm_kernel            0.239   63 x 12800 x 16, bias
  1 gemm_nt<2,2,true>      0.233   3001 x 1003 x 16, no bias
  2 gemm_nt<4,2,true>      0.211   524293 x 50 x 16, no bias
  3 gemm_nt<4,4,true>      0.326   8200 x 8190 x 16, bias
  4 gemm_nt<4,4,false>     0.022   8200 x 8190 x 272, bias
The short contractions come closest (the bound grows with K, the error of a float32 sum of gaussians with sqrt(K)); a wrong
operand, tile edge or k step is an error of the order of the entries themselves, thousands of times the bound.
"""
import numpy as np
import pytest
import torch

import linear_cases as lc
from koemorph_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 1280
U = 2.0 ** -24


def guarded_randn(gen, *shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + n].view(*shape)
    view.copy_(torch.randn(*shape, generator=gen, dtype=torch.float32))
    return buf, view


def sample_rows(M, want=300):
    rows = {0, M - 1} | set(range(0, min(M, 128))) | set(range((M - 1) // 128 * 128, M))
    rows |= {int(i) for i in np.linspace(0, M - 1, max(2, want - len(rows)))}
    return torch.tensor(sorted(rows), dtype=torch.int64)


@pytest.mark.parametrize("M,N,K,code", lc.TABLE)
def test_km_linear_against_float64(M, N, K, code):
    lib = _lib.load()
    assert lib.km_gemm_kernel_choice(M, N, K, 1) == code
    gen = torch.Generator().manual_seed(1000 * code + K + N)
    xb, x = guarded_randn(gen, M, K)
    wb, w = guarded_randn(gen, N, K)
    bb, b = guarded_randn(gen, N)
    assert x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    keep = [t.clone() for t in (xb, wb, bb)]
    rows = sample_rows(M)
    xs = x[rows.cuda()].cpu().double()
    w64, b64 = w.cpu().double(), b.cpu().double()
    mag = xs.abs() @ w64.abs().T
    stream = torch.cuda.current_stream().cuda_stream
    for bias in (True, False):
        ob = torch.full((M * N + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        out = ob[GUARD:GUARD + M * N].view(M, N)
        _lib.check(lib.km_linear(x.data_ptr(), w.data_ptr(), b.data_ptr() if bias else None, M, K, N, out.data_ptr(), stream))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any()), "an entry of the output was not written, or was computed from a guard"
        assert bool(torch.isnan(ob[:GUARD]).all()) and bool(torch.isnan(ob[GUARD + M * N:]).all()), "the output's guards were written"
        got = out[rows.cuda()].cpu().double()
        ref = xs @ w64.T + (b64 if bias else 0.0)
        bound = (K + 2) * U * (mag + (b64.abs() if bias else 0.0))
        ratio = float(((got - ref).abs() / bound).max())
        print(f"LINEAR|{code} {lc.NAMES[code]}|{M} x {N} x {K}|{'bias' if bias else 'no bias'}|{ratio:.4f}|{len(rows)}")
        assert ratio <= 1.0, (M, N, K, bias, ratio)
        del ob, out
    for t, k in zip((xb, wb, bb), keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32)), "an operand or its guard changed"
