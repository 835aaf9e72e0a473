"""Which kernel launch_gemm picks for a product, on the host (km_gemm_kernel_choice): the table of km_linear shapes that
tests/test_gpu_linear.py runs covers all five kernels, and each threshold of the selection has a neighbour on both sides, so a
changed threshold moves a code here instead of silently moving what the GPU tests cover."""
import pytest

import linear_cases as lc
from koemorph_amd import _lib


def choice(M, N, K, batch=1):
    return _lib.load().km_gemm_kernel_choice(M, N, K, batch)


def mirror(M, N, K, batch=1):
    """The selection restated from the description in linear_cases.py."""
    up = lambda a, b: -(-a // b)
    w4, w2, w22 = batch * up(M, 128) * up(N, 128), batch * up(M, 128) * up(N, 64), batch * up(M, 64) * up(N, 64)
    use4 = N > 64 and w4 >= 192
    use2 = not use4 and w2 >= 192
    if K % 16 or M < 64 or M * K >= 2 ** 29 or N * K >= 2 ** 29:
        return 0
    if (not use4 and not use2 and w22 >= 192) or ((use4 or use2) and (w4 if use4 else w2) < 4096):
        return 1
    return (3 if K <= 256 else 4) if use4 else 2 if use2 else 0


@pytest.mark.parametrize("M,N,K,code", lc.TABLE)
def test_table_products_run_on_the_kernel_the_table_names(M, N, K, code):
    assert choice(M, N, K) == code == mirror(M, N, K), (M, N, K, lc.NAMES[code])


@pytest.mark.parametrize("M,N,K,batch,code", lc.NEIGHBOURS)
def test_threshold_neighbours(M, N, K, batch, code):
    assert choice(M, N, K, batch) == code == mirror(M, N, K, batch), (M, N, K, batch)


def test_table_covers_every_kernel_on_and_off_the_tile():
    codes = [c for *_, c in lc.TABLE]
    assert sorted(set(codes)) == [0, 1, 2, 3, 4]
    for code, bm, bn in ((1, 64, 64), (2, 128, 64), (3, 128, 128), (4, 128, 128)):
        rows = [(M, N, K) for M, N, K, c in lc.TABLE if c == code]
        assert any(M % bm and N % bn for M, N, K in rows), f"{lc.NAMES[code]}: no product with off-tile M and N"
    assert any(K == 16 for M, N, K, c in lc.TABLE if c == 3) and any(K > 256 for M, N, K, c in lc.TABLE if c == 4)
    assert any(K % 32 for M, N, K, c in lc.TABLE if c == 0)              # a K tail of gemm_kernel's 32-wide step


def test_bad_arguments_and_the_operand_limit():
    assert choice(0, 8, 16) == -1 and choice(8, 0, 16) == -1 and choice(8, 8, 0) == -1 and choice(8, 8, 16, 0) == -1
    assert choice(2 ** 31, 8, 16) == -1
    # 2^29 floats per operand: the 32-bit byte offsets of the buffer loads (gemm_nt_ok)
    assert choice(2 ** 21, 128, 256) == 0 and choice(2 ** 21 - 1, 128, 256) == 3 == mirror(2 ** 21 - 1, 128, 256)
