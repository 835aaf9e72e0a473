"""km_attn_stats_* on the MI355X through ``koemorph_amd.metrics.AttentionStats``, against the float64 restatement of
tests/attn_stats_cases.py on maps made on the host.

Peak counts and the row count are exact.  A mean-map entry is within rows 2^-52 sum |A| of the float64 NumPy sum (what another
order of a float64 sum can differ by), the entropy within rows 80 2^-52 sum |A ln A| plus 4 float64 ulps per term for the
device's log (attn_stats_cases.mean_map_bound / entropy_bound; both are bounds on the sums, divided by rows for the means).
rows = 300 with max_rows_per_launch = 64 folds five pieces (64 x 4 + 44, the last with a 12-row chunk)."""
import numpy as np
import pytest
import torch

import attn_stats_cases as ac
from koemorph_amd.metrics import AttentionStats

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same_bits(a, b):
    return (a["rows"] == b["rows"] and np.array_equal(a["peak_hist"], b["peak_hist"]) and
            a["mean_map"].tobytes() == b["mean_map"].tobytes() and a["entropy"].tobytes() == b["entropy"].tobytes())


@pytest.mark.parametrize("rows,per_launch", [(1, 0), (7, 0), (300, 64), (300, 0)])
def test_update_and_compute_against_the_restatement(rows, per_launch):
    maps = ac.make_maps(100 + rows, rows)
    acc = AttentionStats(max_rows_per_launch=per_launch)
    acc.update(dev(maps))
    got = acc.compute()
    assert got["rows"] == rows == acc.rows and got["peak_hist"].sum() == rows * ac.Q
    ac.assert_within_bounds(got, maps)
    # the crafted rows, one by one: map 0 carries one_hot / uniform / tie / zeros in queries 0, 5, 10, 15
    if rows == 1:
        assert got["entropy"][0] == 0.0 and got["peak_hist"][0, ac.K - 3] == 1
        assert abs(got["entropy"][5] - np.log(ac.K)) < 1e-6
        assert got["peak_hist"][10, 17] == 1 and got["peak_hist"][10, ac.K - 1] == 0
        assert got["peak_hist"][15, 6] == 1 and np.isfinite(got["entropy"]).all()
    assert abs(sum(got["band_share"].values()) - 4 * got["mean_map"].mean()) < 1e-12
    acc.close()


def test_other_shapes_than_the_models():
    """3 x 8 (two lanes per query, 32 queries' worth of lanes per wave) and 70 x 256 (one query per wave, more queries than the
    workgroup has waves): the lane layout is derived from the shape."""
    for q, k, rows in ((3, 8, 37), (70, 256, 19)):
        maps = ac.softmax_maps(7 + q, rows, q, k)
        maps[rows // 2, q - 1] = 0.0
        maps[rows // 2, q - 1, [k // 2, k - 1]] = 0.5                          # a tie and zeros
        acc = AttentionStats(q, k)
        acc.update(dev(maps))
        got = acc.compute()
        assert "band_mean" not in got or k >= 80
        ac.assert_within_bounds(got, maps)
        acc.close()


def test_determinism_and_state():
    maps = ac.make_maps(31, 300)
    a, b, whole = AttentionStats(), AttentionStats(), AttentionStats()
    for acc in (a, b):
        acc.update(dev(maps[:150]))
        acc.update(dev(maps[150:]))
    ra, rb = a.compute(), b.compute()
    assert same_bits(ra, rb)                                                    # the same rows in the same calls: the same bits
    ac.assert_within_bounds(ra, maps)
    whole.update(dev(maps))
    ac.assert_within_bounds(whole.compute(), maps)
    # compute, update, compute: the state is left as it was
    c = AttentionStats()
    c.update(dev(maps[:150]))
    first = c.compute()
    ac.assert_within_bounds(first, maps[:150])
    assert same_bits(first, c.compute())
    c.update(dev(maps[150:]))
    assert same_bits(c.compute(), ra)
    # rows = 0 is a no-op, with or without rows
    c.update(torch.empty(0, ac.Q, ac.K, device="cuda"))
    assert same_bits(c.compute(), ra) and c.rows == 300
    # reset empties it
    c.reset()
    z = c.compute()
    assert z["rows"] == 0 and not z["mean_map"].any() and not z["entropy"].any() and not z["peak_hist"].any()
    c.update(dev(maps[:150]))
    assert same_bits(c.compute(), first)
    with pytest.raises(ValueError):
        c.update(torch.zeros(2, ac.Q, ac.K - 4, device="cuda"))
    with pytest.raises(ValueError):
        c.update(torch.zeros(2, ac.Q, ac.K))
    for acc in (a, b, whole, c):
        acc.close()


def test_captured_reset_update_compute_replays_on_other_data():
    from koemorph_amd._lib import check, km_attn_stats_count, load
    lib = load()
    first, second = ac.make_maps(41, 70), ac.make_maps(42, 70)
    buf = dev(first).clone()
    out = torch.zeros(km_attn_stats_count(ac.Q, ac.K), device="cuda", dtype=torch.float64)
    acc = AttentionStats(max_rows_per_launch=32)                                # three pieces inside the capture
    h = acc._handle(buf.device)

    def run():
        st = torch.cuda.current_stream().cuda_stream
        check(lib.km_attn_stats_reset(h, st))
        check(lib.km_attn_stats_update(h, buf.data_ptr(), 70, st))
        check(lib.km_attn_stats_compute(h, out.data_ptr(), st))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up outside the capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                               # one linear chain: reset, 3 x (partial, fold), compute
        run()
    for maps in (second, first):
        buf.copy_(dev(maps))
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.cpu().numpy().copy()
        twin = AttentionStats(max_rows_per_launch=32)
        twin.update(dev(maps))
        assert np.array_equal(replayed, ac.pack(twin.compute()))
        twin.close()
    del graph
    acc.close()
