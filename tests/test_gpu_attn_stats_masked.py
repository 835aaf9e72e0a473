"""km_attn_stats_update_masked and km_attn_stats_streams_* on the MI355X, through ``AttentionStats.update(maps, mask=)`` and
``StreamAttentionStats``.

The contracts are bit contracts, so every comparison is ``np.array_equal`` on the packed ``compute()`` vector:
  * a masked update leaves the state that ``update`` leaves on the selected rows compacted on the host, for every mask -- with
    max_rows_per_launch = 64 the 300-row cases are cut into pieces (of ranks, as the dense update cuts the compacted rows);
  * stream s of the per-stream accumulator holds what a plain accumulator holds that was fed that stream's selected maps one
    ``update`` of a single row at a time.
The maps are those of tests/attn_stats_cases.py: softmax rows with the one-hot, uniform, tied and zero-holding rows planted."""
import functools

import numpy as np
import pytest
import torch

import attn_stats_cases as ac
from koemorph_amd import synth
from koemorph_amd._lib import check, km_attn_stats_count, load
from koemorph_amd.metrics import AttentionStats, StreamAttentionStats

pytestmark = pytest.mark.gpu
PER_LAUNCH = 64


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def maps_of(rows):
    m = ac.make_maps(200 + rows, rows)
    m.setflags(write=False)
    return m


def masks_of(rows):
    one = np.zeros(rows, np.uint8)
    one[rows // 2] = 1
    return {"ones": np.ones(rows, np.uint8), "zeros": np.zeros(rows, np.uint8), "one": one,
            "alternating": (np.arange(rows) % 2 == 0).astype(np.uint8),
            "random": (synth.uniform(900 + rows, (rows,)) < 0.5).astype(np.uint8) * 3}     # any non-zero byte selects


def packed(acc):
    return ac.pack(acc.compute())


def dense_on(maps, per_launch=PER_LAUNCH):
    acc = AttentionStats(max_rows_per_launch=per_launch)
    if maps.shape[0]:
        acc.update(dev(maps))
    vec = packed(acc)
    acc.close()
    return vec


@pytest.mark.parametrize("rows", [1, 7, 37, 300])
def test_masked_update_is_the_dense_update_of_the_compacted_rows(rows):
    maps = maps_of(rows)
    maps_d = dev(maps)
    for name, mask in masks_of(rows).items():
        acc = AttentionStats(max_rows_per_launch=PER_LAUNCH)
        acc.update(maps_d, mask=dev(mask))
        got = packed(acc)
        want = dense_on(maps[mask != 0])
        assert got[0] == int((mask != 0).sum()), (rows, name)
        assert np.array_equal(got, want), (rows, name, int(np.flatnonzero(got != want)[0]))
        if name == "zeros":
            assert not got.any()
        acc.close()
    # a bool mask is the same mask
    acc = AttentionStats(max_rows_per_launch=PER_LAUNCH)
    alt = masks_of(rows)["alternating"]
    acc.update(maps_d, mask=dev(alt).bool())
    assert np.array_equal(packed(acc), dense_on(maps[alt != 0]))
    acc.close()


def test_masked_update_on_a_state_that_already_holds_rows_and_the_default_piece_size():
    """compute / update / compute: a masked update after a dense one, then an all-zero mask (nothing changes), then another masked
    one -- against the same calls made densely on compacted rows.  max_rows_per_launch 0 (4096) and 64."""
    a, b = maps_of(300), maps_of(37)
    ma, mb = masks_of(300)["random"], masks_of(37)["alternating"]
    for per_launch in (0, PER_LAUNCH):
        acc, twin = AttentionStats(max_rows_per_launch=per_launch), AttentionStats(max_rows_per_launch=per_launch)
        acc.update(dev(b))
        twin.update(dev(b))
        first = packed(acc)
        assert np.array_equal(first, packed(twin))
        acc.update(dev(a), mask=dev(ma))
        twin.update(dev(a[ma != 0]))
        second = packed(acc)
        assert np.array_equal(second, packed(twin)) and second[0] == 37 + int((ma != 0).sum())
        acc.update(dev(a), mask=dev(np.zeros(300, np.uint8)))
        assert np.array_equal(packed(acc), second)
        acc.update(dev(b), mask=dev(mb))
        twin.update(dev(b[mb != 0]))
        assert np.array_equal(packed(acc), packed(twin))
        assert acc.rows == 37                                       # the host count covers the unmasked updates only
        acc.reset()
        assert not packed(acc).any()
        acc.close()
        twin.close()
    with pytest.raises(ValueError):
        AttentionStats().update(dev(b), mask=dev(np.ones(36, np.uint8)))
    with pytest.raises(ValueError):
        AttentionStats().update(dev(b), mask=torch.ones(37, dtype=torch.uint8))


def test_captured_masked_update_replays_on_other_masks():
    lib = load()
    rows = 70
    maps = maps_of(300)[:rows]
    buf, mask = dev(maps), torch.zeros(rows, dtype=torch.uint8, device="cuda")
    out = torch.zeros(km_attn_stats_count(ac.Q, ac.K), device="cuda", dtype=torch.float64)
    acc = AttentionStats(max_rows_per_launch=32)                    # three pieces inside the capture
    h = acc._handle(buf.device)

    def run():
        st = torch.cuda.current_stream().cuda_stream
        check(lib.km_attn_stats_update_masked(h, buf.data_ptr(), mask.data_ptr(), rows, st))
        check(lib.km_attn_stats_compute(h, out.data_ptr(), st))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up outside the capture: the mask is all zero, nothing is folded
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    eager = AttentionStats(max_rows_per_launch=32)
    all_masks = masks_of(rows)
    for name in ("random", "zeros", "alternating", "ones", "one"):   # the state carries over from replay to replay
        mask.copy_(dev(all_masks[name]))
        graph.replay()
        torch.cuda.synchronize()
        eager.update(buf, mask=mask)
        assert np.array_equal(out.cpu().numpy(), packed(eager)), name
    assert out.cpu().numpy()[0] == sum(int((m != 0).sum()) for m in all_masks.values())
    del graph
    acc.close()
    eager.close()


def test_per_stream_accumulator_is_one_plain_accumulator_per_stream():
    S, UPDATES = 4, 9
    maps = maps_of(300)[:S * UPDATES].reshape(UPDATES, S, ac.Q, ac.K)
    masks = (synth.uniform(77, (UPDATES, S)) < 0.6).astype(np.uint8)
    masks[0], masks[1], masks[2] = 1, 0, (1, 0, 0, 1)               # all, none, some
    masks[:, 3][3:] = 0                                              # stream 3 stops early
    acc = StreamAttentionStats(S)
    plain = [AttentionStats() for _ in range(S)]
    for u in range(UPDATES):
        md = dev(maps[u])
        acc.update(md, dev(masks[u]) if u % 2 else dev(masks[u]).bool())
        for s in range(S):
            if masks[u, s]:
                plain[s].update(md[s:s + 1])
        if u == 4:                                                   # compute / update / compute
            mid = acc.compute()
            for s in range(S):
                assert np.array_equal(ac.pack(mid[s]), packed(plain[s])), s
    got = acc.compute()
    assert len(got) == S and set(got[0]) == {"rows", "mean_map", "entropy", "peak_hist", "band_mean", "band_share"}
    for s in range(S):
        assert got[s]["rows"] == int(masks[:, s].sum()) and np.array_equal(ac.pack(got[s]), packed(plain[s])), s
        chosen = maps[masks[:, s] != 0, s]
        ac.assert_within_bounds(got[s], chosen)
    # a masked reset makes stream 1 fresh and leaves the others untouched; then it accumulates again from nothing
    acc.reset(dev(np.array([0, 1, 0, 0], np.uint8)))
    after = acc.compute()
    assert after[1]["rows"] == 0 and not ac.pack(after[1]).any()
    for s in (0, 2, 3):
        assert np.array_equal(ac.pack(after[s]), ac.pack(got[s])), s
    acc.update(dev(maps[0]), dev(np.array([0, 1, 0, 0], np.uint8)))
    fresh = AttentionStats()
    fresh.update(dev(maps[0][1:2]))
    assert np.array_equal(ac.pack(acc.compute()[1]), packed(fresh))
    acc.reset()
    assert all(not ac.pack(z).any() for z in acc.compute())
    with pytest.raises(ValueError):
        acc.update(dev(maps[0][:3]), dev(masks[0][:3]))
    with pytest.raises(ValueError):
        acc.update(dev(maps[0]), torch.ones(S, dtype=torch.uint8))
    for a in plain + [fresh]:
        a.close()
    acc.close()
