"""The attention-map statistics of koemorph_amd/csrc/km_attn_stats.hip restated in float64 NumPy, the crafted rows and the
float64 bounds shared by tests/test_attn_stats_host.py, tests/test_gpu_attn_stats.py and tests/test_gpu_sequence_attention.py.
Not a test module."""
import numpy as np

from koemorph_amd import synth

Q, K = 28, 80
EPS = 2.0 ** -52


def count(q=Q, k=K):
    """KM_ATTN_STATS_COUNT(Q, K): rows, mean map, mean entropy, peak counts."""
    return 1 + q * k + q + q * k


def entropy_terms(maps):
    """-A ln A of every float32 entry, in float64; an entry of 0 contributes 0."""
    a = np.asarray(maps, np.float32).astype(np.float64)
    t = np.zeros_like(a)
    pos = a > 0
    t[pos] = -a[pos] * np.log(a[pos])
    return t


def stats_f64(maps):
    """(rows, Q, K) float32 maps -> the dict of AttentionStats.compute() without the band keys, all in float64 / int64."""
    a32 = np.asarray(maps, np.float32)
    rows, q, k = a32.shape
    if rows == 0:
        return {"rows": 0, "mean_map": np.zeros((q, k)), "entropy": np.zeros(q), "peak_hist": np.zeros((q, k), np.int64)}
    a = a32.astype(np.float64)
    peak = np.zeros((q, k), np.int64)
    np.add.at(peak, (np.broadcast_to(np.arange(q), (rows, q)), np.argmax(a32, axis=2)), 1)
    return {"rows": rows, "mean_map": a.sum(axis=0) / rows, "entropy": entropy_terms(a32).sum(axis=(0, 2)) / rows, "peak_hist": peak}


def brute_force(maps):
    """The same quantities by loops over rows, queries and keys (math.log, first strict maximum)."""
    import math
    a32 = np.asarray(maps, np.float32)
    rows, q, k = a32.shape
    s, e, p = np.zeros((q, k)), np.zeros(q), np.zeros((q, k), np.int64)
    for r in range(rows):
        for i in range(q):
            best, best_k = None, 0
            for j in range(k):
                v = float(a32[r, i, j])
                s[i, j] += v
                if v > 0.0:
                    e[i] -= v * math.log(v)
                if best is None or v > best:
                    best, best_k = v, j
            p[i, best_k] += 1
    n = max(rows, 1)
    return {"rows": rows, "mean_map": s / n, "entropy": e / n, "peak_hist": p}


def pack(st):
    """A stats dict as km_attn_stats_compute lays it out."""
    return np.concatenate([[float(st["rows"])], st["mean_map"].ravel(), st["entropy"].ravel(), st["peak_hist"].astype(np.float64).ravel()])


# ---- maps ------------------------------------------------------------------------------------------------------------------------
def crafted_rows(k=K):
    """one-hot (entropy 0), uniform (entropy ln k), a two-way tie for the maximum (the lowest key wins), a row with zeros."""
    one_hot = np.zeros(k, np.float32)
    one_hot[k - 3] = 1.0
    uniform = np.full(k, 1.0 / k, np.float32)
    tie = np.full(k, 0.5 / (k - 2), np.float32)
    tie[[17, k - 1]] = 0.25                               # keys 17 and k - 1 tie: 17 it is; they sit in different float4s AND lanes
    zeros = np.zeros(k, np.float32)
    zeros[5:9] = [0.125, 0.5, 0.125, 0.25]                # a float4 straddled (keys 5..8), everything else exactly 0
    return {"one_hot": one_hot, "uniform": uniform, "tie": tie, "zeros": zeros}


def softmax_maps(seed, rows, q=Q, k=K, scale=3.0):
    z = synth.normal(seed, (rows, q, k)).astype(np.float64) * scale
    e = np.exp(z - z.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def make_maps(seed, rows, q=Q, k=K):
    """Softmax rows with the crafted rows planted: map r carries crafted row (r + i) % 4 in query (5 i + r) % q, i = 0..3."""
    maps = softmax_maps(seed, rows, q, k)
    crafted = list(crafted_rows(k).values())
    for r in range(rows):
        for i in range(4):
            maps[r, (5 * i + r) % q] = crafted[(r + i) % 4]
    return maps


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def mean_map_bound(maps):
    """Per (q, k): rows 2^-52 sum |A| on the float64 sum (reordering of a float64 sum), here divided by rows for the mean."""
    a = np.abs(np.asarray(maps, np.float32).astype(np.float64))
    return EPS * a.sum(axis=0)


def entropy_bound(maps):
    """Per q: rows K 2^-52 sum |A ln A| on the sum (reordering) plus 4 float64 ulps per term for the device's log, here
    divided by rows for the mean."""
    t = np.abs(entropy_terms(maps))
    rows, _, k = t.shape
    return (rows * k * EPS * t.sum(axis=(0, 2)) + (4 * np.spacing(t)).sum(axis=(0, 2))) / rows


def assert_within_bounds(got, maps):
    """`got`: a compute() dict (or the restatement) judged against stats_f64(maps): counts exact, sums within the bounds."""
    want = stats_f64(maps)
    assert got["rows"] == want["rows"]
    assert np.array_equal(np.asarray(got["peak_hist"]), want["peak_hist"])
    dm = np.abs(np.asarray(got["mean_map"]) - want["mean_map"])
    de = np.abs(np.asarray(got["entropy"]) - want["entropy"])
    bm, be = mean_map_bound(maps), entropy_bound(maps)
    print(f"ATTNSTATS|rows {want['rows']}|mean map max err {dm.max():.3e} (bound at it {bm.ravel()[dm.argmax()]:.3e})|"
          f"entropy max err {de.max():.3e} (bound at it {be[de.argmax()]:.3e})")
    assert (dm <= bm).all(), float((dm - bm).max())
    assert (de <= be).all(), float((de - be).max())
