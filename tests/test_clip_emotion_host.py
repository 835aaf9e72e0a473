"""The closed form of a clip's emotion track (tests/clip_emotion_cases.py) against the host oracle of the emotion streams: a
one-stream ``EmotionStreamOracle`` fed the clip in chunks of gcd(MIN, U) samples with an update after every push makes exactly the
track's updates, on exactly the track's windows -- and the window -> row mapping against a brute-force "latest update not after the
window's end".  No GPU, no features: integers only.
"""
import numpy as np
import pytest

import clip_emotion_cases as cc
from stream_emotion_cases import EmotionStreamOracle

CASES = [(64777, 1.0, 0.3), (7999, 1.0, 0.3), (8000, 1.0, 0.3), (70001, 1.5, 0.7)]


def stream_updates(n, ctx, itv):
    """[(t, start, length)] of every update of one oracle stream over a ramp whose sample values name their positions."""
    assert n < 2 ** 24                                            # float32 holds every position + 1 exactly
    ramp = np.arange(1, n + 1, dtype=np.float32)
    o, g, out = EmotionStreamOracle(1, ctx, itv), cc.chunk(ctx, itv), []
    for at in range(0, n, g):
        rec = o.step([ramp[at:at + g]])
        if rec["updated"]:
            w = rec["windows"][0]
            assert np.array_equal(w, np.arange(w[0], w[0] + len(w), dtype=np.float32))       # contiguous in the clip
            out.append((o.buf[0].total, int(w[0]) - 1, len(w)))
    return out


@pytest.mark.parametrize("n,ctx,itv", CASES)
def test_closed_form_plan_is_what_a_stream_does(n, ctx, itv):
    want = stream_updates(n, ctx, itv)
    got = cc.plan(n, ctx, itv)
    assert got == want
    assert len(got) == cc.num_rows(n, ctx, itv)
    sh = cc.shape(ctx, itv)
    for t, start, length in got:
        assert 0 <= start and start + length <= t <= n and sh["MIN"] <= length <= sh["C"]


def test_row_counts_at_the_edges():
    assert cc.num_rows(7999, 1.0, 0.3) == 0 and cc.plan(7999, 1.0, 0.3) == []
    assert cc.num_rows(8000, 1.0, 0.3) == 1 and cc.plan(8000, 1.0, 0.3) == [(8000, 0, 8000)]
    p = cc.plan(64777, 1.0, 0.3)
    assert len(p) == 12
    assert [length for _, _, length in p[:2]] == [8000, 12800]                     # two growing windows
    assert all((s, length) == (0, 16000) for _, s, length in p[2:9])               # seven stale ones: the oldest second
    assert [(s, length) for _, s, length in p[9:]] == [(35200, 16000), (40000, 16000), (44800, 16000)]     # three after the wrap
    assert cc.num_rows(368160, 20.0, 0.3) == 76


def brute_row(s, T, hop, n, ctx, itv):
    times = [t for t, _, _ in cc.plan(n, ctx, itv)]
    if not times:
        return 0, 0
    e = min(n, (s + T) * hop)
    upto = [k for k, t in enumerate(times) if t <= e]
    return (upto[-1] if upto else 0), 1


@pytest.mark.parametrize("hop,T", [(533, 256), (266, 512), (533, 4)])
def test_window_to_row_mapping(hop, T):
    """T = 4 at hop 533: windows that end before the first update (e < MIN) take row 0."""
    ctx, itv, n = 1.0, 0.3, 160000
    last = n // hop - T
    starts = [0, 3, 3, last, last + 1, last + 40, 7, 2, 2, 100, 1, last // 2]       # repeated, unordered, ending past the clip
    rows = [cc.window_row(s, T, hop, n, ctx, itv) for s in starts]
    assert rows == [brute_row(s, T, hop, n, ctx, itv) for s in starts]
    K = cc.num_rows(n, ctx, itv)
    assert cc.window_row(last + 40, T, hop, n, ctx, itv) == (K - 1, 1)              # e clamps to n: the last row
    if T == 4:
        assert (0 + T) * hop < 8000 and cc.window_row(0, T, hop, n, ctx, itv) == (0, 1)
    # every start of the clip, against the brute force
    for s in range(0, last + 3):
        assert cc.window_row(s, T, hop, n, ctx, itv) == brute_row(s, T, hop, n, ctx, itv), s


def test_window_of_a_clip_without_rows():
    assert cc.window_row(0, 256, 533, 6400, 1.0, 0.3) == (0, 0)
    assert cc.window_row(5, 256, 533, 7999, 1.0, 0.3) == (0, 0)


def test_cli_flag_defaults_to_noise():
    from koemorph_amd.scripts import train_sequential as ts
    p = ts.build_parser()
    assert p.parse_args(["--data_dir", "x"]).emotion == "noise"
    assert p.parse_args(["--data_dir", "x", "--emotion", "egemaps"]).emotion == "egemaps"
    with pytest.raises(SystemExit):
        p.parse_args(["--data_dir", "x", "--emotion", "opensmile"])
