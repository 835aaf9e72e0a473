"""Span arithmetic of the training step from a resident clip (koemorph_amd.clip_span) against a brute-force statement over
sample ranges: which STFT frames of a window read only clip samples (and which clip frame they are), which see the window's
zero padding, and the hop >= n_fft / 2 rule that makes frames 0 and T the only ones that do."""
import numpy as np
import pytest

from koemorph_amd import clip_span as cs

N_FFT = 1024


def frame_samples(start_sample, f, hop, lo, hi):
    """The n_fft absolute sample indices frame f of a signal that begins at start_sample reads, -1 where it reads padding
    (outside [lo, hi), the signal's extent)."""
    idx = start_sample + f * hop - N_FFT // 2 + np.arange(N_FFT)
    return np.where((idx >= lo) & (idx < hi), idx, -1)


@pytest.mark.parametrize("hop", [533, 512, 266])
@pytest.mark.parametrize("T", [3, 256])
def test_edge_frames_and_span_rows_against_sample_ranges(hop, T):
    starts = [4, 9, 4, 30] if T == 3 else [0, 17, 5, 63]
    lo_f, hi_f = min(starts), max(starts)
    n_rows = cs.n_span(lo_f, hi_f, T)
    assert n_rows == hi_f - lo_f + T + 1
    # the span: a signal that begins at clip frame lo_f and holds (n_rows - 1) * hop samples
    span_lo, span_hi = lo_f * hop, (lo_f + n_rows - 1) * hop
    brute_edges = None
    for s in starts:
        w_lo, w_hi = s * hop, (s + T) * hop
        edges = []
        for f in range(T + 1):
            win = frame_samples(w_lo, f, hop, w_lo, w_hi)
            if (win < 0).any():
                edges.append(f)
                continue
            # a frame that stays inside the window: the span row the helper names reads exactly the same samples
            kind, row = cs.frame_source(s, f, lo_f, T)
            assert kind == "span" and 0 < row < n_rows - 1
            assert np.array_equal(frame_samples(span_lo, row, hop, span_lo, span_hi), win), (s, f)
        assert edges == cs.edge_frames(hop, T, N_FFT)
        brute_edges = edges
    shared = cs.shares_interior_frames(hop, N_FFT)
    assert shared == (brute_edges == [0, T]) == (2 * hop >= N_FFT)
    if shared:
        assert cs.frame_source(starts[1], 0, lo_f, T) == ("edge", 0) and cs.frame_source(starts[1], T, lo_f, T) == ("edge", 1)
    else:
        assert 1 in brute_edges and T - 1 in brute_edges          # hop 266: frames 1 and T - 1 reach into the padding too


def test_packed_columns_and_frame_counts():
    T = 256
    cols = [cs.packed_column_frame(c, T) for c in range(288)]
    assert cols[:T] == list(range(T)) and cols[T:T + 3] == [T - 2, T - 1, T] and set(cols[T + 3:]) == {-1}
    # 8 / 64 stride-1 windows: the span (both of its unread boundary rows included) + two edge frames a window
    assert cs.frames_computed(range(8), T, shared=False) == 8 * 257 and cs.frames_computed(range(8), T, shared=True) == 264 + 16
    assert cs.frames_computed(range(64), T, shared=False) == 64 * 257 and cs.frames_computed(range(64), T, shared=True) == 320 + 128
