"""Frame bookkeeping of the training step from a resident clip (km_train_step_clip), host only.

The windows of a dense batch start at multiples of the hop inside one clip: window ``b`` is samples
``[start[b] * hop, (start[b] + T) * hop)`` and its STFT frame ``f`` (centred, zero padded, ``f = 0 .. T``) covers the window's
samples ``[f * hop - n_fft / 2, f * hop + n_fft / 2)``.  A frame that stays inside the window reads clip samples only: it IS clip
frame ``start[b] + f`` and can be shared by every window that contains it.  A frame that leaves the window sees its zero
padding and belongs to that window alone (an "edge" frame).  With ``hop >= n_fft / 2`` the edge frames are exactly 0 and T;
below that frames 1 and T - 1 leave the window too, which is why the step supports only the former by default.

With option ``clip_assemble`` (km_clip_plan route 2) the step and the eval-mode forward run at every hop: E = ceil((n_fft / 2) / hop)
frames at either end of a window are edge frames (``edge_frames``), and they are computed from two snippets of the window, its
first and its last ``Ls = (2 E - 1) * hop`` samples, each a dense row of 2 E frames for the unchanged front end (``edge_source``):
window frame f < E is row f of the left snippet, window frame T - j (j < E) row 2 E - 1 - j of the right one.  Row k >= E of the
right snippet is centred at k * hop >= n_fft / 2 and sees no left padding; row k < E of the left one reaches sample
(E - 1) * hop + n_fft / 2 <= Ls and sees no right padding.  Frames E .. T - E come from the span image as before.
"""
from __future__ import annotations

from typing import List, Tuple


def shares_interior_frames(hop: int, n_fft: int = 1024) -> bool:
    """True when frames 0 and T are the only frames of a window that see its zero padding."""
    return 2 * hop >= n_fft


def edge_frames(hop: int, T: int, n_fft: int = 1024) -> List[int]:
    """Frames f in 0 .. T of a T * hop sample window whose n_fft samples are not all inside the window."""
    return [f for f in range(T + 1) if f * hop - n_fft // 2 < 0 or f * hop + n_fft // 2 > T * hop]


def n_span(min_start: int, max_start: int, T: int) -> int:
    """Rows of the span image: clip frames min_start .. max_start + T (its first and last row are boundary frames of the
    first / last window and are not read)."""
    return max_start - min_start + T + 1


def frame_source(start: int, f: int, min_start: int, T: int) -> Tuple[str, int]:
    """Where frame f of the window that starts at clip frame ``start`` comes from: ("edge", 0 | 1) for frames 0 and T,
    else ("span", row) with row = start - min_start + f."""
    if f == 0:
        return "edge", 0
    if f == T:
        return "edge", 1
    return "span", start - min_start + f


def packed_column_frame(col: int, T: int) -> int:
    """Window frame held by column ``col`` of a packed encoder row: T long frames, then the last three computed frames
    (T - 2, T - 1, T); -1 for the zero columns up to the padded width."""
    if col < T:
        return col
    return col - 2 if col < T + 3 else -1


def frames_computed(starts, T: int, shared: bool) -> int:
    """STFT frames the front end computes for one batch: every window's T + 1 frames, or the span + 2 edge frames a window."""
    starts = [int(s) for s in starts]
    if not shared:
        return len(starts) * (T + 1)
    return n_span(min(starts), max(starts), T) + 2 * len(starts)


def edges_per_side(hop: int, n_fft: int = 1024) -> int:
    """E: the frames at either end of a window that see its zero padding."""
    return -(-(n_fft // 2) // hop)


def snippet_samples(hop: int, E: int) -> int:
    """Ls: samples of the left / right snippet of a window, 2 E frames each."""
    return (2 * E - 1) * hop


def edge_source(f: int, T: int, E: int) -> Tuple[str, int]:
    """Where frame f of a window comes from on the assembled route: ("left", row) / ("right", row) of the window's 2 E-row
    snippet images, or ("span", f): row start - min_start + f of the span image.  Needs T + 1 >= 2 E."""
    if f < E:
        return "left", f
    if f > T - E:
        return "right", 2 * E - 1 - (T - f)
    return "span", f


def frames_computed_edges(starts, T: int, E: int) -> int:
    """STFT frames the front end computes for one batch on the assembled route: the span + two snippets of 2 E frames a window."""
    starts = [int(s) for s in starts]
    return n_span(min(starts), max(starts), T) + 4 * E * len(starts)
