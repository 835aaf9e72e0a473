"""Sequence mode with an emotion track (km_sequence_forward_track): the window -> row mapping and the refusals, on the host.

``koemorph_amd.engine.sequence_track_row`` restates the kernel's closed form with the arguments the C call takes.  It is pinned
here to ``clip_emotion_cases.window_row`` -- the mapping ``ClipEmotion.rows`` implements, itself pinned to the stream oracle in
tests/test_clip_emotion_host.py -- for whole clips and for the chunks ``parallel.sequence_chunk`` hands the ranks.  The GPU tests
(tests/test_gpu_sequence_track.py) then hold the kernel to the rows this function names.
"""
import ctypes as C

import pytest

import clip_emotion_cases as cc
from koemorph_amd import _lib, parallel
from koemorph_amd._lib import KM_ERR_INVALID_ARG
from koemorph_amd.engine import Engine, sequence_track_row

HOP, T = 533, 256
SHAPES = [(20.0, 0.3), (1.0, 0.3), (5.0, 0.7)]
LENGTHS = [136448 + 533 * 20 + 100, 136448 + 533 * 9 + 100, 136448 - 533 * 40 + 100, 136448, 8000, 12799, 12800, 400000]


def num_outputs(L, stride):
    return max(1, (L // HOP - T) // stride + 1)


@pytest.mark.parametrize("ctx,itv", SHAPES)
@pytest.mark.parametrize("stride", [1, 2, 7])
def test_row_of_a_window_is_clip_emotions_row_for_its_start_frame(ctx, itv, stride):
    sh = cc.shape(ctx, itv)
    for L in LENGTHS:
        K = cc.num_rows(L, ctx, itv)
        assert K >= 1
        for i in range(num_outputs(L, stride)):
            want, valid = cc.window_row(i * stride, T, HOP, L, ctx, itv)
            assert valid == 1
            assert sequence_track_row(i, K, sh["MIN"], sh["U"], 0, L, stride, T, HOP) == want, (L, i)


def test_rows_at_twenty_extra_hops_and_the_clamp():
    """K = 30 and 21 windows on rows 26 x 3, 27 x 9, 28 x 9; the single zero-padded window of a short clip lands on K - 1."""
    L = 136448 + 533 * 20 + 100
    assert cc.num_rows(L, 20.0, 0.3) == 30 and num_outputs(L, 1) == 21
    rows = [sequence_track_row(i, 30, 8000, 4800, 0, L, 1, T, HOP) for i in range(21)]
    assert rows == [26] * 3 + [27] * 9 + [28] * 9
    L = 136448 - 533 * 40 + 100
    assert cc.num_rows(L, 20.0, 0.3) == 23 and num_outputs(L, 1) == 1
    assert sequence_track_row(0, 23, 8000, 4800, 0, L, 1, T, HOP) == 22


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("stride", [1, 2])
def test_a_chunk_maps_as_the_whole_clip_does(world, stride):
    ctx, itv = 20.0, 0.3
    sh = cc.shape(ctx, itv)
    for L in (136448 + 533 * 20 + 100, 136448 + 533 * 9 + 100, 400000, 136448 - 533 * 40 + 100):
        K, N = cc.num_rows(L, ctx, itv), num_outputs(L, stride)
        seen = 0
        for rank in range(world):
            lo, hi, s0, s1 = parallel.sequence_chunk(L, HOP, T, stride, N, rank, world)
            if hi <= lo:
                continue
            assert 0 <= s0 and s1 <= L and num_outputs(s1 - s0, stride) == hi - lo
            for j in range(hi - lo):
                want, _ = cc.window_row((lo + j) * stride, T, HOP, L, ctx, itv)
                assert sequence_track_row(j, K, sh["MIN"], sh["U"], s0, L, stride, T, HOP) == want, (L, rank, j)
            seen += hi - lo
        assert seen == N
    # the offsets matter: the last rank's windows, mapped as if the chunk were the clip, land on other rows
    L = 400000
    N = num_outputs(L, 1)
    lo, hi, s0, s1 = parallel.sequence_chunk(L, HOP, T, 1, N, world - 1, world)
    K = cc.num_rows(L, ctx, itv)
    with_off = [sequence_track_row(j, K, sh["MIN"], sh["U"], s0, L, 1, T, HOP) for j in range(hi - lo)]
    without = [sequence_track_row(j, K, sh["MIN"], sh["U"], 0, s1 - s0, 1, T, HOP) for j in range(hi - lo)]
    assert with_off != without


def test_identity_mapping_is_one_row_per_window():
    for stride in (1, 3):
        L = 136448 + 533 * 12 + 5
        N = num_outputs(L, stride)
        rows = [sequence_track_row(i, N, T * HOP, stride * HOP, 0, L, stride, T, HOP) for i in range(N)]
        assert rows == list(range(N))
    # the single zero-padded window ends with the clip, before T * hop: row 0
    assert sequence_track_row(0, 1, T * HOP, HOP, 0, 100000, 1, T, HOP) == 0


def test_c_call_refuses_bad_track_arguments_before_anything_else():
    """The argument checks come before the handle's state is looked at, so they hold on a handle that was never finalized (and on
    a machine without a GPU): the pointers are never dereferenced."""
    lib = _lib.load()
    eng = Engine()
    buf = (C.c_float * 4)()
    p = C.addressof(buf)
    L = 150000

    def call(K=30, first=8000, interval=4800, offset=0, clip_len=L, B=2, audio=p, track=p, out=p, stride=1):
        return lib.km_sequence_forward_track(eng._h, audio, B, L, track, K, first, interval, offset, clip_len, stride, 1, out, None)

    assert call(K=0) == KM_ERR_INVALID_ARG and b"K 0" in lib.km_last_error()
    assert call(K=-3) == KM_ERR_INVALID_ARG
    assert call(interval=0) == KM_ERR_INVALID_ARG
    assert call(first=-1) == KM_ERR_INVALID_ARG
    assert call(offset=-1) == KM_ERR_INVALID_ARG
    assert call(clip_len=L - 1) == KM_ERR_INVALID_ARG
    assert call(offset=1) == KM_ERR_INVALID_ARG                       # clip_len < sample_offset + L
    assert call(offset=1, clip_len=L + 1) != KM_ERR_INVALID_ARG
    assert call(K=2 ** 31) == KM_ERR_INVALID_ARG                      # B * K beyond 2^31 - 1 rows
    assert call(K=2 ** 30, B=2) == KM_ERR_INVALID_ARG
    assert call(track=None) == KM_ERR_INVALID_ARG and call(audio=None) == KM_ERR_INVALID_ARG and call(out=None) == KM_ERR_INVALID_ARG
    assert call(stride=0) == KM_ERR_INVALID_ARG and call(B=0) == KM_ERR_INVALID_ARG
    # good arguments get as far as the handle: not finalized
    assert call() == _lib.KM_ERR_NOT_FINALIZED
    eng.close()


class _FakeClipEmotion:
    shape = dict(min_samples=8000, update_samples=4800)


def test_python_surface_refusals():
    import torch
    from koemorph_amd.model import SequentialDualStreamModel
    with pytest.raises(ValueError, match="clip_emotion and emotion_provider"):
        SequentialDualStreamModel(clip_emotion=_FakeClipEmotion(), emotion_provider=lambda a: a)
    m = SequentialDualStreamModel(clip_emotion=_FakeClipEmotion())
    audio = torch.zeros(1, 140000)
    with pytest.raises(ValueError, match="emotion_track and emotion_features"):
        m.forward(audio, emotion_features=torch.zeros(1, 256), emotion_track=torch.zeros(1, 3, 256))
    with pytest.raises(ValueError, match="clip_emotion"):
        SequentialDualStreamModel().forward(audio, emotion_track=torch.zeros(1, 3, 256))
    with pytest.raises(ValueError, match="emotion_track"):
        m.forward(audio, emotion_track=torch.zeros(2, 3, 256))       # one track per clip
    with pytest.raises(ValueError, match="track_shape"):
        parallel.sequence_apply(None, audio, None, emotion_track=torch.zeros(1, 3, 256))
    with pytest.raises(ValueError, match="pass one of them"):
        parallel.sequence_apply(None, audio, torch.zeros(1, 256), emotion_track=torch.zeros(1, 3, 256), track_shape=(8000, 4800))
