"""The `basic` back end of a clip's emotion track (km_emotion_clip_create_basic, ClipEmotion(backend="basic")).

Which windows the rows come from is the closed form of tests/clip_emotion_cases.py (pinned on the host to the stream oracle); what
a row holds is checked BIT FOR BIT against a one-stream ``StreamEmotion(backend="basic")`` fed the clip in 1 600-sample chunks with
an update after every push, and against the dense path ``BasicEmotion()(window[None])[0]`` on the plan's window.  The track runs the
stream's kernels on the samples where they lie in the clip, so there is no tolerance anywhere in this file.  Parity with librosa is
UNPINNED, as for the whole basic back end (km_prosody.hip).

Small shape: context 1.0 s, interval 0.1 s -> R = 48 000, C = 16 000, U = 1 600, MIN = 8 000.  A 56 000-sample clip has K = 31 rows:
growing windows k = 0 .. 5 (8 000 and 9 600 samples are no multiple of the 512-sample frame hop), the stale oldest second up to
k = 24, sliding windows from k = 25 on.
"""
import functools

import numpy as np
import pytest
import torch

import clip_emotion_cases as cc
import stream_emotion_cases as ec
from koemorph_amd import _lib
from koemorph_amd._lib import KM_ERR_INVALID_ARG, KM_OK, KoeMorphError
from koemorph_amd.features import ClipEmotion
from koemorph_amd.features.basic_emotion import BasicEmotion
from koemorph_amd.streaming import StreamEmotion

pytestmark = pytest.mark.gpu

CTX, ITV, N, K_N = 1.0, 0.1, 56000, 31
GUARD = 7.25            # what the memory around an output holds before the call


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def clip(seed=2100, n=N) -> np.ndarray:
    x = (0.45 * np.concatenate([ec.speechlike(seed, 2.0), ec.speechlike(seed + 50, 2.0)]))[:n].astype(np.float32)
    assert x.shape == (n,)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def track(max_slots=5, seed=2100) -> np.ndarray:
    ce = ClipEmotion(CTX, ITV, max_slots=max_slots, backend="basic")
    assert ce.num_rows(N) == K_N and ce.emotion_dim == 9 and ce.compression_layer is None
    emotion, features = ce.build(dev(clip(seed)))
    assert features is None and emotion.shape == (K_N, 9)
    torch.cuda.synchronize()
    out = emotion.cpu().numpy()
    ce.close()
    out.setflags(write=False)
    return out


def stream_rows(x: np.ndarray, ctx: float, itv: float):
    """The clip through one basic StreamEmotion stream -> [(total samples, its row)] of every update that set ``updated``."""
    se = StreamEmotion(1, ctx, itv, backend="basic")
    g, out = cc.chunk(ctx, itv), []
    assert g == 1600
    for at in range(0, len(x) - g + 1, g):
        se.push(dev(x[None, at:at + g]))
        emotion, updated = se.update()
        if int(updated[0]):
            out.append((at + g, emotion[0].cpu().numpy().copy()))
    se.close()
    return out


# ---- 1: what a row holds --------------------------------------------------------------------------------------------------------
def test_rows_are_the_streams_bit_for_bit():
    got, stream, plan = track(), stream_rows(clip(), CTX, ITV), cc.plan(N, CTX, ITV)
    assert len(stream) == len(plan) == K_N
    for k, ((t, _, _), (t_stream, row)) in enumerate(zip(plan, stream)):
        assert t == t_stream, k
        assert np.array_equal(bits(got[k]), bits(row)), (k, got[k], row)


def test_rows_are_the_dense_path_on_the_closed_form_window_bit_for_bit():
    got, plan, be = track(), cc.plan(N, CTX, ITV), BasicEmotion()
    assert [length for _, _, length in plan[:6]] == [8000, 9600, 11200, 12800, 14400, 16000]
    assert plan[24] == (46400, 0, 16000) and plan[25] == (48000, 32000, 16000) and plan[30] == (56000, 40000, 16000)
    x = clip()
    for k, (_, start, length) in enumerate(plan):
        want = be(dev(x[start:start + length])[None])[0].cpu().numpy()
        assert np.array_equal(bits(got[k]), bits(want)), (k, start, length, got[k], want)
    be.close()
    assert np.isfinite(got).all()
    assert len({got[k].tobytes() for k in (0, 1, 2, 3, 4, 5, 25, 26, 30)}) == 9            # the windows differ, and so do their rows
    assert all(np.array_equal(bits(got[k]), bits(got[5])) for k in range(5, 25))          # the stale ones: one window
    assert (got[:, 0] > 0).all() and (got[:, 7] > got[:, 8]).all() and (got[:, 3] >= 50).all() and (got[:, 3] <= 400).all()


def test_passes_of_1_5_and_64_slots_give_equal_bits():
    """max_slots 1: one row per pass; 5: six full passes and one of a single row; 64: one pass with 33 empty slots."""
    assert np.array_equal(bits(track(1)), bits(track(5))) and np.array_equal(bits(track(64)), bits(track(5)))


# ---- 2: batches -----------------------------------------------------------------------------------------------------------------
def test_build_batch_equals_build_of_each_clip_and_a_second_batch_works():
    """Three clips at max_slots 4: 93 rows in 24 passes, most of which cross a clip boundary."""
    ce = ClipEmotion(CTX, ITV, max_slots=4, backend="basic")
    seeds = (2100, 2300, 2500)
    clips = dev(np.stack([clip(s) for s in seeds]))
    emotion, features = ce.build_batch(clips)
    assert features is None and emotion.shape == (3, K_N, 9)
    torch.cuda.synchronize()
    got = emotion.cpu().numpy()
    for c, s in enumerate(seeds):
        assert np.array_equal(bits(got[c]), bits(track(5, s))), c
    assert not np.array_equal(bits(got[0]), bits(got[1]))
    again, _ = ce.build_batch(clips.flip(0).contiguous())
    assert np.array_equal(bits(again.cpu().numpy()), bits(got[::-1]))
    one, _ = ce.build(clips[1])                                                   # and a single build after the batches
    assert np.array_equal(bits(one.cpu().numpy()), bits(got[1])) and ce.builds == 3
    ce.close()


# ---- 3: rows --------------------------------------------------------------------------------------------------------------------
def brute_row(s, T, hop, n):
    times = [t for t, _, _ in cc.plan(n, CTX, ITV)]
    e = min(n, (s + T) * hop)
    upto = [k for k, t in enumerate(times) if t <= e]
    return upto[-1] if upto else 0


def test_rows_gather_by_the_brute_force_mapping():
    T, hop = 32, 533
    ce = ClipEmotion(CTX, ITV, backend="basic")
    tr = torch.arange(K_N * 9, dtype=torch.float32, device="cuda").reshape(K_N, 9) + 0.5           # a row names itself
    last = N // hop - T
    assert (last + T) * hop <= N < (last + 1 + T) * hop
    cases = ([0, 1, 2, 9],                                                        # the starts of a first batch
             [last, 3, 40, 3, 0, last - 1, 17, 60, 41, 22, 5, 66, 30, 12, 59, 8, 35],     # unordered, a repeat, 17: a second workgroup
             [44],                                                                # B = 1
             [last + 1, last + 40, 2000])                                         # windows past clip_len: the last row
    seen = set()
    for starts in cases:
        want = [brute_row(s, T, hop, N) for s in starts]
        assert want == [cc.window_row(s, T, hop, N, CTX, ITV)[0] for s in starts]
        B = len(starts)
        buf = torch.full((B + 4, 9), GUARD, device="cuda")
        vbuf = torch.full((B + 32,), 77, dtype=torch.uint8, device="cuda")
        got = ce.rows(tr, N, dev(np.asarray(starts, np.int32)), hop, T, out=buf[2:2 + B], valid=vbuf[16:16 + B])
        assert got.shape == (B, 9) and torch.equal(got, tr[want]), (starts, want)
        assert (vbuf[16:16 + B] == 1).all()
        assert (buf[:2] == GUARD).all() and (buf[2 + B:] == GUARD).all()         # the guard rows around (B, 9)
        assert (vbuf[:16] == 77).all() and (vbuf[16 + B:] == 77).all()
        seen |= set(want)
    assert min(seen) == 5 and max(seen) == K_N - 1 and len(seen) > 10              # a 32-frame window ends after 17 056 samples at least
    assert brute_row(last + 40, T, hop, N) == K_N - 1 and brute_row(0, 4, hop, N) == 0
    got = ce.rows(tr, N, dev(np.asarray([0, 1, 20], np.int32)), hop, 4)           # windows that end before the first update
    assert torch.equal(got, tr[[0, 0, brute_row(20, 4, hop, N)]])
    ce.close()


def test_rows_inside_a_capture_replay_on_new_start_frames():
    T, hop, B = 32, 533, 20
    ce = ClipEmotion(CTX, ITV, backend="basic")
    tr = torch.arange(K_N * 9, dtype=torch.float32, device="cuda").reshape(K_N, 9) * 0.25
    starts = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(B, 9, device="cuda")
    valid = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ce.rows(tr, N, starts, hop, T, out=out, valid=valid)                          # one eager call before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ce.rows(tr, N, starts, hop, T, out=out, valid=valid)
    seen = set()
    for new in (list(range(20)), [72, 45, 30, 30, 9, 0, 21, 44, 3, 3, 70, 71, 72, 1, 2, 60, 50, 40, 10, 11], list(range(53, 73))):
        starts.copy_(dev(np.asarray(new, np.int32)))
        g.replay()
        torch.cuda.synchronize()
        want = [brute_row(s, T, hop, N) for s in new]
        assert torch.equal(out, tr[want]) and valid.all(), new
        seen |= set(want)
    assert len(seen) > 6
    ce.close()


# ---- 4: no rows, guards, memory, refusals ---------------------------------------------------------------------------------------
def test_a_clip_of_7999_samples_has_no_rows():
    ce = ClipEmotion(CTX, ITV, backend="basic")
    assert ce.num_rows(7999) == 0 and ce.num_rows(8000) == 1
    emotion, features = ce.build(dev(clip()[:7999]))
    assert emotion.shape == (0, 9) and features is None
    assert ce._lib.km_emotion_clip_build(ce._h, None, 7999, None, None, 0) == KM_OK          # nothing to launch, nothing to write
    out = torch.ones(3, 9, device="cuda")
    valid = torch.ones(3, dtype=torch.uint8, device="cuda")
    got = ce.rows(emotion, 7999, dev(np.asarray([0, 1, 7], np.int32)), 533, 4, out=out, valid=valid)
    assert got is out and not out.any() and not valid.any()
    ce.close()


def test_build_leaves_the_memory_around_the_track_alone():
    """Passes of 4 slots: the last one holds three rows and an empty slot whose row would lie right behind the track."""
    ce = ClipEmotion(CTX, ITV, max_slots=4, backend="basic")
    x = dev(clip())
    buf = torch.full((K_N + 8, 9), GUARD, device="cuda")
    assert ce._lib.km_emotion_clip_build(ce._h, x.data_ptr(), N, None, buf[4:].data_ptr(), stream_ptr()) == KM_OK
    torch.cuda.synchronize()
    assert (buf[:4] == GUARD).all() and (buf[4 + K_N:] == GUARD).all()
    assert np.array_equal(bits(buf[4:4 + K_N].cpu().numpy()), bits(track()))
    big = torch.full((2 * K_N + 8, 9), GUARD, device="cuda")                       # and around (B, K, 9): 62 rows, two empty slots
    clips = dev(np.stack([clip(), clip(2300)]))
    assert ce._lib.km_emotion_clip_build_batch(ce._h, clips.data_ptr(), 2, N, None, big[4:].data_ptr(), stream_ptr()) == KM_OK
    torch.cuda.synchronize()
    assert (big[:4] == GUARD).all() and (big[4 + 2 * K_N:] == GUARD).all()
    assert np.array_equal(bits(big[4:4 + K_N].cpu().numpy()), bits(track()))
    assert np.array_equal(bits(big[4 + K_N:4 + 2 * K_N].cpu().numpy()), bits(track(5, 2300)))
    ce.close()


def test_the_memory_counter_returns_to_its_baseline():
    live = _lib.load().km_live_device_bytes
    base = live()
    ce = ClipEmotion(CTX, ITV, max_slots=5, backend="basic")
    held = live() - base
    # the slot table, max_slots x (1 + C / 512) x 4 floats of frame records, and the prosody plan's tables (4 096 floats)
    assert held >= 5 * 16 + 5 * 32 * 4 * 4 + 4096 * 4, held
    assert held < 64 * 1024, held                                                  # no eGeMAPS scratch, no 256 x 264 weights
    tr, _ = ce.build(dev(clip()))
    ce.rows(tr, N, dev(np.asarray([0, 5], np.int32)), 533, 32)
    torch.cuda.synchronize()
    assert live() - base == held                                                   # build and rows allocate nothing
    ce.close()
    assert live() == base


def test_refusals():
    ce = ClipEmotion(CTX, ITV, backend="basic")
    eg = ClipEmotion(CTX, 0.3)
    lib = ce._lib
    assert lib.km_emotion_clip_width(ce._h) == 9 and lib.km_emotion_clip_width(eg._h) == 256
    w, b = torch.zeros(256, 264, device="cuda"), torch.zeros(256, device="cuda")
    assert lib.km_emotion_clip_set_compression(ce._h, w.data_ptr(), b.data_ptr(), stream_ptr()) == KM_ERR_INVALID_ARG
    assert b"the basic back end has no compression layer" in lib.km_last_error()
    x = dev(clip())
    out = torch.full((K_N, 9), GUARD, device="cuda")
    feats = torch.full((K_N, 88), GUARD, device="cuda")
    assert lib.km_emotion_clip_build(ce._h, x.data_ptr(), N, feats.data_ptr(), out.data_ptr(), stream_ptr()) == KM_ERR_INVALID_ARG
    assert b"features_out" in lib.km_last_error()
    assert lib.km_emotion_clip_build_batch(ce._h, x.data_ptr(), 1, N, feats.data_ptr(), out.data_ptr(), stream_ptr()) == KM_ERR_INVALID_ARG
    assert b"features_out" in lib.km_last_error()
    torch.cuda.synchronize()
    assert (out == GUARD).all() and (feats == GUARD).all()                         # refused before anything was launched
    for n in (2 ** 31, 2 ** 40):
        assert lib.km_emotion_clip_build(ce._h, x.data_ptr(), n, None, out.data_ptr(), 0) == KM_ERR_INVALID_ARG
    starts = dev(np.asarray([0, 1], np.int32))
    with pytest.raises(ValueError, match=r"\(K, 9\)"):                             # an eGeMAPS track handed to a basic object
        ce.rows(torch.zeros(K_N, 256, device="cuda"), N, starts, 533, 32)
    with pytest.raises(ValueError, match=r"\(K, 256\)"):                           # and the converse
        eg.rows(torch.zeros(eg.num_rows(N), 9, device="cuda"), N, starts, 533, 32)
    with pytest.raises(ValueError, match=r"\(2, 9\)"):
        ce.rows(torch.zeros(K_N, 9, device="cuda"), N, starts, 533, 32, out=torch.zeros(2, 256, device="cuda"))
    with pytest.raises(KoeMorphError, match="rows"):                               # a track of another clip length
        ce.rows(torch.zeros(K_N - 1, 9, device="cuda"), N, starts, 533, 32)
    with pytest.raises(ValueError, match="clip"):
        ce.build(torch.zeros(2, 9000, device="cuda"))
    ce.close()
    eg.close()


# ---- 5: the default shape -------------------------------------------------------------------------------------------------------
def test_default_shape_across_the_wrap_equals_the_stream():
    """Context 20 s, interval 0.3 s, a 23 s clip: R = 352 000 is crossed at row 72, K = 76 in two passes of 64 slots, windows of up
    to 320 000 samples (626 frames)."""
    n = 368000
    x = (0.5 * np.concatenate([ec.speechlike(1500 + 11 * k, 2.5) for k in range(10)])[:n]).astype(np.float32)
    assert x.shape == (n,)
    ce = ClipEmotion(backend="basic")
    assert ce.shape["ring_len"] == 352000 and ce.shape["max_frames"] == 626 and ce.num_rows(n) == 76
    emotion, _ = ce.build(dev(x))
    got = emotion.cpu().numpy()
    plan = cc.plan(n, 20.0, 0.3)
    assert (plan[71], plan[72], plan[75]) == ((348800, 0, 320000), (353600, 33600, 320000), (368000, 48000, 320000))
    stream = stream_rows(x, 20.0, 0.3)
    assert [t for t, _ in stream] == [t for t, _, _ in plan]
    for k, (_, row) in enumerate(stream):
        assert np.array_equal(bits(got[k]), bits(row)), (k, got[k], row)
    assert not np.array_equal(bits(got[71]), bits(got[72]))
    ce.close()
