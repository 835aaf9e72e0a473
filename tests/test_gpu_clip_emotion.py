"""The emotion track of a resident clip (km_emotion_clip_*, koemorph_amd.features.ClipEmotion).

Which windows the rows come from is the closed form of tests/clip_emotion_cases.py, pinned on the host to the stream oracle
(tests/test_clip_emotion_host.py).  What a row holds is checked BIT FOR BIT: against a one-stream ``StreamEmotion`` fed the clip in
1 600-sample chunks with an update after every push, and against the pinned B = 1 path ``EGeMAPSEngine.functionals(window[None])[0]``
on the plan's window -- the track runs the stream's kernels on the samples where they lie in the clip, so a frame's arithmetic is
the same code and no tolerance is needed or given.  The 264 -> 256 product alone has a bound, the project's own for it
(tests/test_gpu_stream_emotion.py): |got - exact| <= 265 * 2^-24 * (|W| . |x| + |b|) per output, derived, not measured.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import clip_emotion_cases as cc
import stream_emotion_cases as ec
from koemorph_amd._lib import KM_ERR_INVALID_ARG, KM_OK, KoeMorphError
from koemorph_amd.features import ClipEmotion
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine
from koemorph_amd.streaming import StreamEmotion

pytestmark = pytest.mark.gpu

N_A, CTX_A, ITV_A = 64777, 1.0, 0.3          # clip A: K = 12, two growing windows, seven stale ones, three after the wrap


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def layer():
    torch.manual_seed(4321)
    return torch.nn.Linear(264, 256)


@functools.lru_cache(maxsize=None)
def egemaps():
    return EGeMAPSEngine("cuda")


def reference(window: np.ndarray) -> np.ndarray:
    f = egemaps().functionals(dev(window)[None])[0].cpu().numpy()
    return np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def clip_a() -> np.ndarray:
    x = (0.45 * ec.speechlike(1300, 4.2))[:N_A].astype(np.float32)
    assert x.shape == (N_A,)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def track_a(max_slots=16):
    ce = ClipEmotion(CTX_A, ITV_A, max_slots=max_slots, compression_layer=layer())
    assert ce.num_rows(N_A) == 12
    emotion, features = ce.build(dev(clip_a()))
    torch.cuda.synchronize()
    out = emotion.cpu().numpy(), features.cpu().numpy()
    ce.close()
    return out


@functools.lru_cache(maxsize=None)
def stream_a():
    """Clip A through one StreamEmotion stream -> [(total samples, features, emotion row)] of every update that set ``updated``."""
    se = StreamEmotion(1, CTX_A, ITV_A, compression_layer=layer())
    g = cc.chunk(CTX_A, ITV_A)
    assert g == 1600
    x, out = clip_a(), []
    for at in range(0, N_A, g):
        se.push(dev(x[None, at:at + g]))
        emotion, updated = se.update()
        if int(updated[0]):
            out.append((min(at + g, N_A), se.features[0].cpu().numpy(), emotion[0].cpu().numpy().copy()))
    se.close()
    return out


# ---- 1: features ----------------------------------------------------------------------------------------------------------------
def test_features_are_the_streams_and_the_pinned_path_bit_for_bit():
    _, features = track_a()
    plan, stream = cc.plan(N_A, CTX_A, ITV_A), stream_a()
    assert features.shape == (12, 88) and len(stream) == len(plan) == 12
    assert [length for _, _, length in plan[:2]] == [8000, 12800]
    for k, ((t, start, length), (t_stream, f_stream, _)) in enumerate(zip(plan, stream)):
        assert t == t_stream, k
        assert np.array_equal(bits(features[k]), bits(f_stream)), (k, float(np.abs(features[k] - f_stream).max()))
        ref = reference(clip_a()[start:start + length])
        assert np.array_equal(bits(features[k]), bits(ref)), (k, start, length, float(np.abs(features[k] - ref).max()))
    assert len({features[k].tobytes() for k in (0, 1, 2, 9, 10, 11)}) == 6       # the windows differ, and so do their rows
    assert all(np.array_equal(bits(features[k]), bits(features[2])) for k in range(2, 9))     # the stale ones: one window


# ---- 2: the 264 -> 256 product --------------------------------------------------------------------------------------------------
def test_emotion_rows_use_the_first_features_in_both_slots():
    emotion, features = track_a()
    W = layer().weight.detach().numpy().astype(np.float64)
    b = layer().bias.detach().numpy().astype(np.float64)
    worst = worst_stream = 0.0
    for k, (_, _, e_stream) in enumerate(stream_a()):
        x = np.concatenate([features[k], features[0], features[0]]).astype(np.float64)
        exact = W @ x + b
        bound = 265 * 2.0 ** -24 * (np.abs(W) @ np.abs(x) + np.abs(b))
        err = np.abs(emotion[k].astype(np.float64) - exact)
        err_stream = np.abs(emotion[k].astype(np.float64) - e_stream.astype(np.float64))
        worst, worst_stream = max(worst, float((err / bound).max())), max(worst_stream, float((err_stream / bound).max()))
        assert (err <= bound).all(), (k, float((err / bound).max()))
        assert (err_stream <= bound).all(), (k, float((err_stream / bound).max()))
        assert np.array_equal(bits(emotion[k]), bits(e_stream)), k       # one summation order in both kernels: the same bits
    print(f"clip A: worst error / bound = {worst:.3f} against float64, {worst_stream:.3f} against the stream")
    # the slots matter: with the row's own features in them the rows after the first would be somewhere else
    x_wrong = np.concatenate([features[11]] * 3).astype(np.float64)
    assert np.abs(W @ x_wrong + b - emotion[11]).max() > 1e-3


# ---- 3: passes ------------------------------------------------------------------------------------------------------------------
def test_three_passes_equal_one_pass_bit_for_bit():
    """max_slots 5: rows 0-4, 5-9 and 10-11 with three empty slots; features[0] reaches the later passes from pass 0."""
    (e5, f5), (e16, f16) = track_a(5), track_a()
    assert np.array_equal(bits(f5), bits(f16)) and np.array_equal(bits(e5), bits(e16))
    e1, f1 = track_a(1)                                     # one row per pass
    assert np.array_equal(bits(f1), bits(f16)) and np.array_equal(bits(e1), bits(e16))


def test_build_without_features_out_and_rebuild_of_another_clip():
    """features_out NULL gives the same emotion rows; a second clip on the same object does not see the first clip's features[0]."""
    ce = ClipEmotion(CTX_A, ITV_A, max_slots=5, compression_layer=layer())
    clip = dev(clip_a())
    other = dev(0.3 * ec.speechlike(1400, 1.5))
    ce.build(other)
    emotion = torch.empty(12, 256, device="cuda")
    rc = ce._lib.km_emotion_clip_build(ce._h, clip.data_ptr(), N_A, None, emotion.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == KM_OK
    torch.cuda.synchronize()
    assert np.array_equal(bits(emotion.cpu().numpy()), bits(track_a()[0]))
    ce.close()


def test_one_row_per_pass_without_features_out():
    """max_slots 1 and features_out NULL: every pass after the first takes features[0] from the object's own buffer."""
    ce = ClipEmotion(CTX_A, ITV_A, max_slots=1, compression_layer=layer())
    clip, emotion = dev(clip_a()), torch.empty(12, 256, device="cuda")
    rc = ce._lib.km_emotion_clip_build(ce._h, clip.data_ptr(), N_A, None, emotion.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == KM_OK
    torch.cuda.synchronize()
    assert np.array_equal(bits(emotion.cpu().numpy()), bits(track_a()[0]))
    ce.close()


# ---- 4: rows --------------------------------------------------------------------------------------------------------------------
def test_rows_gather_by_the_host_mapping():
    n, T, hop = 160000, 256, 533
    ce = ClipEmotion(CTX_A, ITV_A, compression_layer=layer())
    K = ce.num_rows(n)
    assert K == cc.num_rows(n, CTX_A, ITV_A) == 32
    track = torch.arange(K * 256, dtype=torch.float32, device="cuda").reshape(K, 256) + 0.5       # a row names itself
    last = n // hop - T
    starts = [0, 3, 3, last, last + 1]
    assert (last + T) * hop <= n < (last + 1 + T) * hop
    want = [cc.window_row(s, T, hop, n, CTX_A, ITV_A)[0] for s in starts]
    assert want[-1] == K - 1 and want[0] < want[-1]
    valid = torch.zeros(len(starts), dtype=torch.uint8, device="cuda")
    got = ce.rows(track, n, dev(np.asarray(starts, np.int32)), hop, T, valid=valid)
    assert torch.equal(got, track[want]) and valid.cpu().tolist() == [1] * len(starts)
    # windows that end before the first update, a negative start, hop 266
    starts2 = [0, 1, -5, 20, 300, 601]
    got2 = ce.rows(track, n, dev(np.asarray(starts2, np.int32)), 266, 4)
    want2 = [cc.window_row(s, 4, 266, n, CTX_A, ITV_A)[0] for s in starts2]
    assert want2[:3] == [0, 0, 0] and want2[-1] == K - 1
    assert torch.equal(got2, track[want2])
    with pytest.raises(KoeMorphError, match="rows"):                       # a track of another clip length
        ce.rows(track[:K - 1], n, dev(np.asarray(starts, np.int32)), hop, T)
    ce.close()


def test_a_clip_shorter_than_half_a_second_has_no_rows():
    n = 6400
    ce = ClipEmotion(CTX_A, ITV_A, compression_layer=layer())
    assert ce.num_rows(n) == 0 and ce.num_rows(7999) == 0 and ce.num_rows(8000) == 1
    emotion, features = ce.build(dev(clip_a()[:n]))
    assert emotion.shape == (0, 256) and features.shape == (0, 88)
    assert ce._lib.km_emotion_clip_build(ce._h, None, n, None, None, 0) == KM_OK            # nothing to launch, nothing to write
    out = torch.ones(3, 256, device="cuda")
    valid = torch.ones(3, dtype=torch.uint8, device="cuda")
    got = ce.rows(emotion, n, dev(np.asarray([0, 1, 7], np.int32)), 533, 4, out=out, valid=valid)
    assert got is out and not out.any() and not valid.any()
    ce.close()


def test_refusals():
    ce = ClipEmotion(CTX_A, ITV_A, compression_layer=layer())
    lib = ce._lib
    x = torch.zeros(16, device="cuda")
    for n in (2 ** 31, 2 ** 31 + 5, 2 ** 40):                            # window starts are 32-bit; refused before anything is read
        assert lib.km_emotion_clip_build(ce._h, x.data_ptr(), n, None, x.data_ptr(), 0) == KM_ERR_INVALID_ARG
    h = C.c_void_p()
    for args in ((1.0, 0.3, 0), (1.0, 0.05, 4), (0.5, 0.3, 4), (1.0, 1.5, 4), (20.6, 0.3, 4)):
        assert lib.km_emotion_clip_create(C.byref(h), *args) != 0 and not h.value, args
    with pytest.raises(ValueError, match="at most 2048"):
        ClipEmotion(context_window=20.6)
    with pytest.raises(ValueError, match="Linear"):
        ClipEmotion(CTX_A, ITV_A, compression_layer=torch.nn.Linear(88, 256))
    with pytest.raises(ValueError, match="clip"):
        ce.build(torch.zeros(2, 9000, device="cuda"))
    ce.close()


# ---- 5: the default shape -------------------------------------------------------------------------------------------------------
def test_default_shape_across_the_wrap():
    """Context 20 s, a 23.01 s clip: R = 352 000 is crossed, K = 76 in two passes of 64 slots, windows of up to 1 995 frames."""
    n = 368160
    audio = (0.5 * np.concatenate([ec.speechlike(1500 + 11 * k, 2.5) for k in range(10)])[:n]).astype(np.float32)
    assert audio.shape == (n,)
    ce = ClipEmotion(compression_layer=layer())
    assert ce.shape["ring_len"] == 352000 and ce.num_rows(n) == 76
    _, features = ce.build(dev(audio))
    features = features.cpu().numpy()
    plan = cc.plan(n, 20.0, 0.3)
    k_before = max(k for k, (t, _, _) in enumerate(plan) if t < 352000)
    assert (k_before, plan[k_before], plan[k_before + 1], plan[75]) == (71, (348800, 0, 320000), (353600, 33600, 320000), (368000, 48000, 320000))
    for k in (0, k_before, k_before + 1, 75):
        _, start, length = plan[k]
        ref = reference(audio[start:start + length])
        assert np.array_equal(bits(features[k]), bits(ref)), (k, float(np.abs(features[k] - ref).max()))
    ce.close()


# ---- 6: graph replay ------------------------------------------------------------------------------------------------------------
def test_rows_inside_a_capture_replay_on_new_start_frames():
    n, T, hop, B = 160000, 256, 533, 8
    ce = ClipEmotion(CTX_A, ITV_A, compression_layer=layer())
    K = ce.num_rows(n)
    track = torch.arange(K * 256, dtype=torch.float32, device="cuda").reshape(K, 256) * 0.25
    starts = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(B, 256, device="cuda")
    valid = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ce.rows(track, n, starts, hop, T, out=out, valid=valid)               # one eager call before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ce.rows(track, n, starts, hop, T, out=out, valid=valid)
    seen = set()
    for new in ([0, 1, 2, 3, 4, 5, 6, 7], [44, 45, 30, 30, 9, 0, 21, 44], [37, 38, 39, 40, 41, 42, 43, 44]):
        starts.copy_(dev(np.asarray(new, np.int32)))
        g.replay()
        twin = ce.rows(track, n, starts, hop, T)
        torch.cuda.synchronize()
        assert torch.equal(out, twin) and valid.all()
        want = [cc.window_row(s, T, hop, n, CTX_A, ITV_A)[0] for s in new]
        assert torch.equal(out, track[want])
        seen |= set(want)
    assert len(seen) > 2
    ce.close()
