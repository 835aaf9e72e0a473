"""The emotion objects at the GeMAPS feature set (``feature_set="GeMAPS"``: km_emotion_stream_create_set,
km_emotion_clip_create_set), the producers of the ``fast`` variant's emotion input.

The oracle is the TWIN (tests/gemaps_cases.py): an eGeMAPS object -- pinned by tests/test_gpu_stream_emotion.py,
tests/test_gpu_clip_emotion.py and tests/test_gpu_emotion_long.py -- whose Linear(264, 256) holds the GeMAPS object's Linear(186, 256)
in the kept columns and 0.0 elsewhere.  On the same calls the two give EQUAL ``updated`` / ``valid``, EQUAL EMOTION BITS, and the
GeMAPS object's features and slots are the twin's at GEMAPS_COLUMNS, bit for bit.  km_live_device_bytes() is back at its baseline
after every object.
"""
import functools

import numpy as np
import pytest
import torch

import clip_emotion_cases as cc
import egemaps_cases as egc
import gemaps_cases as gc
from koemorph_amd import _lib
from koemorph_amd.features import ClipEmotion
from koemorph_amd.streaming import StreamEmotion, emotion_stream_shape

pytestmark = pytest.mark.gpu

SR = 16000
GM = "GeMAPS"
CTX, ITV = 1.0, 0.1                         # a 3 s ring, windows of 95 frames, an update every 1600 samples
CHUNK = 4000
COLS = gc.COLS


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def live():
    torch.cuda.synchronize()
    return int(_lib.load().km_live_device_bytes())


@functools.lru_cache(maxsize=None)
def twin_layer():
    return gc.scatter_compression(gc.l186())


@functools.lru_cache(maxsize=None)
def speech(seed: int, seconds: float) -> np.ndarray:
    """Speech-like audio in 2.5 s phrases of different voices (tests/test_gpu_emotion_long.py)."""
    n = int(seconds * SR)
    x = np.concatenate([egc.speechlike(seed + 3 * k, 2.5) * (0.3 + 0.1 * (k % 5)) for k in range(n // 40000 + 1)])[:n].astype(np.float32)
    x.setflags(write=False)
    return x


def pair(n, ctx, itv, **kw):
    """A GeMAPS object and its eGeMAPS twin."""
    return (StreamEmotion(n, ctx, itv, compression_layer=gc.l186(), feature_set=GM, **kw),
            StreamEmotion(n, ctx, itv, compression_layer=twin_layer(), **kw))


def check_pair(se, tw, what):
    torch.cuda.synchronize()
    assert torch.equal(se.updated, tw.updated) and torch.equal(se.valid, tw.valid), what
    assert gc.same_bits(se.emotion, tw.emotion), (what, (se.emotion != tw.emotion).nonzero()[:6].tolist())
    assert gc.same_bits(se.features, tw.features[:, COLS]), what
    assert gc.same_bits(se.slots, tw.slots[:, :, COLS]), what


# ---- streams ----------------------------------------------------------------------------------------------------------
def schedule():
    """[(samples (3, CHUNK), counts (3), reset mask or None)] over 18 pushes of 0.25 s: stream 0 runs through (growing windows, a full
    one after 1 s, a wrapped ring after 3 s) and is reset at push 13; stream 1 joins at push 4 and brings odd counts; stream 2 pauses
    for pushes 6-9."""
    audio = [speech(700 + 50 * s, 5.0) for s in range(3)]
    at = [0, 0, 0]
    out = []
    for t in range(18):
        cnt = [CHUNK, 0 if t < 4 else CHUNK - 37 * (t % 3), 0 if 6 <= t <= 9 else CHUNK]
        x = np.zeros((3, CHUNK), np.float32)
        for s in range(3):
            x[s, :cnt[s]] = audio[s][at[s]:at[s] + cnt[s]]
            at[s] += cnt[s]
        out.append((x, np.asarray(cnt, np.int32), np.array([True, False, False]) if t == 13 else None))
    return out


@pytest.mark.parametrize("max_updates", [None, 1])
def test_streams_equal_their_twin_on_every_step(max_updates):
    base = live()
    se, tw = pair(3, CTX, ITV, max_updates=max_updates)
    assert se.feature_dim == 62 and tw.feature_dim == 88 and se.emotion_dim == 256 and se.shape == tw.shape == emotion_stream_shape(CTX, ITV)
    assert se.shape["ring_len"] == 48000 and se.shape["max_frames"] == 95
    lib = _lib.load()
    assert lib.km_emotion_stream_feature_width(se._h) == 62 and lib.km_emotion_stream_feature_width(tw._h) == 88
    assert se.features.shape == (3, 62) and se.slots.shape == (3, 2, 62)
    seen = np.zeros(3, int)
    for t, (x, cnt, mask) in enumerate(schedule()):
        for o in (se, tw):
            if mask is not None:
                o.reset_streams(dev(mask))
            o.push(dev(x), dev(cnt))
            o.update()
        check_pair(se, tw, t)
        seen += se.updated.cpu().numpy()
        if mask is not None:                                          # the reset stream starts a new life: its slots are refilled
            assert gc.same_bits(se.slots[0, 0], se.features[0])
    assert (seen >= (3 if max_updates else 8)).all(), seen          # every stream was served, again and again
    assert bool(se.features.any()) and bool((se.emotion != 0).all())
    for o in (se, tw):
        o.close()
    assert live() == base


def test_capture_and_replay_equal_an_eager_twin():
    base = live()
    se, tw = pair(3, CTX, ITV)
    for t, (x, cnt, mask) in enumerate(schedule()):
        if mask is not None:
            se.reset_streams(dev(mask)); tw.reset_streams(dev(mask))
        tw.push(dev(x), dev(cnt))
        tw.update()
        if t == 0:
            se.push(dev(x), dev(cnt))
            se.update()
        else:
            if t == 1:
                se.capture(CHUNK)
            se.replay(dev(x), dev(cnt))
        check_pair(se, tw, t)
    for o in (se, tw):
        o.close()
    assert live() == base


def one_update(ctx, itv, seconds, push, frames, **kw):
    base = live()
    se, tw = pair(2, ctx, itv, **kw)
    assert se.shape["max_frames"] == frames
    audio = [speech(900 + 10 * s, seconds) for s in range(2)]
    for at in range(0, int(seconds * SR), push):
        x = np.stack([a[at:at + push] for a in audio])
        for o in (se, tw):
            o.push(dev(x))
    for o in (se, tw):
        o.update()
    check_pair(se, tw, (ctx, itv))
    assert list(se.updated.cpu().numpy()) == [1, 1] and int((se.features[0] != 0).sum()) >= 56
    for o in (se, tw):
        o.close()
    assert live() == base


def test_one_update_at_the_fast_timing():
    """10 s / 0.5 s: 13 s of audio wrap the 12 s ring; the window is full, 995 frames."""
    one_update(10.0, 0.5, 13.0, 52000, 995)


def test_one_update_with_long_windows():
    """21 s / 0.3 s with long_windows: 2095 frames, the long tier of the per-window kernels."""
    one_update(21.0, 0.3, 22.0, 176000, 2095, long_windows=True)


def test_python_refusals_on_the_device():
    with pytest.raises(ValueError, match=r"compression_layer must be a Linear\(186, 256\), got weight \(256, 264\)"):
        StreamEmotion(2, CTX, ITV, compression_layer=twin_layer(), feature_set=GM)
    with pytest.raises(ValueError, match=r"compression_layer must be a Linear\(186, 256\), got weight \(256, 264\)"):
        ClipEmotion(CTX, ITV, compression_layer=twin_layer(), feature_set=GM)
    with pytest.raises(ValueError, match=r"compression_layer must be a Linear\(264, 256\), got weight \(256, 186\)"):
        StreamEmotion(2, CTX, ITV, compression_layer=gc.l186())
    with pytest.raises(ValueError, match=r"2095 frames per window, at most 2048 \(20\.5 s\)"):
        StreamEmotion(2, 21.0, 0.3, feature_set=GM)


def test_the_extractor_mirror_at_gemaps():
    from koemorph_amd.egemaps_names import GEMAPS_FEATURE_NAMES
    from koemorph_amd.features.opensmile_extractor import create_opensmile_extractor
    cfg = dict(context_window=10.0, update_interval=0.5, device="cuda", use_concatenation=True)
    ex = create_opensmile_extractor({**cfg, "feature_set": GM})
    full = create_opensmile_extractor(cfg)
    assert ex.feature_dim == 62 and ex.get_feature_names() == GEMAPS_FEATURE_NAMES and ex.get_stats()["feature_dim"] == 62
    x = speech(900, 13.0)[:3 * SR]
    f, f88 = ex.process_audio_frame(x, force_update=True), full.process_audio_frame(x, force_update=True)
    assert f.shape == (62,) and gc.same_bits(f, f88[COLS])
    ex.compression_layer, full.compression_layer = gc.l186(), twin_layer()
    e, e88 = ex.get_concatenated_features(), full.get_concatenated_features()
    # km_linear at K = 186 and at K = 264 with 78 zero weights: each within (K + 2) 2^-24 (|W| |x| + |b|) of the one exact product
    W, bias = gc.l186().weight.detach().numpy().astype(np.float64), gc.l186().bias.detach().numpy().astype(np.float64)
    bound = (188 + 266) * 2.0 ** -24 * (np.abs(W) @ np.abs(np.tile(f, 3).astype(np.float64)) + np.abs(bias))
    assert e.shape == (256,) and (np.abs(e.astype(np.float64) - e88) <= bound).all()
    batch = dev(np.stack([x, speech(910, 13.0)[:3 * SR]]))
    assert ex.emotion_features_batch(batch).shape == (2, 256)
    ex.compression_layer = twin_layer()
    with pytest.raises(ValueError, match=r"Linear\(186, 256\)"):
        ex.get_concatenated_features()


# ---- clips ------------------------------------------------------------------------------------------------------------
CLIP_N = 40000                              # 2.5 s: 21 rows, 6 passes of 4 slots


def clip_pair(ctx, itv, max_slots, **kw):
    return (ClipEmotion(ctx, itv, max_slots=max_slots, compression_layer=gc.l186(), feature_set=GM, **kw),
            ClipEmotion(ctx, itv, max_slots=max_slots, compression_layer=twin_layer(), **kw))


@functools.lru_cache(maxsize=None)
def track(max_slots=4):
    """(emotion (21, 256), features (21, 62)) of the 2.5 s clip, checked against the twin on the way."""
    base = live()
    ce, tw = clip_pair(CTX, ITV, max_slots)
    clip = dev(speech(300, 2.5))
    assert clip.shape[0] == CLIP_N and ce.num_rows(CLIP_N) == cc.num_rows(CLIP_N, CTX, ITV) == 21 and ce.feature_dim == 62
    assert _lib.load().km_emotion_clip_feature_width(ce._h) == 62 and _lib.load().km_emotion_clip_feature_width(tw._h) == 88
    emotion, features = ce.build(clip)
    emotion_t, features_t = tw.build(clip)
    assert features.shape == (21, 62) and emotion.shape == (21, 256)
    assert gc.same_bits(emotion, emotion_t) and gc.same_bits(features, features_t[:, COLS])
    # rows: the same gather as the twin's
    starts = torch.tensor([0, 1, 20, 37, 60, 74, 75, 90], dtype=torch.int32, device="cuda")
    got = ce.rows(emotion, CLIP_N, starts, 533, 8)
    assert gc.same_bits(got, tw.rows(emotion_t, CLIP_N, starts, 533, 8))
    rows = [cc.window_row(int(s), 8, 533, CLIP_N, CTX, ITV)[0] for s in starts.cpu()]
    assert len(set(rows)) >= 5 and rows[-1] == 20
    for g, r in zip(got, rows):
        assert gc.same_bits(g, emotion[r])
    out = emotion.cpu().numpy(), features.cpu().numpy()
    ce.close(); tw.close()
    del clip, emotion, features, emotion_t, features_t, got
    assert live() == base
    return out


def test_track_equals_its_twin_and_a_stream_row_by_row():
    emotion, features = track()
    assert np.isfinite(emotion).all() and (features != 0).sum(axis=1).max() >= 56        # not zeros against zeros
    base = live()
    se = StreamEmotion(1, CTX, ITV, compression_layer=gc.l186(), feature_set=GM)
    x = dev(speech(300, 2.5))
    g = cc.chunk(CTX, ITV)
    k = 0
    for at in range(0, CLIP_N, g):
        se.push(x[None, at:at + g])
        _, upd = se.update()
        if at + g >= 8000 and (at + g - 8000) % 1600 == 0:
            assert bool(upd[0]), k
            assert gc.same_bits(se.features[0], features[k]) and gc.same_bits(se.emotion[0], emotion[k]), k
            k += 1
    assert k == 21
    se.close()
    del x
    assert live() == base


@pytest.mark.parametrize("max_slots", [1, 64])
def test_track_does_not_depend_on_the_passes(max_slots):
    a, b = track(), track(max_slots)
    assert gc.same_bits(a[0], b[0]) and gc.same_bits(a[1], b[1])


def test_build_batch_of_two_clips():
    base = live()
    ce, tw = clip_pair(CTX, ITV, 4)
    clips = dev(np.stack([speech(300, 2.5), speech(420, 2.5)]))
    emotion, features = ce.build_batch(clips)
    assert emotion.shape == (2, 21, 256) and features.shape == (2, 21, 62)
    emotion_t, features_t = tw.build_batch(clips)
    assert gc.same_bits(emotion, emotion_t) and gc.same_bits(features, features_t[:, :, COLS])
    for c in range(2):
        e, f = ce.build(clips[c])
        assert gc.same_bits(e, emotion[c]) and gc.same_bits(f, features[c]), c
    assert gc.same_bits(emotion[0], track()[0])
    ce.close(); tw.close()
    del clips, emotion, features, emotion_t, features_t, e, f
    assert live() == base


def test_one_track_at_the_fast_timing():
    """10 s / 0.5 s on a 12 s clip: 24 rows, growing windows up to the full 995 frames, the last row after the 12 s ring has wrapped."""
    base = live()
    ce, tw = clip_pair(10.0, 0.5, 24)
    clip = dev(speech(300, 12.0))
    assert ce.num_rows(clip.shape[0]) == 24 and ce.shape["max_frames"] == 995
    assert cc.plan(clip.shape[0], 10.0, 0.5)[-1][1] > 0
    emotion, features = ce.build(clip)
    emotion_t, features_t = tw.build(clip)
    assert gc.same_bits(emotion, emotion_t) and gc.same_bits(features, features_t[:, COLS])
    # not zeros against zeros: the last row's window is 10 s of voiced, silent and noisy stretches (row 0 is half a second of one vowel,
    # whose unvoiced statistics are rightly zero)
    assert int((features[-1] != 0).sum()) >= 56
    ce.close(); tw.close()
    del clip, emotion, features, emotion_t, features_t
    assert live() == base
