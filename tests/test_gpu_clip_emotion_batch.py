"""The emotion tracks of B clips of one length in one call (km_emotion_clip_build_batch, ``ClipEmotion.build_batch``).

Rows are numbered g = c K + k and a pass takes ``max_slots`` consecutive g, so a pass may straddle a clip boundary and a row's
``features[0]`` may come from its own pass or from an earlier one.  Every clip's slice must be what ``build`` gives for that clip
alone, BIT FOR BIT: the same eGeMAPS kernels run on the same samples, and the 264 -> 256 product keeps ``build``'s summation
order -- so no tolerance is needed or given.  ``build`` itself is pinned in tests/test_gpu_clip_emotion.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import stream_emotion_cases as ec
from koemorph_amd._lib import KM_ERR_INVALID_ARG, KM_ERR_NOT_READY, KM_OK
from koemorph_amd.features import ClipEmotion

pytestmark = pytest.mark.gpu

N_A, CTX_A, ITV_A, K_A = 64777, 1.0, 0.3, 12      # clip A of tests/test_gpu_clip_emotion.py: growing, stale and wrapped windows
SEEDS = (1300, 1310, 1320)


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy(), np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def layer():
    torch.manual_seed(4321)
    return torch.nn.Linear(264, 256)


@functools.lru_cache(maxsize=None)
def clips(seeds=SEEDS) -> torch.Tensor:
    x = np.stack([(0.45 * ec.speechlike(s, 4.2))[:N_A].astype(np.float32) for s in seeds])
    assert x.shape == (len(seeds), N_A)
    return torch.from_numpy(x).cuda()


@functools.lru_cache(maxsize=None)
def singles(seeds=SEEDS):
    """build() of every clip alone, on an object of its own per clip: [(emotion (12, 256), features (12, 88))]."""
    out = []
    for c in range(len(seeds)):
        ce = ClipEmotion(CTX_A, ITV_A, max_slots=16, compression_layer=layer())
        assert ce.num_rows(N_A) == K_A
        emotion, features = ce.build(clips(seeds)[c])
        torch.cuda.synchronize()
        out.append((emotion.clone(), features.clone()))
        ce.close()
    return out


@pytest.mark.parametrize("max_slots", [16, 5, 64])
def test_every_clip_of_a_batch_is_its_own_build_bit_for_bit(max_slots):
    """16: c0 k0-11 | c1 k0-3, then c1 k4-11 | c2 k0-7, then c2 k8-11 -- a pass across a clip boundary, f_0 from the same pass
    (c0, c1 in pass 0, c2 in pass 1) and from an earlier one (c1 in pass 1, c2 in pass 2).  5: f_0 two and three passes back.
    64: everything in one pass."""
    ce = ClipEmotion(CTX_A, ITV_A, max_slots=max_slots, compression_layer=layer())
    builds = ce.builds
    emotion, features = ce.build_batch(clips())
    assert ce.builds == builds + 1
    assert emotion.shape == (3, K_A, 256) and features.shape == (3, K_A, 88)
    for c, (e1, f1) in enumerate(singles()):
        assert np.array_equal(bits(features[c]), bits(f1)), (c, float((features[c] - f1).abs().max()))
        assert np.array_equal(bits(emotion[c]), bits(e1)), (c, float((emotion[c] - e1).abs().max()))
    # the clips are different clips: had a row taken another clip's f_0, or another clip's samples, it would show
    assert not np.array_equal(bits(features[0, 0]), bits(features[1, 0])) and not np.array_equal(bits(features[1, 0]), bits(features[2, 0]))
    assert not np.array_equal(bits(emotion[0]), bits(emotion[1])) and not np.array_equal(bits(emotion[1]), bits(emotion[2]))
    ce.close()


def test_a_second_batch_does_not_see_the_first_ones_f0():
    other = (1320, 1300)                                   # other clips, another B, on the same object
    ce = ClipEmotion(CTX_A, ITV_A, max_slots=16, compression_layer=layer())
    ce.build_batch(clips())
    emotion, features = ce.build_batch(clips(other))
    ref = singles()
    for c, src in enumerate((2, 0)):
        assert np.array_equal(bits(features[c]), bits(ref[src][1])) and np.array_equal(bits(emotion[c]), bits(ref[src][0])), c
    # ... nor does build() after a batch, or a batch after build()
    e1, f1 = ce.build(clips()[1])
    assert np.array_equal(bits(e1), bits(ref[1][0])) and np.array_equal(bits(f1), bits(ref[1][1]))
    emotion, features = ce.build_batch(clips())
    assert np.array_equal(bits(emotion[2]), bits(ref[2][0]))
    ce.close()


def test_clips_without_rows_and_refusals():
    ce = ClipEmotion(CTX_A, ITV_A, max_slots=16, compression_layer=layer())
    emotion, features = ce.build_batch(torch.zeros(3, 7999, device="cuda"))
    assert emotion.shape == (3, 0, 256) and features.shape == (3, 0, 88)
    emotion, features = ce.build_batch(torch.zeros(0, N_A, device="cuda"))
    assert emotion.shape == (0, K_A, 256) and features.shape == (0, K_A, 88)
    with pytest.raises(ValueError):
        ce.build_batch(clips()[0])                         # one clip is build()'s
    with pytest.raises(ValueError):
        ce.build_batch(clips().double())
    with pytest.raises(ValueError):
        ce.build_batch(clips().cpu())
    lib, st = ce._lib, torch.cuda.current_stream().cuda_stream
    x = clips()
    e, f = torch.empty(3, K_A, 256, device="cuda"), torch.empty(3, K_A, 88, device="cuda")
    p = x.data_ptr()
    assert lib.km_emotion_clip_build_batch(ce._h, p, 3, N_A, None, e.data_ptr(), st) == KM_ERR_INVALID_ARG      # features_out is required
    assert lib.km_emotion_clip_build_batch(ce._h, p, 3, N_A, f.data_ptr(), None, st) == KM_ERR_INVALID_ARG
    assert lib.km_emotion_clip_build_batch(ce._h, None, 3, N_A, f.data_ptr(), e.data_ptr(), st) == KM_ERR_INVALID_ARG
    assert lib.km_emotion_clip_build_batch(None, p, 3, N_A, f.data_ptr(), e.data_ptr(), st) == KM_ERR_INVALID_ARG
    assert lib.km_emotion_clip_build_batch(ce._h, p, -1, N_A, f.data_ptr(), e.data_ptr(), st) == KM_ERR_INVALID_ARG
    assert lib.km_emotion_clip_build_batch(ce._h, p, 3, -1, f.data_ptr(), e.data_ptr(), st) == KM_ERR_INVALID_ARG
    # what the ragged kernels cannot address: refused before anything is read
    assert lib.km_emotion_clip_build_batch(ce._h, p, 3, 2 ** 30 + 1, f.data_ptr(), e.data_ptr(), st) == KM_ERR_INVALID_ARG
    assert lib.km_emotion_clip_build_batch(ce._h, p, 2 ** 31, N_A, f.data_ptr(), e.data_ptr(), st) == KM_ERR_INVALID_ARG   # B K > 2^31 - 1
    assert lib.km_emotion_clip_build_batch(ce._h, p, 2 ** 31 // K_A + 1, N_A, f.data_ptr(), e.data_ptr(), st) == KM_ERR_INVALID_ARG
    assert lib.km_emotion_clip_build_batch(ce._h, None, 3, 100, None, None, st) == KM_OK                        # no rows: nothing to launch
    ce.close()
    # before the compression layer is set
    h = C.c_void_p()
    assert lib.km_emotion_clip_create(C.byref(h), CTX_A, ITV_A, 16) == KM_OK
    assert lib.km_emotion_clip_build_batch(h, p, 3, N_A, f.data_ptr(), e.data_ptr(), st) == KM_ERR_NOT_READY
    lib.km_emotion_clip_destroy(h)
