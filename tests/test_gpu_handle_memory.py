"""Device memory of the handles, watched through km_live_device_bytes: whatever a handle allocated during its life is back when
it is destroyed, a rebuild in place holds what the first build held, and a create that fails holds nothing and leaves the handle
usable.  The counter is the library's own (every allocation goes through one owning type), so other users of the GPU and torch's
allocator do not move it."""
import ctypes as C

import numpy as np
import pytest
import torch

from koemorph_amd import _lib, synth
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.features.clip_emotion import ClipEmotion
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine
from koemorph_amd.model import SimplifiedKoeMorphModel
from koemorph_amd.streaming import ChunkedStreamEngine, LegacyStreamEngine, StreamEmotion, StreamEngine, StreamResampler
from koemorph_amd.training import LegacyTrainer, Trainer

pytestmark = pytest.mark.gpu

HOP = 533
WINDOW = 256 * HOP          # samples of one window of the fused shape


def live():
    return _lib.load().km_live_device_bytes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def fused_engine(seed=3, windows=4):
    e = Engine()
    e.load_state_dict(synth.make_core_params(seed))
    e.finalize()
    e.reserve(windows, WINDOW)
    return e


def test_fused_engine_through_its_whole_life():
    base = live()
    e = fused_engine()
    assert live() > base
    audio, emo = dev(synth.make_audio(11, 4, WINDOW)), dev(synth.normal(12, (4, 256)))
    e.forward_audio(audio, emo)
    clip = dev(synth.make_audio(13, 1, 258 * HOP))                     # three windows at stride 1: the shared-frame images grow
    assert e.sequence_num_outputs(clip.shape[1], 1) == 3
    e.sequence_forward(clip, emo[:1], stride_frames=1)
    e.forward_clip(clip[0], [0, 1, 2], emo[:3])
    e.forward_audio_pipelined(audio, emo)
    e.pipeline_flush()
    se = ChunkedStreamEngine(e, 2)                                     # km_stream_create + km_stream_fifo_create
    se.feed(dev(synth.make_audio(14, 2, se.frame_samples)))
    se.step(emo[:2])
    tr = Trainer(e, max_windows=2, use_smoothing=False)
    target = torch.rand(2, 52, device="cuda")
    tr.step(audio[:2], emo[:2], target)
    assert tr.clip_supported()
    tr.step_clip(clip[0], [0, 2], emo[:2], target)
    torch.cuda.synchronize()
    e.close()
    assert live() == base


def test_generic_engine():
    base = live()
    g = Engine(d_model=64, num_heads=4, mel_sequence_length=32)
    g.load_state_dict(synth.make_core_params(5, 64, 32, 256, "init"))
    g.finalize()
    g.reserve(4, 32 * HOP)
    g.forward_audio(dev(synth.make_audio(21, 4, 32 * HOP)), dev(synth.normal(22, (4, 256))))
    torch.cuda.synchronize()
    assert live() > base
    g.close()
    assert live() == base


def test_legacy_model_handle():
    base = live()
    m = SimplifiedKoeMorphModel().cuda().eval()
    se = LegacyStreamEngine(m, 2)                                      # km_legacy_stream_create
    se.push(dev(synth.make_audio(31, 2, se.audio_length)))
    se.tick()
    tr = LegacyTrainer(m, max_windows=2, max_frames=32)                # km_legacy_train_init
    tr.step(dev(synth.make_audio(32, 2, 16000)), torch.rand(2, 52, device="cuda"))
    torch.cuda.synchronize()
    assert live() > base
    _lib.load().km_destroy(m._h)
    m._h = None
    assert live() == base


def test_every_small_handle_created_and_destroyed_once():
    lib = _lib.load()
    for create, args, destroy in (("km_attn_stats_create", (28, 80, 0), "km_attn_stats_destroy"),
                                  ("km_attn_stats_streams_create", (2, 28, 80), "km_attn_stats_streams_destroy"),
                                  ("km_metrics_create", (), "km_metrics_destroy"),
                                  ("km_loss_terms_create", (), "km_loss_terms_destroy")):
        base = live()
        h = C.c_void_p()
        _lib.check(getattr(lib, create)(C.byref(h), *args))
        assert live() > base, create
        _lib.check(getattr(lib, destroy)(h))
        assert live() == base, create
    for make in (lambda: StreamEmotion(1), lambda: ClipEmotion(max_slots=4), lambda: StreamResampler(1, 48000), lambda: EGeMAPSEngine()):
        base = live()
        obj = make()
        assert live() > base, type(obj).__name__
        obj.close()
        assert live() == base, type(obj).__name__


def test_rebuild_in_place_holds_what_the_first_build_held():
    base = live()
    e = fused_engine()
    lib = _lib.load()
    StreamEngine(e, 2)
    first = live()
    StreamEngine(e, 2)
    assert live() == first
    Trainer(e, max_windows=2, use_smoothing=False)
    first = live()
    Trainer(e, max_windows=2, use_smoothing=False)
    assert live() == first
    _lib.check(lib.km_reserve(e._h, 6, WINDOW))                       # grows
    first = live()
    _lib.check(lib.km_reserve(e._h, 6, WINDOW))
    assert live() == first
    e.close()
    assert live() == base


def test_failed_stream_create_leaves_a_usable_handle():
    lib = _lib.load()
    params = synth.make_core_params(7, style="trained")

    def engine():
        e = Engine()
        e.load_state_dict(params)
        e.finalize()
        e.reserve(2, WINDOW)
        return e

    def run(e):
        se = StreamEngine(e, 2)
        audio = dev(synth.make_audio(41, 2, 257 * se.ring_hop))
        for i in range(257):                                           # 8.5 s: both rings full
            se.push(audio[:, i * se.ring_hop:(i + 1) * se.ring_hop])
        out, ready = se.tick(dev(synth.normal(42, (2, 256))))
        torch.cuda.synchronize()
        assert ready.tolist() == [1, 1]
        return out.clone()

    a = engine()
    before = live()
    cfg = MelConfig.sliding_window(n_fft=1024, hop_length=a.mel.hop_length).to_c()
    # 2^31 rings of 8.5 s are about 10^15 bytes: the allocator refuses at once, nothing is launched
    rc = lib.km_stream_create(a._h, 1 << 31, 8.5, 0.0333, C.byref(cfg))
    assert rc == _lib.KM_ERR_HIP, (rc, lib.km_last_error())
    assert live() == before
    got = run(a)
    b = engine()
    want = run(b)
    assert torch.equal(got, want)
    a.close()
    b.close()
