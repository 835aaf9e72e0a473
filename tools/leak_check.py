#!/usr/bin/env python3
"""Create / finalize / reserve / run / destroy handles in a loop: the library's own count of live device bytes
(km_live_device_bytes) must return to its baseline exactly.  The device's free memory is printed too, but other users of
a shared GPU move it, so it judges nothing."""
import gc, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koemorph_amd import _lib, synth
from koemorph_amd.engine import Engine
from koemorph_amd.model import KoeMorphModel, SimplifiedKoeMorphModel
from koemorph_amd.training import Trainer


def free_mb():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0] / 2 ** 20


def cycle(i):
    eng = Engine(); eng.load_state_dict(synth.make_core_params(i, style="init")); eng.finalize(); eng.reserve(32, 136448)
    audio = torch.from_numpy(synth.make_audio(1, 32, 136448, "uniform")).cuda()
    emo = torch.from_numpy(synth.normal(2, (32, 256))).cuda()
    eng.forward_audio(audio, emo)
    tr = Trainer(eng, max_windows=8, use_smoothing=False)
    tr.step(audio[:8], emo[:8], torch.rand(8, 52, device="cuda"))
    g = Engine(d_model=64, num_heads=4, mel_sequence_length=32); g.load_state_dict(synth.make_core_params(i, 64, 32, 256, "init")); g.finalize()
    g.reserve(4, 32 * 533); g.forward_audio(audio[:4, :32 * 533].contiguous(), emo[:4])
    g.set_option("seq_assemble", 1)                      # one assembled sequence call: the clip and edge images grow
    assert g.sequence_plan(40 * 533, B=2)["route"] == 2
    g.sequence_forward(audio[:2, :40 * 533].contiguous(), emo[:2])
    # one training step and one forward from a resident clip on the assembled route (option clip_assemble): the span, snippet and edge images grow
    from koemorph_amd.engine import MelConfig
    c = Engine(d_model=64, num_heads=4, mel_sequence_length=32, mel=MelConfig.model_batch(target_fps=60))
    c.load_state_dict(synth.make_core_params(i, 64, 32, 256, "init")); c.finalize(); c.set_option("clip_assemble", 1)
    assert c.clip_plan(4, 0, 9, training=True)["route"] == 2 and c.clip_plan(4, 0, 9)["route"] == 2
    ctr = Trainer(c, max_windows=4, use_smoothing=False)
    clip = audio[0, :60 * 266].contiguous()
    ctr.step_clip(clip, [0, 1, 2, 9], emo[:4], torch.rand(4, 52, device="cuda"))
    c.forward_clip(clip, [0, 1, 2, 9], emo[:4])
    # one basic emotion track of that clip and one rows call on it: the prosody plan, the slot table and the frame records
    from koemorph_amd.features import ClipEmotion
    ce = ClipEmotion(1.0, 0.1, max_slots=4, backend="basic")
    track, _ = ce.build(clip)
    ce.rows(track, clip.shape[0], torch.tensor([0, 1, 2, 9], dtype=torch.int32, device="cuda"), 266, 32)
    ce.close()
    # one long eGeMAPS track (a 21 s window has 2095 frames, beyond the 2048 of the plain object) and one long stream update: the
    # plan and the frame records behind the per-window kernels for long windows
    from koemorph_amd.streaming import StreamEmotion
    long_clip = audio[:4].reshape(-1)[:22 * 16000].contiguous()
    lce = ClipEmotion(21.0, 10.0, max_slots=2, long_windows=True)
    ltrack, _ = lce.build(long_clip)
    lce.rows(ltrack, long_clip.shape[0], torch.tensor([0, 1, 2, 9], dtype=torch.int32, device="cuda"), 266, 32)
    lce.close()
    lse = StreamEmotion(1, 21.0, 10.0, long_windows=True)
    lse.push(long_clip[None]); lse.update(); lse.close()
    # one GeMAPS stream update and one GeMAPS clip track (feature_set="GeMAPS": 62 functionals, a Linear(186, 256))
    gse = StreamEmotion(2, 1.0, 0.1, feature_set="GeMAPS")
    gse.push(audio[:2, :16000].contiguous()); gse.update(); gse.close()
    gce = ClipEmotion(1.0, 0.1, max_slots=4, feature_set="GeMAPS")
    gtrack, _ = gce.build(clip)
    gce.rows(gtrack, clip.shape[0], torch.tensor([0, 1, 2, 9], dtype=torch.int32, device="cuda"), 266, 32)
    gce.close()
    del gse, gce, gtrack
    del ctr, c, clip, ce, track, long_clip, lce, ltrack, lse
    m = KoeMorphModel(d_model=64, d_query=64, num_heads=4, num_encoder_layers=1, num_attention_layers=1, decoder_hidden_dim=32, emotion_dim=8).cuda().eval()
    with torch.no_grad():
        m(torch.randn(2, 12, 80, device="cuda"), torch.randn(2, 12, 8, device="cuda"))
    mf = KoeMorphModel(d_query=256).cuda().eval()       # default width: the two fused kernels and their weight blobs
    with torch.no_grad():
        mf(torch.randn(3, 30, 80, device="cuda"), torch.randn(3, 30, 256, device="cuda"))
        # one rollout on each route: the rollout workspace group (per-frame launches at d_model 64; gather, encoder and rollout kernel
        # in chunks at the default width)
        m.reset_temporal_state(); mf.reset_temporal_state()
        assert m.rollout_plan(2, 12, 5)["route"] == 0 and mf.rollout_plan(2, 20, 9)["route"] == 1
        m.rollout(torch.randn(2, 12, 80, device="cuda"), torch.randn(2, 12, 8, device="cuda"), context_frames=5)
        mf.rollout(torch.randn(2, 20, 80, device="cuda"), torch.randn(2, 20, 256, device="cuda"), context_frames=9, chunk_frames=4)
    # one stream engine on the default width: create, one step, reset; the handle's km_destroy frees the group (no close())
    from koemorph_amd.streaming import KoeMorphStreams
    ks = KoeMorphStreams(mf, 3, context_frames=9, max_rows=2)
    ks.step(torch.randn(3, 2, 80, device="cuda"), torch.randn(3, 2, 256, device="cuda"))
    ks.reset()
    ks._open = False                                       # the engine object is dropped without close(): km_destroy frees its group
    del ks
    # one audio engine in front of a stream engine: create, pushes, reset; km_destroy frees both groups and the two plans
    from koemorph_amd.streaming import KoeMorphAudioStreams
    ka = KoeMorphAudioStreams(mf, 3, context_frames=9, emotion_window=0.5)
    ka.push(audio[:3, :1600].contiguous()); ka.push(audio[:3, 1600:2133].contiguous())
    ka.reset()
    ka.push(audio[:3, :533].contiguous())
    ka.rows._open = ka.frames_engine._open = False
    del ka
    del tr, eng, g, m, mf, audio, emo
    gc.collect(); torch.cuda.empty_cache()


live = _lib.load().km_live_device_bytes
live0 = live()
cycle(0)
base = free_mb()
n = int(os.environ.get("REPS", 30))
for i in range(1, n + 1):
    cycle(i)
    if i % 10 == 0:
        print(f"after {i} cycles: {live() - live0} live bytes; free {free_mb():.1f} MiB (start {base:.1f})", flush=True)
leak = live() - live0
print(f"leak over {n} cycles: {leak} bytes (free memory moved by {base - free_mb():.1f} MiB)")
sys.exit(1 if leak != 0 else 0)
