"""SequentialTrainer with a ClipEmotion: the emotion rows of every batch come from the clip's emotion track, gathered by start
frame, and the step stays on the resident clip (Trainer.step_clip / Engine.forward_clip).

The bar is bit-identity with a hand loop that does by hand what the trainer is meant to do: ``track_for`` + ``rows`` + ``step_clip``
with the EMA reset at file changes.  The track itself is pinned in tests/test_gpu_clip_emotion.py.
"""
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from koemorph_amd import synth
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.data import SequentialKoeMorphDataset
from koemorph_amd.engine import Engine
from koemorph_amd.features import ClipEmotion
from koemorph_amd.scripts import train_sequential as ts

pytestmark = pytest.mark.gpu

KW = dict(shuffle_files=False, loop_dataset=False, batch_size=8)
TRAINER_KW = dict(learning_rate=1e-3, l1_weight=0.1, seed=3)


def write_pair(d, name, seconds, seed):
    n = int(seconds * 16000)
    wavfile.write(d / f"{name}.wav", 16000, synth.uniform(seed, (n,), -0.5, 0.5).astype(np.float32))
    F = int(seconds * 30)
    labels = synth.uniform(seed + 1, (F, 52), 0, 1).astype(np.float32)
    with open(d / f"{name}.jsonl", "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    """Two clips of 267 and 264 frames: 12 and 9 windows, so at batch 8 both end in a short batch and the file changes in between."""
    d = tmp_path_factory.mktemp("clip_emotion_train")
    write_pair(d, "a", 8.9, 40)
    write_pair(d, "b", 8.8, 50)
    return d


@pytest.fixture(scope="module")
def layer():
    torch.manual_seed(99)
    return torch.nn.Linear(264, 256)


def engine():
    eng = Engine()
    eng.load_state_dict(synth.make_core_params(0))
    eng.finalize()
    return eng


def test_epoch_equals_the_hand_loop_and_builds_each_track_once(data_dir, layer, monkeypatch):
    ce = ClipEmotion(2.0, 0.3, compression_layer=layer)            # R = 64 000: both clips cross the wrap
    ds = SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW)
    st = ts.SequentialTrainer(engine(), ds, SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW), from_clip=True,
                              clip_emotion=ce, **TRAINER_KW)
    losses = []
    real_step_clip = st.trainer.step_clip

    def step_clip(*a, **k):
        loss = real_step_clip(*a, **k)
        losses.append(float(loss.item()))
        return loss

    monkeypatch.setattr(st.trainer, "step_clip", step_clip)
    monkeypatch.setattr(st.trainer, "step", lambda *a, **k: pytest.fail("a resident batch was gathered"))
    m = st.train_epoch()
    assert m["batches"] == len(losses) == 4 and ce.builds == 2

    # the hand loop, on a trainer of its own and a ClipEmotion of its own with the same layer
    ce2 = ClipEmotion(2.0, 0.3, compression_layer=layer)
    ds2 = SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW)
    st2 = ts.SequentialTrainer(engine(), ds2, from_clip=True, **TRAINER_KW)
    tracks, want, current = {}, [], None
    for batch in ds2:
        fi = int(batch["file_indices"][0])
        if fi != current:
            current = fi
            st2.trainer.reset_temporal_state()
        clip, sf = batch["clip_audio"], batch["start_frames"]
        if fi not in tracks:
            tracks[fi] = ce2.build(clip)[0]
            assert tracks[fi].shape[0] == ce2.num_rows(clip.shape[0]) > 20
        emo = ce2.rows(tracks[fi], clip.shape[0], batch["start_frames_dev"], ds2.hop_length, ds2.window_frames)
        loss = st2.trainer.step_clip(clip, batch["start_frames_dev"], emo, batch["target"], global_batch=batch["target"].shape[0],
                                     extremes=(int(sf.min()), int(sf.max())))
        want.append(float(loss.item()))
    assert losses == want, (losses, want)
    for (k, a), (_, b) in zip(st.state_dict().items(), st2.state_dict().items()):
        assert torch.equal(a, b), k
    assert len({e for e in want}) == len(want)

    # the second epoch gathers from the cached tracks
    st.train_epoch()
    assert ce.builds == 2 and len(losses) == 8

    # validation from the resident clip: forward_clip, never the gather; the validation set's tracks are its own
    calls = []
    real_forward_clip = st.engine.forward_clip
    monkeypatch.setattr(st.engine, "forward_clip", lambda *a, **k: (calls.append(1), real_forward_clip(*a, **k))[1])
    monkeypatch.setattr(st.engine, "forward_audio", lambda *a, **k: pytest.fail("a resident validation batch was gathered"))
    v = st.validate(components=True)
    assert v["batches"] == len(calls) == 4 and not st._val_clip_logged and np.isfinite(v["total"])
    assert ce.builds == 4
    st.validate(components=True)
    assert ce.builds == 4
    ce.clear()
    st.validate(components=True)
    assert ce.builds == 6
    ce.close()
    ce2.close()


def test_the_emotion_rows_are_not_the_noise_rows(data_dir, layer):
    """Without a ClipEmotion the trainer's rows are the seeded noise they always were; with one they are the track's."""
    ce = ClipEmotion(2.0, 0.3, compression_layer=layer)
    ds = SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW)
    batch = next(iter(ds))
    plain = ts.SequentialTrainer(engine(), ds, from_clip=True, **TRAINER_KW)
    noise = plain._emotion(batch)
    want = torch.from_numpy(np.stack([0.1 * synth.normal(1000003 * 0 + w, (256,)) for w in range(8)])).cuda()
    assert torch.equal(noise, want)
    with_ce = ts.SequentialTrainer(engine(), ds, from_clip=True, clip_emotion=ce, **TRAINER_KW)
    rows = with_ce._emotion(batch)
    track = ce.track_for((0, batch["clip_audio"].data_ptr()), batch["clip_audio"])
    assert ce.builds == 1 and rows.shape == (8, 256) and not torch.equal(rows, noise)
    # windows 0 .. 7 end at (s + 256) * 533 samples: rows (e - 8000) // 4800
    k = [((s + 256) * 533 - 8000) // 4800 for s in range(8)]
    assert torch.equal(rows, track[k])
    ce.close()


def test_refusals(data_dir, layer):
    ce = ClipEmotion(2.0, 0.3, compression_layer=layer)
    eng = engine()
    with pytest.raises(ValueError, match="emotion_provider"):
        ts.SequentialTrainer(eng, SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW), clip_emotion=ce,
                             emotion_provider=lambda audio: torch.zeros(audio.shape[0], 256, device="cuda"))
    st = ts.SequentialTrainer(eng, SequentialKoeMorphDataset(data_dir, **KW), clip_emotion=ce, **TRAINER_KW)
    with pytest.raises(KoeMorphError, match="resident_windows=True"):
        st.train_epoch()
    assert ce.builds == 0
    ce.close()

