"""Training and rendering on the GeMAPS emotion track at the ``fast`` shape of configs/model/dual_stream.yaml (d_model 128, 4 heads,
window 128, emotion_dim 256; track timing 10 s / 0.5 s).

The track is pinned against its eGeMAPS twin in tests/test_gpu_emotion_gemaps.py (equal emotion bits), so an epoch on it equals the
epoch on the twin's track bit for bit: every step's loss, the weights, the optimizer state, and ``validate(components=True)``.  Then
train -> render through both command lines with the reference's ``fast`` recipe.

The clip has 4.5 s, not 3: a window of the ``fast`` shape is 128 frames (4.27 s at 30 fps), so a clip of 90 frames has no window at
all; 135 frames give 8 windows, two batches of 4.
"""
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import egemaps_cases as egc
import gemaps_cases as gc
from koemorph_amd import synth
from koemorph_amd.data import SequentialKoeMorphDataset
from koemorph_amd.engine import Engine
from koemorph_amd.features import ClipEmotion
from koemorph_amd.model import SequentialDualStreamModel
from koemorph_amd.scripts import render_sequential as rs
from koemorph_amd.scripts import train_sequential as ts

pytestmark = pytest.mark.gpu

SR, HOP = 16000, 533
CTX, ITV = 10.0, 0.5
SECONDS = 4.5
FAST = dict(d_model=128, num_heads=4, mel_sequence_length=128, emotion_dim=256)
KW = dict(window_frames=128, stride_frames=1, shuffle_files=False, loop_dataset=False, batch_size=4)
TRAINER_KW = dict(learning_rate=1e-3, l1_weight=0.1, seed=3)


def samples():
    return np.concatenate([egc.speechlike(1300, 2.5), 0.6 * egc.speechlike(1303, 2.5)])[:int(SECONDS * SR)].astype(np.float32)


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemaps_train")
    wavfile.write(d / "a.wav", SR, samples())
    F = int(SECONDS * 30)
    labels = synth.uniform(1301, (F, 52), 0, 1).astype(np.float32)
    with open(d / "a.jsonl", "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")
    return d


def fast_engine():
    eng = Engine(**FAST)
    eng.load_state_dict(synth.make_core_params(0, d_model=128, mel_sequence_length=128, emotion_dim=256, style="init"))
    eng.finalize()
    return eng


def run(data_dir, ce):
    """One epoch and one validation on the track of ``ce`` -> (losses per step, state dict, optimizer state, validation)."""
    ds = SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW)
    val = SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW)
    st = ts.SequentialTrainer(fast_engine(), ds, val, clip_emotion=ce, **TRAINER_KW)
    losses = []
    real_step = st.trainer.step
    st.trainer.step = lambda *a, **k: (lambda loss: (losses.append(float(loss.item())), loss)[1])(real_step(*a, **k))
    m = st.train_epoch()
    assert m["batches"] == len(losses) == 2 and ce.builds == 1
    v = st.validate(components=True)
    return losses, st.state_dict(), st.trainer.optimizer_state(), v


def same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            same_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same_tree(x, y, f"{path}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def test_epoch_on_the_gemaps_track_equals_the_epoch_on_the_twins(data_dir):
    ce = ClipEmotion(CTX, ITV, compression_layer=gc.l186(), feature_set="GeMAPS")
    tw = ClipEmotion(CTX, ITV, compression_layer=gc.scatter_compression(gc.l186()))
    assert ce.feature_dim == 62 and ce.emotion_dim == tw.emotion_dim == 256 and ce.num_rows(int(SECONDS * SR)) == 9
    got, want = run(data_dir, ce), run(data_dir, tw)
    assert got[0] == want[0] and len(set(got[0])) == 2 and all(np.isfinite(got[0])), (got[0], want[0])
    same_tree(got[1], want[1], "weights")
    same_tree(got[2], want[2], "optimizer")
    v, vt = got[3], want[3]
    assert v["batches"] == 2 and np.isfinite(v["total"]) and {"mse", "l1", "sequence_stats"} <= set(v)
    same_tree({k: x for k, x in v.items() if k != "seconds"}, {k: x for k, x in vt.items() if k != "seconds"}, "validate")
    # ... and the rows are not those of the noise fallback or of another layer: a second layer moves the first loss
    other = ClipEmotion(CTX, ITV, compression_layer=gc.l186(187), feature_set="GeMAPS")
    assert run(data_dir, other)[0][0] != got[0][0]
    for o in (ce, tw, other):
        o.close()


def test_train_then_render_from_the_command_line(data_dir, tmp_path):
    ckdir = tmp_path / "ck"
    ts.main(["--data_dir", str(data_dir), "--variant", "fast", "--emotion", "gemaps", "--emotion-context-window", "10",
             "--emotion-update-interval", "0.5", "--epochs", "1", "--batch_size", "4", "--checkpoint_dir", str(ckdir)])
    path = ckdir / "checkpoint_epoch_1.pth"
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["model_config"] == {"d_model": 128, "num_heads": 4, "mel_sequence_length": 128, "emotion_dim": 256, "emotion_backend": "egemaps",
                                    "emotion_feature_set": "GeMAPS", "emotion_context_window": 10.0, "emotion_update_interval": 0.5}
    assert tuple(ckpt["emotion_compression"]["weight"].shape) == (256, 186) and tuple(ckpt["emotion_compression"]["bias"].shape) == (256,)
    assert torch.equal(ckpt["emotion_compression"]["weight"], ts.gemaps_compression_layer().weight.detach())
    assert ckpt["global_step"] == 2 and ckpt["epoch"] == 1

    out, wav = tmp_path / "out.jsonl", data_dir / "a.wav"
    common = ["--model_path", str(path), "--input_audio", str(wav), "--output_json", str(out), "--stride", "3"]
    assert rs.main(common + ["--emotion", "gemaps"]) == 0               # the set, the layer and the timing are the checkpoint's
    lines = out.read_text().splitlines()
    with pytest.raises(SystemExit) as exit_:                            # the default, --emotion egemaps, contradicts the checkpoint
        rs.main(common)
    assert exit_.value.code == 2
    with pytest.raises(rs.EmotionTimingError, match=r"--emotion egemaps .* contradicts the checkpoint, which was trained with --emotion gemaps"):
        rs.load_model(path)

    layer, source = rs.compression_layer(ckpt, 186)
    assert source == "checkpoint"
    ce = ClipEmotion(CTX, ITV, compression_layer=layer, long_windows=True, feature_set="GeMAPS")
    m = SequentialDualStreamModel(d_model=128, num_heads=4, mel_sequence_length=128, stride_frames=3, clip_emotion=ce,
                                  emotion_config={"emotion_dim": 256, "backend": "opensmile"}).cuda().eval()
    m.load_state_dict(ckpt["model_state_dict"])
    x = samples()
    with torch.no_grad():
        want = m(torch.from_numpy(x).cuda()[None])["blendshapes"][0].cpu().numpy()
    assert len(lines) == want.shape[0] >= 3
    for i, line in enumerate(lines):
        rec = json.loads(line)
        assert rec["timestamp"] == min(len(x), (i * 3 + 128) * HOP) / 16000.0
        assert np.array_equal(np.asarray(rec["blendshapes"], np.float32), want[i]), i
    ce.close()
