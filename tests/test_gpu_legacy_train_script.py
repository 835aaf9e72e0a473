"""koemorph_amd.scripts.train (the reference's src/train.py loop) on two synthetic WAV + JSONL pairs: two epochs, the loss
decreases, and the checkpoint's model_state_dict has exactly the keys and shapes the reference module would load."""
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from koemorph_amd import synth
from oracle.legacy import make_legacy_params

pytestmark = pytest.mark.gpu


def write_pair(d, name, seconds, seed):
    audio = synth.make_audio(seed, 1, int(seconds * 16000))[0].astype(np.float32)
    wavfile.write(d / f"{name}.wav", 16000, audio)
    labels = synth.uniform(seed + 1, (int(seconds * 30), 52), 0, 1).astype(np.float32)
    with open(d / f"{name}.jsonl", "w") as f:
        for i in range(labels.shape[0]):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


def test_train_script_two_epochs(tmp_path):
    from koemorph_amd.scripts import train
    data = tmp_path / "data"
    data.mkdir()
    write_pair(data, "a", 0.6, 1)
    write_pair(data, "b", 0.9, 3)
    res = train.main(["--data-dir", str(data), "--checkpoint-dir", str(tmp_path / "ck"), "--epochs", "2", "--batch-size", "2",
                      "--lr", "1e-3", "--dropout", "0.0", "--audio-max-length", "0.8", "--save-every", "1"])
    losses = res["epoch_losses"]
    print("\nepoch losses", losses)
    assert len(losses) == 2 and np.all(np.isfinite(losses)) and losses[1] < losses[0]
    ck = torch.load(res["checkpoint"], map_location="cpu")
    want = make_legacy_params(0)
    sd = ck["model_state_dict"]
    assert sorted(sd) == sorted(want)
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape and sd[k].dtype == torch.float32, k
    assert (tmp_path / "ck" / "checkpoint_epoch_1.pth").exists()
    assert 0.0 <= res["metrics"]["mae"] <= 1.0
