"""SequentialKoeMorphDataset(device_resample=True): a 3 s 48 kHz int16 WAV is uploaded at its own rate and converted on the device.
The resident clip must be within the resampler's bound of the float64 oracle (tests/resample_cases.py) fed the file's float32
samples; the default path (host conversion before the upload) is compared in lengths, label rows and window count only."""
import json

import numpy as np
import pytest
import torch

import resample_cases as rc
from koemorph_amd import synth
from koemorph_amd.data.sequential_dataset import SequentialKoeMorphDataset, _read_wav

pytestmark = pytest.mark.gpu
RATE_IN, SECONDS, FPS = 48000, 3, 30


def write_pair(tmp_path):
    from scipy.io import wavfile
    x = synth.make_audio(321, 1, RATE_IN * SECONDS)[0]
    pcm = np.clip(np.round(x / max(1.0, float(np.abs(x).max())) * 30000.0), -32768, 32767).astype(np.int16)
    wavfile.write(str(tmp_path / "take.wav"), RATE_IN, pcm)
    rows = synth.uniform(322, (SECONDS * FPS, 52), 0.0, 1.0)
    with open(tmp_path / "take.jsonl", "w") as f:
        for i, r in enumerate(rows):
            f.write(json.dumps({"timestamp": i / FPS, "blendshapes": [float(v) for v in r]}) + "\n")
    return pcm, rows


def test_device_resample_against_the_oracle_and_the_default_path(tmp_path):
    pcm, rows = write_pair(tmp_path)
    kw = dict(window_frames=16, stride_frames=2, shuffle_files=False, loop_dataset=False, batch_size=4)
    host = SequentialKoeMorphDataset(tmp_path, **kw)
    devd = SequentialKoeMorphDataset(tmp_path, device_resample=True, **kw)
    assert not host.device_resample and devd.device_resample
    a, b = host.clip(0), devd.clip(0)
    assert a.audio.shape == b.audio.shape == (16000 * SECONDS,) and b.audio.dtype == torch.float32
    assert a.num_windows == b.num_windows == (SECONDS * FPS - 16) // 2 + 1 and a.name == b.name
    assert torch.equal(a.labels, b.labels) and np.array_equal(b.labels.cpu().numpy(), rows.astype(np.float32))
    assert host.get_num_windows() == devd.get_num_windows()

    sr, x = _read_wav(tmp_path / "take.wav")                # integer -> float stays where it was: pcm / 32768 in float32
    assert sr == RATE_IN and np.array_equal(x, pcm.astype(np.float32) / 32768.0)
    y, bound = rc.oracle(x, RATE_IN)
    got = b.audio.cpu().numpy().astype(np.float64)
    err = np.abs(got - y)
    print(f"device_resample: max |hip - oracle| {err.max():.3e}, largest fraction of the bound {(err[bound > 0] / bound[bound > 0]).max():.3f}")
    assert np.all(err <= bound)

    ga, gb = next(iter(host)), next(iter(devd))
    assert ga["audio"].shape == gb["audio"].shape and torch.equal(ga["blendshapes"], gb["blendshapes"])
    assert torch.equal(gb["audio"][1], b.audio[2 * devd.hop_length:2 * devd.hop_length + devd.window_samples])
