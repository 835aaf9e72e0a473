"""The emotion objects with eGeMAPS windows beyond 2048 frames (``long_windows=True``: km_emotion_stream_create_long,
km_emotion_clip_create_long) at the timing of the reference's ``long_context`` variant, 30 s / 0.2 s (2995 frames per window), and
training / rendering on them.

What a row holds is checked BIT FOR BIT against ``EGeMAPSEngine.functionals(window[None], long_windows=True)[0]`` on the oracle's
window (tests/test_gpu_egemaps_long.py pins that call), the track against a long stream, the trainer against a hand loop; the
264 -> 256 product has the derived bound of tests/test_gpu_stream_emotion.py.  km_live_device_bytes() is back at its baseline after
every object is closed.
"""
import functools
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import clip_emotion_cases as cc
import egemaps_cases as egc
from koemorph_amd import _lib, synth
from koemorph_amd.data import SequentialKoeMorphDataset
from koemorph_amd.engine import Engine
from koemorph_amd.features import ClipEmotion
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine
from koemorph_amd.model import SequentialDualStreamModel
from koemorph_amd.scripts import render_sequential as rs
from koemorph_amd.scripts import train_sequential as ts
from koemorph_amd.streaming import StreamEmotion, emotion_stream_shape
from oracle.buffers import AudioBufferOracle

pytestmark = pytest.mark.gpu

CTX, ITV = 30.0, 0.2                       # configs/model/dual_stream.yaml, variant long_context
SR = 16000
CHUNK = 88000                              # 5.5 s: the coarse chunks the streams are fed
SECONDS = (33.0, 25.0, 5.0)                # stream 0 wraps the 32 s ring; 1: 2495 frames, window not full; 2: a short window in a long object
HOP, WINDOW_FRAMES = 533, 512              # the long_context model's windows: 512 frames at 30 fps


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def live():
    torch.cuda.synchronize()
    return int(_lib.load().km_live_device_bytes())


@functools.lru_cache(maxsize=None)
def layer():
    torch.manual_seed(2468)
    return torch.nn.Linear(264, 256)


@functools.lru_cache(maxsize=None)
def egemaps():
    return EGeMAPSEngine("cuda")


def reference(window: np.ndarray) -> np.ndarray:
    f = egemaps().functionals(dev(window)[None], long_windows=True)[0].cpu().numpy()
    return np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def speech(seed: int, seconds: float) -> np.ndarray:
    """Speech-like audio in 2.5 s phrases of different voices."""
    n = int(seconds * SR)
    x = np.concatenate([egc.speechlike(seed + 3 * k, 2.5) * (0.3 + 0.1 * (k % 5)) for k in range(n // 40000 + 1)])[:n].astype(np.float32)
    x.setflags(write=False)
    return x


# ---- streams ----------------------------------------------------------------------------------------------------------
def stream_audio():
    return [speech(500 + 100 * s, sec) for s, sec in enumerate(SECONDS)]


def pushes():
    """[(samples (3, CHUNK), counts (3))]: every stream's audio in chunks of CHUNK, the last one partial, then nothing."""
    audio = stream_audio()
    out = []
    for at in range(0, max(len(a) for a in audio), CHUNK):
        x = np.zeros((3, CHUNK), np.float32)
        cnt = np.zeros(3, np.int32)
        for s, a in enumerate(audio):
            piece = a[at:at + CHUNK]
            x[s, :len(piece)] = piece
            cnt[s] = len(piece)
        out.append((x, cnt))
    return out


def snapshot(se):
    torch.cuda.synchronize()
    return dict(features=se.features.cpu().numpy(), slots=se.slots.cpu().numpy(), emotion=se.emotion.cpu().numpy().copy(),
                valid=se.valid.cpu().numpy().copy(), updated=se.updated.cpu().numpy().copy())


def same(a, b, keys=("features", "slots", "emotion", "valid")):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


@functools.lru_cache(maxsize=None)
def eager_run():
    """The three streams pushed chunk by chunk with an update after every push -> (snapshot per push, live bytes while open - before)."""
    base = live()
    se = StreamEmotion(3, CTX, ITV, compression_layer=layer(), long_windows=True)
    assert se.shape == emotion_stream_shape(CTX, ITV, long_windows=True) and se.shape["max_frames"] == 2995
    held = live() - base
    out = []
    for x, cnt in pushes():
        se.push(dev(x), dev(cnt))
        se.update()
        out.append(snapshot(se))
    se.close()
    assert live() == base
    return out, held


def test_stream_rows_are_the_functionals_of_the_oracles_windows():
    snaps, held = eager_run()
    assert len(snaps) == 6
    # the object's one allocation holds the frame records of its slots: 3 x 2995 x 36 floats, and three rings of 32 s
    assert held >= 3 * 2995 * 36 * 4 + 3 * 512000 * 4
    last = snaps[-1]
    frames = []
    for s, a in enumerate(stream_audio()):
        buf = AudioBufferOracle(CTX + 2.0)
        for at in range(0, len(a), CHUNK):
            buf.append(a[at:at + CHUNK])
        win = buf.get_window(CTX)
        frames.append((len(win) - 960) // 160 + 1)
        assert buf.full == (s == 0)
        ref = reference(win)
        assert np.array_equal(bits(last["features"][s]), bits(ref)), (s, len(win), float(np.abs(last["features"][s] - ref).max()))
        first = reference(a[:CHUNK])                                 # the 300 / 600 ms slots: the features of the stream's first update
        assert np.array_equal(bits(last["slots"][s, 0]), bits(first)) and np.array_equal(bits(last["slots"][s, 1]), bits(first)), s
    assert frames == [2995, 2495, 495]
    assert list(last["valid"]) == [1, 1, 1] and list(last["updated"]) == [1, 0, 0] and list(snaps[4]["updated"]) == [1, 1, 0]
    # emotion = the three slots through the layer, within the derived bound of a 264-term float32 dot product plus bias
    W = layer().weight.detach().numpy().astype(np.float64)
    b = layer().bias.detach().numpy().astype(np.float64)
    for s in range(3):
        x = np.concatenate([last["features"][s], last["slots"][s, 0], last["slots"][s, 1]]).astype(np.float64)
        bound = 265 * 2.0 ** -24 * (np.abs(W) @ np.abs(x) + np.abs(b))
        err = np.abs(last["emotion"][s].astype(np.float64) - (W @ x + b))
        assert (err <= bound).all(), (s, float((err / bound).max()))


def test_one_update_per_call_gives_the_same_rows():
    snaps, _ = eager_run()
    base = live()
    se = StreamEmotion(3, CTX, ITV, max_updates=1, compression_layer=layer(), long_windows=True)
    for (x, cnt), want in zip(pushes(), snaps):
        se.push(dev(x), dev(cnt))
        served = np.zeros(3, np.uint8)
        for _ in range(3):
            _, upd = se.update()
            assert int(upd.sum()) <= 1
            served |= upd.cpu().numpy()
        assert np.array_equal(served, want["updated"]) and same(snapshot(se), want)
    se.close()
    assert live() == base


def test_captured_push_and_update_replayed_on_other_samples():
    snaps, _ = eager_run()
    base = live()
    se = StreamEmotion(3, CTX, ITV, compression_layer=layer(), long_windows=True)
    for t, ((x, cnt), want) in enumerate(zip(pushes(), snaps)):
        if t == 0:                                                  # the first push and update are eager, the rest one captured graph
            se.push(dev(x), dev(cnt))
            se.update()
        else:
            if t == 1:
                se.capture(CHUNK)
            se.replay(dev(x), dev(cnt))
        got = snapshot(se)
        assert same(got, want) and np.array_equal(got["updated"], want["updated"]), t
    # reset_streams makes a fresh stream: stream 0 fed stream 2's audio holds what stream 2 holds; the others do not notice
    mask = torch.tensor([True, False, False], device="cuda")
    se.reset_streams(mask)
    z = snapshot(se)
    assert not z["features"][0].any() and not z["slots"][0].any() and not z["emotion"][0].any() and not z["valid"][0]
    a2 = stream_audio()[2]
    x = np.zeros((3, CHUNK), np.float32)
    x[0, :len(a2)] = a2
    se.replay(dev(x), dev(np.array([len(a2), 0, 0], np.int32)))
    got = snapshot(se)
    assert list(got["updated"]) == [1, 0, 0]
    for k in ("features", "slots", "emotion"):
        assert np.array_equal(bits(got[k][0]), bits(snaps[-1][k][2])), k
        assert np.array_equal(bits(got[k][1:]), bits(snaps[-1][k][1:])), k
    se.close()
    assert live() == base


def test_the_extractor_mirror_takes_a_30_s_window():
    """OpenSMILEeGeMAPSExtractor(context_window=30.0): with the keyword its state machine extracts the window its AudioBuffer returns
    (the oldest 30 s of an unwrapped ring); without it the first extraction fails as before."""
    from koemorph_amd.features.opensmile_extractor import OpenSMILEeGeMAPSExtractor
    x = speech(500, 33.0)[:31 * SR]
    ex = OpenSMILEeGeMAPSExtractor(context_window=CTX, update_interval=ITV, device="cuda", long_windows=True)
    f = ex.process_audio_frame(x, force_update=True)
    assert f is not None and ex.failed_extractions == 0 and np.array_equal(bits(f), bits(reference(x[:480000])))
    plain = OpenSMILEeGeMAPSExtractor(context_window=CTX, update_interval=ITV, device="cuda")
    assert plain.process_audio_frame(x, force_update=True) is None and plain.failed_extractions == 1


# ---- clip track -------------------------------------------------------------------------------------------------------
CLIP_SECONDS = 40.0


@functools.lru_cache(maxsize=None)
def track(max_slots=4):
    base = live()
    ce = ClipEmotion(CTX, ITV, max_slots=max_slots, compression_layer=layer(), long_windows=True)
    clip = dev(speech(900, CLIP_SECONDS))
    assert ce.num_rows(clip.shape[0]) == cc.num_rows(clip.shape[0], CTX, ITV) == 198
    emotion, features = ce.build(clip)
    # rows gathers by the host mapping
    starts = [0, 1, 37, 200, 421, 687, 688, 700]
    got = ce.rows(emotion, clip.shape[0], torch.tensor(starts, dtype=torch.int32, device="cuda"), HOP, WINDOW_FRAMES).cpu().numpy()
    torch.cuda.synchronize()
    out = emotion.cpu().numpy(), features.cpu().numpy()
    rows = [cc.window_row(s, WINDOW_FRAMES, HOP, clip.shape[0], CTX, ITV)[0] for s in starts]
    assert len(set(rows)) >= 5 and rows[-1] == 197
    for g, r in zip(got, rows):
        assert np.array_equal(bits(g), bits(out[0][r])), r
    ce.close()
    del clip, emotion, features
    assert live() == base
    return out


def test_track_rows_equal_a_long_streams_rows():
    emotion, features = track()
    plan = cc.plan(int(CLIP_SECONDS * SR), CTX, ITV)
    lengths = [n for _, _, n in plan]
    assert min(lengths) == 8000 and max(lengths) == 480000 and sum(n > 960 + 160 * 2047 for n in lengths) > 50
    assert any(start > 0 for _, start, _ in plan)                  # ... and the last rows come after the wrap
    se = StreamEmotion(1, CTX, ITV, compression_layer=layer(), long_windows=True)
    g = cc.chunk(CTX, ITV)
    x = speech(900, CLIP_SECONDS)
    xd = dev(x)
    k = 0
    for at in range(0, len(x), g):
        se.push(xd[None, at:at + g])
        _, upd = se.update()
        if (at + g - 8000) % 3200 == 0 and at + g >= 8000:
            if k % 9 == 0 or k >= 190:                              # every ninth row and the rows after the wrap: a read-back each
                assert bool(upd[0]), k
                assert torch.equal(se.features[0].cpu(), torch.from_numpy(features[k])), k
                assert torch.equal(se.emotion[0].cpu(), torch.from_numpy(emotion[k])), k
            k += 1
    assert k == 198
    se.close()
    # ... and the pinned B = 1 call on the plan's window, for a growing, a stale and a wrapped row
    for k in (0, 120, 150, 197):
        _, start, n = plan[k]
        assert np.array_equal(bits(features[k]), bits(reference(x[start:start + n]))), k


@pytest.mark.parametrize("max_slots", [1, 64])
def test_track_does_not_depend_on_the_passes(max_slots):
    a, b = track(), track(max_slots)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_short_windows_with_the_flag_are_the_plain_object():
    clip = dev(speech(900, 25.0))
    out = []
    for flag in (False, True):
        base = live()
        ce = ClipEmotion(20.0, 0.3, max_slots=64, compression_layer=layer(), long_windows=flag)
        held = live() - base
        emotion, features = ce.build(clip)
        out.append((emotion.cpu().numpy(), features.cpu().numpy(), held))
        ce.close()
        del emotion, features
        assert live() == base
    assert out[0][0].shape == (82, 256) and out[0][2] == out[1][2]
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))


def test_python_refusals_are_unchanged():
    with pytest.raises(ValueError, match=r"2995 frames per window, at most 2048 \(20\.5 s\)"):
        StreamEmotion(3, CTX, ITV)
    with pytest.raises(ValueError, match=r"2995 frames per window, at most 2048 \(20\.5 s\)"):
        ClipEmotion(CTX, ITV)
    with pytest.raises(ValueError, match=r"a window of 1056000 samples, at most 1048576 \(65\.5 s\)"):
        ClipEmotion(66.0, 0.3, long_windows=True)


# ---- training and rendering -------------------------------------------------------------------------------------------
def write_pair(d, name, seconds, seed):
    n = int(seconds * SR)
    wavfile.write(d / f"{name}.wav", SR, speech(seed, seconds)[:n])
    F = int(seconds * 30)
    labels = synth.uniform(seed + 1, (F, 52), 0, 1).astype(np.float32)
    with open(d / f"{name}.jsonl", "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    """One clip of 24 s: 720 frames, three windows of 512 at stride 100; its track's windows reach 2395 frames."""
    d = tmp_path_factory.mktemp("emotion_long_train")
    write_pair(d, "a", 24.0, 1200)
    return d


KW = dict(window_frames=WINDOW_FRAMES, stride_frames=100, shuffle_files=False, loop_dataset=False, batch_size=2)
TRAINER_KW = dict(learning_rate=1e-3, l1_weight=0.1, seed=3)


def long_context_engine():
    eng = Engine(d_model=512, num_heads=16, mel_sequence_length=WINDOW_FRAMES, emotion_dim=256)
    eng.load_state_dict(synth.make_core_params(0, d_model=512, mel_sequence_length=WINDOW_FRAMES, emotion_dim=256, style="init"))
    eng.finalize()
    return eng


def test_epoch_at_the_long_context_shape_equals_the_hand_loop(data_dir):
    """Without --resident-clip train_sequential gathers the windows and runs Trainer.step; the emotion rows come from the track."""
    ce = ClipEmotion(CTX, ITV, compression_layer=layer(), long_windows=True)
    ds = SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW)
    st = ts.SequentialTrainer(long_context_engine(), ds, clip_emotion=ce, **TRAINER_KW)
    losses = []
    real_step = st.trainer.step
    st.trainer.step = lambda *a, **k: (lambda loss: (losses.append(float(loss.item())), loss)[1])(real_step(*a, **k))
    m = st.train_epoch()
    assert m["batches"] == len(losses) == 2 and ce.builds == 1

    ce2 = ClipEmotion(CTX, ITV, compression_layer=layer(), long_windows=True)
    ds2 = SequentialKoeMorphDataset(data_dir, resident_windows=True, **KW)
    st2 = ts.SequentialTrainer(long_context_engine(), ds2, **TRAINER_KW)
    want, tr = [], None
    for batch in ds2:
        clip = batch["clip_audio"]
        if tr is None:
            st2.trainer.reset_temporal_state()
            tr = ce2.build(clip)[0]
            assert tr.shape[0] == ce2.num_rows(clip.shape[0]) == 118
        emo = ce2.rows(tr, clip.shape[0], batch["start_frames_dev"], ds2.hop_length, ds2.window_frames)
        assert batch["target"].shape[0] <= 4
        gathered = st2._with_audio(batch)
        want.append(float(st2.trainer.step(gathered["audio"], emo, batch["target"], global_batch=batch["target"].shape[0]).item()))
    assert losses == want and len(set(want)) == 2, (losses, want)
    for (k, a), (_, b) in zip(st.state_dict().items(), st2.state_dict().items()):
        assert torch.equal(a, b), k
    ce.close()
    ce2.close()


def test_train_then_render_from_the_command_line(data_dir, tmp_path):
    ckdir = tmp_path / "ck"
    ts.main(["--data_dir", str(data_dir), "--variant", "long_context", "--emotion", "egemaps", "--emotion-context-window", "30",
             "--emotion-update-interval", "0.2", "--epochs", "1", "--batch_size", "2", "--stride_frames", "100", "--checkpoint_dir", str(ckdir)])
    path = ckdir / "checkpoint_epoch_1.pth"
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["model_config"] == {"d_model": 512, "num_heads": 16, "mel_sequence_length": 512, "emotion_dim": 256, "emotion_backend": "egemaps",
                                    "emotion_context_window": 30.0, "emotion_update_interval": 0.2}
    assert ckpt["global_step"] == 2 and ckpt["epoch"] == 1

    out, wav = tmp_path / "out.jsonl", data_dir / "a.wav"
    common = ["--model_path", str(path), "--input_audio", str(wav), "--output_json", str(out), "--stride", "60"]
    assert rs.main(common) == 0                                                  # the timing is the checkpoint's
    lines = out.read_text().splitlines()
    assert rs.main(common + ["--emotion-context-window", "30", "--emotion-update-interval", "0.2"]) == 0      # agreeing flags are fine
    assert out.read_text().splitlines() == lines
    for flags in (["--emotion-context-window", "20"], ["--emotion-update-interval", "0.3"]):
        with pytest.raises(SystemExit) as exit_:
            rs.main(common + flags)
        assert exit_.value.code == 2
    with pytest.raises(ValueError, match="contradicts the checkpoint, which was trained with 30"):
        rs.load_model(path, emotion_context_window=20.0)

    ce = ClipEmotion(CTX, ITV, compression_layer=rs.compression_layer(ckpt)[0], long_windows=True)
    m = SequentialDualStreamModel(d_model=512, num_heads=16, mel_sequence_length=512, stride_frames=60, clip_emotion=ce,
                                  emotion_config={"emotion_dim": 256, "backend": "opensmile"}).cuda().eval()
    m.load_state_dict(ckpt["model_state_dict"])
    samples = speech(1200, 24.0)
    with torch.no_grad():
        want = m(dev(samples)[None])["blendshapes"][0].cpu().numpy()
    assert len(lines) == want.shape[0] >= 3
    for i, line in enumerate(lines):
        rec = json.loads(line)
        assert rec["timestamp"] == min(len(samples), (i * 60 + 512) * HOP) / 16000.0
        assert np.array_equal(np.asarray(rec["blendshapes"], np.float32), want[i]), i
    ce.close()


def test_a_checkpoint_without_flags_carries_no_timing(data_dir, tmp_path):
    """Neither flag given: the 20.0 s / 0.3 s object as ever, and model_config as ever."""
    args = ts.parse_args(["--data_dir", str(data_dir), "--emotion", "egemaps"])
    assert not args.emotion_timing_given
    ce = ts.clip_emotion_from_args(args, "cuda")
    assert (ce.context_window, ce.update_interval, ce.long_windows) == (20.0, 0.3, False)
    ce.close()
    args = ts.parse_args(["--data_dir", str(data_dir), "--emotion", "egemaps", "--emotion-update-interval", "0.2"])
    ce = ts.clip_emotion_from_args(args, "cuda")
    assert (ce.context_window, ce.update_interval, ce.long_windows) == (20.0, 0.2, True)
    ce.close()
    assert rs.emotion_timing({}, None, None) is None and rs.emotion_timing({}, 30.0, None) == (30.0, 0.3)
    with pytest.raises(SystemExit):
        ts.parse_args(["--data_dir", str(data_dir), "--emotion-context-window", "30"])       # noise has no track
