"""Training, validating and rendering on a clip's `basic` emotion track (ClipEmotion(backend="basic"), emotion_dim 9): the
SequentialTrainer, the resident-clip step and forward at the `basic` shape (d_model 128, 4 heads, window 256), the sequence model
and the two command-line tools.

The bar is bit-identity with what exists and is pinned: a hand loop of ``rows`` + ``step_clip``, ``forward_backward`` /
``forward_audio`` on the gathered windows with the same rows, ``sequence_forward_track`` on the built track.  The track itself is
pinned in tests/test_gpu_clip_emotion_basic.py.  No tolerance anywhere.
"""
import json
import logging

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import stream_emotion_cases as ec
from koemorph_amd import synth
from koemorph_amd._lib import check, load
from koemorph_amd.data import SequentialKoeMorphDataset
from koemorph_amd.engine import Engine
from koemorph_amd.features import ClipEmotion
from koemorph_amd.model import SequentialDualStreamModel
from koemorph_amd.scripts import render_sequential as rs
from koemorph_amd.scripts import train_sequential as ts
from koemorph_amd.training import Trainer

pytestmark = pytest.mark.gpu

CTX, ITV = 1.0, 0.1                      # R = 48 000, C = 16 000, U = 1 600, MIN = 8 000
HOP = 533
TRAINER_KW = dict(learning_rate=1e-3, l1_weight=0.1, seed=3)


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def speech(seed, seconds):
    n = round(seconds * 16000)
    x = 0.45 * np.concatenate([ec.speechlike(seed + 7 * k, 2.0) for k in range(int(seconds // 2) + 1)])[:n]
    assert x.shape == (n,)
    return x.astype(np.float32)


def write_pair(d, name, seconds, seed):
    wavfile.write(d / f"{name}.wav", 16000, speech(seed, seconds))
    F = round(seconds * 30)
    labels = synth.uniform(seed + 1, (F, 52), 0, 1).astype(np.float32)
    with open(d / f"{name}.jsonl", "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


def engine(d_model, heads, T, emotion_dim=9, seed=0, style="init", **options):
    eng = Engine(d_model=d_model, num_heads=heads, mel_sequence_length=T, emotion_dim=emotion_dim)
    eng.load_state_dict(synth.make_core_params(seed, d_model, T, emotion_dim, style))
    eng.finalize()
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


def gather(clip_dev, starts, window):
    st = dev(np.asarray(starts, np.int32))
    out = torch.empty(len(starts), window, device="cuda")
    check(load().km_gather_windows(clip_dev.data_ptr(), clip_dev.shape[0], st.data_ptr(), len(starts), HOP, window, out.data_ptr(),
                                   None, 0, 0, 0, None, None, torch.cuda.current_stream().cuda_stream))
    return out


def same_trainer_state(a: Trainer, b: Trainer, shapes):
    pa, pb = a.params(shapes), b.params(shapes)
    for k in pa:
        assert np.array_equal(pa[k].view(np.uint32), pb[k].view(np.uint32)), k
    oa, ob = a.optimizer_state(), b.optimizer_state()
    for part in ("exp_avg", "exp_avg_sq"):
        for k in oa[part]:
            assert torch.equal(oa[part][k], ob[part][k]), (part, k)
    assert torch.equal(oa["steps"], ob["steps"]) and oa["step_count"] == ob["step_count"]


# ---- 1: the trainer on a small engine -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_dir(tmp_path_factory):
    """One 3.5 s clip: 105 frames, 19 windows of 32 frames at stride 4 -> batches of 8, 8 and 3; K = 31 track rows."""
    d = tmp_path_factory.mktemp("basic_track_small")
    write_pair(d, "a", 3.5, 40)
    return d


SMALL_KW = dict(window_frames=32, stride_frames=4, shuffle_files=False, loop_dataset=False, batch_size=8, resident_windows=True)


def test_epoch_equals_the_hand_loop_and_the_second_epoch_builds_nothing(small_dir, monkeypatch):
    ce = ClipEmotion(CTX, ITV, backend="basic")
    ds = SequentialKoeMorphDataset(small_dir, **SMALL_KW)
    st = ts.SequentialTrainer(engine(64, 4, 32), ds, SequentialKoeMorphDataset(small_dir, **SMALL_KW), from_clip=True, clip_emotion=ce,
                              **TRAINER_KW)
    losses, emos = [], []
    real_step_clip = st.trainer.step_clip

    def step_clip(clip, starts, emo, *a, **k):
        loss = real_step_clip(clip, starts, emo, *a, **k)
        losses.append(float(loss.item()))
        emos.append(emo.clone())
        return loss

    monkeypatch.setattr(st.trainer, "step_clip", step_clip)
    monkeypatch.setattr(st.trainer, "step", lambda *a, **k: pytest.fail("a resident batch left step_clip"))
    m = st.train_epoch()
    assert m["batches"] == len(losses) == 3 and ce.builds == 1
    assert all(e.shape[1] == 9 for e in emos) and [e.shape[0] for e in emos] == [8, 8, 3]

    ce2 = ClipEmotion(CTX, ITV, backend="basic")
    ds2 = SequentialKoeMorphDataset(small_dir, **SMALL_KW)
    st2 = ts.SequentialTrainer(engine(64, 4, 32), ds2, from_clip=True, **TRAINER_KW)
    want, track = [], None
    st2.trainer.reset_temporal_state()
    for i, batch in enumerate(ds2):
        clip, sf = batch["clip_audio"], batch["start_frames"]
        if track is None:
            track = ce2.build(clip)[0]
            assert tuple(track.shape) == (31, 9) and clip.shape[0] == 56000
        emo = ce2.rows(track, clip.shape[0], batch["start_frames_dev"], ds2.hop_length, ds2.window_frames)
        assert torch.equal(emo, emos[i])
        loss = st2.trainer.step_clip(clip, batch["start_frames_dev"], emo, batch["target"], global_batch=batch["target"].shape[0],
                                     extremes=(int(sf.min()), int(sf.max())))
        want.append(float(loss.item()))
    assert losses == want, (losses, want)
    assert len(set(want)) == 3 and len({e.cpu().numpy().tobytes() for e in emos}) == 3
    for (k, a), (_, b) in zip(st.state_dict().items(), st2.state_dict().items()):
        assert torch.equal(a, b), k
    same_trainer_state(st.trainer, st2.trainer, st._shapes)

    st.train_epoch()                                                              # the second epoch gathers from the cached track
    assert ce.builds == 1 and len(losses) == 6

    v = st.validate(components=True)                                              # the validation set's track is its own
    assert v["batches"] == 3 and np.isfinite(v["total"]) and ce.builds == 2
    st.validate(components=True)
    assert ce.builds == 2
    ce.close()
    ce2.close()


def test_noise_rows_have_the_engines_width_and_a_width_mismatch_raises(small_dir):
    ds = SequentialKoeMorphDataset(small_dir, **SMALL_KW)
    batch = next(iter(ds))
    narrow, wide = engine(64, 4, 32), engine(64, 4, 32, emotion_dim=256)
    plain = ts.SequentialTrainer(narrow, ds, from_clip=True, **TRAINER_KW)
    want = torch.from_numpy(np.stack([0.1 * synth.normal(1000003 * 0 + w, (9,)) for w in range(8)])).cuda()
    assert torch.equal(plain._emotion(batch), want)
    eg, ba = ClipEmotion(CTX, 0.3), ClipEmotion(CTX, ITV, backend="basic")
    with pytest.raises(ValueError) as exc:
        ts.SequentialTrainer(narrow, ds, from_clip=True, clip_emotion=eg, **TRAINER_KW)
    assert "256" in str(exc.value) and "9" in str(exc.value)
    with pytest.raises(ValueError) as exc:
        ts.SequentialTrainer(wide, ds, from_clip=True, clip_emotion=ba, **TRAINER_KW)
    assert "256" in str(exc.value) and "9" in str(exc.value)
    with pytest.raises(ValueError) as exc:
        SequentialDualStreamModel(d_model=64, num_heads=4, mel_sequence_length=32, clip_emotion=ba)
    assert "256" in str(exc.value) and "9" in str(exc.value)
    del exc                                                                       # the traceback holds the frames of the refusals
    for o in (eg, ba, narrow, wide):                                              # nothing of this test waits for a collection
        o.close()


# ---- 2: the step and the forward from the resident clip at the basic shape ------------------------------------------------------
@pytest.fixture(scope="module")
def nine_seconds():
    clip = dev(speech(300, 9.0))                                                  # 144 000 samples, 270 frames, K = 86
    ce = ClipEmotion(CTX, ITV, backend="basic")
    track = ce.build(clip)[0]
    starts = [13, 0, 5]
    emo = ce.rows(track, clip.shape[0], dev(np.asarray(starts, np.int32)), HOP, 256)
    assert tuple(track.shape) == (86, 9) and tuple(emo.shape) == (3, 9) and len({r.cpu().numpy().tobytes() for r in emo}) == 3
    torch.cuda.synchronize()
    ce.close()
    return clip, starts, emo.clone()


@pytest.mark.parametrize("assemble", [0, 1])
def test_step_clip_at_the_basic_shape_equals_the_gathered_step(nine_seconds, assemble):
    """At hop 533 the step runs from the resident clip on the default shared route, whatever clip_assemble says."""
    clip, starts, emo = nine_seconds
    target = dev(synth.uniform(11, (3, 52), 0, 1).astype(np.float32))
    kw = dict(max_windows=3, lr=1e-3, l1_weight=0.1, dropout=0.1, seed=5)
    e1, e2 = engine(128, 4, 256, seed=1, clip_assemble=assemble), engine(128, 4, 256, seed=1)
    assert e1.clip_plan(3, 0, 13, training=True)["route"] == 1
    a, b = Trainer(e1, **kw), Trainer(e2, **kw)
    assert a.clip_supported()                                                     # not the gather inside forward_backward_clip
    la = a.step_clip(clip, starts, emo, target)
    b.forward_backward(gather(clip, starts, 256 * HOP), emo, target)
    grad = b.flat_grad.clone()
    b.optimizer_step()
    assert torch.equal(la, b.loss) and torch.equal(a.out[:3], b.out[:3]) and np.isfinite(float(la.item()))
    assert float(grad.abs().max()) > 0
    shapes = {k: tuple(v.shape) for k, v in e1.state_dict_shapes().items()}
    same_trainer_state(a, b, shapes)
    other = Trainer(engine(128, 4, 256, seed=1), **kw)                             # the rows matter: another emotion input, another loss
    other.forward_backward(gather(clip, starts, 256 * HOP), emo.flip(0).contiguous(), target)
    assert not torch.equal(other.loss, b.loss)


def test_forward_clip_at_the_basic_shape_equals_the_gathered_forward(nine_seconds):
    clip, starts, emo = nine_seconds
    """Route 2 (span image + edge rows) under clip_assemble + core128, against forward_audio through the same core."""
    e1, e2 = engine(128, 4, 256, seed=1, style="trained", clip_assemble=1, core128=1), engine(128, 4, 256, seed=1, style="trained", core128=1)
    assert e1.forward_clip_supported() and e1.clip_plan(3, 0, 14)["route"] == 2 and not e2.forward_clip_supported()
    s1, s2 = torch.zeros(3, 52, device="cuda"), torch.zeros(3, 52, device="cuda")
    got = e1.forward_clip(clip, starts, emo, state=s1, first=True)
    want = e2.forward_audio(gather(clip, starts, 256 * HOP), emo, state=s2, first=True)
    assert torch.equal(got, want) and torch.equal(s1, s2)
    got = e1.forward_clip(clip, [14, 1, 6], emo, state=s1, first=False)
    want = e2.forward_audio(gather(clip, [14, 1, 6], 256 * HOP), emo, state=s2, first=False)
    assert torch.equal(got, want) and torch.equal(s1, s2)


# ---- 3: the model ---------------------------------------------------------------------------------------------------------------
def full_state(params, alpha=0.8):
    sd = {"dual_stream_attention." + k: torch.from_numpy(v) for k, v in params.items()}
    sd["smoothing_alpha"] = torch.tensor(alpha)
    return sd


def test_model_with_a_basic_track(caplog):
    stride = 3
    ce = ClipEmotion(CTX, ITV, backend="basic")
    params = synth.make_core_params(21, 64, 32, 9, "trained")
    m = SequentialDualStreamModel(d_model=64, num_heads=4, mel_sequence_length=32, stride_frames=stride, clip_emotion=ce,
                                  emotion_config={"backend": "basic"}).cuda().eval()
    assert m.emotion_dim == 9
    m.load_state_dict(full_state(params))
    audio = dev(np.stack([speech(500, 3.5), speech(600, 3.5)]))
    with caplog.at_level(logging.WARNING):
        auto = m(audio)
    assert ce.builds == 1 and not [r for r in caplog.records if "Emotion extraction failed" in r.getMessage()]
    assert auto["emotion_backend"] == "basic_track" and auto["num_frames"] == auto["blendshapes"].shape[1] > 20
    track = ce.build_batch(audio)[0]
    assert tuple(track.shape) == (2, 31, 9)
    eng = m.dual_stream_attention.engine()
    sh = ce.shape
    assert torch.equal(auto["blendshapes"], eng.sequence_forward_track(audio, track, sh["min_samples"], sh["update_samples"], stride))
    assert torch.equal(auto["blendshapes"], m(audio, emotion_track=track)["blendshapes"])
    # the track matters, and a constant track is the one-vector call
    v = dev(synth.normal(193, (2, 9)))
    const = m(audio, emotion_track=v[:, None, :].expand(2, 31, 9).contiguous())["blendshapes"]
    assert torch.equal(const, eng.sequence_forward(audio, v, stride)) and not torch.equal(const, auto["blendshapes"])
    with pytest.raises(ValueError, match="emotion_track"):
        m(audio, emotion_track=torch.zeros(2, 31, 256, device="cuda"))
    ce.close()


# ---- 4: the command line --------------------------------------------------------------------------------------------------------
def test_train_then_render_from_the_command_line(tmp_path):
    """train_sequential --variant basic --emotion basic writes a checkpoint that names its width and back end; render_sequential
    --emotion basic renders it, and the lines are the model's forward on the file's samples."""
    data = tmp_path / "data"
    data.mkdir()
    write_pair(data, "a", 8.7, 70)                                                # 261 frames: 6 windows of 256
    write_pair(data, "b", 8.6, 80)                                                # 258 frames: 3 windows
    ckdir = tmp_path / "ck"
    ts.main(["--data_dir", str(data), "--variant", "basic", "--emotion", "basic", "--epochs", "1", "--batch_size", "4",
             "--checkpoint_dir", str(ckdir)])
    path = ckdir / "checkpoint_epoch_1.pth"
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["model_config"] == {"d_model": 128, "num_heads": 4, "mel_sequence_length": 256, "emotion_dim": 9, "emotion_backend": "basic"}
    steps = sum(1 for _ in SequentialKoeMorphDataset(data, shuffle_files=False, loop_dataset=False, batch_size=4))
    assert ckpt["global_step"] == steps == 3 and ckpt["epoch"] == 1
    assert tuple(ckpt["model_state_dict"]["dual_stream_attention.emotion_encoder.weight"].shape)[1] == 9
    init = synth.make_core_params(0, 128, 256, 9, "init")
    assert not np.array_equal(ckpt["model_state_dict"]["dual_stream_attention.mel_channel_encoder.weight"].numpy(), init["mel_channel_encoder.weight"])

    out = tmp_path / "out.jsonl"
    wav = data / "a.wav"
    assert rs.main(["--model_path", str(path), "--input_audio", str(wav), "--output_json", str(out), "--emotion", "basic",
                    "--stride", "2"]) == 0
    lines = out.read_text().splitlines()
    with pytest.raises(ValueError) as exc:                                        # the eGeMAPS track is 256 wide, the checkpoint 9
        rs.load_model(path, emotion="egemaps")
    assert "256" in str(exc.value) and "9" in str(exc.value)

    ce = ClipEmotion(backend="basic")
    m = SequentialDualStreamModel(d_model=128, num_heads=4, mel_sequence_length=256, stride_frames=2, clip_emotion=ce,
                                  emotion_config={"backend": "basic"}).cuda().eval()
    m.load_state_dict(ckpt["model_state_dict"])
    samples = speech(70, 8.7)
    res = m(dev(samples)[None])
    want = res["blendshapes"][0].cpu().numpy()
    assert res["emotion_backend"] == "basic_track" and len(lines) == want.shape[0] >= 3
    for i, line in enumerate(lines):
        rec = json.loads(line)
        assert rec["timestamp"] == min(len(samples), (i * 2 + 256) * HOP) / 16000.0
        assert np.array_equal(np.asarray(rec["blendshapes"], np.float32), want[i]), i
    ce.close()
