"""The `basic` back end of a clip's emotion track (km_emotion_clip_create_basic, ClipEmotion(backend="basic"), train_sequential
--variant / --emotion basic): what is decided on the host.  No GPU: the argument refusals that come before any device call, the
shape arithmetic against the row count law of tests/clip_emotion_cases.py, and the command line.
"""
import ctypes as C

import pytest
import torch

import clip_emotion_cases as cc
from koemorph_amd import _lib
from koemorph_amd.features import ClipEmotion
from koemorph_amd.scripts import render_sequential as rs
from koemorph_amd.scripts import train_sequential as ts
from koemorph_amd.streaming import emotion_stream_shape


def test_create_basic_refuses_bad_arguments_before_any_device_call():
    lib = _lib.load()
    h = C.c_void_p(1)
    assert lib.km_emotion_clip_create_basic(None, 1.0, 0.1, 4) == _lib.KM_ERR_INVALID_ARG
    assert b"km_emotion_clip_create_basic" in lib.km_last_error()
    for args, rc, text in (((0.5, 0.3, 4), _lib.KM_ERR_INVALID_ARG, b"Context window must be at least 1.0"),
                           ((1.0, 0.05, 4), _lib.KM_ERR_INVALID_ARG, b"Update interval must be at least 0.1"),
                           ((1.0, 1.5, 4), _lib.KM_ERR_INVALID_ARG, b"cannot be larger than context window"),
                           ((float("nan"), 0.3, 4), _lib.KM_ERR_INVALID_ARG, b"Context window"),
                           ((1.0, 0.1, 0), _lib.KM_ERR_INVALID_ARG, b"max_slots 0"),
                           ((1.0, 0.1, 65536), _lib.KM_ERR_INVALID_ARG, b"max_slots 65536"),
                           ((3601.0, 0.3, 4), _lib.KM_ERR_UNSUPPORTED, b"context window of 3601"),
                           ((66.0, 0.3, 4), _lib.KM_ERR_UNSUPPORTED, b"1056000 samples, at most 1048576")):       # C > 2^20
        h = C.c_void_p(1)
        assert lib.km_emotion_clip_create_basic(C.byref(h), *args) == rc, args
        assert not h.value and text in lib.km_last_error(), (args, lib.km_last_error())
    assert lib.km_emotion_clip_width(None) == 0
    assert lib.km_emotion_clip_num_rows(None, 56000) == 0


@pytest.mark.parametrize("ctx,itv", [(1.0, 0.1), (20.0, 0.3), (20.6, 0.3), (65.5, 0.5), (1.5, 0.7)])
def test_basic_shape_follows_the_row_count_law(ctx, itv):
    """R, C, U and MIN are the stream's whatever the back end; only the frame count and the window limit differ."""
    sh, want = emotion_stream_shape(ctx, itv, backend="basic"), cc.shape(ctx, itv)
    assert (sh["ring_len"], sh["window_len"], sh["update_samples"], sh["min_samples"]) == (want["R"], want["C"], want["U"], want["MIN"])
    assert sh["max_frames"] == 1 + want["C"] // 512
    for n in (0, want["MIN"] - 1, want["MIN"], want["MIN"] + want["U"] - 1, want["MIN"] + want["U"], want["R"] + 3 * want["U"] + 17):
        K = 0 if n < sh["min_samples"] else (n - sh["min_samples"]) // sh["update_samples"] + 1
        assert K == cc.num_rows(n, ctx, itv) == len(cc.plan(n, ctx, itv))
        for t, start, length in cc.plan(n, ctx, itv):
            assert 1 + length // 512 <= sh["max_frames"] and start + length <= n


def test_the_small_shape_of_the_gpu_tests():
    sh = emotion_stream_shape(1.0, 0.1, backend="basic")
    assert sh == dict(ring_len=48000, window_len=16000, update_samples=1600, min_samples=8000, max_frames=32)
    p = cc.plan(56000, 1.0, 0.1)
    assert len(p) == 31 and cc.num_rows(7999, 1.0, 0.1) == 0
    assert [length for _, _, length in p[:6]] == [8000, 9600, 11200, 12800, 14400, 16000]          # growing; 8000 and 9600 % 512 != 0
    assert all((s, length) == (0, 16000) for _, s, length in p[5:25])                              # the stale oldest second
    assert [(s, length) for _, s, length in p[25:]] == [(32000 + 1600 * i, 16000) for i in range(6)]     # sliding from t = R on
    assert cc.num_rows(368000, 20.0, 0.3) == 76


def test_basic_shape_refusals():
    with pytest.raises(ValueError, match="at most 1048576"):
        emotion_stream_shape(66.0, 0.3, backend="basic")
    with pytest.raises(ValueError, match="backend"):
        emotion_stream_shape(1.0, 0.1, backend="opensmile")
    assert emotion_stream_shape(20.6, 0.3, backend="basic")["max_frames"] == 644               # the 2048-frame eGeMAPS limit is not this one
    with pytest.raises(ValueError, match="at most 2048"):
        emotion_stream_shape(20.6, 0.3)


def test_clip_emotion_basic_value_errors():
    """Raised before a device is asked for, so they hold without one."""
    with pytest.raises(ValueError, match="no compression layer"):
        ClipEmotion(1.0, 0.1, backend="basic", compression_layer=torch.nn.Linear(264, 256))
    with pytest.raises(ValueError, match="no compression layer"):
        ClipEmotion(backend="basic", compression_layer=torch.nn.Linear(9, 9))
    with pytest.raises(ValueError, match="backend"):
        ClipEmotion(1.0, 0.1, backend="prosody")
    with pytest.raises(ValueError, match="at most 1048576"):
        ClipEmotion(66.0, 0.3, backend="basic")
    with pytest.raises(ValueError, match="max_slots"):
        ClipEmotion(1.0, 0.1, max_slots=0, backend="basic")


def test_train_sequential_variant_and_emotion_parsing(capsys):
    a = ts.parse_args(["--data_dir", "x"])
    assert (a.variant, a.emotion, a.d_model, a.num_heads, a.window_frames, a.emotion_dim) == ("default", "noise", 256, 8, 256, 256)
    a = ts.parse_args(["--data_dir", "x", "--variant", "basic", "--emotion", "basic"])
    assert (a.d_model, a.num_heads, a.window_frames, a.emotion_dim, a.emotion) == (128, 4, 256, 9, "basic")
    a = ts.parse_args(["--data_dir", "x", "--variant", "basic"])                   # noise at width 9 is allowed
    assert (a.emotion, a.emotion_dim) == ("noise", 9)
    a = ts.parse_args(["--data_dir", "x", "--variant", "fast"])
    assert (a.d_model, a.num_heads, a.window_frames, a.emotion_dim) == (128, 4, 128, 256)
    a = ts.parse_args(["--data_dir", "x", "--variant", "long_context", "--emotion", "egemaps"])
    assert (a.d_model, a.num_heads, a.window_frames, a.emotion_dim) == (512, 16, 512, 256)
    a = ts.parse_args(["--data_dir", "x", "--variant", "fast", "--window_frames", "64"])          # an explicit window wins
    assert a.window_frames == 64
    assert ts.build_parser().parse_args(["--data_dir", "x"]).window_frames == 256
    for argv in (["--emotion", "basic"], ["--variant", "default", "--emotion", "basic"], ["--variant", "fast", "--emotion", "basic"],
                 ["--variant", "long_context", "--emotion", "basic"]):
        with pytest.raises(SystemExit) as exc:
            ts.parse_args(["--data_dir", "x"] + argv)
        assert exc.value.code == 2
        err = capsys.readouterr().err
        assert "9" in err and "256" in err and "--variant basic" in err, err
    with pytest.raises(SystemExit):
        ts.parse_args(["--data_dir", "x", "--variant", "basic", "--emotion", "egemaps"])
    with pytest.raises(SystemExit):
        ts.parse_args(["--data_dir", "x", "--variant", "emotion2vec_fallback"])


def test_render_sequential_knows_basic_and_refuses_another_width(tmp_path):
    p = rs.build_parser()
    assert p.parse_args(["--model_path", "m", "--input_audio", "a", "--output_json", "o", "--emotion", "basic"]).emotion == "basic"
    assert p.parse_args(["--model_path", "m", "--input_audio", "a", "--output_json", "o"]).emotion == "egemaps"
    for cfg, emotion, a, b in (({"d_model": 128, "num_heads": 4, "mel_sequence_length": 256, "emotion_dim": 9}, "egemaps", "256", "9"),
                               ({"d_model": 256, "num_heads": 8, "mel_sequence_length": 256}, "basic", "9", "256")):
        path = tmp_path / f"{emotion}.pth"
        torch.save({"model_config": cfg, "model_state_dict": {}}, path)
        with pytest.raises(ValueError) as exc:                                     # before a model or a track object is built
            rs.load_model(path, emotion=emotion)
        assert a in str(exc.value) and b in str(exc.value) and emotion in str(exc.value)
