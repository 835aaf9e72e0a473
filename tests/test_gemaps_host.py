"""The GeMAPS feature set without a GPU: its definition (the 62 of the 88 columns, their names), the twin layer of
tests/gemaps_cases.py against a float64 product, that ``emotion_stream_shape`` returns what it returned, the Python refusals with
their texts, and how the two scripts resolve ``--emotion gemaps``."""
import numpy as np
import pytest
import torch

import gemaps_cases as gc
from koemorph_amd import egemaps_names as names
from koemorph_amd.features import ClipEmotion
from koemorph_amd.features.opensmile_extractor import OpenSMILEeGeMAPSExtractor, create_opensmile_extractor
from koemorph_amd.scripts import render_sequential as rs
from koemorph_amd.scripts import train_sequential as ts
from koemorph_amd.streaming import StreamEmotion, emotion_stream_shape


# ---- the definition ---------------------------------------------------------------------------------------------------
def test_columns_are_the_88_without_the_listed_26():
    assert list(names.GEMAPS_COLUMNS) == list(gc.COLUMNS) == sorted(names.GEMAPS_COLUMNS)
    assert len(names.GEMAPS_COLUMNS) == 62 and len(gc.REMOVED) == 26 and len(set(gc.REMOVED)) == 26
    assert len(names.GEMAPS_COLUMNS) + len(gc.REMOVED) == 88 == len(names.FEATURE_NAMES)
    assert sorted(set(names.GEMAPS_COLUMNS) | set(gc.REMOVED)) == list(range(88))


def test_names():
    assert names.GEMAPS_FEATURE_NAMES == [names.FEATURE_NAMES[i] for i in names.GEMAPS_COLUMNS]
    gone = [names.FEATURE_NAMES[i] for i in gc.REMOVED]
    for word, count in (("spectralFlux", 5), ("mfcc", 16), ("F2bandwidth", 2), ("F3bandwidth", 2), ("equivalentSoundLevel", 1)):
        assert sum(word in n for n in gone) == count, word
        assert not any(word in n for n in names.GEMAPS_FEATURE_NAMES), word
    assert len(set(names.GEMAPS_FEATURE_NAMES)) == 62
    # what GeMAPS keeps of the families it thins: F1's bandwidth, and nothing else of the removed kinds
    assert "F1bandwidth_sma3nz_amean" in names.GEMAPS_FEATURE_NAMES and names.GEMAPS_FEATURE_NAMES[-1] == "StddevUnvoicedSegmentLength"
    assert names.FEATURE_SET_DIMS == {"eGeMAPSv02": 88, "GeMAPS": 62}
    assert names.feature_set_code("eGeMAPSv02") == 0 and names.feature_set_code("GeMAPS") == 1


# ---- the twin ---------------------------------------------------------------------------------------------------------
def test_scatter_compression_against_a_float64_product():
    layer = gc.l186()
    twin = gc.scatter_compression(layer)
    assert tuple(twin.weight.shape) == (256, 264) and int((twin.weight == 0).sum()) == 256 * 78
    assert torch.equal(twin.bias, layer.bias)
    rng = np.random.RandomState(7)
    x = rng.normal(0.0, 30.0, (5, 3, 88))                            # three windows of 88, as the objects concatenate them
    W186, W264 = layer.weight.detach().numpy().astype(np.float64), twin.weight.detach().numpy().astype(np.float64)
    want = x[:, :, gc.COLS].reshape(5, 186) @ W186.T
    got = x.reshape(5, 264) @ W264.T
    scale = np.abs(x[:, :, gc.COLS].reshape(5, 186)) @ np.abs(W186).T
    assert (np.abs(got - want) <= 264 * 2.0 ** -53 * scale).all()    # the same 186 products, summed in another order
    # every kept column carries its weight, window by window
    for w in range(3):
        assert torch.equal(twin.weight[:, gc.COLS + 88 * w], layer.weight[:, 62 * w:62 * (w + 1)])


# ---- emotion_stream_shape ---------------------------------------------------------------------------------------------
KEYS = {"ring_len", "window_len", "update_samples", "min_samples", "max_frames"}


@pytest.mark.parametrize("args, kw", [((), {}), ((10.0, 0.5), {}), ((1.0, 0.1), {}), ((30.0, 0.2), {"long_windows": True}),
                                      ((20.0, 0.3), {"backend": "basic"}), ((20.0, 0.3, 16000), {"backend": "egemaps"})])
def test_emotion_stream_shape_is_unchanged(args, kw):
    plain = emotion_stream_shape(*args, **kw)
    assert set(plain) == KEYS
    assert emotion_stream_shape(*args, feature_set="eGeMAPSv02", **kw) == plain
    if kw.get("backend") != "basic":
        assert emotion_stream_shape(*args, feature_set="GeMAPS", **kw) == plain
    assert emotion_stream_shape() == dict(ring_len=352000, window_len=320000, update_samples=4800, min_samples=8000, max_frames=1995)
    assert emotion_stream_shape(10.0, 0.5)["max_frames"] == 995            # the `fast` variant's windows


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_python_refusals():
    for make in (lambda: emotion_stream_shape(feature_set="GeMAPSv01b"), lambda: StreamEmotion(2, feature_set="GeMAPSv01b"),
                 lambda: ClipEmotion(feature_set="GeMAPSv01b"), lambda: OpenSMILEeGeMAPSExtractor(feature_set="GeMAPSv01b"),
                 lambda: create_opensmile_extractor({"feature_set": "GeMAPSv01b"})):
        with pytest.raises(ValueError, match=r"^Unsupported feature set: GeMAPSv01b$"):
            make()
    for make in (lambda: emotion_stream_shape(backend="basic", feature_set="GeMAPS"), lambda: StreamEmotion(2, backend="basic", feature_set="GeMAPS"),
                 lambda: ClipEmotion(backend="basic", feature_set="GeMAPS")):
        with pytest.raises(ValueError, match="feature_set is the eGeMAPS back end's choice"):
            make()
    with pytest.raises(ValueError, match=r"compression_layer must be a Linear\(186, 256\), got weight \(256, 264\)"):
        names.check_compression_shape(torch.nn.Linear(264, 256), "GeMAPS")
    with pytest.raises(ValueError, match=r"compression_layer must be a Linear\(264, 256\), got weight \(256, 186\)"):
        names.check_compression_shape(torch.nn.Linear(186, 256))
    names.check_compression_shape(torch.nn.Linear(186, 256), "GeMAPS")


# ---- the scripts ------------------------------------------------------------------------------------------------------
def test_train_sequential_arguments(capsys):
    fast = ["--data_dir", "x", "--variant", "fast", "--emotion", "gemaps", "--emotion-context-window", "10", "--emotion-update-interval", "0.5"]
    args = ts.parse_args(fast)
    assert (args.emotion, args.d_model, args.num_heads, args.window_frames, args.emotion_dim) == ("gemaps", 128, 4, 128, 256)
    assert args.emotion_timing_given and (args.emotion_context_window, args.emotion_update_interval) == (10.0, 0.5)
    assert not ts.parse_args(["--data_dir", "x", "--emotion", "gemaps"]).emotion_timing_given
    with pytest.raises(SystemExit) as exit_:
        ts.parse_args(["--data_dir", "x", "--variant", "basic", "--emotion", "gemaps"])
    assert exit_.value.code == 2
    assert "--emotion gemaps produces 256 values per window, the emotion_dim of --variant basic is 9" in capsys.readouterr().err
    layer = ts.gemaps_compression_layer()
    assert tuple(layer.weight.shape) == (256, 186) and torch.equal(layer.weight, ts.gemaps_compression_layer().weight)


def test_render_sequential_refuses_the_other_feature_set(tmp_path, capsys):
    assert rs.emotion_feature_set({}, "egemaps") == "eGeMAPSv02"
    assert rs.emotion_feature_set({"emotion_feature_set": "GeMAPS"}, "gemaps") == "GeMAPS"
    assert rs.emotion_feature_set({"emotion_feature_set": "GeMAPS"}, "noise") == "eGeMAPSv02"      # no track, nothing to contradict
    with pytest.raises(rs.EmotionTimingError, match=r"--emotion egemaps \(eGeMAPSv02.*contradicts the checkpoint.*--emotion gemaps \(GeMAPS"):
        rs.emotion_feature_set({"emotion_feature_set": "GeMAPS"}, "egemaps")
    with pytest.raises(rs.EmotionTimingError, match=r"--emotion gemaps \(GeMAPS.*contradicts the checkpoint.*--emotion egemaps \(eGeMAPSv02"):
        rs.emotion_feature_set({"emotion_backend": "egemaps"}, "gemaps")
    # through the command line: a usage error before anything touches the device
    cfg = {"d_model": 128, "num_heads": 4, "mel_sequence_length": 128, "emotion_dim": 256, "emotion_backend": "egemaps"}
    for name, extra, flag in (("g.pth", {"emotion_feature_set": "GeMAPS"}, "egemaps"), ("e.pth", {}, "gemaps")):
        torch.save({"model_config": {**cfg, **extra}, "model_state_dict": {}}, tmp_path / name)
        with pytest.raises(SystemExit) as exit_:
            rs.main(["--model_path", str(tmp_path / name), "--input_audio", "a.wav", "--output_json", str(tmp_path / "o.jsonl"), "--emotion", flag])
        assert exit_.value.code == 2 and "contradicts the checkpoint" in capsys.readouterr().err
    layer, source = rs.compression_layer({"emotion_compression": {"weight": torch.ones(256, 186), "bias": torch.zeros(256)}}, 186)
    assert source == "checkpoint" and tuple(layer.weight.shape) == (256, 186)
