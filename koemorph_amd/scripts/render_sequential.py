"""Offline rendering of one audio file with a ``train_sequential`` checkpoint:

    python -m koemorph_amd.scripts.render_sequential --model_path ckpt.pth --input_audio a.wav --output_json out.jsonl
                                                     [--stride 1] [--emotion egemaps|basic|noise] [--attention-summary summary.json]
                                                     [--share-frames] [--emotion-context-window S] [--emotion-update-interval S]

The clip goes through ``SequentialDualStreamModel.forward`` (one output frame per window position, EMA along the clip) and every
frame is written as one ``{"timestamp", "blendshapes"}`` line, encoded by ``koemorph_amd.wire`` as the streaming scripts encode
theirs.  A frame's timestamp is the time at which its window ends.  ``--emotion egemaps`` gives every window the row of the
clip's eGeMAPS emotion track a live stream would hold at that time (``ClipEmotion``), the input ``train_sequential --emotion
egemaps`` trains on; ``basic`` is the same with the nine prosodic values per row (``ClipEmotion(backend="basic")``), for
checkpoints trained with ``--variant basic --emotion basic``; ``noise`` is the reference's extraction-failure fallback, one
``0.1 * randn`` vector per clip.  The checkpoint's ``model_config["emotion_dim"]`` (256 when absent) sizes the model.
``--attention-summary`` writes what the reference's AttentionVisualizer reduces the clip's attention maps to (``AttentionStats``:
mean map, mean entropy and peak histogram per mouth query, mean and share per frequency band) as one JSON object; the maps are
reduced on the device tile by tile, no (frames, 28, 80) array is made.  ``--share-frames`` computes the clip's STFT once at every
model shape and hop (``SequentialDualStreamModel(share_frames=True)``).  The emotion track's context window and update interval are
the checkpoint's (``model_config["emotion_context_window"]`` / ``["emotion_update_interval"]``, written by ``train_sequential`` when
its flags of the same names were given), else 20.0 s / 0.3 s; the two flags here set them for a checkpoint that carries none and are
refused where they contradict the checkpoint.
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .. import wire
from ..data.sequential_dataset import _load_wav, _read_wav
from ..features.clip_emotion import ClipEmotion
from ..metrics import AttentionStats
from ..model import SequentialDualStreamModel

logger = logging.getLogger(__name__)

COMPRESSION_SEED = 0          # the Linear(264, 256) of a checkpoint that carries none: torch's default initialisation under this seed


def compression_layer(ckpt: dict, n_in: int = 264) -> "tuple[torch.nn.Linear, str]":
    """The 264 -> 256 layer behind the emotion track and where it came from: ``ckpt["emotion_compression"]`` (``weight`` (256, 264),
    ``bias`` (256)) when the checkpoint carries one, else a seeded default initialisation.  ``n_in`` 186: the layer of a GeMAPS track."""
    saved = ckpt.get("emotion_compression")
    if saved is not None:
        layer = torch.nn.Linear(n_in, 256)
        layer.load_state_dict({"weight": torch.as_tensor(saved["weight"], dtype=torch.float32),
                               "bias": torch.as_tensor(saved["bias"], dtype=torch.float32)})
        return layer, "checkpoint"
    with torch.random.fork_rng(devices=[]):                # the caller's generator is left as it was
        torch.manual_seed(COMPRESSION_SEED)
        layer = torch.nn.Linear(n_in, 256)
    return layer, f"default initialisation, seed {COMPRESSION_SEED}"


class EmotionTimingError(ValueError):
    """A timing flag that contradicts the checkpoint, or one given without an emotion track (a usage error on the command line)."""


def emotion_timing(cfg: dict, context_window: Optional[float], update_interval: Optional[float]) -> "Optional[tuple[float, float]]":
    """(context window, update interval) of the emotion track, or None for the 20.0 s / 0.3 s object as ever: the checkpoint's
    values where it carries them, else the flags; a flag that contradicts the checkpoint is a ValueError."""
    saved = (cfg.get("emotion_context_window"), cfg.get("emotion_update_interval"))
    for name, flag, have in (("--emotion-context-window", context_window, saved[0]), ("--emotion-update-interval", update_interval, saved[1])):
        if flag is not None and have is not None and float(flag) != float(have):
            raise EmotionTimingError(f"{name} {flag:g} contradicts the checkpoint, which was trained with {float(have):g}")
    cw = saved[0] if saved[0] is not None else context_window
    ui = saved[1] if saved[1] is not None else update_interval
    if cw is None and ui is None:
        return None
    return float(20.0 if cw is None else cw), float(0.3 if ui is None else ui)


def emotion_feature_set(cfg: dict, emotion: str) -> str:
    """The feature set of the eGeMAPS track, from the checkpoint; ``--emotion egemaps`` on a checkpoint trained with ``--emotion gemaps``
    (``model_config["emotion_feature_set"] == "GeMAPS"``) and the reverse are refused with a text that names both."""
    saved = "gemaps" if cfg.get("emotion_feature_set", "eGeMAPSv02") == "GeMAPS" else "egemaps"
    if emotion in ("egemaps", "gemaps") and emotion != saved:
        names = {"egemaps": "eGeMAPSv02, 88 functionals", "gemaps": "GeMAPS, 62 functionals"}
        raise EmotionTimingError(f"--emotion {emotion} ({names[emotion]}) contradicts the checkpoint, which was trained with "
                                 f"--emotion {saved} ({names[saved]})")
    return "GeMAPS" if emotion == "gemaps" else "eGeMAPSv02"


def load_model(model_path, stride: int = 1, emotion: str = "egemaps", device: str = "cuda", share_frames: bool = False,
               emotion_context_window: Optional[float] = None, emotion_update_interval: Optional[float] = None) -> SequentialDualStreamModel:
    ckpt = torch.load(model_path, map_location="cpu", weights_only=True)
    cfg = dict(ckpt.get("model_config") or {})
    timing = emotion_timing(cfg, emotion_context_window, emotion_update_interval)
    feature_set = emotion_feature_set(cfg, emotion)
    if timing is not None and emotion == "noise":
        raise EmotionTimingError("the emotion track's context window and update interval need --emotion egemaps or basic")
    emotion_dim = int(cfg.get("emotion_dim", 256))
    width = {"egemaps": 256, "gemaps": 256, "basic": 9}.get(emotion)
    if width is not None and width != emotion_dim:
        raise ValueError(f"--emotion {emotion} produces {width} values per window, the checkpoint's emotion_dim is {emotion_dim}")
    clip_emotion: Optional[ClipEmotion] = None
    if emotion == "egemaps":
        layer, source = compression_layer(ckpt)
        logger.info("emotion track: eGeMAPS, compression layer from the %s", source)
        clip_emotion = (ClipEmotion(compression_layer=layer, device=device) if timing is None else
                        ClipEmotion(*timing, compression_layer=layer, device=device, long_windows=True))
    elif emotion == "gemaps":
        layer, source = compression_layer(ckpt, 186)
        logger.info("emotion track: GeMAPS (62 functionals), compression layer from the %s", source)
        clip_emotion = (ClipEmotion(compression_layer=layer, device=device, feature_set=feature_set) if timing is None else
                        ClipEmotion(*timing, compression_layer=layer, device=device, long_windows=True, feature_set=feature_set))
    elif emotion == "basic":
        logger.info("emotion track: the nine basic prosodic values per row")
        clip_emotion = ClipEmotion(device=device, backend="basic") if timing is None else ClipEmotion(*timing, device=device, backend="basic")
    model = SequentialDualStreamModel(d_model=int(cfg.get("d_model", 256)), num_heads=int(cfg.get("num_heads", 8)),
                                      mel_sequence_length=int(cfg.get("mel_sequence_length", 256)), stride_frames=stride,
                                      emotion_config={"emotion_dim": emotion_dim, "backend": "basic" if emotion_dim == 9 else "opensmile"},
                                      device=device, clip_emotion=clip_emotion, share_frames=share_frames)
    model.load_state_dict(ckpt["model_state_dict"])
    return model.to(device).eval()


def frame_timestamps(n_frames: int, audio_length: int, model: SequentialDualStreamModel) -> np.ndarray:
    """Seconds at which each output frame's window ends (the last, zero-padded window ends with the clip)."""
    ends = (np.arange(n_frames, dtype=np.int64) * model.stride_frames + model.window_frames) * model.hop_length
    return np.minimum(ends, audio_length) / float(model.sample_rate)


def attention_summary(stats: AttentionStats) -> dict:
    """``AttentionStats.compute()`` with lists for arrays."""
    plain = lambda v: v.tolist() if isinstance(v, np.ndarray) else v
    return {k: ({b: plain(x) for b, x in v.items()} if isinstance(v, dict) else plain(v)) for k, v in stats.compute().items()}


def load_audio_device_resample(path, sample_rate: int, device) -> torch.Tensor:
    """The file at its own rate, uploaded and converted to ``sample_rate`` on the device (``koemorph_amd.features.Resampler``)."""
    from ..features.resample import Resampler
    sr, data = _read_wav(Path(path))
    audio = torch.from_numpy(data).to(device)
    if sr == sample_rate or audio.shape[0] == 0:
        return audio
    return Resampler(sr, sample_rate, audio.device).clip(audio)


def render(model: SequentialDualStreamModel, audio, output_json, attention_summary_json=None) -> int:
    """audio (L), a NumPy array or a tensor already on the device -> one JSONL line per output frame; returns the number of frames
    written.  ``attention_summary_json``: where the attention statistics of the rendered windows go."""
    dev = next(model.parameters()).device
    stats = AttentionStats() if attention_summary_json is not None else None
    with torch.no_grad():
        x = audio.to(dev, torch.float32) if isinstance(audio, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(audio, np.float32)).to(dev)
        out = model(x[None], attention_stats=stats)
    if stats is not None:
        path = Path(attention_summary_json)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(attention_summary(stats)))
        stats.close()
    frames = out["blendshapes"][0].cpu().numpy()
    lines = wire.format_frames(frames, frame_timestamps(frames.shape[0], audio.shape[0], model))
    output_json = Path(output_json)
    output_json.parent.mkdir(parents=True, exist_ok=True)
    with open(output_json, "wb") as f:
        for line in lines:
            f.write(line + b"\n")
    return len(lines)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model_path", required=True)
    p.add_argument("--input_audio", required=True)
    p.add_argument("--output_json", required=True)
    p.add_argument("--stride", type=int, default=1, help="frames between two window positions")
    p.add_argument("--emotion", choices=("egemaps", "noise", "basic", "gemaps"), default="egemaps",
                   help="gemaps: the track of the 62 GeMAPS functionals, for checkpoints of train_sequential --emotion gemaps (the feature "
                        "set and the Linear(186, 256) are the checkpoint's; egemaps on such a checkpoint, and gemaps on any other, is "
                        "refused); basic: the clip's track of nine prosodic values per row, for checkpoints of train_sequential --variant basic "
                        "--emotion basic (emotion_dim 9); a back end whose width is not the checkpoint's emotion_dim is refused")
    p.add_argument("--attention-summary", default=None, metavar="PATH",
                   help="write the clip's attention statistics (AttentionStats.compute()) as JSON")
    p.add_argument("--device-resample", dest="device_resample", action="store_true",
                   help="upload the file at its own rate and convert it to the model's rate on the device")
    p.add_argument("--share-frames", dest="share_frames", action="store_true",
                   help="compute the clip's STFT once and assemble the windows on the device (engine option seq_assemble)")
    p.add_argument("--emotion-context-window", dest="emotion_context_window", type=float, default=None, metavar="SECONDS",
                   help="seconds of audio behind a row of the emotion track, for a checkpoint that does not say (default 20.0; "
                        "configs/model/dual_stream.yaml: fast 10, long_context 30); refused where it contradicts the checkpoint")
    p.add_argument("--emotion-update-interval", dest="emotion_update_interval", type=float, default=None, metavar="SECONDS",
                   help="seconds between two rows of the emotion track (default 0.3; fast 0.5, long_context 0.2); as above")
    p.add_argument("--device", default="cuda")
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    try:
        model = load_model(args.model_path, args.stride, args.emotion, args.device, args.share_frames, args.emotion_context_window,
                           args.emotion_update_interval)
    except EmotionTimingError as exc:
        build_parser().error(str(exc))
    if args.device_resample:
        audio = load_audio_device_resample(args.input_audio, model.sample_rate, next(model.parameters()).device)
    else:
        audio = _load_wav(Path(args.input_audio), model.sample_rate)
    n = render(model, audio, args.output_json, args.attention_summary)
    logger.info("%d frames (%.2f s of audio, stride %d, emotion %s) -> %s", n, audio.shape[0] / model.sample_rate, args.stride,
                args.emotion, args.output_json)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
