#!/usr/bin/env python3
"""Real-time blendshape inference with ``SimplifiedKoeMorphModel`` -- drop-in for the reference's ``scripts/rt_simplified.py``,
its one working real-time entry point, for checkpoints written by ``koemorph_amd.scripts.train`` or the reference's ``src/train.py``.

Same behaviour (scripts/rt_simplified.py:315-405): audio chunks go into a 2 s consuming FIFO; whenever ``audio_length`` samples
are available they are consumed and the model maps them to one 52-coefficient frame.  Here the FIFO and the model live on the GPU
(``LegacyStreamEngine`` with one stream: km_legacy_stream_push / km_legacy_stream_tick); a chunk is the only upload, a frame the only
readback.  The capture, output and file-reading classes are those of ``scripts/rt.py``.

``--input_file`` is deterministic, unlike the reference's playback thread (:124-149): the chunks are pushed in order with the last
one zero padded (:134-136), one ``inference_step`` follows each chunk, nothing sleeps, and a frame's timestamp is the audio time
at which it was produced.
"""
from __future__ import annotations

import argparse
import logging
import queue
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import rt
from ..streaming import LegacyStreamEngine

logger = logging.getLogger(__name__)


class SimplifiedRealTimeInference:
    """``process_audio_chunk`` / ``inference_step`` / ``reset`` / ``frame_count`` of the reference class (:315-405)."""

    def __init__(self, model_path: Optional[str], sample_rate: int = 16000, target_fps: float = 30.0, buffer_duration: float = 2.0,
                 device: str = "auto", audio_length: int = 16000, model=None):
        self.sample_rate, self.target_fps, self.audio_length = sample_rate, target_fps, audio_length
        if device == "auto":
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("koemorph_amd runs on the GPU only (no CPU fallback by design)")
        self.model = model if model is not None else self._load_model(model_path)
        self.engine = LegacyStreamEngine(self.model, 1, buffer_duration=buffer_duration, audio_length=audio_length)
        self.frame_count = 0

    def _load_model(self, model_path: str):
        from ..model import SimplifiedKoeMorphModel
        checkpoint = torch.load(model_path, map_location="cpu", weights_only=True)
        model = SimplifiedKoeMorphModel(d_model=256, num_blendshapes=52, sample_rate=self.sample_rate, target_fps=int(self.target_fps))
        model.load_state_dict(checkpoint["model_state_dict"])
        return model.to(self.device).eval()

    def process_audio_chunk(self, audio_chunk: np.ndarray) -> None:
        chunk = np.ascontiguousarray(audio_chunk, dtype=np.float32).reshape(1, -1)
        if chunk.shape[1]:
            self.engine.push(torch.from_numpy(chunk).to(self.device))

    def inference_step(self) -> Optional[np.ndarray]:
        out, ready = self.engine.tick()
        if not int(ready[0]):
            return None
        self.frame_count += 1
        return out[0].cpu().numpy()

    def reset(self) -> None:
        self.frame_count = 0
        self.engine.reset()
        self.model.reset_temporal_state()


def run_file(inference: SimplifiedRealTimeInference, streamer: "rt.BlendshapeStreamer", input_file: str, chunk_size: int = 1024,
             duration: Optional[float] = None) -> int:
    """Feed the file chunk by chunk, one inference step per chunk.  Returns the number of frames sent."""
    sent = 0
    for i, chunk in enumerate(rt.AudioFileReader(input_file, inference.sample_rate, chunk_size)):
        now = (i + 1) * chunk_size / float(inference.sample_rate)
        if duration and now > duration:
            break
        inference.process_audio_chunk(chunk)
        blendshapes = inference.inference_step()
        if blendshapes is not None:
            streamer.send(blendshapes, now)
            sent += 1
    return sent


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Real-time simplified KoeMorph inference")
    parser.add_argument("--model_path", type=str, required=True, help="Path to trained model checkpoint")
    parser.add_argument("--sample_rate", type=int, default=16000, help="Audio sample rate")
    parser.add_argument("--target_fps", type=float, default=30.0, help="Target blendshape frame rate")
    parser.add_argument("--chunk_size", type=int, default=1024, help="Audio chunk size for capture")
    parser.add_argument("--audio_length", type=int, default=16000, help="Audio length for each inference (samples)")
    parser.add_argument("--input_file", type=str, help="Input audio file for processing (instead of microphone)")
    parser.add_argument("--output_mode", type=str, default="udp", choices=["udp", "osc", "file"], help="Output mode for blendshapes")
    parser.add_argument("--host", type=str, default="127.0.0.1", help="Output host")
    parser.add_argument("--port", type=int, default=9001, help="Output port")
    parser.add_argument("--output_file", type=str, help="Output file for file mode")
    parser.add_argument("--device", type=str, default="auto", help="Computation device")
    parser.add_argument("--duration", type=float, help="Duration to run (seconds), None for infinite")
    parser.add_argument("--no_audio", action="store_true", help="Disable audio capture (test mode)")
    return parser


def main(argv=None) -> Optional[int]:
    args = build_parser().parse_args(argv)
    if not Path(args.model_path).exists():
        logger.error(f"Model file not found: {args.model_path}")
        return None
    if args.input_file and not Path(args.input_file).exists():
        logger.error(f"Input file not found: {args.input_file}")
        return None
    inference = SimplifiedRealTimeInference(model_path=args.model_path, sample_rate=args.sample_rate, target_fps=args.target_fps,
                                            device=args.device, audio_length=args.audio_length)
    streamer = rt.BlendshapeStreamer(output_mode=args.output_mode, host=args.host, port=args.port, output_file=args.output_file)
    audio_capture = None
    try:
        if args.input_file:
            sent = run_file(inference, streamer, args.input_file, args.chunk_size, args.duration)
        else:
            audio_queue: queue.Queue = queue.Queue(maxsize=100)
            if not args.no_audio and rt.HAS_PYAUDIO:
                audio_capture = rt.AudioCapture(sample_rate=args.sample_rate, chunk_size=args.chunk_size, audio_queue=audio_queue)
                audio_capture.start()
            sent = rt.run_loop(inference, streamer, args, audio_queue)
        logger.info(f"Sent {sent} frames")
        return sent
    except KeyboardInterrupt:
        logger.info("Interrupted by user")
        return None
    finally:
        if audio_capture:
            audio_capture.stop()
        streamer.close()


if __name__ == "__main__":
    main()
