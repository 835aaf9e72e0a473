"""The emotion track of a resident clip (km_emotion_clip_*): the offline producer of the model's 256-D emotion input.

A window's emotion vector is what a live ``StreamEmotion`` stream would hold at the moment the window ends -- a function of the
clip and an audio time, not of the window.  Updates are ``update_interval`` apart (0.3 s) and windows 33 ms, so about nine
windows share a row: ``build`` extracts the clip's track once, with the kernels the streams run, and a training step gathers
rows from it by start frame (``rows``), which reads no audio and so keeps the step on the resident clip.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Hashable, Optional, Tuple

import torch

from .. import _lib
from .._lib import check
from ..egemaps_names import feature_set_code
from ..engine import _ptr, _stream_ptr
from ..streaming import _create_emotion_backend, emotion_stream_shape


class ClipEmotion:
    """``build(clip)`` -> the clip's emotion track ``(K, 256)`` and its eGeMAPS functionals ``(K, 88)``: row ``k`` is what one
    ``StreamEmotion(1, context_window, update_interval)`` stream holds after ``min_samples + k * update_samples`` samples of the
    clip (pushed in chunks of ``gcd(min_samples, update_samples)`` with an update after each).  ``rows`` maps windows to rows:
    a window that starts at frame ``s`` with ``T`` frames of hop ``h`` ends at ``e = min(n, (s + T) h)`` and takes row
    ``clamp((e - min_samples) // update_samples, 0, K - 1)``; a clip shorter than half a second has no rows and every window of it
    a zero vector.  ``max_slots`` windows are extracted per pass (scratch: ``max_slots`` x frames x 36 floats of frame records).

    ``compression_layer``: ``StreamEmotion``'s contract -- a ``torch.nn.Linear(264, 256)``, created with torch's default
    initialisation when absent, copied at construction; hand the same layer to the server's ``StreamEmotion``.
    ``track_for(key, clip)`` keeps built tracks on the device: the layer is fixed, so a clip is extracted once per run.

    ``backend="basic"`` (km_emotion_clip_create_basic): the same windows and the same window -> row mapping, but a row is the nine
    raw prosodic values of its window -- bit for bit what a ``StreamEmotion(1, context_window, update_interval, backend="basic")``
    stream holds after that many samples, and bit for bit ``BasicEmotion()(window[None])[0]``.  ``emotion_dim`` is 9, the input of a
    model with ``emotion_dim`` 9; ``build`` -> ``(emotion (K, 9), None)``, ``build_batch`` -> ``((B, K, 9), None)``, ``rows`` takes and
    returns width 9.  There is no compression layer (passing one raises ``ValueError``); the window may hold up to 2**20 samples and
    the scratch is ``max_slots`` x ``(1 + window_len // 512)`` x 4 floats.

    ``long_windows=True`` (km_emotion_clip_create_long): eGeMAPS windows of up to 2**20 samples (65.5 s) instead of 2048 frames --
    ``ClipEmotion(30.0, 0.2, long_windows=True)`` is the track of the reference's ``long_context`` variant, bit for bit the rows of a
    ``StreamEmotion(1, 30.0, 0.2, long_windows=True)`` stream.  The scratch grows with the window: 0.43 MB per slot at 30 s.

    ``feature_set="GeMAPS"`` (km_emotion_clip_create_set): the 62 functionals of GeMAPS -- ``ClipEmotion(10.0, 0.5,
    feature_set="GeMAPS")`` is the track of the reference's ``fast`` variant.  ``feature_dim`` is 62, ``build`` -> ``(emotion (K, 256),
    features (K, 62))``, the layer a ``Linear(186, 256)``; ``StreamEmotion``'s notes on the set apply."""

    def __init__(self, context_window: float = 20.0, update_interval: float = 0.3, max_slots: int = 64,
                 compression_layer: Optional[torch.nn.Module] = None, device="cuda", backend: str = "egemaps", long_windows: bool = False,
                 feature_set: str = "eGeMAPSv02"):
        self.shape = emotion_stream_shape(context_window, update_interval, backend=backend, long_windows=long_windows, feature_set=feature_set)
        self.backend, self.long_windows, self.feature_set = backend, long_windows, feature_set
        if backend == "basic" and compression_layer is not None:
            raise ValueError("the basic back end has no compression layer: its nine features are the emotion input as they are")
        if not 1 <= max_slots <= 65535:
            raise ValueError(f"expected 1 <= max_slots <= 65535, got {max_slots}")
        if not torch.cuda.is_available():
            raise _lib.KoeMorphError(_lib.KM_ERR_HIP, "no GPU visible: the clip emotion track has no CPU fallback")
        self.context_window, self.update_interval, self.max_slots = context_window, update_interval, max_slots
        self._lib = _lib.load()
        create = (self._lib.km_emotion_clip_create_basic if backend == "basic" else
                  self._lib.km_emotion_clip_create_long if long_windows else self._lib.km_emotion_clip_create)
        make = lambda h: create(h, context_window, update_interval, max_slots)
        if feature_set_code(feature_set):
            make = lambda h: self._lib.km_emotion_clip_create_set(h, context_window, update_interval, max_slots, feature_set_code(feature_set),
                                                                  1 if long_windows else 0)
        self.device, self._h, self.compression_layer, self.emotion_dim, self.feature_dim = _create_emotion_backend(
            backend, compression_layer, device, make, self._lib.km_emotion_clip_set_compression, feature_set)
        self._tracks: Dict[Hashable, Tuple[torch.Tensor, int]] = {}
        self.builds = 0                                                   # calls of build() / build_batch(), track_for's misses included

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.km_emotion_clip_destroy(self._h)
            self._h = C.c_void_p()
        self._tracks = {}

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def num_rows(self, clip_len: int) -> int:
        return int(self._lib.km_emotion_clip_num_rows(self._h, int(clip_len)))

    def _check_clip(self, clip: torch.Tensor) -> torch.Tensor:
        if clip.dim() != 1 or clip.dtype != torch.float32 or not clip.is_cuda:
            raise ValueError(f"expected a 1-D float32 clip on the device, got {tuple(clip.shape)} {clip.dtype} on {clip.device}")
        return clip.contiguous()

    def build(self, clip: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """clip (n) fp32 on the device -> (emotion (K, 256), features (K, 88)); (emotion (K, 9), None) on the basic back end.
        No synchronisation."""
        clip = self._check_clip(clip)
        n = clip.shape[0]
        K = self.num_rows(n)
        emotion = torch.empty(K, self.emotion_dim, device=clip.device)
        features = torch.empty(K, self.feature_dim, device=clip.device) if self.backend != "basic" else None
        with torch.cuda.device(clip.device):
            check(self._lib.km_emotion_clip_build(self._h, _ptr(clip), n, _ptr(features) if features is not None else None, _ptr(emotion),
                                                  _stream_ptr(clip.device)))
        self.builds += 1
        return emotion, features

    def build_batch(self, clips: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """clips (B, L) fp32 on the device, B clips of one length -> (emotion (B, K, 256), features (B, K, 88)) -- ((B, K, 9), None) on
        the basic back end --; every clip's slice is bit-identical to ``build`` of that clip.  The passes of ``max_slots`` windows are filled across clip boundaries
        (km_emotion_clip_build_batch), so short clips do not leave them mostly empty.  One build in ``builds``; no synchronisation."""
        if clips.dim() != 2 or clips.dtype != torch.float32 or not clips.is_cuda:
            raise ValueError(f"expected (B, L) float32 clips on the device, got {tuple(clips.shape)} {clips.dtype} on {clips.device}")
        clips = clips.contiguous()
        B, L = clips.shape
        K = self.num_rows(L)
        emotion = torch.empty(B, K, self.emotion_dim, device=clips.device)
        features = torch.empty(B, K, self.feature_dim, device=clips.device) if self.backend != "basic" else None
        with torch.cuda.device(clips.device):
            check(self._lib.km_emotion_clip_build_batch(self._h, _ptr(clips), B, L, _ptr(features) if features is not None else None,
                                                        _ptr(emotion), _stream_ptr(clips.device)))
        self.builds += 1
        return emotion, features

    def rows(self, track: torch.Tensor, clip_len: int, start_frames_dev: torch.Tensor, hop: int, window_frames: int,
             out: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """track (K, 256) of a clip of ``clip_len`` samples, start_frames_dev (B) int32 on the device -> (B, 256): every window's
        row.  ``out`` (B, 256) fp32 and ``valid`` (B) uint8 are written in place when given (static buffers of a captured step);
        ``valid`` is 1 where the clip has a track at all.  One gather kernel, no synchronisation.  On the basic back end the
        width is 9 throughout."""
        D = self.emotion_dim
        if start_frames_dev.dim() != 1 or start_frames_dev.dtype != torch.int32 or not start_frames_dev.is_cuda:
            raise ValueError("expected (B,) int32 start frames on the device")
        if track.dim() != 2 or track.shape[1] != D or track.dtype != torch.float32:
            raise ValueError(f"expected a (K, {D}) float32 track, got {tuple(track.shape)} {track.dtype}")
        B = start_frames_dev.shape[0]
        dev = start_frames_dev.device
        if out is None:
            out = torch.empty(B, D, device=dev)
        elif tuple(out.shape) != (B, D) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"expected a contiguous ({B}, {D}) float32 out")
        if valid is not None and (tuple(valid.shape) != (B,) or valid.dtype != torch.uint8):
            raise ValueError(f"expected a ({B},) uint8 valid")
        track, starts = track.contiguous(), start_frames_dev.contiguous()
        with torch.cuda.device(dev):
            check(self._lib.km_emotion_clip_rows(self._h, _ptr(track) if track.shape[0] else None, track.shape[0], int(clip_len), _ptr(starts),
                                                 B, int(hop), int(window_frames), _ptr(out), _ptr(valid) if valid is not None else None,
                                                 _stream_ptr(dev)))
        return out

    def track_for(self, key: Hashable, clip: torch.Tensor) -> torch.Tensor:
        """The emotion track of ``clip``, built on first use and kept on the device under ``key`` (the data set's file index)."""
        hit = self._tracks.get(key)
        if hit is not None and hit[1] == clip.shape[0]:
            return hit[0]
        track, _ = self.build(clip)
        self._tracks[key] = (track, clip.shape[0])
        return track

    def clear(self) -> None:
        self._tracks = {}
