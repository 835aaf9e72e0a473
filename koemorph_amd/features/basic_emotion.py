"""The ``basic`` prosodic emotion features on the device (km_prosody_*): the producer of the model's 9-D emotion input.

Mirrors ``EmotionExtractor._extract_basic`` of the reference (src/features/emotion_extractor.py:503-545), which ``forward`` calls
once per batch row on the whole audio it was handed (:280-300): ``[energy, zcr, spectral_centroid, f0_mean, f0_std, mean, std,
max, min]``, raw, with no normalisation.

PARITY UNPINNED.  The reference computes three of the nine with librosa (``zero_crossing_rate``, ``spectral_centroid``,
``yin(fmin=50, fmax=400)``) and pins only ``librosa>=0.10.0``.  The kernels follow a restatement of what those functions do at
their 0.10 defaults (tests/prosody_cases.py, the header of km_prosody.hip) which has not been checked against the package; what is
tested is kernels == that restatement in float64, plus known answers.  One deliberate deviation: yin's difference function is the
direct sum of squared differences instead of librosa's FFT autocorrelation with terms below 1e-6 zeroed.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from .._lib import check
from ..engine import _ptr, _stream_ptr

FEATURE_NAMES = ("energy", "zcr", "spectral_centroid", "f0_mean", "f0_std", "mean", "std", "max", "min")
FRAME_FIELDS = ("zcr", "spectral_centroid", "f0", "period_index")
MAX_SAMPLES, MAX_ROWS = 1 << 20, 65535


class BasicEmotion:
    """``BasicEmotion()(audio (B, L)) -> (B, 9)``; usable as a model's ``emotion_provider``.  ``frames`` gives the per-frame records
    ``(B, F, 4)`` = (crossing rate, centroid in Hz, f0 in Hz, the chosen index into yin's 281 candidate periods) of the ``F = 1 + L
    // 512`` centred 2048-sample frames; ``windows`` extracts windows of a clip that stays where it is.  A window gives the same
    bits through each of the three (and through ``StreamEmotion(backend="basic")``).  The scratch buffer grows on demand and is
    kept, so a call at a shape already seen allocates only its result."""

    FEATURE_NAMES = FEATURE_NAMES

    def __init__(self, device="cuda"):
        if not torch.cuda.is_available():
            raise _lib.KoeMorphError(_lib.KM_ERR_HIP, "no GPU visible: the basic emotion features have no CPU fallback")
        self.device = torch.device(device if device not in (None, "cpu", "auto") else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _lib.load()
        self._plan = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self._lib.km_prosody_plan_create(C.byref(self._plan)))
        self._work: Optional[torch.Tensor] = None

    def close(self) -> None:
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self._lib.km_prosody_plan_destroy(self._plan)
            self._plan = C.c_void_p()
        self._work = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def num_frames(self, L: int) -> int:
        return int(self._lib.km_prosody_num_frames(int(L)))

    def _workspace(self, rows: int, L: int) -> torch.Tensor:
        need = int(self._lib.km_prosody_workspace_floats(rows, L))
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, device=self.device)
        return self._work

    def _rows(self, audio: torch.Tensor) -> torch.Tensor:
        if audio.dim() != 2:
            raise ValueError(f"Expected 2D audio (B, L), got {audio.dim()}D")
        B, L = audio.shape
        if not 1 <= L <= MAX_SAMPLES or not 1 <= B <= MAX_ROWS:
            raise ValueError(f"expected 1 <= B <= {MAX_ROWS} rows of 1 <= L <= {MAX_SAMPLES} samples, got {(B, L)}")
        audio = audio.to(self.device, torch.float32)
        if audio.stride(1) != 1 or (B > 1 and audio.stride(0) < L):        # rows of a wider matrix are read where they lie
            audio = audio.contiguous()
        return audio

    def __call__(self, audio: torch.Tensor) -> torch.Tensor:
        """audio (B, L) fp32 -> (B, 9) on the device.  No synchronisation."""
        audio = self._rows(audio)
        B, L = audio.shape
        work = self._workspace(B, L)
        out = torch.empty(B, 9, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.km_prosody_features(self._plan, _ptr(audio), B, L, audio.stride(0) if B > 1 else L, _ptr(work), work.numel(),
                                                _ptr(out), None, _stream_ptr(self.device)))
        return out

    def frames(self, audio: torch.Tensor) -> torch.Tensor:
        """audio (B, L) fp32 -> the per-frame records (B, F, 4), fields ``FRAME_FIELDS``."""
        audio = self._rows(audio)
        B, L = audio.shape
        rec = torch.empty(B, self.num_frames(L), 4, device=self.device)
        out = torch.empty(B, 9, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.km_prosody_features(self._plan, _ptr(audio), B, L, audio.stride(0) if B > 1 else L, None, 0, _ptr(out), _ptr(rec),
                                                _stream_ptr(self.device)))
        return rec

    def windows(self, clip: torch.Tensor, start_samples: torch.Tensor, length: int) -> torch.Tensor:
        """clip (n) fp32 on the device, start_samples (W) int32 on the device -> (W, 9): row w is ``self(clip[s:s + length][None])[0]``
        for s = start_samples[w], bit for bit -- shortened to what the clip holds, and a zero row where that is nothing.  Reads the
        clip in place and the starts on the device: no gather, no synchronisation."""
        if clip.dim() != 1 or clip.dtype != torch.float32 or not clip.is_cuda or clip.shape[0] < 1:
            raise ValueError(f"expected a non-empty 1-D float32 clip on the device, got {tuple(clip.shape)} {clip.dtype} on {clip.device}")
        if start_samples.dim() != 1 or start_samples.dtype != torch.int32 or not start_samples.is_cuda:
            raise ValueError("expected (W,) int32 start samples on the device")
        W, length = start_samples.shape[0], int(length)
        if not 1 <= length <= MAX_SAMPLES or not 1 <= W <= MAX_ROWS:
            raise ValueError(f"expected 1 <= W <= {MAX_ROWS} windows of 1 <= length <= {MAX_SAMPLES} samples, got {(W, length)}")
        clip, starts = clip.contiguous(), start_samples.contiguous()
        work = self._workspace(W, length)
        out = torch.empty(W, 9, device=clip.device)
        with torch.cuda.device(clip.device):
            check(self._lib.km_prosody_windows(self._plan, _ptr(clip), clip.shape[0], _ptr(starts), W, length, _ptr(work), work.numel(),
                                               _ptr(out), _stream_ptr(clip.device)))
        return out
