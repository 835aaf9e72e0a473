"""Rational sample-rate conversion: the filter, the integer laws and the device resampler (km_resampler_* / km_resample_clip).

The filter is the one of ``scipy.signal.resample_poly`` (a Kaiser-windowed sinc, ``firwin(2 half_len + 1, 1 / max(up, down),
window=('kaiser', beta)) * up`` with ``half_len = zeros * max(up, down)``), restated with NumPy alone.

The output law.  For input ``x[0..N)`` output ``m`` is ``y[m] = sum_j x[j] h[m down - j up + half_len]`` over the ``j`` whose tap
index lies in ``[0, 2 half_len]`` and ``0 <= j < N``; ``n_out(N) = ceil(N up / down)``.

The streaming law.  After a stream has consumed ``N`` samples the outputs that no longer depend on future input are
``m < emitted(N) = max(0, ceil((N up - half_len) / down))``: output ``m`` reads samples up to ``floor((m down + half_len) / up)``.
A stream therefore needs two things only, neither of which grows with the session: the last ``ceil(2 half_len / up)`` input
samples and the integer ``d = emitted down + half_len - N up`` -- the tap position of its next output relative to the next
sample -- which stays inside ``[0, max(half_len, down - 1)]``.  ``StreamPlan`` is that state in Python; the kernels keep the same.
"""
from __future__ import annotations

import ctypes as C
from math import gcd
from typing import Optional, Tuple

import numpy as np

CLIP_TILE = 1024      # outputs per workgroup of the kernels (km_resample.hip: RS_TILE)


def resample_ratio(rate_in: int, rate_out: int) -> Tuple[int, int]:
    """(up, down): both rates divided by their gcd."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError(f"sample rates must be positive, got {rate_in} -> {rate_out}")
    g = gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def resample_filter(up: int, down: int, zeros: int = 10, beta: float = 5.0) -> Tuple[np.ndarray, int]:
    """(h float64 of 2 half_len + 1 taps, half_len): fc sinc(fc k) kaiser(beta), normalised to unit sum, times ``up``."""
    if up < 1 or down < 1:
        raise ValueError(f"up and down must be positive, got {up}, {down}")
    max_rate = max(up, down)
    half_len = zeros * max_rate
    fc = 1.0 / max_rate
    k = np.arange(2 * half_len + 1, dtype=np.float64) - half_len
    h = fc * np.sinc(fc * k) * np.kaiser(2 * half_len + 1, beta)
    h /= h.sum()
    return h * up, half_len


def n_out(n: int, up: int, down: int) -> int:
    return -((-n * up) // down)


def emitted(n: int, up: int, down: int, half_len: int) -> int:
    return max(0, -((half_len - n * up) // down))


def history_len(up: int, half_len: int) -> int:
    return -((-2 * half_len) // up)


class StreamPlan:
    """The per-stream state of the streaming law in Python integers: ``d`` and (optionally) the history tail."""

    def __init__(self, up: int, down: int, half_len: int):
        self.up, self.down, self.half_len = up, down, half_len
        self.history = history_len(up, half_len)
        self.reset()

    def reset(self) -> None:
        self.d = self.half_len
        self.tail = np.zeros(self.history, dtype=np.float32)

    def push(self, n: int, samples: Optional[np.ndarray] = None) -> int:
        """Consume ``n`` samples; the number of outputs that became final."""
        if n < 0:
            raise ValueError("n must not be negative")
        if n == 0:
            return 0
        total = n * self.up
        count = -((self.d - total) // self.down) if total > self.d else 0
        self.d += count * self.down - total
        if samples is not None:
            self.tail = np.concatenate([self.tail, np.asarray(samples, dtype=np.float32)[:n]])[-self.history:] \
                if self.history else self.tail
        return count

    def flush(self) -> int:
        """The outputs still owed up to n_out(N), as though zeros followed; the stream is reset."""
        count = -((self.d - self.half_len) // self.down) if self.d < self.half_len else 0
        self.reset()
        return count


def _check_rate_pair(rate_in: int, rate_out: int) -> Tuple[int, int]:
    up, down = resample_ratio(rate_in, rate_out)
    if up == down:
        raise ValueError(f"nothing to resample: {rate_in} -> {rate_out}")
    return up, down


def create_handle(lib, n_streams: int, up: int, down: int) -> Tuple[C.c_void_p, int]:
    """km_resampler_create with ``resample_filter``'s taps -> (handle, half_len)."""
    from .._lib import check
    h, half_len = resample_filter(up, down)
    h = np.ascontiguousarray(h, dtype=np.float64)
    handle = C.c_void_p()
    check(lib.km_resampler_create(C.byref(handle), n_streams, up, down, h.ctypes.data_as(C.POINTER(C.c_double)), h.size))
    return handle, half_len


class Resampler:
    """Whole clips at ``rate_in`` -> ``rate_out`` on the device (km_resample_clip): the output law with zero-padded edges."""

    def __init__(self, rate_in: int, rate_out: int = 16000, device="cuda"):
        import torch
        from .. import _lib
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self.up, self.down = _check_rate_pair(rate_in, rate_out)
        if not torch.cuda.is_available():
            raise _lib.KoeMorphError(_lib.KM_ERR_HIP, "no GPU visible: the resampler has no CPU fallback")
        self.device = torch.device(device if device not in (None, "cpu", "auto") else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _lib.load()
        with torch.cuda.device(self.device):
            self._h, self.half_len = create_handle(self._lib, 1, self.up, self.down)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.km_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def n_out(self, n: int) -> int:
        return n_out(n, self.up, self.down)

    def clip(self, audio):
        """audio (n,) fp32 on the device -> (ceil(n up / down),) fp32."""
        import torch
        from .._lib import check
        if audio.dim() != 1 or audio.dtype != torch.float32 or audio.device != self.device or audio.shape[0] < 1:
            raise ValueError(f"expected a non-empty (n,) float32 tensor on {self.device}, got {tuple(audio.shape)} {audio.dtype} "
                             f"on {audio.device}")
        audio = audio.contiguous()
        out = torch.empty(self.n_out(audio.shape[0]), device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.km_resample_clip(self._h, audio.data_ptr(), audio.shape[0], out.data_ptr(), out.shape[0],
                                             torch.cuda.current_stream(self.device).cuda_stream))
        return out
