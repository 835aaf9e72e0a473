"""Many concurrent speaker streams with device-resident state (BASELINE config 5: 1024 streams, 128 per GPU).

Five model shapes have a streaming core -- every variant of the reference's model config: d_model 256 / 8 heads / window 256 (the
30 fps configuration: 8.5 s ring, hop 532), d_model 128 / 4 heads / window 128 (``fast``) and window 256 (``basic``) on the same ring
and front end, d_model 256 / 8 heads / window 512 (what the ``frame_rate=60`` recipe trains) and d_model 512 / 8 or 16 heads / window
512 (``long_context``); the two 60 fps shapes with ``update_interval=1/60``, ring hop 266 and the front end at hop 266.
Any other shape raises ``KoeMorphError`` from ``tick``.

Each stream owns an 8.5 s audio ring (``MelAudioBuffer`` semantics, reference
src/features/mel_sliding_window.py:28-140), and an EMA state; both live in the km_handle on the GPU and never
move.  A tick is ``push`` (one ~hop-sized frame per stream, the only host->device traffic: n_streams x 533
floats) followed by ``tick`` (emotion kernel, sliding-window front end over every full ring, fused core with
per-stream EMA).  Neither allocates nor synchronises, so ``capture()`` records one tick into a hipGraph and
``replay()`` re-launches it with a single API call per 33 ms frame.

``tick`` / ``step`` with ``return_attention=True`` also return the model's other two outputs for the streams they computed (km_stream_tick_attn
/ km_stream_step_attn): ``raw``, the sigmoid values before the stream weights and the EMA, and ``mel_attention_weights``, the head-averaged
attention map of the mel stream.  ``capture(..., return_attention=True, stats=acc)`` records them and, gated on ``ready`` / ``fired``, the
masked update of an ``AttentionStats`` / ``StreamAttentionStats`` accumulator into the same graph.

``ChunkedStreamEngine`` serves streams that are out of phase: chunks of any size are fed into a consuming FIFO per stream
(the reference's ``RingBuffer``, scripts/rt.py:48-99), a step pops one frame from every stream that holds one and computes only
the streams that popped onto a full ring, and ``reset_streams`` hands one slot to the next speaker (km_stream_fifo_create / _feed /
_step / _reset_streams).

``StreamEmotion`` keeps the emotion half of the streams on the device as well: the audio pushed into it feeds one ring per stream,
and ``update`` runs the reference's eGeMAPS extractor state machine (src/features/opensmile_extractor.py) for all streams at once;
its ``emotion`` matrix is what ``tick`` / ``step`` read (km_emotion_stream_*).

``LegacyStreamEngine`` is the counterpart for ``SimplifiedKoeMorphModel``: the reference's consuming FIFO
(scripts/rt_simplified.py:46-97) per stream instead of a sliding ring, no EMA, no emotion input (km_legacy_stream_*).

``KoeMorphStreams`` serves the multi-layer ``KoeMorphModel`` at the row level: per stream the last rows of both feature tracks, the
frame counter, the previous frame and the smoother state on the device, one ragged four-launch ``step`` per tick (km_koemorph_stream_*).

``AudioRowStreams`` produces those rows from pushed 16 kHz audio -- per stream a ring of samples and a sample counter on the device, a
seven-launch ``push`` that gives the mel and eGeMAPS descriptor rows of the frames that became due -- and ``KoeMorphAudioStreams`` puts
it in front of a ``KoeMorphStreams``: audio in, blendshape frames out (km_koemorph_audio_*).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .egemaps_names import FEATURE_SET_DIMS, check_compression_shape, feature_set_code
from .engine import Engine, MelConfig, _ptr, _stream_ptr


def stream_shape(context_window: float, update_interval: float, mel_hop: int, sample_rate: int = 16000) -> dict:
    """The reference's stream arithmetic (mel_sliding_window.py:46-50, 300), which km_stream_create follows as well: the ring's
    length and hop in samples, the frames a front end of hop ``mel_hop`` computes over a full ring and the rows the extractor keeps."""
    ring_len = int(context_window * sample_rate)
    return dict(ring_len=ring_len, ring_hop=int(sample_rate / (1.0 / update_interval)), n_frames=1 + ring_len // mel_hop,
                stream_out_frames=int(context_window / update_interval))


class StreamEngine:
    def __init__(self, engine: Engine, n_streams: int, context_window: float = 8.5, update_interval: float = 0.0333,
                 mel: Optional[MelConfig] = None):
        if engine.device is None:
            raise _lib.KoeMorphError(_lib.KM_ERR_NOT_FINALIZED, "finalize the Engine before creating streams")
        self.engine = engine
        self.n_streams = n_streams
        self.mel = mel or MelConfig.sliding_window(n_fft=1024, hop_length=engine.mel.hop_length)
        self._lib = engine._lib
        cfg = self.mel.to_c()
        with torch.cuda.device(engine.device):
            check(self._lib.km_stream_create(engine._h, n_streams, context_window, update_interval, C.byref(cfg)))
        self.shape = stream_shape(context_window, update_interval, self.mel.hop_length, self.mel.sample_rate)
        self.ring_hop = self.shape["ring_hop"]
        dev = engine.device
        self.out = torch.zeros(n_streams, engine.num_blendshapes, device=dev)
        self.ready = torch.zeros(n_streams, dtype=torch.uint8, device=dev)
        self._graph = None
        self._g_samples = self._g_emotion = None
        self._g_attention = False
        self.raw = self.attention = None

    def attention_outputs(self) -> dict:
        """{"raw": (n_streams, 52), "mel_attention_weights": (n_streams, 28, 80)}: persistent device tensors owned by the engine,
        allocated (zero) on first use; a row is rewritten whenever its stream is computed with ``return_attention=True``."""
        if self.raw is None:
            dev = self.engine.device
            self.raw = torch.zeros(self.n_streams, self.engine.num_blendshapes, device=dev)
            self.attention = torch.zeros(self.n_streams, 28, self.engine.n_mels, device=dev)
        return {"raw": self.raw, "mel_attention_weights": self.attention}

    def _zero_attention(self, gone: Optional[torch.Tensor] = None) -> None:
        if self.raw is None:
            return
        if gone is None:
            self.raw.zero_()
            self.attention.zero_()
        else:
            self.raw.masked_fill_(gone.view(-1, 1), 0.0)
            self.attention.masked_fill_(gone.view(-1, 1, 1), 0.0)

    def _record_stats(self, stats, gate: torch.Tensor) -> None:
        if stats is not None:
            stats.update(self.attention, mask=gate)

    def push(self, samples: torch.Tensor) -> None:
        """samples (n_streams, n) fp32 on the device, n within +/-1 of the ring hop (532)."""
        if samples.dim() != 2 or samples.shape[0] != self.n_streams:
            raise ValueError(f"expected ({self.n_streams}, n) samples, got {tuple(samples.shape)}")
        samples = samples.contiguous()
        check(self._lib.km_stream_push(self.engine._h, _ptr(samples), samples.shape[1], _stream_ptr(samples.device)))

    def tick(self, emotion: torch.Tensor, return_attention: bool = False):
        """emotion (n_streams, emotion_dim) -> (out (n_streams, 52), ready (n_streams) uint8); with ``return_attention`` also the
        dict of ``attention_outputs()``, whose rows of the ready streams this tick has rewritten."""
        emotion = emotion.contiguous()
        if return_attention:
            extra = self.attention_outputs()
            check(self._lib.km_stream_tick_attn(self.engine._h, _ptr(emotion), _ptr(self.out), _ptr(self.ready), _ptr(self.raw),
                                                _ptr(self.attention), _stream_ptr(emotion.device)))
            return self.out, self.ready, extra
        check(self._lib.km_stream_tick(self.engine._h, _ptr(emotion), _ptr(self.out), _ptr(self.ready),
                                       _stream_ptr(emotion.device)))
        return self.out, self.ready

    def reset(self) -> None:
        check(self._lib.km_stream_reset(self.engine._h, _stream_ptr(self.engine.device)))
        self.out.zero_()
        self.ready.zero_()
        self._zero_attention()

    # ---- hipGraph replay ------------------------------------------------------------------------
    def _prepare_attention_capture(self, return_attention: bool, stats) -> bool:
        """What must exist before a capture that records the attention outputs: the output tensors, the accumulator, and one
        launch of the masked update's kernels outside the capture (over a mask of zeros, which changes nothing)."""
        if stats is not None and not return_attention:
            raise ValueError("stats needs return_attention=True: the accumulator is fed from the captured maps")
        if return_attention:
            self.attention_outputs()
        if stats is not None:
            stats.update(self.attention, mask=torch.zeros(self.n_streams, dtype=torch.uint8, device=self.engine.device))
        return bool(return_attention)

    def capture(self, n_per_stream: Optional[int] = None, host_out: Optional[torch.Tensor] = None, return_attention: bool = False,
                stats=None) -> None:
        """Record push + tick on static input buffers into a hipGraph (torch.cuda.CUDAGraph drives
        hipStreamBeginCapture on the current stream; the kernels are launched by libkoemorph_hip).  ``n_per_stream``: the
        frame size every replay() will bring, within +/-1 of ``ring_hop``; default 533 wherever push accepts it (ring hop 532
        or 533: every 30 fps engine, as before), otherwise ``ring_hop + 1`` (267 at 60 fps).  ``host_out``: a pinned
        (n_streams, 52) host tensor -- the tick's result readback becomes the graph's last node instead of a call per tick.
        ``return_attention``: record the tick that also writes ``attention_outputs()``; replay() then returns them as tick does.
        ``stats``: an ``AttentionStats`` or ``StreamAttentionStats`` whose masked update, gated on ``ready``, is recorded behind it."""
        dev = self.engine.device
        self._g_attention = self._prepare_attention_capture(return_attention, stats)
        if n_per_stream is None:
            n_per_stream = 533 if abs(533 - self.ring_hop) <= 1 else self.ring_hop + 1
        if host_out is not None and (not host_out.is_pinned() or tuple(host_out.shape) != tuple(self.out.shape)):
            raise ValueError("host_out must be a pinned host tensor of the shape of the result")
        self._g_samples = torch.zeros(self.n_streams, n_per_stream, device=dev)
        self._g_emotion = torch.zeros(self.n_streams, self.engine.emotion_dim, device=dev)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.push(self._g_samples)
            self.tick(self._g_emotion, return_attention=self._g_attention)
            self._record_stats(stats, self.ready)
            if host_out is not None:
                host_out.copy_(self.out, non_blocking=True)
        self._graph = g
        self._g_host_out = host_out

    def replay(self, samples: torch.Tensor, emotion: torch.Tensor):
        if self._graph is None:
            raise RuntimeError("capture() first")
        self._g_samples.copy_(samples, non_blocking=True)
        self._g_emotion.copy_(emotion, non_blocking=True)
        self._graph.replay()
        if self._g_attention:
            return self.out, self.ready, self.attention_outputs()
        return self.out, self.ready


def chunked_stream_shape(context_window: float = 8.5, update_interval: float = 0.0333, buffer_duration: float = 2.0,
                         frame_samples: Optional[int] = None, sample_rate: int = 16000) -> dict:
    """The arithmetic of the reference's real-time loop around the production model, which km_stream_fifo_create follows: the FIFO's
    size ``int(buffer_duration * sample_rate)`` (scripts/rt.py:259) and the frame one step reads, ``int(sample_rate / target_fps)``
    (:255) with target_fps the stream's nominal rate round(1 / update_interval): 533 at 30 fps, 266 at 60 fps.  ValueError where
    km_stream_fifo_create refuses: a non-positive size, a frame not within +/-1 of the ring hop (mel_sliding_window.py:80-82) or
    longer than the FIFO."""
    ring_hop = int(sample_rate / (1.0 / update_interval))
    fifo_samples = int(buffer_duration * sample_rate)
    if frame_samples is None:
        frame_samples = int(sample_rate / round(1.0 / update_interval))
    if fifo_samples <= 0 or frame_samples <= 0:
        raise ValueError("buffer_duration and frame_samples must be positive")
    if abs(frame_samples - ring_hop) > 1:
        raise ValueError(f"Frame size mismatch: expected ~{ring_hop}, got {frame_samples}")
    if fifo_samples < frame_samples:
        raise ValueError(f"frames of {frame_samples} samples exceed the FIFO of {fifo_samples}: no read could ever succeed")
    return dict(fifo_samples=fifo_samples, frame_samples=frame_samples, ring_hop=ring_hop)


class ChunkedStreamEngine(StreamEngine):
    """Streams that are out of phase.  ``feed`` is ``RingBuffer.write`` for every stream (what does not fit is dropped), ``step`` is
    ``read(frame_samples)`` + ``process_audio_frame_realtime`` for every stream that holds a frame: the frame advances the stream's
    ring, and a stream whose ring is full after it *fires* -- only fired streams are computed, every other stream keeps its row of
    ``out``, its ring and its EMA state.  ``backlog`` says how many whole frames each FIFO still holds: step again without a feed
    to drain them.  ``push`` / ``tick`` of the base class stay available and keep gating on a full ring alone."""

    def __init__(self, engine: Engine, n_streams: int, context_window: float = 8.5, update_interval: float = 0.0333,
                 mel: Optional[MelConfig] = None, buffer_duration: float = 2.0, frame_samples: Optional[int] = None):
        sr = (mel or engine.mel).sample_rate
        self.chunk = chunked_stream_shape(context_window, update_interval, buffer_duration, frame_samples, sr)
        super().__init__(engine, n_streams, context_window, update_interval, mel)
        self.fifo_samples, self.frame_samples = self.chunk["fifo_samples"], self.chunk["frame_samples"]
        with torch.cuda.device(engine.device):
            check(self._lib.km_stream_fifo_create(engine._h, self.fifo_samples, self.frame_samples))
        self.fired = torch.zeros(n_streams, dtype=torch.uint8, device=engine.device)
        self.backlog = torch.zeros(n_streams, dtype=torch.int32, device=engine.device)
        self._g_counts = None

    def feed(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None) -> None:
        """samples (n_streams, n) fp32 on the device; counts (n_streams) int32 on the device: how many of the n samples each
        stream brings (default: all)."""
        if samples.dim() != 2 or samples.shape[0] != self.n_streams or samples.dtype != torch.float32:
            raise ValueError(f"expected ({self.n_streams}, n) float32 samples, got {tuple(samples.shape)} {samples.dtype}")
        if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (self.n_streams,)):
            raise ValueError(f"expected ({self.n_streams},) int32 counts")
        samples = samples.contiguous()
        check(self._lib.km_stream_feed(self.engine._h, _ptr(samples), samples.shape[1],
                                       _ptr(counts.contiguous()) if counts is not None else None, _stream_ptr(samples.device)))

    def step(self, emotion: torch.Tensor, return_attention: bool = False):
        """emotion (n_streams, emotion_dim) -> (out (n_streams, 52), fired (n_streams) uint8); ``ready`` and ``backlog`` are
        updated as well.  Rows of streams that did not fire keep what they held.  With ``return_attention`` also the dict of
        ``attention_outputs()``, whose rows of the fired streams this step has rewritten."""
        emotion = emotion.contiguous()
        if return_attention:
            extra = self.attention_outputs()
            check(self._lib.km_stream_step_attn(self.engine._h, _ptr(emotion), _ptr(self.out), _ptr(self.fired), _ptr(self.ready),
                                                _ptr(self.backlog), _ptr(self.raw), _ptr(self.attention), _stream_ptr(emotion.device)))
            return self.out, self.fired, extra
        check(self._lib.km_stream_step(self.engine._h, _ptr(emotion), _ptr(self.out), _ptr(self.fired), _ptr(self.ready),
                                       _ptr(self.backlog), _stream_ptr(emotion.device)))
        return self.out, self.fired

    def reset_streams(self, mask: torch.Tensor) -> None:
        """mask (n_streams) bool or uint8 on the device: those streams become freshly created ones (empty FIFO, empty ring, no EMA
        history, a zero row of ``out``); the others are untouched.  No synchronisation."""
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (self.n_streams,):
            raise ValueError(f"expected a ({self.n_streams},) bool or uint8 mask")
        m8 = mask.to(torch.uint8).contiguous()
        check(self._lib.km_stream_reset_streams(self.engine._h, _ptr(m8), _stream_ptr(m8.device)))
        gone = m8 != 0
        self.out.masked_fill_(gone.unsqueeze(1), 0.0)
        self._zero_attention(gone)
        for flags in (self.ready, self.fired, self.backlog):
            flags.masked_fill_(gone, 0)

    def reset(self) -> None:
        super().reset()
        self.fired.zero_()
        self.backlog.zero_()

    # ---- hipGraph replay ------------------------------------------------------------------------
    def capture(self, n_per_stream: int, host_out: Optional[torch.Tensor] = None, return_attention: bool = False, stats=None) -> None:
        """Record feed (with per-stream counts) + step on static input buffers into a hipGraph: one linear chain.  ``host_out``: a
        pinned (n_streams, 52) host tensor -- the result readback becomes the graph's last node.  ``return_attention`` / ``stats``:
        as ``StreamEngine.capture``, the masked update gated on ``fired``."""
        dev = self.engine.device
        if host_out is not None and (not host_out.is_pinned() or tuple(host_out.shape) != tuple(self.out.shape)):
            raise ValueError("host_out must be a pinned host tensor of the shape of the result")
        self._g_attention = self._prepare_attention_capture(return_attention, stats)
        self._g_samples = torch.zeros(self.n_streams, n_per_stream, device=dev)
        self._g_counts = torch.full((self.n_streams,), n_per_stream, dtype=torch.int32, device=dev)
        self._g_emotion = torch.zeros(self.n_streams, self.engine.emotion_dim, device=dev)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.feed(self._g_samples, self._g_counts)
            self.step(self._g_emotion, return_attention=self._g_attention)
            self._record_stats(stats, self.fired)
            if host_out is not None:
                host_out.copy_(self.out, non_blocking=True)
        self._graph = g
        self._g_host_out = host_out

    def replay(self, samples: torch.Tensor, counts: Optional[torch.Tensor], emotion: torch.Tensor):
        """One captured feed + step; counts None: every stream brings all ``n_per_stream`` samples."""
        if self._graph is None:
            raise RuntimeError("capture() first")
        self._g_samples.copy_(samples, non_blocking=True)
        if counts is not None:
            self._g_counts.copy_(counts, non_blocking=True)
        else:
            self._g_counts.fill_(self._g_samples.shape[1])
        self._g_emotion.copy_(emotion, non_blocking=True)
        self._graph.replay()
        if self._g_attention:
            return self.out, self.fired, self.attention_outputs()
        return self.out, self.fired


def legacy_stream_shape(buffer_duration: float = 2.0, audio_length: int = 16000, hop: int = 533, sample_rate: int = 16000) -> dict:
    """The arithmetic of the reference's simplified real-time loop, which km_legacy_stream_create follows: the FIFO's size in samples
    (scripts/rt_simplified.py:333), the mel frames of one popped window (simplified_model.py:40: 1 + L // hop) and whether the
    stream kernel holds them (at most 32).  A window longer than the FIFO can never be read: ValueError."""
    buffer_samples = int(buffer_duration * sample_rate)
    if audio_length <= 0 or buffer_samples <= 0 or hop <= 0:
        raise ValueError("buffer_duration, audio_length and hop must be positive")
    if audio_length > buffer_samples:
        raise ValueError(f"audio_length {audio_length} exceeds the buffer of {buffer_samples} samples: no read could ever succeed")
    n_frames = 1 + audio_length // hop
    return dict(buffer_samples=buffer_samples, n_frames=n_frames, supported=n_frames <= 32)


class LegacyStreamEngine:
    """Streams of a ``SimplifiedKoeMorphModel`` with the reference's consuming FIFO (scripts/rt_simplified.py:46-97) resident on the
    device: ``push`` is ``RingBuffer.write`` for every stream, ``tick`` is ``RingBuffer.read(audio_length)`` + ``model(audio)``
    (:378-399) for every stream that holds a whole window.  No EMA and no emotion input: the model has neither.  The weights are
    those the model held when the engine was created."""

    def __init__(self, model, n_streams: int, buffer_duration: float = 2.0, audio_length: int = 16000):
        lib, h, dev = model._handle()
        self.model, self.n_streams, self.audio_length = model, n_streams, audio_length
        self._lib, self._h, self.device = lib, h, dev
        self.shape = legacy_stream_shape(buffer_duration, audio_length, model.hop_length, model.sample_rate)
        self.buffer_samples = self.shape["buffer_samples"]
        with torch.cuda.device(dev):
            torch.cuda.synchronize(dev)
            check(lib.km_legacy_stream_create(h, n_streams, self.buffer_samples, audio_length))
        # km_legacy_stream_create reserved the workspace for (n_streams, audio_length): the model's own forward must not shrink it
        model._reserved = (max(model._reserved[0], n_streams), max(model._reserved[1], audio_length))
        self.out = torch.zeros(n_streams, model.num_blendshapes, device=dev)
        self.ready = torch.zeros(n_streams, dtype=torch.uint8, device=dev)
        self._graph = None
        self._g_samples = self._g_counts = self._g_host_out = None

    def push(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None) -> None:
        """samples (n_streams, n) fp32 on the device; counts (n_streams) int32 on the device: how many of the n samples each
        stream brings (default: all).  What does not fit a stream's FIFO is dropped."""
        if samples.dim() != 2 or samples.shape[0] != self.n_streams or samples.dtype != torch.float32:
            raise ValueError(f"expected ({self.n_streams}, n) float32 samples, got {tuple(samples.shape)} {samples.dtype}")
        if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (self.n_streams,)):
            raise ValueError(f"expected ({self.n_streams},) int32 counts")
        samples = samples.contiguous()
        check(self._lib.km_legacy_stream_push(self._h, _ptr(samples), samples.shape[1],
                                              _ptr(counts.contiguous()) if counts is not None else None, _stream_ptr(samples.device)))

    def tick(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (out (n_streams, 52), ready (n_streams) uint8); rows of streams that are not ready keep what they held."""
        check(self._lib.km_legacy_stream_tick(self._h, _ptr(self.out), _ptr(self.ready), _stream_ptr(self.device)))
        return self.out, self.ready

    def reset(self) -> None:
        check(self._lib.km_legacy_stream_reset(self._h, _stream_ptr(self.device)))
        self.out.zero_()
        self.ready.zero_()

    # ---- hipGraph replay ------------------------------------------------------------------------
    def capture(self, n_per_stream: int, host_out: Optional[torch.Tensor] = None) -> None:
        """Record push (with per-stream counts) + tick on static input buffers into a hipGraph: a linear chain of four kernels.
        ``host_out``: a pinned (n_streams, 52) host tensor -- the result readback becomes the graph's last node."""
        dev = self.device
        if host_out is not None and (not host_out.is_pinned() or tuple(host_out.shape) != tuple(self.out.shape)):
            raise ValueError("host_out must be a pinned host tensor of the shape of the result")
        self._g_samples = torch.zeros(self.n_streams, n_per_stream, device=dev)
        self._g_counts = torch.full((self.n_streams,), n_per_stream, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.push(self._g_samples, self._g_counts)
            self.tick()
            if host_out is not None:
                host_out.copy_(self.out, non_blocking=True)
        self._graph = g
        self._g_host_out = host_out
        self._g_counts_full = True

    def replay(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._graph is None:
            raise RuntimeError("capture() first")
        self._g_samples.copy_(samples, non_blocking=True)
        if counts is not None:
            self._g_counts.copy_(counts, non_blocking=True)
            self._g_counts_full = False
        elif not self._g_counts_full:
            self._g_counts.fill_(self._g_samples.shape[1])
            self._g_counts_full = True
        self._graph.replay()
        return self.out, self.ready


class KoeMorphStreams:
    """Live streams of a ``KoeMorphModel`` (km_koemorph_stream_*): ``n_streams`` independent streams, out of phase, each with its
    last ``context_frames - 1 + max_rows`` feature rows, its frame counter, its previous rendered frame and its own smoother state
    resident on the device.

    The law: a ``step`` that gives stream s ``n_s`` new rows (0 .. ``max_rows``) renders ``n_s`` frames for it, in order.  Frame i,
    counted since the stream's last reset, is ``model.forward`` at B = 1 on the stream's rows ``i - T_i + 1 .. i``,
    ``T_i = min(i + 1, context_frames)`` (a dense window, no ``audio_mask``), ``prev_blendshapes`` = the stream's previous frame
    (frame 0 has none and runs as ``inference_step(prev=None)``), with the stream's own smoother state -- bit for bit.  Streams share
    nothing; a stream with ``n_s = 0`` keeps everything and its rows of the outputs keep what they held.  The model's own
    ``_smoother_state`` is neither read nor written.

    One ``step`` is four launches whatever the sizes and phases are, allocates nothing in the library and reads nothing back, so it
    can be captured (``capture`` / ``replay``).  The model's current weights are used: a changed parameter is uploaded by the next
    ``step`` (not by ``replay``) and every stream keeps its rows, counter, previous frame and state.

    Served: the fused width (d_model 256, 8 heads, decoder width 128, ``mel_dim`` / ``emotion_dim`` multiples of 16, at least one
    attention layer), ``context_frames <= 32``; anything else raises ``KoeMorphError`` (KM_ERR_UNSUPPORTED) here."""

    def __init__(self, model, n_streams: int, context_frames: Optional[int] = None, max_rows: int = 1, apply_smoothing: bool = True,
                 apply_constraints: bool = True):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise _lib.KoeMorphError(_lib.KM_ERR_WORKSPACE, "km_koemorph_stream_create: allocates, so not inside a stream capture: "
                                     "create the engine first")
        lib, h, dev = model._handle()
        self.model, self.n_streams, self.max_rows = model, int(n_streams), int(max_rows)
        self.context_frames = model._context(context_frames)
        self.apply_smoothing, self.apply_constraints = bool(apply_smoothing), bool(apply_constraints)
        self._lib, self._h, self.device = lib, h, dev
        with torch.cuda.device(dev):
            check(lib.km_koemorph_stream_create(h, self.n_streams, self.context_frames, self.max_rows, 1 if apply_smoothing else 0,
                                                1 if apply_constraints else 0))
        self.plan = koemorph_stream_plan(lib, h, self.n_streams, self.context_frames, self.max_rows)
        nb = model.num_blendshapes
        self.out = torch.zeros(self.n_streams, self.max_rows, nb, device=dev)
        self.raw = torch.zeros(self.n_streams, self.max_rows, nb, device=dev)
        self.rendered = torch.zeros(self.n_streams, dtype=torch.int32, device=dev)
        self._graph = None
        self._g_mel = self._g_emo = self._g_counts = None
        self._open = True
        model._stream_engine = weakref.ref(self)           # a handle holds ONE engine: a later one on this model replaces this one

    def _live(self) -> None:
        owner = getattr(self.model, "_stream_engine", None)
        if not self._open or owner is None or owner() is not self:
            raise RuntimeError("this KoeMorphStreams was closed, or replaced by a later one on the same model")

    def close(self) -> None:
        """Free the engine's device memory; the model and its handle stay."""
        if not getattr(self, "_open", False):
            return
        self._open = False
        self._graph = None
        owner = getattr(self.model, "_stream_engine", None)
        if owner is not None and owner() is self:              # a replaced engine's memory went with the second create
            self.model._stream_engine = None
            with torch.cuda.device(self.device):
                torch.cuda.synchronize(self.device)
                check(self._lib.km_koemorph_stream_destroy(self._h))

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def check_rows(n_streams: int, max_rows: int, mel_dim: int, emotion_dim: int, mel_rows: torch.Tensor, emotion_rows: torch.Tensor,
                   counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """What ``step`` accepts, judged before any device work: (N, r, mel_dim) and (N, r, n <= emotion_dim) rows with 1 <= r <=
        ``max_rows`` -- (N, dim) is one row per stream -- and (N,) int32 counts.  Returns the two as 3-d tensors; ValueError otherwise."""
        if mel_rows.dim() == 2:
            mel_rows = mel_rows.unsqueeze(1)
        if emotion_rows.dim() == 2:
            emotion_rows = emotion_rows.unsqueeze(1)
        if mel_rows.dim() != 3 or emotion_rows.dim() != 3 or mel_rows.shape[:2] != emotion_rows.shape[:2]:
            raise ValueError(f"expected (N, rows, mel_dim) and (N, rows, emotion_dim), got {tuple(mel_rows.shape)} and {tuple(emotion_rows.shape)}")
        if mel_rows.shape[0] != n_streams:
            raise ValueError(f"expected rows of {n_streams} streams, got {mel_rows.shape[0]}")
        if not 1 <= mel_rows.shape[1] <= max_rows:
            raise ValueError(f"{mel_rows.shape[1]} rows per stream, the engine takes 1 .. {max_rows} per step")
        if mel_rows.shape[2] != mel_dim:
            raise ValueError(f"mel rows are {mel_rows.shape[2]} wide, the model's mel_dim is {mel_dim}")
        if emotion_rows.shape[2] > emotion_dim:
            raise ValueError(f"emotion rows are {emotion_rows.shape[2]} wide, the model's emotion_dim is {emotion_dim}")
        if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (n_streams,)):
            raise ValueError(f"expected ({n_streams},) int32 counts")
        return mel_rows, emotion_rows

    def _prepare(self, mel_rows, emotion_rows, counts):
        """-> (N, max_rows, dim) float32 contiguous rows on the device and the counts (None: every stream brings every row)."""
        m = self.model
        mel, emo = self.check_rows(self.n_streams, self.max_rows, m.mel_dim, m.emotion_dim, mel_rows, emotion_rows, counts)
        r = mel.shape[1]
        mel = mel.to(self.device, torch.float32)
        emo = m._pad_emotion_rows(emo.to(self.device, torch.float32), m.emotion_dim)
        if r < self.max_rows:
            mel = torch.nn.functional.pad(mel, (0, 0, 0, self.max_rows - r))
            emo = torch.nn.functional.pad(emo, (0, 0, 0, self.max_rows - r))
            counts = (torch.full((self.n_streams,), r, dtype=torch.int32, device=self.device) if counts is None
                      else counts.to(self.device).clamp(max=r))
        elif counts is not None:
            counts = counts.to(self.device)
        return mel.contiguous(), emo.contiguous(), None if counts is None else counts.contiguous()

    def _result(self):
        return {"blendshapes": self.out, "raw_blendshapes": self.raw, "rendered": self.rendered}

    def step(self, mel_rows: torch.Tensor, emotion_rows: torch.Tensor, counts: Optional[torch.Tensor] = None):
        """mel_rows (N, r, mel_dim), emotion_rows (N, r, n <= emotion_dim; zero-padded on the right as ``render`` pads), r <= max_rows
        -- (N, dim): one row per stream --, counts (N,) int32 on the device: how many of its r rows each stream brings (default all)
        -> {"blendshapes": (N, max_rows, 52), "raw_blendshapes": ..., "rendered": (N,) int32}, owned by the engine: row (s, j) is
        stream s's j-th new frame for j < rendered[s]; the other rows keep what they held."""
        mel, emo, cnt = self._prepare(mel_rows, emotion_rows, counts)
        self._live()
        self.model._handle()                                     # uploads changed weights; the streams' state is kept
        with torch.cuda.device(self.device):
            check(self._lib.km_koemorph_stream_step(self._h, _ptr(mel), _ptr(emo), _ptr(cnt) if cnt is not None else None, _ptr(self.out),
                                                    _ptr(self.raw), _ptr(self.rendered), _stream_ptr(self.device)))
        return self._result()

    def reset_streams(self, mask: torch.Tensor) -> None:
        """mask (N,) bool or uint8: those streams become freshly created ones (counter 0, no previous frame, zero state)."""
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (self.n_streams,):
            raise ValueError(f"expected a ({self.n_streams},) bool or uint8 mask")
        self._live()
        m8 = mask.to(self.device, torch.uint8).contiguous()
        check(self._lib.km_koemorph_stream_reset(self._h, _ptr(m8), _stream_ptr(self.device)))

    def reset(self) -> None:
        self._live()
        check(self._lib.km_koemorph_stream_reset(self._h, None, _stream_ptr(self.device)))

    def frames(self) -> torch.Tensor:
        """(N,) int64: every stream's frames since its last reset; a copy."""
        self._live()
        out = torch.empty(self.n_streams, dtype=torch.int64, device=self.device)
        check(self._lib.km_koemorph_stream_frames(self._h, _ptr(out), _stream_ptr(self.device)))
        return out

    def smoother_state(self) -> Optional[torch.Tensor]:
        """(N, state floats per stream): the streams' smoother states in ``forward``'s layout for B = 1; None without smoothing."""
        if not self.plan["state_floats"] or not self.apply_smoothing:
            return None
        self._live()
        out = torch.empty(self.n_streams, self.plan["state_floats"], device=self.device)
        check(self._lib.km_koemorph_stream_state(self._h, _ptr(out), None, _stream_ptr(self.device)))
        return out

    # ---- hipGraph replay ------------------------------------------------------------------------
    def capture(self, max_rows: Optional[int] = None) -> None:
        """Record one step with per-stream counts on static input buffers of ``max_rows`` (default: the engine's) rows per stream."""
        r = self.max_rows if max_rows is None else int(max_rows)
        if not 1 <= r <= self.max_rows:
            raise ValueError(f"max_rows {r} outside 1 .. {self.max_rows}")
        self._live()
        dev, m = self.device, self.model
        self.model._handle()
        self._g_rows = r
        self._g_mel = torch.zeros(self.n_streams, self.max_rows, m.mel_dim, device=dev)
        self._g_emo = torch.zeros(self.n_streams, self.max_rows, m.emotion_dim, device=dev)
        self._g_counts = torch.zeros(self.n_streams, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            check(self._lib.km_koemorph_stream_step(self._h, _ptr(self._g_mel), _ptr(self._g_emo), _ptr(self._g_counts), _ptr(self.out),
                                                    _ptr(self.raw), _ptr(self.rendered), _stream_ptr(dev)))
        self._graph = g

    def replay(self, mel_rows: torch.Tensor, emotion_rows: torch.Tensor, counts: Optional[torch.Tensor] = None):
        """One captured step; counts None: every stream brings all its rows."""
        if self._graph is None:
            raise RuntimeError("capture() first")
        self._live()
        m = self.model
        mel, emo = self.check_rows(self.n_streams, self._g_rows, m.mel_dim, m.emotion_dim, mel_rows, emotion_rows, counts)
        r, n = mel.shape[1], emo.shape[2]
        self._g_mel[:, :r].copy_(mel, non_blocking=True)
        if n < m.emotion_dim:
            self._g_emo[:, :r, n:].zero_()
        self._g_emo[:, :r, :n].copy_(emo, non_blocking=True)
        if counts is not None:
            self._g_counts.copy_(counts.clamp(max=r), non_blocking=True)
        else:
            self._g_counts.fill_(r)
        self._graph.replay()
        return self._result()


def koemorph_stream_plan(lib, h, n_streams: int, context_frames: int, max_rows: int) -> dict:
    """km_koemorph_stream_plan as a dict (host only)."""
    out = (C.c_int64 * 6)()
    check(lib.km_koemorph_stream_plan(h, n_streams, context_frames, max_rows, out))
    return dict(zip(("supported", "ring_rows", "launches", "device_floats", "chain_lds_bytes", "state_floats"), (int(v) for v in out)))


def koemorph_audio_plan(lib, h, n_streams: int, fps: float, emotion_window: float, max_samples: int, feature_set: str = "eGeMAPSv02") -> dict:
    """km_koemorph_audio_plan as a dict (host only): ``supported`` 0 leaves the reason in ``km_last_error``."""
    out = (C.c_int64 * 8)()
    check(lib.km_koemorph_audio_plan(h, int(n_streams), float(fps), float(emotion_window), int(max_samples), feature_set_code(feature_set), out))
    return dict(zip(("supported", "hop", "max_rows", "ring_len", "window_samples", "window_frames", "launches", "device_bytes"),
                    (int(v) for v in out)))


def check_samples(n_streams: int, max_samples: int, samples: torch.Tensor, counts: Optional[torch.Tensor] = None) -> None:
    """What ``push`` accepts, judged before any device work: (N, M) samples with 1 <= M <= max_samples and (N,) int32 counts."""
    if samples.dim() != 2 or samples.shape[0] != n_streams:
        raise ValueError(f"expected ({n_streams}, M) samples, got {tuple(samples.shape)}")
    if not 1 <= samples.shape[1] <= max_samples:
        raise ValueError(f"{samples.shape[1]} samples per stream, the engine takes 1 .. {max_samples} per push")
    if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (n_streams,)):
        raise ValueError(f"expected ({n_streams},) int32 counts")


class AudioRowStreams:
    """The rows of ``KoeMorphStreams.step`` from pushed 16 kHz audio (km_koemorph_audio_*): per stream a ring of samples and a sample
    counter on the device; a ``push`` is seven launches and gives the mel and emotion rows of the frames that became due, and their counts.

    The law: ``hop = int(16000 / fps)``; frame k of a stream is due as soon as the stream holds ``(k + 1) * hop`` samples, so a push that
    takes it from ``n0`` to ``n`` samples renders frames ``n0 // hop .. n // hop - 1``.  Mel row k is the row of the STFT frame centred on
    sample ``k * hop`` in ``MelSpectrogramExtractor``'s configuration, reflected at the stream's first sample only -- a function of the
    stream's samples alone.  Emotion row k is read, at ``p = k * hop / 160``, from the eGeMAPS descriptors of the stream's last
    ``emotion_window`` seconds as they stand at the end of the push (tests/koemorph_audio_cases.py restates the window and the grid), so it
    depends on where the pushes end.  ``emotion_window`` = 2 s is a choice nobody has measured for quality.

    Served: ``hop >= 257`` and ``fps >= 10``, ``int(emotion_window * 16000) >= max_samples + hop + 1120``, a window of at most 2048
    frames (20.5 s); anything else raises ``KoeMorphError`` here.  A handle holds one: a later one on the same model replaces this one."""

    def __init__(self, model, n_streams: int, fps: float = 30.0, emotion_window: float = 2.0, max_samples: int = 1600,
                 feature_set: str = "eGeMAPSv02"):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise _lib.KoeMorphError(_lib.KM_ERR_WORKSPACE, "km_koemorph_audio_create: allocates, so not inside a stream capture: "
                                     "create the engine first")
        lib, h, dev = model._handle()
        self.model, self.n_streams, self.fps, self.max_samples = model, int(n_streams), float(fps), int(max_samples)
        self.emotion_window, self.feature_set = float(emotion_window), feature_set
        self._lib, self._h, self.device = lib, h, dev
        code = feature_set_code(feature_set)
        with torch.cuda.device(dev):
            check(lib.km_koemorph_audio_create(h, self.n_streams, self.fps, self.emotion_window, self.max_samples, code))
        self.plan = koemorph_audio_plan(lib, h, self.n_streams, self.fps, self.emotion_window, self.max_samples, feature_set)
        self.hop, self.max_rows = self.plan["hop"], self.plan["max_rows"]
        self.mel_rows = torch.zeros(self.n_streams, self.max_rows, model.mel_dim, device=dev)
        self.emotion_rows = torch.zeros(self.n_streams, self.max_rows, model.emotion_dim, device=dev)
        self.row_counts = torch.zeros(self.n_streams, dtype=torch.int32, device=dev)
        self._open = True
        model._audio_engine = weakref.ref(self)

    def _live(self) -> None:
        owner = getattr(self.model, "_audio_engine", None)
        if not self._open or owner is None or owner() is not self:
            raise RuntimeError("this AudioRowStreams was closed, or replaced by a later one on the same model")

    def close(self) -> None:
        """Free the engine's device memory; the model and its handle stay."""
        if not getattr(self, "_open", False):
            return
        self._open = False
        owner = getattr(self.model, "_audio_engine", None)
        if owner is not None and owner() is self:              # a replaced engine's memory went with the second create
            self.model._audio_engine = None
            with torch.cuda.device(self.device):
                torch.cuda.synchronize(self.device)
                check(self._lib.km_koemorph_audio_destroy(self._h))

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _prepare(self, samples, counts):
        check_samples(self.n_streams, self.max_samples, samples, counts)
        x = samples.to(self.device, torch.float32).contiguous()
        return x, None if counts is None else counts.to(self.device).contiguous()

    def _launch(self, x, cnt) -> None:
        check(self._lib.km_koemorph_audio_rows(self._h, _ptr(x), x.shape[1], _ptr(cnt) if cnt is not None else None, _ptr(self.mel_rows),
                                               _ptr(self.emotion_rows), _ptr(self.row_counts), _stream_ptr(self.device)))

    def push(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None):
        """samples (N, M <= max_samples), counts (N,) int32 on the device: how many of its M samples each stream brings (default all,
        clamped to 0 .. M) -> (mel_rows (N, max_rows, mel_dim), emotion_rows (N, max_rows, emotion_dim), row_counts (N,) int32), owned
        by the object: row (s, j) is stream s's j-th new frame for j < row_counts[s]; the other rows keep what they held."""
        x, cnt = self._prepare(samples, counts)
        self._live()
        with torch.cuda.device(self.device):
            self._launch(x, cnt)
        return self.mel_rows, self.emotion_rows, self.row_counts

    def reset_streams(self, mask: torch.Tensor) -> None:
        """mask (N,) bool or uint8: those streams start again at sample 0."""
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (self.n_streams,):
            raise ValueError(f"expected a ({self.n_streams},) bool or uint8 mask")
        self._live()
        m8 = mask.to(self.device, torch.uint8).contiguous()
        check(self._lib.km_koemorph_audio_reset(self._h, _ptr(m8), _stream_ptr(self.device)))

    def reset(self) -> None:
        self._live()
        check(self._lib.km_koemorph_audio_reset(self._h, None, _stream_ptr(self.device)))

    def samples(self) -> torch.Tensor:
        """(N,) int64: every stream's samples since its last reset; a copy."""
        self._live()
        out = torch.empty(self.n_streams, dtype=torch.int64, device=self.device)
        check(self._lib.km_koemorph_audio_samples(self._h, _ptr(out), _stream_ptr(self.device)))
        return out


class KoeMorphAudioStreams:
    """``KoeMorphModel`` streams from pushed audio: an ``AudioRowStreams`` in front of a ``KoeMorphStreams(max_rows = the plan's)`` on
    one model.  ``push`` is the seven launches of the rows and the four of the step on the same device buffers -- exactly
    ``KoeMorphStreams.step(mel_rows, emotion_rows, row_counts)``, that engine's law unchanged -- with no allocation, synchronisation
    or readback, so it can be captured (``capture`` / ``replay``)."""

    def __init__(self, model, n_streams: int, fps: float = 30.0, context_frames: Optional[int] = None, emotion_window: float = 2.0,
                 max_samples: int = 1600, feature_set: str = "eGeMAPSv02", apply_smoothing: bool = True, apply_constraints: bool = True):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise _lib.KoeMorphError(_lib.KM_ERR_WORKSPACE, "km_koemorph_audio_create: allocates, so not inside a stream capture: "
                                     "create the engine first")
        self.rows = AudioRowStreams(model, n_streams, fps, emotion_window, max_samples, feature_set)
        try:
            self.frames_engine = KoeMorphStreams(model, n_streams, context_frames=context_frames, max_rows=self.rows.max_rows,
                                                 apply_smoothing=apply_smoothing, apply_constraints=apply_constraints)
        except Exception:
            self.rows.close()
            raise
        self.model, self.n_streams, self.fps, self.hop = model, int(n_streams), float(fps), self.rows.hop
        self.max_samples, self.max_rows, self.device = self.rows.max_samples, self.rows.max_rows, self.rows.device
        self._graph = None
        self._g_samples = self._g_counts = None

    def close(self) -> None:
        self._graph = None
        self.frames_engine.close()
        self.rows.close()

    def _launch(self, x, cnt) -> None:
        r, f = self.rows, self.frames_engine
        r._launch(x, cnt)
        check(f._lib.km_koemorph_stream_step(f._h, _ptr(r.mel_rows), _ptr(r.emotion_rows), _ptr(r.row_counts), _ptr(f.out), _ptr(f.raw),
                                             _ptr(f.rendered), _stream_ptr(self.device)))

    def push(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None):
        """samples (N, M <= max_samples), counts (N,) int32 (default: all M) -> ``KoeMorphStreams.step``'s dict, owned by the engine:
        ``rendered[s]`` is the frames this push gave stream s, ``blendshapes[s, j]`` its j-th new frame for j < rendered[s]."""
        x, cnt = self.rows._prepare(samples, counts)
        self.rows._live()
        self.frames_engine._live()
        self.model._handle()                                     # uploads changed weights; the streams' state is kept
        with torch.cuda.device(self.device):
            self._launch(x, cnt)
        return self.frames_engine._result()

    def reset_streams(self, mask: torch.Tensor) -> None:
        self.rows.reset_streams(mask)
        self.frames_engine.reset_streams(mask)

    def reset(self) -> None:
        self.rows.reset()
        self.frames_engine.reset()

    def frames(self) -> torch.Tensor:
        """(N,) int64: every stream's frames since its last reset; a copy."""
        return self.frames_engine.frames()

    def smoother_state(self) -> Optional[torch.Tensor]:
        return self.frames_engine.smoother_state()

    # ---- hipGraph replay ------------------------------------------------------------------------
    def capture(self, n_per_stream: Optional[int] = None) -> None:
        """Record one push of ``n_per_stream`` (default ``max_samples``) samples per stream with per-stream counts on static inputs."""
        m = self.max_samples if n_per_stream is None else int(n_per_stream)
        if not 1 <= m <= self.max_samples:
            raise ValueError(f"{m} samples per stream outside 1 .. {self.max_samples}")
        self.rows._live()
        self.frames_engine._live()
        self.model._handle()
        dev = self.device
        self._g_samples = torch.zeros(self.n_streams, m, device=dev)
        self._g_counts = torch.zeros(self.n_streams, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._launch(self._g_samples, self._g_counts)
        self._graph = g

    def replay(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None):
        """One captured push; samples (N, M <= the captured width), counts None: every stream brings all M."""
        if self._graph is None:
            raise RuntimeError("capture() first")
        self.rows._live()
        self.frames_engine._live()
        check_samples(self.n_streams, self._g_samples.shape[1], samples, counts)
        m = samples.shape[1]
        self._g_samples[:, :m].copy_(samples, non_blocking=True)
        if counts is not None:
            self._g_counts.copy_(counts.clamp(max=m), non_blocking=True)
        else:
            self._g_counts.fill_(m)
        self._graph.replay()
        return self.frames_engine._result()


def emotion_stream_shape(context_window: float = 20.0, update_interval: float = 0.3, sample_rate: int = 16000,
                         backend: str = "egemaps", long_windows: bool = False, feature_set: str = "eGeMAPSv02") -> dict:
    """The arithmetic of the reference's OpenSMILEeGeMAPSExtractor in samples, which km_emotion_stream_create follows: the
    AudioBuffer of ``context_window + 2`` seconds (opensmile_extractor.py:245-248), the window ``get_window(context_window)`` returns
    once that much audio has arrived, the samples between two updates of a stream, the half second below which nothing is extracted
    (:388-389) and the 10 ms frames of a full window.  ValueError where km_emotion_stream_create refuses: the constructor's own
    checks (:204-209) and a window of more than 2048 frames (20.5 s), which the functionals kernel cannot hold.
    ``backend="basic"`` (km_emotion_stream_create_basic): the same rings and rule; ``max_frames`` counts the 32 ms frames of the
    prosodic features, ``1 + window_len // 512``, and the window may hold up to 2**20 samples (65.5 s).
    ``long_windows=True`` (eGeMAPS only; km_emotion_stream_create_long): the window limit is the basic back end's, 2**20 samples or
    6548 frames, instead of 2048 frames -- the reference's ``long_context`` variant has 30 s / 0.2 s, 2995 frames.
    ``feature_set`` ("eGeMAPSv02" or "GeMAPS", eGeMAPS back end only) is checked and changes none of the five numbers: the feature
    count is the object's ``feature_dim``."""
    if backend not in ("egemaps", "basic"):
        raise ValueError(f"backend must be 'egemaps' or 'basic', got {backend!r}")
    if feature_set_code(feature_set) and backend != "egemaps":
        raise ValueError("feature_set is the eGeMAPS back end's choice: the basic back end has its nine prosodic values")
    if long_windows and backend != "egemaps":
        raise ValueError("long_windows is the eGeMAPS back end's switch: the basic back end takes windows of 2**20 samples as it is")
    if sample_rate != 16000:
        raise ValueError("the GPU eGeMAPS extractor is built for 16 kHz audio")
    if not context_window >= 1.0:
        raise ValueError("Context window must be at least 1.0 seconds")
    if not update_interval >= 0.1:
        raise ValueError("Update interval must be at least 0.1 seconds")
    if update_interval > context_window:
        raise ValueError("Update interval cannot be larger than context window")
    ring_len = int((context_window + 2.0) * sample_rate)
    window_len = min(int(context_window * sample_rate), ring_len)
    if backend == "basic":
        max_frames = 1 + window_len // 512
        if window_len > 1 << 20:
            raise ValueError(f"a window of {window_len} samples, at most {1 << 20} (65.5 s)")
    else:
        max_frames = (window_len - 960) // 160 + 1
        if long_windows and window_len > 1 << 20:
            raise ValueError(f"a window of {window_len} samples, at most {1 << 20} (65.5 s)")
        if not long_windows and max_frames > 2048:
            raise ValueError(f"{max_frames} frames per window, at most 2048 (20.5 s)")
    return dict(ring_len=ring_len, window_len=window_len, update_samples=int(update_interval * sample_rate),
                min_samples=int(0.5 * sample_rate), max_frames=max_frames)


def _create_emotion_backend(backend: str, compression_layer: Optional[torch.nn.Module], device, create, set_compression,
                            feature_set: str = "eGeMAPSv02"):
    """What ``StreamEmotion`` and ``ClipEmotion`` do with their back end: ``create(handle_ref)`` on the resolved device (``"cpu"``,
    ``"auto"`` and None mean the current GPU), and for eGeMAPS the ``Linear(264, 256)`` -- torch's default when absent -- copied
    into the object with ``set_compression(handle, w, b, stream)``.  Returns (device, handle, the layer kept, emotion_dim,
    feature_dim); the basic back end keeps no layer and both widths are 9.  ``feature_set="GeMAPS"``: 62 features and a
    ``Linear(186, 256)``."""
    device = torch.device(device if device not in (None, "cpu", "auto") else "cuda")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    h = C.c_void_p()
    if backend == "basic":
        with torch.cuda.device(device):
            check(create(C.byref(h)))
        return device, h, None, 9, 9
    feature_dim = FEATURE_SET_DIMS[feature_set]
    if compression_layer is None:
        compression_layer = torch.nn.Linear(3 * feature_dim, 256)
    check_compression_shape(compression_layer, feature_set)
    with torch.cuda.device(device):
        check(create(C.byref(h)))
        w = compression_layer.weight.detach().to(device, torch.float32).contiguous()
        b = compression_layer.bias.detach().to(device, torch.float32).contiguous()
        check(set_compression(h, _ptr(w), _ptr(b), _stream_ptr(device)))
        torch.cuda.current_stream(device).synchronize()                   # w and b may go once the copy is done
    return device, h, compression_layer, 256, feature_dim


class StreamEmotion:
    """The emotion input of ``n_streams`` streams, computed on the device from the audio pushed into it: per stream the reference's
    ``AudioBuffer``, the update rule of ``process_audio_frame``, the three window slots and ``Linear(264, 256)``
    (OpenSMILEeGeMAPSExtractor with ``use_concatenation=True``).  ``push`` appends audio, ``update`` re-extracts the eGeMAPS
    functionals of every stream that is due -- at most ``max_updates`` per call, longest waiting first -- and returns the
    ``(n_streams, 256)`` matrix ``StreamEngine.tick`` / ``ChunkedStreamEngine.step`` take.  Time is audio time: a stream is due
    ``update_interval`` seconds *of its own samples* after its last update (the reference reads the wall clock), and a stream without
    audio has no features (the reference would extract the zeros of an empty buffer).  Neither call allocates or synchronises.

    ``compression_layer``: a ``torch.nn.Linear(264, 256)``; created with torch's default initialisation when absent, as the
    reference does on first use (:589-591).  Its weights are copied at construction.

    ``backend="basic"`` (km_emotion_stream_create_basic): the same rings, update rule, reset and capture contract, but a selected
    stream's row is the nine raw prosodic values of its window -- bit for bit ``BasicEmotion()(window[None])[0]``
    (koemorph_amd.features.basic_emotion: EmotionExtractor._extract_basic).  ``emotion`` and ``features`` are ``(n_streams, 9)``,
    the input of a model with ``emotion_dim`` 9; there is no peak normalisation, no slots (``slots`` raises) and no compression
    layer (passing one raises ``ValueError``).

    ``long_windows=True`` (km_emotion_stream_create_long): eGeMAPS windows of up to 2**20 samples (65.5 s) instead of 2048 frames
    (20.5 s) -- ``StreamEmotion(n, 30.0, 0.2, long_windows=True)`` is the reference's ``long_context`` variant.  Every call is
    unchanged; an object whose window has at most 2048 frames is the plain object.

    ``feature_set="GeMAPS"`` (km_emotion_stream_create_set): the 62 functionals of GeMAPS instead of the 88 --
    ``StreamEmotion(n, 10.0, 0.5, feature_set="GeMAPS")`` is the reference's ``fast`` variant.  ``features`` is ``(n_streams, 62)``,
    ``slots`` ``(n_streams, 2, 62)``, the layer a ``Linear(186, 256)`` (a deliberate deviation: the reference's hard-coded
    ``Linear(264, 256)`` never compresses GeMAPS features).  Feature j is feature ``GEMAPS_COLUMNS[j]`` of the eGeMAPS object on the
    same pushes, bit for bit; parity with openSMILE's own GeMAPSv01b is UNPINNED."""

    def __init__(self, n_streams: int, context_window: float = 20.0, update_interval: float = 0.3, max_updates: Optional[int] = None,
                 compression_layer: Optional[torch.nn.Module] = None, device="cuda", backend: str = "egemaps",
                 long_windows: bool = False, feature_set: str = "eGeMAPSv02"):
        self.shape = emotion_stream_shape(context_window, update_interval, backend=backend, long_windows=long_windows,
                                          feature_set=feature_set)
        self.backend, self.long_windows, self.feature_set = backend, long_windows, feature_set
        if backend == "basic" and compression_layer is not None:
            raise ValueError("the basic back end has no compression layer: its nine features are the emotion input as they are")
        if max_updates is None:
            max_updates = n_streams
        if n_streams < 1 or not 1 <= max_updates <= n_streams:
            raise ValueError(f"expected 1 <= max_updates <= n_streams, got max_updates {max_updates}, n_streams {n_streams}")
        if not torch.cuda.is_available():
            raise _lib.KoeMorphError(_lib.KM_ERR_HIP, "no GPU visible: the emotion streams have no CPU fallback")
        self.n_streams, self.max_updates = n_streams, max_updates
        self.context_window, self.update_interval = context_window, update_interval
        self.ring_len = self.shape["ring_len"]
        self._lib = _lib.load()
        create = (self._lib.km_emotion_stream_create_basic if backend == "basic" else
                  self._lib.km_emotion_stream_create_long if long_windows else self._lib.km_emotion_stream_create)
        make = lambda h: create(h, n_streams, context_window, update_interval, max_updates)
        if feature_set_code(feature_set):
            make = lambda h: self._lib.km_emotion_stream_create_set(h, n_streams, context_window, update_interval, max_updates,
                                                                    feature_set_code(feature_set), 1 if long_windows else 0)
        self.device, self._h, self.compression_layer, self.emotion_dim, self.feature_dim = _create_emotion_backend(
            backend, compression_layer, device, make, self._lib.km_emotion_stream_set_compression, feature_set)
        self.emotion = torch.zeros(n_streams, self.emotion_dim, device=self.device)
        self.valid = torch.zeros(n_streams, dtype=torch.uint8, device=self.device)
        self.updated = torch.zeros(n_streams, dtype=torch.uint8, device=self.device)
        self._graph = None
        self._g_samples = self._g_counts = None

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.km_emotion_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def push(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None) -> None:
        """samples (n_streams, n) fp32 on the device, n at most the ring; counts (n_streams) int32 on the device: how many of the
        n samples each stream brings (default: all).  A stream that brings none is untouched."""
        if samples.dim() != 2 or samples.shape[0] != self.n_streams or samples.dtype != torch.float32:
            raise ValueError(f"expected ({self.n_streams}, n) float32 samples, got {tuple(samples.shape)} {samples.dtype}")
        if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (self.n_streams,)):
            raise ValueError(f"expected ({self.n_streams},) int32 counts")
        samples = samples.contiguous()
        check(self._lib.km_emotion_stream_push(self._h, _ptr(samples), samples.shape[1],
                                               _ptr(counts.contiguous()) if counts is not None else None, _stream_ptr(samples.device)))

    def update(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (emotion (n_streams, 256) -- (n_streams, 9) on the basic back end --, updated (n_streams) uint8); ``valid`` says which streams have features at all.  Rows of
        streams that were not selected keep what they held; a stream that never had features has a zero row."""
        check(self._lib.km_emotion_stream_update(self._h, _ptr(self.emotion), _ptr(self.valid), _ptr(self.updated),
                                                 _stream_ptr(self.device)))
        return self.emotion, self.updated

    @property
    def features(self) -> torch.Tensor:
        """(n_streams, 88): every stream's current eGeMAPS functionals (zero before its first update); a copy.  (n_streams, 9) on
        the basic back end."""
        out = torch.empty(self.n_streams, self.feature_dim, device=self.device)
        check(self._lib.km_emotion_stream_features(self._h, _ptr(out), None, _stream_ptr(self.device)))
        return out

    @property
    def slots(self) -> torch.Tensor:
        """(n_streams, 2, 88): the 300 ms and 600 ms window slots, i.e. the first features of each stream's current life; a copy."""
        if self.backend == "basic":
            raise AttributeError("the basic back end has no window slots")
        feats = torch.empty(self.n_streams, self.feature_dim, device=self.device)
        out = torch.empty(self.n_streams, 2, self.feature_dim, device=self.device)
        check(self._lib.km_emotion_stream_features(self._h, _ptr(feats), _ptr(out), _stream_ptr(self.device)))
        return out

    def reset_streams(self, mask: torch.Tensor) -> None:
        """mask (n_streams) bool or uint8 on the device: those streams become freshly created ones (OpenSMILEeGeMAPSExtractor.reset
        :640-659: empty ring, no features, empty slots, a zero row of ``emotion``); the others are untouched.  No synchronisation."""
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (self.n_streams,):
            raise ValueError(f"expected a ({self.n_streams},) bool or uint8 mask")
        m8 = mask.to(self.device, torch.uint8).contiguous()
        check(self._lib.km_emotion_stream_reset_streams(self._h, _ptr(m8), _stream_ptr(self.device)))
        gone = m8 != 0
        self.emotion.masked_fill_(gone.unsqueeze(1), 0.0)
        for flags in (self.valid, self.updated):
            flags.masked_fill_(gone, 0)

    def reset(self) -> None:
        check(self._lib.km_emotion_stream_reset_streams(self._h, None, _stream_ptr(self.device)))
        self.emotion.zero_()
        self.valid.zero_()
        self.updated.zero_()

    # ---- hipGraph replay ------------------------------------------------------------------------
    def capture(self, n_per_stream: int) -> None:
        """Record push (with per-stream counts) + update on static input buffers into a hipGraph: one linear chain."""
        dev = self.device
        self._g_samples = torch.zeros(self.n_streams, n_per_stream, device=dev)
        self._g_counts = torch.zeros(self.n_streams, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.push(self._g_samples, self._g_counts)
            self.update()
        self._graph = g

    def replay(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One captured push + update; counts None: every stream brings all ``n_per_stream`` samples."""
        if self._graph is None:
            raise RuntimeError("capture() first")
        self._g_samples.copy_(samples, non_blocking=True)
        if counts is not None:
            self._g_counts.copy_(counts, non_blocking=True)
        else:
            self._g_counts.fill_(self._g_samples.shape[1])
        self._graph.replay()
        return self.emotion, self.updated


class StreamResampler:
    """Audio of ``n_streams`` streams at its capture rate -> the 16 kHz every other entry point takes, with the per-stream filter
    state on the device (km_resampler_*; the filter and the laws: ``koemorph_amd.features.resample``).  ``push`` takes chunks of
    any size -- ``(n_streams, n)`` samples plus per-stream counts, the convention of ``ChunkedStreamEngine.feed`` and
    ``StreamEmotion.push`` -- and returns each stream's newly determined outputs and their number, which go unchanged into those
    two.  The outputs are those of ``Resampler.clip`` on the concatenated input, bit for bit and whatever the chunking: a stream lags
    its input by ``half_len / up`` samples (30 at 48 kHz) and ``flush`` emits that remainder.  No call allocates or synchronises, so
    ``push`` -> ``feed`` -> ``step`` captures into one ``torch.cuda.graph``."""

    def __init__(self, n_streams: int, rate_in: int, rate_out: int = 16000, device="cuda"):
        from .features import resample as _rs
        self.n_streams, self.rate_in, self.rate_out = n_streams, int(rate_in), int(rate_out)
        self.up, self.down = _rs._check_rate_pair(rate_in, rate_out)
        if n_streams < 1:
            raise ValueError(f"expected n_streams >= 1, got {n_streams}")
        if not torch.cuda.is_available():
            raise _lib.KoeMorphError(_lib.KM_ERR_HIP, "no GPU visible: the resampler has no CPU fallback")
        self.device = torch.device(device if device not in (None, "cpu", "auto") else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _lib.load()
        with torch.cuda.device(self.device):
            self._h, self.half_len = _rs.create_handle(self._lib, n_streams, self.up, self.down)
        self._flush_max = -(-self.half_len // self.down)
        self._bufs = {}

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.km_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def out_max(self, n: int) -> int:
        """The row length that holds whatever a push of ``n`` samples per stream emits: ceil(n up / down) + 1."""
        v = C.c_int64()
        check(self._lib.km_resampler_out_max(self._h, n, C.byref(v)))
        return v.value

    def _out(self, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """One (out, out_counts) pair per row length, created on first use and kept: what a captured graph wrote into stays valid."""
        if width not in self._bufs:
            self._bufs[width] = (torch.zeros(self.n_streams, width, device=self.device),
                                 torch.zeros(self.n_streams, dtype=torch.int32, device=self.device))
        return self._bufs[width]

    def push(self, samples: torch.Tensor, counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """samples (n_streams, n) fp32 on the device; counts (n_streams) int32 on the device: how many of the n samples each stream
        brings (default: all) -> (out (n_streams, out_max(n)), out_counts (n_streams) int32), owned by this object and overwritten by
        the next push of the same n.  A stream that brings nothing is untouched and reports 0."""
        if samples.dim() != 2 or samples.shape[0] != self.n_streams or samples.dtype != torch.float32 or samples.shape[1] < 1:
            raise ValueError(f"expected ({self.n_streams}, n) float32 samples, got {tuple(samples.shape)} {samples.dtype}")
        if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (self.n_streams,)):
            raise ValueError(f"expected ({self.n_streams},) int32 counts")
        samples = samples.contiguous()
        out, out_counts = self._out(self.out_max(samples.shape[1]))
        check(self._lib.km_resampler_push(self._h, _ptr(samples), samples.shape[1], _ptr(counts.contiguous()) if counts is not None else None,
                                          _ptr(out), out.shape[1], _ptr(out_counts), _stream_ptr(samples.device)))
        return out, out_counts

    def flush(self, mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The streams of ``mask`` (None: all) emit the outputs they still owe up to ``ceil(N up / down)``, as though zeros followed,
        and are left reset; the others report 0 -> (out (n_streams, ceil(half_len / down)), out_counts)."""
        m8 = self._mask(mask)
        out, out_counts = self._out(max(1, self._flush_max))
        check(self._lib.km_resampler_flush(self._h, _ptr(m8), _ptr(out), out.shape[1], _ptr(out_counts), _stream_ptr(self.device)))
        return out, out_counts

    def _mask(self, mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        if mask is None:
            return None
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (self.n_streams,):
            raise ValueError(f"expected a ({self.n_streams},) bool or uint8 mask")
        return mask.to(self.device, torch.uint8).contiguous()

    def reset_streams(self, mask: torch.Tensor) -> None:
        """mask (n_streams) bool or uint8 on the device: those streams become freshly created ones; the others are untouched."""
        m8 = self._mask(mask)
        if m8 is None:
            raise ValueError("reset_streams needs a mask; reset() resets every stream")
        check(self._lib.km_resampler_reset_streams(self._h, _ptr(m8), _stream_ptr(self.device)))

    def reset(self) -> None:
        check(self._lib.km_resampler_reset_streams(self._h, None, _stream_ptr(self.device)))
