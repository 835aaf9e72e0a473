"""Drop-in mirror of the reference's ``SequentialDualStreamModel``
(reference src/model/sequential_dual_stream_model.py:17-180).

``forward(audio (B, T)) -> {'blendshapes': (B, T_out, 52), 'num_frames', 'fps', ...}`` with one output
frame per window position (window = mel_sequence_length frames, stride = stride_frames).  The reference
walks the positions in a Python loop and recomputes the whole 257-frame mel on the CPU for each one
(:101-145); here every window of every clip is one workgroup of the same HIP kernels, addressed in place
inside the clip (km_sequence_forward), followed by an EMA scan along the frame axis.  ``return_attention=True`` is the same
call with the head-averaged attention map of every window written as well (km_sequence_forward_attn): 'mel_attention_weights'
(B, T_out, 28, 80), 'emotion_attention_weights' all ones, and the same 'blendshapes' bits.

Not in the reference: ``clip_emotion`` (a ``koemorph_amd.features.ClipEmotion``) or ``forward(emotion_track=...)`` give every
window the row of the clip's eGeMAPS emotion track that a live stream would hold when the window ends -- the input
``train_sequential --emotion egemaps`` trains on -- instead of one vector per clip (km_sequence_forward_track).  With a
``ClipEmotion(backend="basic")`` and ``emotion_config={"backend": "basic"}`` (emotion_dim 9) the track holds the nine prosodic values
per row (``--emotion basic``) and 'emotion_backend' reports ``basic_track``.
``share_frames=True`` computes each clip's STFT once at every model shape and hop and assembles the windows on the device (engine
option "seq_assemble"); the default leaves the engine's schedule as it is.
"""
from __future__ import annotations

import logging
from typing import Dict, Optional

import torch

from .simplified_dual_stream_model import SimplifiedDualStreamModel

logger = logging.getLogger(__name__)


class SequentialDualStreamModel(SimplifiedDualStreamModel):
    def __init__(
        self,
        d_model: int = 256,
        num_heads: int = 8,
        num_blendshapes: int = 52,
        sample_rate: int = 16000,
        target_fps: int = 30,
        mel_sequence_length: int = 256,
        emotion_config: Optional[Dict] = None,
        device: str = "cuda",
        real_time_mode: bool = False,
        stride_frames: int = 1,
        emotion_provider=None,
        shard_across_ranks: bool = False,
        clip_emotion=None,
        share_frames: bool = False,
    ):
        if clip_emotion is not None and emotion_provider is not None:
            raise ValueError("clip_emotion and emotion_provider both produce the emotion input: pass one of them")
        super().__init__(d_model=d_model, num_heads=num_heads, num_blendshapes=num_blendshapes,
                         sample_rate=sample_rate, target_fps=target_fps, mel_sequence_length=mel_sequence_length,
                         emotion_config=emotion_config, device=device, real_time_mode=real_time_mode,
                         emotion_provider=emotion_provider)
        self.stride_frames = stride_frames
        # not in the reference (single process): under torch.distributed the output frames of a clip are computed in contiguous
        # chunks, one per rank, and smoothed once over the gathered sequence (koemorph_amd.parallel.sequence_apply)
        self.shard_across_ranks = shard_across_ranks
        # not in the reference either: the clips' emotion tracks, built per forward call (ClipEmotion.build_batch)
        width = getattr(clip_emotion, "emotion_dim", self.emotion_dim)       # an object that only maps windows to rows names none
        if width != self.emotion_dim:
            raise ValueError(f"clip_emotion produces rows of {width} values, the model's emotion_dim is {self.emotion_dim}")
        self.clip_emotion = clip_emotion
        # not in the reference: each clip's STFT once at every shape and hop, the windows assembled on the device (engine option
        # "seq_assemble", Engine.sequence_plan route 2); off, the engine keeps its default schedule for the shape
        self.share_frames = bool(share_frames)
        self._share_frames_applied = False
        self.window_frames = mel_sequence_length                      # reference :51
        self.window_samples = self.window_frames * self.hop_length    # :54
        self.stride_samples = self.stride_frames * self.hop_length    # :55

    def _track_mapping(self):
        if self.clip_emotion is None:
            raise ValueError("emotion_track needs the model's clip_emotion: its shape maps windows to rows")
        sh = self.clip_emotion.shape
        return int(sh["min_samples"]), int(sh["update_samples"])

    def forward(self, audio: torch.Tensor, return_attention: bool = False,
                emotion_features: Optional[torch.Tensor] = None,
                emotion_track: Optional[torch.Tensor] = None, attention_stats=None) -> Dict[str, torch.Tensor]:
        """``attention_stats`` (not in the reference): a ``koemorph_amd.metrics.AttentionStats`` that takes the attention map of
        every window on the device, tile by tile, whether or not the maps are returned."""
        if audio.dim() != 2:
            raise ValueError(f"Expected 2D input, got {audio.dim()}D")
        if emotion_track is not None and emotion_features is not None:
            raise ValueError("emotion_track and emotion_features both produce the emotion input: pass one of them")
        batch_size, audio_length = audio.shape
        emotion_metadata = {"backend_used": self.emotion_backend}
        mapping = None
        if emotion_track is not None:
            mapping = self._track_mapping()
        elif emotion_features is None and self.clip_emotion is not None:
            mapping = self._track_mapping()
            emotion_track, _ = self.clip_emotion.build_batch(audio.to(torch.float32).contiguous())
            emotion_metadata = {"backend_used": getattr(self.clip_emotion, "backend", "egemaps") + "_track"}     # or 'basic_track'
        elif emotion_features is None:                                 # emotion features ONCE per clip (:88)
            emotion_features, emotion_metadata = self.extract_emotion_features(audio)
        if mapping is not None:
            if emotion_track.dim() != 3 or emotion_track.shape[0] != batch_size or emotion_track.shape[2] != self.emotion_dim:
                raise ValueError(f"expected a ({batch_size}, K, {self.emotion_dim}) emotion_track, got {tuple(emotion_track.shape)}")
            if emotion_track.shape[1] == 0:                            # no update yet: the zero vector ClipEmotion.rows gives
                emotion_track = torch.zeros(batch_size, 1, emotion_track.shape[2], device=audio.device)
        eng = self.dual_stream_attention.engine()
        if self.share_frames or self._share_frames_applied:            # (a model that never asked leaves the engine's switch alone)
            eng.set_option("seq_assemble", int(self.share_frames))
            self._share_frames_applied = self.share_frames
        self.reset_temporal_state()                                    # :99
        self.dual_stream_attention.require_eval_mode()
        results: Dict[str, object] = {}
        if self.shard_across_ranks:
            # with return_attention every rank computes the whole sequence: the maps are not gathered
            from .. import parallel
            seq = parallel.sequence_apply(eng, audio, emotion_features, self.stride_frames, smooth=self.use_temporal_smoothing,
                                          emotion_track=emotion_track, track_shape=mapping, return_attention=return_attention,
                                          stats=attention_stats)
        elif mapping is not None:
            seq = eng.sequence_forward_track(audio, emotion_track, mapping[0], mapping[1], self.stride_frames,
                                             smooth=self.use_temporal_smoothing, return_attention=return_attention,
                                             stats=attention_stats)
        else:
            seq = eng.sequence_forward(audio, emotion_features, self.stride_frames,
                                       smooth=self.use_temporal_smoothing, return_attention=return_attention,
                                       stats=attention_stats)
        if return_attention:
            # one call for every window (km_sequence_forward_attn): the blendshapes are the bits of the plain call
            results['mel_attention_weights'] = seq['mel_attention_weights']
            # softmax over a single key (reference dual_stream_attention.py:234-239)
            results['emotion_attention_weights'] = torch.ones(seq['raw'].shape[0], seq['raw'].shape[1], 24, 1, device=audio.device)
            seq = seq['blendshapes']
        if self.use_temporal_smoothing and seq.shape[1] > 0:
            self.prev_blendshapes = seq[:, -1].clone()                 # the state the reference is left with
        results['blendshapes'] = seq
        results['num_frames'] = seq.shape[1]
        results['fps'] = self.target_fps
        results['emotion_backend'] = emotion_metadata.get("backend_used", "unknown")
        results['emotion_processing_time'] = emotion_metadata.get("processing_time", 0.0)
        return results

    def forward_single_frame(self, audio: torch.Tensor, frame_idx: int = None) -> Dict[str, torch.Tensor]:
        return SimplifiedDualStreamModel.forward(self, audio, return_attention=False)
