"""Sequential (time-series aware) training -- mirror of the reference's ``src/train_sequential.py``.

``SequentialTrainer`` keeps the reference's shape: ``train_epoch()`` walks the windows of each clip in time order,
resets the model's temporal (EMA) state whenever the file changes (:136-155), runs forward, loss, backward, global-norm
clipping and AdamW (:157-181), steps the CosineAnnealingWarmRestarts schedule once per epoch (:209); ``validate()``,
``save_checkpoint()`` / ``load_checkpoint()`` with the reference's checkpoint keys (:303-339).  What differs is where the
work happens: batches come from the device-resident ``koemorph_amd.data.SequentialKoeMorphDataset`` and the whole step is
the HIP training step behind the C-ABI (``koemorph_amd.training.Trainer``).  Data parallel: one process per GPU
(``torchrun``), every rank takes a contiguous share of each batch and the flat gradient is all-reduced over RCCL.

The reference's ``MultiTaskLoss`` does not exist in its ``src/model/losses.py``; the loss here is ``KoeMorphLoss``
(mse + optional terms, src/model/losses.py:29-178) against the label of each window's last frame.  The 256-D emotion
vector is an input of the model: a ``ClipEmotion`` (``--emotion egemaps``) gives every window the row of its clip's eGeMAPS
emotion track that a live stream would hold when the window ends, gathered by start frame, so the step stays on the resident
clip; ``--variant basic --emotion basic`` is the same at the ``basic`` shape (d_model 128, 4 heads, emotion_dim 9) with the track of
nine prosodic values per row (``ClipEmotion(backend="basic")``); ``--variant fast --emotion gemaps --emotion-context-window 10
--emotion-update-interval 0.5`` is the reference's ``fast`` recipe, the track of the 62 GeMAPS functionals through a ``Linear(186, 256)``
that goes into the checkpoint (``ClipEmotion(feature_set="GeMAPS")``); ``emotion_provider(audio) -> (B, emotion_dim)`` is handed window
audio instead; without either the reference's own failure fallback is used (``randn * 0.1`` of the engine's emotion width,
simplified_dual_stream_model.py:250-267), seeded per window for reproducibility.
No hydra / TensorBoard dependency: plain argparse, metrics to the log.
"""
from __future__ import annotations

import argparse
import logging
import time
from pathlib import Path
from typing import Callable, Dict, Optional

import numpy as np
import torch

from .. import parallel, synth
from ..data import SequentialKoeMorphDataset
from .._lib import KM_ERR_INVALID_ARG, KoeMorphError
from ..engine import Engine
from ..features.clip_emotion import ClipEmotion
from ..metrics import BlendshapeMetrics, LossTerms
from ..training import Trainer

logger = logging.getLogger(__name__)


class SequentialTrainer:
    def __init__(self, engine: Engine, train_data: SequentialKoeMorphDataset, val_data: Optional[SequentialKoeMorphDataset] = None,
                 device: str = "cuda", learning_rate: float = 1e-4, weight_decay: float = 1e-5, gradient_clip: float = 1.0,
                 mse_weight: float = 1.0, l1_weight: float = 0.0, extra_loss_terms: Optional[Dict[str, float]] = None,
                 emotion_provider: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, dropout: float = 0.1, seed: int = 0,
                 from_clip: bool = False, clip_emotion: Optional[ClipEmotion] = None, clip_assemble: bool = False,
                 record_emotion_timing: bool = False):
        """``from_clip``: batches that name their windows inside the resident clip (``resident_windows=True`` data sets) go
        through ``Trainer.step_clip`` -- no window copy, shared STFT frames; same losses and weights, bit for bit.  An
        ``emotion_provider`` is handed window audio, so with one installed the trainer stays on the gathered path.
        ``clip_assemble``: sets the engine's option of that name, with which ``step_clip`` / ``forward_clip`` also run at the
        shapes and hops they refuse by default (hop below n_fft / 2, no fused core: ``Engine.clip_plan`` route 2) instead of
        gathering; same bits again.  Off, the engine's option is left as it is.
        ``clip_emotion``: the emotion rows come from each clip's emotion track (built once per clip and kept on the device),
        gathered by start frame; it reads no window audio, so ``step_clip`` / ``forward_clip`` stay in use.  It needs batches that
        name their clip (``resident_windows=True``) and excludes an ``emotion_provider``.
        ``dropout``: the reference trains under ``model.train()`` (src/train_sequential.py:118) on a model built with
        dropout 0.1 (simplified_dual_stream_model.py:155): the attention weights of both streams and the decoder's hidden
        layer are dropped per step; ``validate()`` runs the eval-mode inference kernels.  Every rank draws its own masks
        (generator seed = ``seed`` + rank); the generator's step counter is part of the checkpoint."""
        self.engine, self.device = engine, torch.device(device)
        self.train_data, self.val_data = train_data, val_data
        if clip_emotion is not None and emotion_provider is not None:
            raise ValueError("clip_emotion and emotion_provider both produce the emotion input: pass one of them")
        if clip_emotion is not None and clip_emotion.emotion_dim != engine.emotion_dim:
            raise ValueError(f"clip_emotion produces rows of {clip_emotion.emotion_dim} values ({clip_emotion.backend} back end), "
                             f"the engine's emotion_dim is {engine.emotion_dim}")
        self.emotion_provider = emotion_provider
        self.clip_emotion = clip_emotion
        # the track's context window and update interval go into the checkpoint's model_config (render_sequential builds the same track)
        self.record_emotion_timing = record_emotion_timing and clip_emotion is not None
        self.from_clip = from_clip
        if clip_assemble:
            engine.set_option("clip_assemble", 1)
        self._from_clip_logged = False
        self.rank, self.world = (torch.distributed.get_rank(), torch.distributed.get_world_size()) \
            if torch.distributed.is_initialized() else (0, 1)
        self.trainer = Trainer(engine, max_windows=train_data.batch_size, lr=learning_rate, weight_decay=weight_decay,
                               grad_clip=gradient_clip, mse_weight=mse_weight, l1_weight=l1_weight, use_smoothing=True,
                               dropout=dropout, seed=seed + self.rank)
        if extra_loss_terms:
            self.trainer.set_loss_terms(**extra_loss_terms)
        self.mse_weight, self.l1_weight = mse_weight, l1_weight
        self.extra_loss_terms = dict(extra_loss_terms or {})
        self._val_clip_logged = False
        self.epoch = 0
        self.global_step = 0
        self.best_val_loss = float("inf")
        self.current_file_idx = None
        self._shapes = {k: tuple(v.shape) for k, v in engine.state_dict_shapes().items()}

    # ---- helpers ----------------------------------------------------------------------------------------
    def _emotion(self, batch) -> torch.Tensor:
        if self.clip_emotion is not None:
            if "clip_audio" not in batch or "start_frames_dev" not in batch:
                raise KoeMorphError(KM_ERR_INVALID_ARG, "clip_emotion reads the resident clip: build the data set with resident_windows=True")
            ce, ds, clip = self.clip_emotion, self.train_data, batch["clip_audio"]
            # keyed by file index and by where the clip lies: the training and validation sets number their files alike
            track = ce.track_for((int(batch["file_indices"][0]), clip.data_ptr()), clip)
            return ce.rows(track, clip.shape[0], batch["start_frames_dev"], ds.hop_length, ds.window_frames)
        if self.emotion_provider is not None:
            return self.emotion_provider(batch["audio"]).to(self.device, torch.float32)
        D = self.engine.emotion_dim
        rows = [0.1 * synth.normal(1000003 * int(f) + int(w), (D,)) for f, w in zip(batch["file_indices"], batch["window_indices"])]
        return torch.from_numpy(np.stack(rows)).to(self.device)

    def _my_share(self, batch):
        """This rank's contiguous share of the batch (windows shard embarrassingly; only the gradient is reduced)."""
        B = batch["target"].shape[0]
        lo, hi = parallel.shard_range(B, self.rank, self.world)
        return {k: (v[lo:hi] if isinstance(v, (torch.Tensor, list)) and k != "clip_audio" else v) for k, v in batch.items()}, hi - lo

    def _with_audio(self, batch):
        """A resident-window batch with its windows gathered (validation, an emotion provider): the keys ``gather`` gives."""
        if "audio" in batch:
            return batch
        ds = self.train_data
        B = batch["target"].shape[0]
        audio = torch.empty(B, ds.window_samples, device=self.device)
        clip = batch["clip_audio"]
        from .._lib import check
        with torch.cuda.device(self.device):
            check(ds._lib.km_gather_windows(clip.data_ptr(), clip.shape[0], batch["start_frames_dev"].data_ptr(), B, ds.hop_length,
                                            ds.window_samples, audio.data_ptr(), None, 0, 0, 0, None, None,
                                            torch.cuda.current_stream(self.device).cuda_stream))
        return {**batch, "audio": audio}

    # ---- reference API ----------------------------------------------------------------------------------
    def train_epoch(self, metrics: bool = False) -> Dict[str, float]:
        """``metrics=True``: every step's output (``Trainer.out``) and target also go into a ``BlendshapeMetrics`` on the
        device (src/train.py:214: the reference's trainer feeds its train_metrics the same way); its ``compute()`` is merged
        into the result.  The loss and the weights are what they are without it."""
        total, n = 0.0, 0
        bm = BlendshapeMetrics() if metrics else None
        t0 = time.time()
        for batch in self.train_data:
            file_idx = int(batch["file_indices"][0])
            if self.current_file_idx != file_idx:            # new clip: the EMA state must not leak across files
                self.current_file_idx = file_idx
                self.trainer.reset_temporal_state()
            share, nb = self._my_share(batch)
            B_global = batch["target"].shape[0]
            if nb == 0:                                      # fewer windows than ranks: weight 0 in the global mean
                self.trainer.flat_grad.zero_()
                self.trainer.optimizer_step(weight=0.0)
                continue
            # every rank's gradient is weighted by its share of the GLOBAL batch (shares differ by one window when the
            # batch does not divide, and the last batch of a clip is short): the sum is the full-batch gradient
            if "clip_audio" in share and self.from_clip and self.emotion_provider is None:
                sf = share["start_frames"]
                loss = self.trainer.step_clip(share["clip_audio"], share["start_frames_dev"], self._emotion(share), share["target"],
                                              global_batch=B_global, extremes=(int(sf.min()), int(sf.max())))
            else:
                if "clip_audio" in share and not self._from_clip_logged:
                    self._from_clip_logged = True
                    logger.info("resident-window batches are gathered before the step (%s)",
                                "the emotion provider reads window audio" if self.emotion_provider is not None else "from_clip is off")
                share = self._with_audio(share)
                loss = self.trainer.step(share["audio"], self._emotion(share), share["target"], global_batch=B_global)
            if bm is not None:
                bm.update(self.trainer.out[:nb], share["target"])
            total += float(loss.item())
            n += 1
            self.global_step += 1
        self.trainer.end_epoch()                             # CosineAnnealingWarmRestarts(T_0=10, T_mult=2, eta_min=1e-6)
        self.epoch += 1
        out = {"total": total / max(n, 1), "batches": n, "lr": self.trainer.lr, "seconds": time.time() - t0}
        if bm is not None:
            out.update(bm.compute())
            bm.close()
        return out

    def validate(self, metrics: bool = False, components: bool = False) -> Dict[str, float]:
        """``metrics=True``: the reference's validation metrics (src/train.py:239, :260-298) over every window of the pass,
        accumulated on the device with no host round trip per batch and merged into the result; "total" is unchanged.
        ``components=True``: the loss by component and per-sequence statistics, as the reference's validate() reports them
        (src/train_sequential.py:213-295), see ``_validate_components``."""
        if self.val_data is None:
            return {}
        if components:
            return self._validate_components(metrics)
        self.trainer.sync_inference_weights()
        total, n = 0.0, 0
        bm = BlendshapeMetrics() if metrics else None
        state = None
        current = None
        with torch.no_grad():
            for batch in self.val_data:
                batch = self._with_audio(batch)
                file_idx = int(batch["file_indices"][0])
                B = batch["audio"].shape[0]
                first = current != file_idx or state is None or state.shape[0] != B
                if first:
                    current, state = file_idx, torch.zeros(B, 52, device=self.device)
                pred = self.engine.forward_audio(batch["audio"], self._emotion(batch), state=state, first=first)
                if bm is not None:
                    bm.update(pred, batch["target"])
                total += float(torch.nn.functional.mse_loss(pred, batch["target"]).item())
                n += 1
        out = {"total": total / max(n, 1), "batches": n}
        if bm is not None:
            out.update(bm.compute())
            bm.close()
        return out

    def _loss_term_inputs(self):
        """The trainer's own weights and the static inputs of its extra terms, as ``LossTerms.update`` takes them; the
        per-batch inputs (prev_pred / prev_target / ds_prev_pred / audio features) are validation's own."""
        ex = self.extra_loss_terms
        weights = {"mse_weight": self.mse_weight, "l1_weight": self.l1_weight}
        for k in ("perceptual_weight", "temporal_weight", "sparsity_weight", "smoothness_weight", "landmark_weight", "velocity_weight",
                  "ds_velocity_weight", "ds_separation_weight"):
            weights[k] = float(ex.get(k, 0.0))
        return weights, ex.get("landmark_weights")

    def _validate_components(self, metrics: bool) -> Dict[str, float]:
        """The validation pass with the loss summed by component on the device (``LossTerms``): no ``.item()`` per batch.
        Batches that name their windows inside the resident clip go through ``Engine.forward_clip`` -- no window copy, the
        STFT frames the windows share computed once, same bits -- under the conditions ``train_epoch`` applies to
        ``step_clip`` (``from_clip``, no emotion provider) and where ``forward_clip_supported()``; every other batch is
        gathered.  ``prev_pred`` / ``prev_target`` of a batch are the previous batch's prediction and target of the same
        file (absent on a file's first batch and when the batch size changes: the EMA state's own ``first`` rule).
        Returns "total" (mean per-batch MSE), "batches", one key per loss term, "weighted_total", and "sequence_stats":
        ``{file name or index: {"loss", "smoothness", "batches"}}``, read back once per file."""
        self.trainer.sync_inference_weights()
        weights, landmark_w = self._loss_term_inputs()
        clip_ok = self.from_clip and self.emotion_provider is None and self.engine.forward_clip_supported()
        lt_all, lt_file = LossTerms(**weights), LossTerms(**weights)
        bm = BlendshapeMetrics() if metrics else None
        stats: Dict[object, Dict[str, float]] = {}
        state = prev_pred = prev_target = None
        current = current_name = None
        n = 0

        def close_file():
            m = lt_file.compute()                            # the one readback per file
            if m:
                stats[current_name] = {"loss": m["total"], "smoothness": m["row_smoothness"], "batches": int(m["updates"])}
            lt_file.reset()

        with torch.no_grad():
            for batch in self.val_data:
                file_idx = int(batch["file_indices"][0])
                B = batch["target"].shape[0]
                new_file = current != file_idx
                first = new_file or state is None or state.shape[0] != B
                if new_file:
                    if current is not None:
                        close_file()
                    names = batch.get("file_names")
                    current, current_name = file_idx, (names[0] if names else file_idx)
                if first:
                    state, prev_pred, prev_target = torch.zeros(B, 52, device=self.device), None, None
                if "clip_audio" in batch and "audio" not in batch and clip_ok:
                    sf = batch["start_frames"]
                    pred = self.engine.forward_clip(batch["clip_audio"], batch["start_frames_dev"], self._emotion(batch), state=state,
                                                    first=first, extremes=(int(sf.min()), int(sf.max())))
                else:
                    if "clip_audio" in batch and "audio" not in batch and not self._val_clip_logged:
                        self._val_clip_logged = True
                        logger.info("resident-window validation batches are gathered before the forward (%s)",
                                    "the emotion provider reads window audio" if self.emotion_provider is not None else
                                    ("from_clip is off" if not self.from_clip else "forward_clip is not supported at this shape"))
                    batch = self._with_audio(batch)
                    pred = self.engine.forward_audio(batch["audio"], self._emotion(batch), state=state, first=first)
                target = batch["target"]
                kw = dict(prev_pred=prev_pred, prev_target=prev_target, landmark_w=landmark_w,
                          ds_prev_pred=prev_pred if weights["ds_velocity_weight"] > 0 else None)
                lt_all.update(pred, target, **kw)
                lt_file.update(pred, target, **kw)
                if bm is not None:
                    bm.update(pred, target)
                prev_pred, prev_target = pred, target
                n += 1
        if current is not None:
            close_file()
        m = lt_all.compute()
        out = {"total": m.get("mse", 0.0), "batches": n}
        for k, v in m.items():
            if k == "total":
                out["weighted_total"] = v
            elif k not in ("updates", "row_smoothness"):
                out[k] = v
        out["sequence_stats"] = stats
        lt_all.close(); lt_file.close()
        if bm is not None:
            out.update(bm.compute())
            bm.close()
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference model's state dict (keys of SimplifiedDualStreamModel: dual_stream_attention.* + smoothing_alpha)."""
        p = self.trainer.params(self._shapes)
        out = {}
        for k, v in p.items():
            out[k if k == "smoothing_alpha" else "dual_stream_attention." + k] = torch.from_numpy(np.asarray(v))
        return out

    def save_checkpoint(self, path, is_best: bool = False):
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        ckpt = {"epoch": self.epoch, "global_step": self.global_step, "model_state_dict": self.state_dict(),
                "best_val_loss": self.best_val_loss, "optimizer_state_dict": self.trainer.optimizer_state(),
                "current_file_idx": -1 if self.current_file_idx is None else int(self.current_file_idx),
                "model_config": {"d_model": self.engine.d_model, "num_heads": self.engine.num_heads,
                                 "mel_sequence_length": self.engine.mel_sequence_length, "emotion_dim": self.engine.emotion_dim,
                                 "emotion_backend": self.clip_emotion.backend if self.clip_emotion is not None else
                                 ("provider" if self.emotion_provider is not None else "noise")}}
        if self.clip_emotion is not None and getattr(self.clip_emotion, "feature_set", "eGeMAPSv02") == "GeMAPS":
            # render_sequential --emotion gemaps reads both: the set, and the Linear(186, 256) the track went through
            layer = self.clip_emotion.compression_layer
            ckpt["model_config"]["emotion_feature_set"] = "GeMAPS"
            ckpt["emotion_compression"] = {"weight": layer.weight.detach().cpu().clone(), "bias": layer.bias.detach().cpu().clone()}
        if self.record_emotion_timing:
            ckpt["model_config"].update(emotion_context_window=float(self.clip_emotion.context_window),
                                        emotion_update_interval=float(self.clip_emotion.update_interval))
        if self.rank == 0:
            torch.save(ckpt, path)
            if is_best:
                torch.save(ckpt, path.parent / "best_model.pth")

    def load_checkpoint(self, path):
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        sd = {k.replace("dual_stream_attention.", "", 1): v.numpy() for k, v in ckpt["model_state_dict"].items()}
        self.trainer.load_params(sd)
        self.epoch = int(ckpt["epoch"]); self.global_step = int(ckpt["global_step"])
        self.best_val_loss = float(ckpt.get("best_val_loss", float("inf")))
        try:
            self.trainer.load_optimizer_state(ckpt["optimizer_state_dict"])
        except (ValueError, KeyError, TypeError, AttributeError) as exc:
            # a checkpoint of the reference's own trainer (optimizer_state_dict = a torch.optim dict keyed by parameter index,
            # src/train_sequential.py:303-339) or of a build that predates the per-key layout: the weights above are what
            # matters, the moments restart -- the same thing torch users do with load_state_dict(strict=False) on a new optimizer
            import warnings
            warnings.warn(f"optimizer state of {path} not loaded ({exc}); resuming from the model weights with fresh AdamW moments",
                          RuntimeWarning, stacklevel=2)
            self.trainer.restart_optimizer(self.epoch)
        cf = int(ckpt.get("current_file_idx", -1))
        self.current_file_idx = None if cf < 0 else cf


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Sequential training of the dual-stream KoeMorph model on MI355X")
    p.add_argument("--data_dir", required=True, help="directory with *.wav + *.jsonl pairs")
    p.add_argument("--val_dir", help="validation directory (optional)")
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--batch_size", type=int, default=8, help="windows per step over ALL ranks")
    p.add_argument("--window_frames", type=int, default=256, help="frames per window (with --variant: the variant's unless given)")
    p.add_argument("--stride_frames", type=int, default=1)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-5)
    p.add_argument("--gradient_clip", type=float, default=1.0)
    p.add_argument("--l1_weight", type=float, default=0.0)
    p.add_argument("--dropout", type=float, default=0.1, help="train-mode dropout probability (the reference's model: 0.1; 0 = eval-mode arithmetic)")
    p.add_argument("--seed", type=int, default=0, help="dropout generator seed (rank r uses seed + r)")
    p.add_argument("--checkpoint_dir", default="checkpoints")
    p.add_argument("--resume", help="checkpoint to resume from")
    p.add_argument("--max_files", type=int)
    p.add_argument("--resident-clip", dest="resident_clip", action="store_true",
                   help="train from the clips resident in GPU memory (Trainer.step_clip): no window copies, the STFT frames the "
                        "windows of a batch share are computed once; same losses and weights")
    p.add_argument("--clip-assemble", dest="clip_assemble", action="store_true",
                   help="with --resident-clip: train and validate from the resident clip at every shape and hop (engine option "
                        "clip_assemble: span image + edge rows per window) instead of gathering where the default refuses")
    p.add_argument("--device-resample", dest="device_resample", action="store_true",
                   help="WAV files at another rate are uploaded as they are and converted to 16 kHz on the device")
    p.add_argument("--loss-components", dest="loss_components", action="store_true",
                   help="validation reports the loss by component (LossTerms) and per-sequence loss / smoothness; with "
                        "--resident-clip the validation forward runs from the resident clip (Engine.forward_clip)")
    p.add_argument("--emotion", choices=("noise", "egemaps", "basic", "gemaps"), default="noise",
                   help="the model's emotion input: noise = the reference's extraction-failure fallback (randn * 0.1 per window); "
                        "egemaps = each clip's eGeMAPS emotion track, computed once on the device and gathered by start frame "
                        "(ClipEmotion; implies resident batches, what a StreamEmotion serves at inference); basic = the same track "
                        "of nine prosodic values per row (ClipEmotion(backend='basic'), what StreamEmotion(backend='basic') serves; "
                        "needs an emotion_dim of 9: --variant basic); gemaps = the eGeMAPS track's kernels at the 62 functionals of "
                        "GeMAPS through a Linear(186, 256) that is saved with the checkpoint (ClipEmotion(feature_set='GeMAPS'); with "
                        "--variant fast --emotion-context-window 10 --emotion-update-interval 0.5 the reference's `fast` recipe)")
    p.add_argument("--emotion-context-window", dest="emotion_context_window", type=float, default=None, metavar="SECONDS",
                   help="seconds of audio behind a row of the emotion track (default 20.0).  configs/model/dual_stream.yaml: fast 10, "
                        "long_context 30.  Given, the eGeMAPS track takes windows beyond 20.5 s (ClipEmotion(long_windows=True), up to "
                        "65.5 s) and both values are written into the checkpoint's model_config")
    p.add_argument("--emotion-update-interval", dest="emotion_update_interval", type=float, default=None, metavar="SECONDS",
                   help="seconds between two rows of the emotion track (default 0.3).  configs/model/dual_stream.yaml: fast 0.5, "
                        "long_context 0.2.  Given, as --emotion-context-window")
    p.add_argument("--variant", choices=tuple(VARIANTS), default="default",
                   help="the model shape, as configs/model/dual_stream.yaml names its variants: d_model, heads, emotion_dim and the "
                        "default of --window_frames")
    p.add_argument("--metrics", action="store_true", help="log mae / rmse / mean_correlation / f1_score of every epoch (BlendshapeMetrics)")
    return p


# d_model, num_heads, mel_sequence_length, emotion_dim of configs/model/dual_stream.yaml and its `variants`
VARIANTS = {"default": dict(d_model=256, num_heads=8, window_frames=256, emotion_dim=256),
            "fast": dict(d_model=128, num_heads=4, window_frames=128, emotion_dim=256),
            "basic": dict(d_model=128, num_heads=4, window_frames=256, emotion_dim=9),
            "long_context": dict(d_model=512, num_heads=16, window_frames=512, emotion_dim=256)}


def parse_args(argv=None) -> argparse.Namespace:
    """The command line with the variant resolved: ``d_model``, ``num_heads`` and ``emotion_dim`` are the variant's, ``window_frames``
    is the variant's unless --window_frames is given.  ``--emotion basic`` with an emotion_dim other than 9 is a usage error."""
    p = build_parser()
    p.set_defaults(window_frames=None)                   # None: not given on the command line
    args = p.parse_args(argv)
    v = VARIANTS[args.variant]
    args.d_model, args.num_heads, args.emotion_dim = v["d_model"], v["num_heads"], v["emotion_dim"]
    if args.window_frames is None:
        args.window_frames = v["window_frames"]
    if args.emotion == "basic" and args.emotion_dim != 9:
        p.error(f"--emotion basic produces 9 values per window, the emotion_dim of --variant {args.variant} is {args.emotion_dim}: "
                "use --variant basic")
    if args.emotion in ("egemaps", "gemaps") and args.emotion_dim != 256:
        p.error(f"--emotion {args.emotion} produces 256 values per window, the emotion_dim of --variant {args.variant} is {args.emotion_dim}")
    args.emotion_timing_given = args.emotion_context_window is not None or args.emotion_update_interval is not None
    if args.emotion_timing_given and args.emotion == "noise":
        p.error("--emotion-context-window / --emotion-update-interval shape the emotion track: use --emotion egemaps or basic")
    return args


GEMAPS_COMPRESSION_SEED = 0   # the Linear(186, 256) of --emotion gemaps: torch's default initialisation under this seed, saved with the checkpoint


def gemaps_compression_layer() -> torch.nn.Linear:
    with torch.random.fork_rng(devices=[]):                # the caller's generator is left as it was
        torch.manual_seed(GEMAPS_COMPRESSION_SEED)
        return torch.nn.Linear(186, 256)


def clip_emotion_from_args(args, device) -> Optional[ClipEmotion]:
    """The ClipEmotion of the command line: none for noise; without the two timing flags the 20.0 s / 0.3 s object as ever; with
    either, that timing and -- eGeMAPS -- windows beyond 2048 frames (the basic back end takes them as it is).  gemaps: the eGeMAPS
    back end at the GeMAPS feature set, with a seeded Linear(186, 256)."""
    if args.emotion not in ("egemaps", "basic", "gemaps"):
        return None
    kw = dict(device=device, backend=args.emotion)
    if args.emotion == "gemaps":
        kw = dict(device=device, backend="egemaps", feature_set="GeMAPS", compression_layer=gemaps_compression_layer())
    if not args.emotion_timing_given:
        return ClipEmotion(**kw)
    return ClipEmotion(20.0 if args.emotion_context_window is None else args.emotion_context_window,
                       0.3 if args.emotion_update_interval is None else args.emotion_update_interval,
                       long_windows=args.emotion != "basic", **kw)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    rank, world, local = parallel.init_from_env()
    device = f"cuda:{local}"
    torch.cuda.set_device(local)
    eng = Engine(d_model=args.d_model, num_heads=args.num_heads, mel_sequence_length=args.window_frames, emotion_dim=args.emotion_dim)
    eng.load_state_dict(synth.make_core_params(0, d_model=args.d_model, mel_sequence_length=args.window_frames,
                                               emotion_dim=args.emotion_dim, style="init"))
    eng.finalize(device)
    kw = dict(window_frames=args.window_frames, stride_frames=args.stride_frames, shuffle_files=False, loop_dataset=False,
              batch_size=args.batch_size, device=device, max_files=args.max_files, device_resample=args.device_resample)
    track = args.emotion in ("egemaps", "basic", "gemaps")       # the track is read from the resident clip: every batch must name it
    train = SequentialKoeMorphDataset(args.data_dir, resident_windows=args.resident_clip or track, **kw)
    val = SequentialKoeMorphDataset(args.val_dir, resident_windows=(args.resident_clip and args.loss_components) or track, **kw) \
        if args.val_dir else None
    st = SequentialTrainer(eng, train, val, device=device, learning_rate=args.learning_rate, weight_decay=args.weight_decay,
                           gradient_clip=args.gradient_clip, l1_weight=args.l1_weight, dropout=args.dropout, seed=args.seed,
                           from_clip=args.resident_clip,
                           clip_emotion=clip_emotion_from_args(args, device), clip_assemble=args.clip_assemble,
                           record_emotion_timing=args.emotion_timing_given)
    if args.resume:
        st.load_checkpoint(args.resume)
    for _ in range(st.epoch, args.epochs):
        m = st.train_epoch(metrics=args.metrics)
        v = st.validate(metrics=args.metrics, components=args.loss_components)
        is_best = bool(v) and v["total"] < st.best_val_loss
        if is_best:
            st.best_val_loss = v["total"]
        if rank == 0:
            logger.info(f"epoch {st.epoch}: train {m['total']:.6f} ({m['batches']} steps, {m['seconds']:.1f} s, lr {m['lr']:.2e})"
                        + (f", val {v['total']:.6f}" if v else ""))
            if args.loss_components and v:
                logger.info("  val terms: " + ", ".join(f"{k} {v[k]:.6f}" for k in ("mse", "l1", "perceptual", "temporal", "velocity",
                                                                                    "sparsity", "smoothness", "landmark") if k in v)
                            + f"; {len(v['sequence_stats'])} sequences")
            if args.metrics:                                 # the reference logs these four per epoch (src/train.py:368-373)
                for tag, d in (("train", m), ("val", v)):
                    if "mae" in d:
                        logger.info(f"  {tag} metrics: mae {d['mae']:.6f}, rmse {d['rmse']:.6f}, "
                                    f"mean_correlation {d['mean_correlation']:.4f}, f1_score {d['f1_score']:.4f}")
        st.save_checkpoint(Path(args.checkpoint_dir) / f"checkpoint_epoch_{st.epoch}.pth", is_best=is_best)


if __name__ == "__main__":
    main()
