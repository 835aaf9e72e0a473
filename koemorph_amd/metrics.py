"""Evaluation metrics -- mirror of the reference's ``BlendshapeMetrics`` (src/model/losses.py:421-521) and
``compute_lip_sync_metrics`` (:524-583).

The reference copies every batch to the host, concatenates the epoch and reduces it with torch on the CPU.  Here device
tensors are folded into a float64 accumulator in device memory by the HIP kernels behind ``km_metrics_*``
(koemorph_amd/csrc/km_metrics.hip): ``update`` enqueues one call on the current stream and returns, ``compute`` enqueues
the finalisation and does the only readback.  CPU tensors run ``metrics_f64`` below, the float64 NumPy restatement of
both reference functions; it is also the yardstick of the GPU tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np

from ._lib import KM_LOSS_TERM_NAMES, KM_LOSS_TERMS, KM_METRICS_COUNT, KM_METRICS_NAMES, check, km_attn_stats_count, load

REFERENCE_KEYS = KM_METRICS_NAMES[:16]           # BlendshapeMetrics.compute(), in the reference's order
TEMPORAL_KEYS = ("temporal_consistency", "pred_smoothness", "target_smoothness")   # absent when one row was seen (:492)
LIP_SYNC_KEYS = KM_METRICS_NAMES[16:19]          # compute_lip_sync_metrics()
DIAGNOSTIC_KEYS = ("rows", "valid_correlations")  # ours: rows folded, columns that passed the std() > 1e-6 gate
MOUTH = slice(12, 32)                            # losses.py:543
ACTIVITY_THRESHOLD = np.float32(0.1)             # `tensor_f32 > 0.1` compares against 0.1 rounded to float32 (:501-503)


def _corr(x: np.ndarray, y: np.ndarray, gate_x: bool = True, gate_y: bool = True) -> Optional[float]:
    """torch.corrcoef(...)[0, 1] behind the reference's gates: unbiased std() > 1e-6 where gated, NaN -> None."""
    n = x.shape[0]
    if n < 2:
        return None                                          # std() of one value is NaN: the gate is closed
    x, y = x - x[0], y - y[0]                                # exact for constant input: its variance is exactly 0
    xc, yc = x - x.mean(), y - y.mean()
    vx, vy = float((xc * xc).sum()), float((yc * yc).sum())
    if gate_x and not np.sqrt(vx / (n - 1)) > 1e-6:
        return None
    if gate_y and not np.sqrt(vy / (n - 1)) > 1e-6:
        return None
    den = np.sqrt(vx) * np.sqrt(vy)
    if not den > 0.0:
        return None                                          # 0 / 0 in corrcoef
    return float(np.clip(float((xc * yc).sum()) / den, -1.0, 1.0))


def metrics_f64(pred, target, energy=None) -> Dict[str, float]:
    """Both reference functions over (N, 52) float32 rows, evaluated in float64: every key of
    ``BlendshapeMetrics.compute()`` (the three temporal keys only when N > 1), ``mouth_mae`` / ``mouth_correlation`` of
    ``compute_lip_sync_metrics``, ``audiovisual_sync`` when a per-row ``energy`` (N) is given, and DIAGNOSTIC_KEYS."""
    p32 = np.ascontiguousarray(np.asarray(pred, np.float32).reshape(-1, 52))
    t32 = np.ascontiguousarray(np.asarray(target, np.float32).reshape(-1, 52))
    if p32.shape != t32.shape:
        raise ValueError(f"pred {p32.shape} and target {t32.shape} differ")
    n = p32.shape[0]
    if n == 0:
        return {}
    p, t = p32.astype(np.float64), t32.astype(np.float64)
    m: Dict[str, float] = {}
    ad = np.abs(p - t)
    m["mae"] = float(ad.mean())
    m["mse"] = float(((p - t) ** 2).mean())
    m["rmse"] = float(np.sqrt(m["mse"]))
    per = ad.mean(axis=0)
    m["max_bs_mae"], m["min_bs_mae"], m["std_bs_mae"] = float(per.max()), float(per.min()), float(per.std(ddof=1))
    corrs = [c for c in (_corr(p[:, i], t[:, i]) for i in range(52)) if c is not None]
    m["mean_correlation"] = sum(corrs) / len(corrs) if corrs else 0.0
    m["min_correlation"] = min(corrs) if corrs else 0.0
    if n > 1:
        dp, dt = np.diff(p, axis=0), np.diff(t, axis=0)
        m["temporal_consistency"] = float(np.abs(dp - dt).mean())
        m["pred_smoothness"] = float(np.abs(dp).mean())
        m["target_smoothness"] = float(np.abs(dt).mean())
    pa, ta = p32 > ACTIVITY_THRESHOLD, t32 > ACTIVITY_THRESHOLD
    m["pred_activity"], m["target_activity"] = float(pa.sum()) / pa.size, float(ta.sum()) / ta.size
    tp, fp, fn = float((pa & ta).sum()), float((pa & ~ta).sum()), float((~pa & ta).sum())
    precision, recall = tp / (tp + fp + 1e-8), tp / (tp + fn + 1e-8)
    m["precision"], m["recall"] = precision, recall
    m["f1_score"] = 2 * precision * recall / (precision + recall + 1e-8)
    # compute_lip_sync_metrics
    m["mouth_mae"] = float(ad[:, MOUTH].mean())
    ap, at = p[:, MOUTH].sum(axis=1), t[:, MOUTH].sum(axis=1)
    c = _corr(ap, at)
    m["mouth_correlation"] = 0.0 if c is None else c
    if energy is not None:
        e = np.asarray(energy, np.float32).astype(np.float64).reshape(-1)
        if e.shape[0] != n:
            raise ValueError(f"energy has {e.shape[0]} rows, pred {n}")
        c = _corr(ap, e, gate_x=False)
        m["audiovisual_sync"] = 0.0 if c is None else c
    m["rows"] = float(n)
    m["valid_correlations"] = float(len(corrs))
    return m


def _energy_host(features) -> np.ndarray:
    """Per-row energy as compute_lip_sync_metrics reduces its features (losses.py:567-570), float64 -> float32."""
    f = np.asarray(features, np.float32).astype(np.float64)
    if f.ndim == 3:
        return np.sqrt((f * f).sum(-1)).mean(-1).astype(np.float32)
    if f.ndim == 2:
        return np.sqrt((f * f).sum(-1)).astype(np.float32)
    raise ValueError(f"audio_features must be 2-D or 3-D, got {f.ndim}-D")


def _rows(pred, target):
    if pred.shape[-1] != 52 or target.shape[-1] != 52:
        raise ValueError(f"last dimension must be 52 blendshapes, got pred {tuple(pred.shape)} target {tuple(target.shape)}")
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    return pred.reshape(-1, 52), target.reshape(-1, 52)


class BlendshapeMetrics:
    """``reset()``, ``update(pred, target, audio_features=None)``, ``compute() -> Dict[str, float]`` as the reference's
    class.  The first ``update`` after a reset decides where the epoch lives: device tensors go to the HIP accumulator of
    their device, CPU tensors / arrays are kept and reduced by ``metrics_f64``."""

    def __init__(self):
        self._acc = C.c_void_p()
        self._device = None
        self._lib = None
        self.reset()

    # ---- device plumbing --------------------------------------------------------------------------------
    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._device).cuda_stream

    def _open(self, device):
        import torch
        if self._acc and self._device != device:
            self.close()
        if not self._acc:
            self._lib = load()
            self._device = device
            with torch.cuda.device(device):
                check(self._lib.km_metrics_create(C.byref(self._acc)))

    def close(self):
        if self._acc:
            import torch
            torch.cuda.synchronize(self._device)
            self._lib.km_metrics_destroy(self._acc)
            self._acc = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference interface ----------------------------------------------------------------------------
    def reset(self):
        """Reset accumulated metrics (losses.py:432-436)."""
        self.rows = 0
        self._where: Optional[str] = None            # "device" | "host" after the first update
        self._host: List = []
        self._has_energy = False
        if self._acc:
            import torch
            with torch.cuda.device(self._device):
                check(self._lib.km_metrics_reset(self._acc, self._stream()))

    def update(self, pred_blendshapes, target_blendshapes, audio_features=None):
        """Fold a batch in (losses.py:438-449).  Any leading shape over 52 columns; ``audio_features`` (rows, D) or
        (rows, T, D) gives the per-row energy of ``audiovisual_sync``."""
        pred, target = _rows(pred_blendshapes, target_blendshapes)
        n = int(pred.shape[0])
        on_device = bool(getattr(pred, "is_cuda", False))
        where = "device" if on_device else "host"
        if self._where is not None and where != self._where:
            raise ValueError("one epoch mixes device and host tensors; reset() first")
        if audio_features is not None and int(audio_features.shape[0]) != n:
            raise ValueError(f"audio_features has {int(audio_features.shape[0])} rows, pred {n}")
        if audio_features is not None and audio_features.ndim not in (2, 3):
            raise ValueError(f"audio_features must be 2-D or 3-D, got {audio_features.ndim}-D")
        if n == 0:
            return
        self._where = where
        if not on_device:
            as_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
            self._host.append((np.array(as_np(pred), np.float32), np.array(as_np(target), np.float32),
                               None if audio_features is None else _energy_host(as_np(audio_features))))
            self.rows += n
            return
        import torch
        if target.device != pred.device:
            raise ValueError("pred and target are on different devices")
        self._open(pred.device)
        pred = pred.detach().to(torch.float32).contiguous()
        target = target.detach().to(torch.float32).contiguous()
        with torch.cuda.device(self._device):
            energy = None
            if audio_features is not None:
                af = audio_features.detach().to(self._device, torch.float32).contiguous()
                if af.dim() == 2:
                    af = af.unsqueeze(1)
                energy = torch.empty(n, device=self._device)
                check(self._lib.km_audio_energy(af.data_ptr(), n, af.shape[1], af.shape[2], energy.data_ptr(), self._stream()))
                self._has_energy = True
            check(self._lib.km_metrics_update(self._acc, pred.data_ptr(), target.data_ptr(),
                                              0 if energy is None else energy.data_ptr(), n, self._stream()))
        self.rows += n

    def _vector(self) -> np.ndarray:
        """km_metrics_compute on the current stream + the one readback: KM_METRICS_COUNT float32."""
        import torch
        with torch.cuda.device(self._device):
            out = torch.empty(KM_METRICS_COUNT, device=self._device)
            check(self._lib.km_metrics_compute(self._acc, out.data_ptr(), self._stream()))
            return out.cpu().numpy()

    def _all(self) -> Dict[str, float]:
        if self._where == "host":
            p = np.concatenate([h[0] for h in self._host])
            t = np.concatenate([h[1] for h in self._host])
            with_e = [h[2] is not None for h in self._host]
            if any(with_e) and not all(with_e):
                raise ValueError("audio_features were given for some host batches only")
            return metrics_f64(p, t, np.concatenate([h[2] for h in self._host]) if all(with_e) else None)
        v = self._vector()
        m = {k: float(v[i]) for i, k in enumerate(KM_METRICS_NAMES)}
        if m.pop("has_energy") == 0.0:
            del m["audiovisual_sync"]
        if self.rows < 2:
            for k in TEMPORAL_KEYS:
                del m[k]
        return m

    def compute(self, lip_sync: bool = False) -> Dict[str, float]:
        """Accumulated metrics (losses.py:451-521): the reference's keys in its order; ``{}`` before any update.
        ``lip_sync=True`` adds the keys of ``compute_lip_sync_metrics`` over the same rows and DIAGNOSTIC_KEYS."""
        if self.rows == 0:
            return {}
        m = self._all()
        keys = REFERENCE_KEYS + ((LIP_SYNC_KEYS + DIAGNOSTIC_KEYS) if lip_sync else ())
        return {k: m[k] for k in keys if k in m}


# KoeMorphLoss's default weights (src/model/losses.py:36-47); the two DualStreamLoss terms are off unless asked for
LOSS_TERM_DEFAULT_WEIGHTS = {"mse_weight": 1.0, "l1_weight": 0.1, "perceptual_weight": 0.5, "temporal_weight": 0.2,
                             "sparsity_weight": 0.01, "smoothness_weight": 0.1, "landmark_weight": 0.3, "velocity_weight": 0.05,
                             "ds_velocity_weight": 0.0, "ds_separation_weight": 0.0}


class LossTerms:
    """The loss by component, accumulated on the device (``km_loss_terms_*``, koemorph_amd/csrc/km_loss_terms.hip): what
    the reference reads back per batch as the ``metrics`` dict of ``KoeMorphLoss.forward`` (src/model/losses.py:111-183) and
    averages over the batches of a validation pass (src/train_sequential.py:262-290).

    ``update`` enqueues one call on the current stream and returns the batch's ``KM_LOSS_TERM_NAMES`` values as a device
    tensor (float32, nothing is read back); ``compute`` enqueues the finalisation and does the only readback.  Weights given
    to the constructor are the defaults of every ``update`` (``KoeMorphLoss``'s own where not given)."""

    def __init__(self, **weights):
        self._check_weights(weights)
        self.weights = {**LOSS_TERM_DEFAULT_WEIGHTS, **weights}
        self._acc = C.c_void_p()
        self._device = None
        self._lib = None
        self.updates = 0

    @staticmethod
    def _check_weights(weights):
        unknown = sorted(set(weights) - set(LOSS_TERM_DEFAULT_WEIGHTS))
        if unknown:
            raise TypeError(f"unknown loss weights {unknown}; known: {sorted(LOSS_TERM_DEFAULT_WEIGHTS)}")

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._device).cuda_stream

    def _open(self, device):
        import torch
        if self._acc and self._device != device:
            self.close()
        if not self._acc:
            self._lib = load()
            self._device = device
            with torch.cuda.device(device):
                check(self._lib.km_loss_terms_create(C.byref(self._acc)))

    def close(self):
        if self._acc:
            import torch
            torch.cuda.synchronize(self._device)
            self._lib.km_loss_terms_destroy(self._acc)
            self._acc = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.updates = 0
        if self._acc:
            import torch
            with torch.cuda.device(self._device):
                check(self._lib.km_loss_terms_reset(self._acc, self._stream()))

    def update(self, pred, target, prev_pred=None, prev_target=None, landmark_w=None, audio_energy=None, ds_prev_pred=None,
               extra_terms: bool = True, **weights):
        """Fold one batch in.  ``pred`` / ``target``: device tensors, any leading shape over 52 columns.  ``prev_pred`` /
        ``prev_target`` (same shape) switch the temporal and velocity terms on, ``landmark_w`` (136, 52) the landmark term,
        ``ds_prev_pred`` DualStreamLoss's velocity, ``ds_separation_weight`` > 0 its separation term; ``audio_energy`` (rows)
        -- or audio features (rows, D) / (rows, T, D), reduced by ``km_audio_energy`` -- adds the audio-visual part to
        ``perceptual``.  A term whose input is missing reports 0 and does not count in its mean.  ``extra_terms=False``
        evaluates mse and l1 only (the C call with cfg = NULL)."""
        import torch
        from ._lib import KM_ABI_VERSION, KMLossConfig
        self._check_weights(weights)
        w = {**self.weights, **weights}
        pred, target = _rows(pred, target)
        if not bool(getattr(pred, "is_cuda", False)):
            raise ValueError("LossTerms takes device tensors (the float64 restatement for host data is oracle.core.koemorph_loss)")
        n = int(pred.shape[0])
        if n == 0:
            raise ValueError("LossTerms.update needs at least one row")
        self._open(pred.device)
        keep = []

        def dev(t, shape):
            if t is None:
                return None
            t = t.detach().to(self._device, torch.float32).reshape(shape).contiguous()
            keep.append(t)
            return t.data_ptr()

        pred = pred.detach().to(torch.float32).contiguous()
        target = target.detach().to(self._device, torch.float32).contiguous()
        with torch.cuda.device(self._device):
            energy = None
            if audio_energy is not None:
                if audio_energy.dim() == 1:
                    energy = dev(audio_energy, (n,))
                else:
                    af = audio_energy.detach().to(self._device, torch.float32).contiguous()
                    if af.dim() == 2:
                        af = af.unsqueeze(1)
                    if af.dim() != 3 or int(af.shape[0]) != n:
                        raise ValueError(f"audio features must be (rows, D) or (rows, T, D) with {n} rows, got {tuple(af.shape)}")
                    e = torch.empty(n, device=self._device)
                    check(self._lib.km_audio_energy(af.data_ptr(), n, af.shape[1], af.shape[2], e.data_ptr(), self._stream()))
                    keep.append(e)
                    energy = e.data_ptr()
            cfg = None
            if extra_terms:
                cfg = KMLossConfig(KM_ABI_VERSION, w["perceptual_weight"], w["temporal_weight"], w["sparsity_weight"],
                                   w["smoothness_weight"], w["landmark_weight"], w["velocity_weight"], dev(prev_pred, (n, 52)),
                                   dev(prev_target, (n, 52)), dev(landmark_w, (136, 52)), energy, w["ds_velocity_weight"],
                                   w["ds_separation_weight"], dev(ds_prev_pred, (n, 52)))
            terms = torch.empty(KM_LOSS_TERMS, device=self._device)
            check(self._lib.km_loss_terms_update(self._acc, None if cfg is None else C.byref(cfg), w["mse_weight"], w["l1_weight"],
                                                 pred.data_ptr(), target.data_ptr(), n, terms.data_ptr(), self._stream()))
        self.updates += 1
        return terms

    def compute(self) -> Dict[str, float]:
        """Means over the updates since the last reset: one key per ``KM_LOSS_TERM_NAMES`` entry (a term's mean runs over the
        updates that evaluated it; 0.0 if none did), ``updates``, and ``row_smoothness`` = the mean over all rows of
        mean_j |pred[b, j + 1] - pred[b, j]|.  ``{}`` before any update.  One readback."""
        if self.updates == 0:
            return {}
        import torch
        with torch.cuda.device(self._device):
            out = torch.empty(KM_LOSS_TERMS + 2, device=self._device)
            check(self._lib.km_loss_terms_compute(self._acc, out.data_ptr(), self._stream()))
            v = out.cpu().numpy()
        m = {k: float(v[i]) for i, k in enumerate(KM_LOSS_TERM_NAMES)}
        m["updates"] = float(v[KM_LOSS_TERMS])
        m["row_smoothness"] = float(v[KM_LOSS_TERMS + 1])
        return m


def frequency_bands() -> Dict[str, List[int]]:
    """``DualStreamCrossAttention.get_frequency_bands()``: the mel channels of each band."""
    from .model.dual_stream_attention import FREQUENCY_BANDS
    return {band: list(idx) for band, idx in FREQUENCY_BANDS.items()}


def band_reductions(mean_map: np.ndarray, bands: Optional[Dict[str, List[int]]] = None):
    """The two reductions the reference's AttentionVisualizer draws from a (queries, keys) map
    (src/visualization/attention_viz.py): ``band_mean[band]`` = ``map[:, idx].mean(axis=1)`` per query (:96-98) and
    ``band_share[band]`` = ``map[:, idx].mean()`` (:329-331)."""
    bands = frequency_bands() if bands is None else bands
    band_mean = {band: mean_map[:, idx].mean(axis=1) for band, idx in bands.items()}
    band_share = {band: float(mean_map[:, idx].mean()) for band, idx in bands.items()}
    return band_mean, band_share


def unpack_attention_stats(vec: np.ndarray, n_queries: int, n_keys: int) -> Dict[str, object]:
    """km_attn_stats_compute's float64 vector (KM_ATTN_STATS_COUNT(Q, K): rows, mean map, mean entropy, peak counts) as the
    dict ``AttentionStats.compute()`` returns, band reductions included when the maps have the model's 80 keys."""
    q, k = n_queries, n_keys
    vec = np.asarray(vec, np.float64)
    if vec.shape != (km_attn_stats_count(q, k),):
        raise ValueError(f"expected {km_attn_stats_count(q, k)} values for {q} x {k} maps, got {vec.shape}")
    mean_map = vec[1:1 + q * k].reshape(q, k).copy()
    res: Dict[str, object] = {"rows": int(vec[0]), "mean_map": mean_map, "entropy": vec[1 + q * k:1 + q * k + q].copy(),
                              "peak_hist": np.rint(vec[1 + q * k + q:]).astype(np.int64).reshape(q, k)}
    bands = frequency_bands()
    if k > max(max(idx) for idx in bands.values()):
        res["band_mean"], res["band_share"] = band_reductions(mean_map, bands)
    return res


class AttentionStats:
    """What the reference's AttentionVisualizer reduces the mel stream's attention maps to, accumulated on the device
    (``km_attn_stats_*``, koemorph_amd/csrc/km_attn_stats.hip): the mean map, the mean entropy per query, a histogram of each
    query's peak key, and the band reductions of the mean map.  ``update`` takes (..., n_queries, n_keys) device maps;
    ``Engine.sequence_forward(..., stats=acc)`` feeds it tile by tile without the maps ever existing as a whole.  ``update``
    enqueues on the current stream and returns; ``compute`` enqueues the finalisation and does the only readback.
    ``max_rows_per_launch`` = 0 is the library's default; larger updates are cut into pieces inside."""

    def __init__(self, n_queries: int = 28, n_keys: int = 80, max_rows_per_launch: int = 0):
        self.n_queries, self.n_keys, self.max_rows_per_launch = int(n_queries), int(n_keys), int(max_rows_per_launch)
        self._acc = C.c_void_p()
        self._device = None
        self._lib = None
        self.rows = 0
        self._masked = False                                            # a masked update may have folded rows `rows` does not count

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._device).cuda_stream

    def _handle(self, device, n_queries: Optional[int] = None, n_keys: Optional[int] = None):
        """The accumulator on ``device`` (created on first use), after checking that it holds maps of the caller's shape."""
        import torch
        if n_queries is not None and (n_queries, n_keys) != (self.n_queries, self.n_keys):
            raise ValueError(f"AttentionStats holds {self.n_queries} x {self.n_keys} maps, got {n_queries} x {n_keys}")
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._acc and self._device != device:
            if self.rows or self._masked:
                raise ValueError("one accumulation mixes devices; reset() first")
            self.close()
        if not self._acc:
            self._lib = load()
            self._device = device
            with torch.cuda.device(device):
                check(self._lib.km_attn_stats_create(C.byref(self._acc), self.n_queries, self.n_keys, self.max_rows_per_launch))
        return self._acc

    def close(self):
        if self._acc:
            import torch
            torch.cuda.synchronize(self._device)
            self._lib.km_attn_stats_destroy(self._acc)
            self._acc = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.rows = 0
        self._masked = False
        if self._acc:
            import torch
            with torch.cuda.device(self._device):
                check(self._lib.km_attn_stats_reset(self._acc, self._stream()))

    def update(self, maps, mask=None):
        """Fold (..., n_queries, n_keys) float32 device maps in; any leading shape, also empty.  ``mask``: a bool or uint8 device
        tensor with one entry per map -- only the maps whose entry is non-zero are folded, in index order, with the bits a plain
        update of those maps alone would leave (km_attn_stats_update_masked).  How many were selected stays on the device, so
        ``rows`` counts the maps of the unmasked updates only; ``compute()['rows']`` is the number folded."""
        import torch
        if not isinstance(maps, torch.Tensor) or not maps.is_cuda:
            raise ValueError("AttentionStats takes device tensors (the float64 restatement for host data is tests/attn_stats_cases.py)")
        if maps.dim() < 2 or tuple(maps.shape[-2:]) != (self.n_queries, self.n_keys):
            raise ValueError(f"expected (..., {self.n_queries}, {self.n_keys}) maps, got {tuple(maps.shape)}")
        maps = maps.detach().to(torch.float32).contiguous()
        n = int(maps.numel() // (self.n_queries * self.n_keys))
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.device != maps.device or mask.dtype not in (torch.bool, torch.uint8) or mask.numel() != n:
                raise ValueError(f"expected a bool or uint8 mask of {n} entries on the maps' device")
            mask = mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.contiguous()
        acc = self._handle(maps.device)
        with torch.cuda.device(self._device):
            if mask is None:
                check(self._lib.km_attn_stats_update(acc, maps.data_ptr() if n else None, n, self._stream()))
            else:
                check(self._lib.km_attn_stats_update_masked(acc, maps.data_ptr() if n else None, mask.data_ptr() if n else None, n,
                                                            self._stream()))
                self._masked = True
                return
        self.rows += n

    def compute(self) -> Dict[str, object]:
        """'rows', 'mean_map' (Q, K) float64, 'entropy' (Q,), 'peak_hist' (Q, K) int64, 'band_mean' {band: (Q,)} and 'band_share'
        {band: float} over every map since the last reset; all zero before any.  One readback."""
        import torch
        n = km_attn_stats_count(self.n_queries, self.n_keys)
        if not self._acc:
            return unpack_attention_stats(np.zeros(n), self.n_queries, self.n_keys)
        with torch.cuda.device(self._device):
            out = torch.empty(n, device=self._device, dtype=torch.float64)
            check(self._lib.km_attn_stats_compute(self._acc, out.data_ptr(), self._stream()))
            vec = out.cpu().numpy()
        return unpack_attention_stats(vec, self.n_queries, self.n_keys)


class StreamAttentionStats:
    """One ``AttentionStats`` state per stream, on the device (``km_attn_stats_streams_*``): ``update(maps, mask)`` takes the
    (n_streams, n_queries, n_keys) maps of ``StreamEngine.tick`` / ``ChunkedStreamEngine.step`` and the ``ready`` / ``fired`` flags of the
    same call -- stream ``s`` folds its map when ``mask[s]`` is non-zero, with the bits an ``AttentionStats`` of its own fed one map
    at a time would hold.  ``reset(mask)`` makes the masked streams fresh (None: all); ``compute()`` returns one dict per stream."""

    def __init__(self, n_streams: int, n_queries: int = 28, n_keys: int = 80):
        self.n_streams, self.n_queries, self.n_keys = int(n_streams), int(n_queries), int(n_keys)
        self._acc = C.c_void_p()
        self._device = None
        self._lib = None

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._device).cuda_stream

    def _handle(self, device):
        import torch
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._acc and self._device != device:
            raise ValueError("the per-stream states live on another device")
        if not self._acc:
            self._lib = load()
            self._device = device
            with torch.cuda.device(device):
                check(self._lib.km_attn_stats_streams_create(C.byref(self._acc), self.n_streams, self.n_queries, self.n_keys))
        return self._acc

    def close(self):
        if self._acc:
            import torch
            torch.cuda.synchronize(self._device)
            self._lib.km_attn_stats_streams_destroy(self._acc)
            self._acc = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mask(self, mask, device):
        import torch
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype not in (torch.bool, torch.uint8) or \
                tuple(mask.shape) != (self.n_streams,):
            raise ValueError(f"expected a ({self.n_streams},) bool or uint8 device mask")
        if device is not None and mask.device != device:
            raise ValueError("the mask lives on another device than the maps")
        return mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.contiguous()

    def update(self, maps, mask):
        import torch
        if not isinstance(maps, torch.Tensor) or not maps.is_cuda:
            raise ValueError("StreamAttentionStats takes device tensors")
        if tuple(maps.shape) != (self.n_streams, self.n_queries, self.n_keys):
            raise ValueError(f"expected ({self.n_streams}, {self.n_queries}, {self.n_keys}) maps, got {tuple(maps.shape)}")
        maps = maps.detach().to(torch.float32).contiguous()
        m8 = self._mask(mask, maps.device)
        acc = self._handle(maps.device)
        with torch.cuda.device(self._device):
            check(self._lib.km_attn_stats_streams_update(acc, maps.data_ptr(), m8.data_ptr(), self._stream()))

    def reset(self, mask=None):
        if not self._acc:
            return
        import torch
        m8 = self._mask(mask, self._device) if mask is not None else None
        with torch.cuda.device(self._device):
            check(self._lib.km_attn_stats_streams_reset(self._acc, m8.data_ptr() if m8 is not None else None, self._stream()))

    def compute(self) -> List[Dict[str, object]]:
        """One ``AttentionStats.compute()`` dict per stream (band reductions included); all zero before any update.  One readback."""
        import torch
        n = km_attn_stats_count(self.n_queries, self.n_keys)
        if not self._acc:
            return [unpack_attention_stats(np.zeros(n), self.n_queries, self.n_keys) for _ in range(self.n_streams)]
        with torch.cuda.device(self._device):
            out = torch.empty(self.n_streams, n, device=self._device, dtype=torch.float64)
            check(self._lib.km_attn_stats_streams_compute(self._acc, out.data_ptr(), self._stream()))
            vec = out.cpu().numpy()
        return [unpack_attention_stats(vec[s], self.n_queries, self.n_keys) for s in range(self.n_streams)]


def compute_lip_sync_metrics(pred_blendshapes, target_blendshapes, audio_features=None) -> Dict[str, float]:
    """``mouth_mae``, ``mouth_correlation`` and, with ``audio_features``, ``audiovisual_sync`` (losses.py:524-583), on a
    fresh accumulator."""
    acc = BlendshapeMetrics()
    try:
        acc.update(pred_blendshapes, target_blendshapes, audio_features)
        m = acc.compute(lip_sync=True)
    finally:
        acc.close()
    return {k: m[k] for k in LIP_SYNC_KEYS if k in m}
