"""Shared by tests/test_koemorph_rollout_host.py and tests/test_gpu_koemorph_rollout.py: the window law of
km_koemorph_rollout, a restatement of its plan, seeded models and rows, and the two loops a rollout is pinned to --
``KoeMorphModel.forward`` per frame (the launches the call replaces) and the float64-backed oracle per frame."""
import ctypes as C

import numpy as np

from koemorph_amd import _lib, synth
from oracle import koemorph_model as okm

NB = 52
FUSED_TMAX = 32
DEFAULT_CHUNK = 256
SMALL = dict(d_model=64, num_heads=4, num_encoder_layers=1, num_attention_layers=1, decoder_hidden_dim=32, decoder_layers=1,
             emotion_dim=24)


def window_law(F, T, first):
    """[(start row, T_i)] of frames first .. F - 1: the last min(i + 1, T) rows up to and including row i."""
    return [(i - min(i + 1, T) + 1, min(i + 1, T)) for i in range(first, F)]


def window_brute(F, T, first):
    """The same by walking rows: frame i sees every row j <= i that is fewer than T rows back."""
    out = []
    for i in range(first, F):
        rows = [j for j in range(F) if j <= i and i - j < T]
        out.append((rows[0], len(rows)))
    return out


def up4(n):
    return (n + 3) // 4 * 4


def fused_width(cfg: okm.KoeMorphConfig):
    return (cfg.d_model == 256 and cfg.num_heads == 8 and cfg.num_blendshapes == 52 and cfg.decoder_hidden_dim == 128 and
            cfg.mel_dim % 16 == 0 and cfg.emotion_dim % 16 == 0 and 0 < cfg.mel_dim <= 256 and 0 < cfg.emotion_dim <= 256 and
            cfg.num_attention_layers >= 1)


def chain_launches(cfg, prev=True):
    """Launches of one forward on the launch-per-step chain: per stream the input product and LayerNorm + 9 per encoder layer,
    the average, the conditioning net (2), the query rows, K / V of all layers, 6 per cross-attention layer, the decoder's input
    product + 3 per hidden layer, the tail."""
    return (2 * (2 + 9 * cfg.num_encoder_layers) + 1 + (2 if prev else 0) + 1 + (1 if cfg.num_attention_layers > 0 else 0) +
            6 * cfg.num_attention_layers + 1 + 3 * cfg.decoder_layers + 1)


def expected_plan(cfg, B, F, T, first, chunk=DEFAULT_CHUNK, no_fuse=False):
    fused = lambda t: fused_width(cfg) and not no_fuse and 1 <= t <= FUSED_TMAX
    route = 1 if fused(T) else 0
    law = window_law(F, T, first)
    short = sum(1 for _, ti in law if ti < T)
    full = len(law) - short
    if route == 1:
        chunks = -(-full // chunk)
        W = B * max(min(full, chunk), 1)
        ws = up4(W * T * cfg.mel_dim) + up4(W * T * cfg.emotion_dim) + 2 * W * T * 256 + 3 * up4(B * NB)
        launches = 4 * short + 3 * chunks
    else:
        chunks = 0
        Tm = min(T, F)
        ws = up4(B * Tm * cfg.mel_dim) + up4(B * Tm * cfg.emotion_dim) + 3 * up4(B * NB)
        launches = sum(2 + (2 if fused(ti) else chain_launches(cfg)) for _, ti in law)
    return {"route": route, "chunks": chunks, "short_frames": short, "launches": launches, "workspace_floats": ws}


def torch_model(cfg: okm.KoeMorphConfig, params=None):
    """KoeMorphModel of this configuration on the CPU (tests/test_gpu_koemorph.py's ``build`` without the move)."""
    import torch
    from koemorph_amd.model import KoeMorphModel
    m = KoeMorphModel(mel_dim=cfg.mel_dim, emotion_dim=cfg.emotion_dim, d_model=cfg.d_model, d_query=cfg.d_model,
                      num_heads=cfg.num_heads, num_encoder_layers=cfg.num_encoder_layers,
                      num_attention_layers=cfg.num_attention_layers, decoder_hidden_dim=cfg.decoder_hidden_dim,
                      decoder_layers=cfg.decoder_layers, decoder_activation=cfg.decoder_activation,
                      output_activation=cfg.output_activation, smoothing_method=cfg.smoothing_method,
                      use_temporal_smoothing=cfg.use_temporal_smoothing, use_constraints=cfg.use_constraints, causal=cfg.causal,
                      window_size=cfg.window_size)
    if params is not None:
        sd = m.state_dict()
        sd.update({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        m.load_state_dict(sd, strict=True)
    return m.eval()


def build(cfg, params):
    return torch_model(cfg, params).cuda().eval()


class HostHandle:
    """A km_koemorph handle finalized on the host only: enough for km_koemorph_rollout_plan and the argument refusals."""

    def __init__(self, cfg: okm.KoeMorphConfig):
        self.lib = _lib.load()
        m = torch_model(cfg)
        self.h = C.c_void_p()
        c = m._c_config()
        _lib.check(self.lib.km_koemorph_create(C.byref(c), C.byref(self.h)))
        for k, v in m.named_parameters():
            a = np.ascontiguousarray(v.detach().numpy(), dtype=np.float32)
            shape = (C.c_int64 * max(1, v.dim()))(*v.shape)
            _lib.check(self.lib.km_load_param(self.h, k.encode(), a.ctypes.data_as(C.c_void_p), shape, v.dim()))
        _lib.check(self.lib.km_finalize_host(self.h))

    def plan(self, B, F, T, first):
        out = (C.c_int64 * 5)()
        _lib.check(self.lib.km_koemorph_rollout_plan(self.h, B, F, T, first, out))
        return dict(zip(("route", "chunks", "short_frames", "launches", "workspace_floats"), (int(v) for v in out)))

    def set_option(self, name, value):
        _lib.check(self.lib.km_set_option(self.h, name.encode(), value))

    def close(self):
        if self.h:
            self.lib.km_destroy(self.h)
            self.h = None


def rows(seed, B, F, cfg):
    """Seeded per-frame rows (B, F, mel_dim), (B, F, emotion_dim)."""
    return synth.normal(seed, (B, F, cfg.mel_dim)), synth.normal(seed + 1, (B, F, cfg.emotion_dim))


def forward_loop(m, mel, emo, T, first=0, prev0=None, apply_smoothing=True, apply_constraints=True):
    """The loop a rollout replaces: one ``forward`` per frame on the sliced window, the output fed back.  mel / emo: device tensors.
    The model's smoother state is used and left as the loop leaves it."""
    import torch
    outs, raws, prev = [], [], prev0
    with torch.no_grad():
        for start, ti in window_law(mel.shape[1], T, first):
            o = m(mel[:, start:start + ti].contiguous(), emo[:, start:start + ti].contiguous(), prev_blendshapes=prev,
                  apply_smoothing=apply_smoothing, apply_constraints=apply_constraints)
            prev = o["blendshapes"]
            outs.append(prev)
            raws.append(o["raw_blendshapes"])
    return torch.stack(outs, 1), torch.stack(raws, 1)


def oracle_loop(params, cfg, mel, emo, T, first=0, prev0=None, state=None, apply_smoothing=True, apply_constraints=True):
    """The same loop on oracle.koemorph_model.koemorph_forward, carrying prev and smoother_state."""
    outs, raws, prev = [], [], prev0
    for start, ti in window_law(mel.shape[1], T, first):
        o = okm.koemorph_forward(params, cfg, mel[:, start:start + ti], emo[:, start:start + ti], prev_blendshapes=prev,
                                 smoother_state=state, apply_smoothing=apply_smoothing, apply_constraints=apply_constraints)
        prev, state = o["blendshapes"], o["smoother_state"]
        outs.append(np.asarray(prev))
        raws.append(np.asarray(o["raw_blendshapes"]))
    return np.stack(outs, 1), np.stack(raws, 1), state
