"""Float64 restatement of SimplifiedKoeMorphModel in TRAINING mode (reference src/model/simplified_model.py:44-72, :114-149)
with explicit keep masks at its five dropout sites, KoeMorphLoss through oracle.core.koemorph_loss, gradients from torch CPU
autograd; and the torch containers the reference instantiates, for pinning the restatement (tests/test_legacy_train_host.py)
and for measuring what float32 autograd of those containers is worth (D32, tests/test_gpu_legacy_train.py).

Masks: {"enc1": (B,T,d), "enc2": (B,T,d), "attn": (B,H,52,T), "dec1": (B,52,hidden), "dec2": (B,52,hidden)} keep flags, applied as
x * keep / (1 - p); the attention mask acts on the softmaxed weights, as nn.MultiheadAttention applies its dropout.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from koemorph_amd import synth
from oracle import core

SITES = ("enc1", "enc2", "attn", "dec1", "dec2")
SHAPES = ((1, 1), (3, 37), (2, 257), (4, 301))
LOSS_PLAIN = dict(mse_weight=1.0, l1_weight=0.1)
LOSS_FULL = dict(mse_weight=1.0, l1_weight=0.1, perceptual_weight=0.5, sparsity_weight=0.01, smoothness_weight=0.1)


def loss_kwargs(kw):
    """oracle.core.koemorph_loss arguments: every term the setting does not name is off."""
    full = dict(mse_weight=0.0, l1_weight=0.0, perceptual_weight=0.0, temporal_weight=0.0, sparsity_weight=0.0,
                smoothness_weight=0.0, landmark_weight=0.0, velocity_weight=0.0)
    full.update(kw)
    return full


def mask_shapes(B, T, d=256, H=8, hidden=128, nq=52):
    return {"enc1": (B, T, d), "enc2": (B, T, d), "attn": (B, H, nq, T), "dec1": (B, nq, hidden), "dec2": (B, nq, hidden)}


def draw_masks(seed, B, T, p=0.1):
    rng = np.random.RandomState(seed)
    return {k: rng.random_sample(s) >= p for k, s in mask_shapes(B, T).items()}


def inputs(seed, B, T):
    """(mel (B,T,80) in the front end's range, target (B,52))."""
    return synth.uniform(seed, (B, T, 80), 0.0, 1.0), synth.uniform(seed + 1, (B, 52), 0.0, 1.0)


def forward(P, mel, masks=None, p=0.0, num_heads=8):
    """P: dict of torch tensors; mel: tensor (B,T,80) of P's dtype -> out (B,52)."""
    sc = 1.0 / (1.0 - p)
    def drop(x, site):
        if masks is None or p == 0.0:
            return x
        return x * torch.as_tensor(np.asarray(masks[site])).to(x.dtype) * sc
    e = drop(torch.relu(F.linear(mel, P["audio_encoder.0.weight"], P["audio_encoder.0.bias"])), "enc1")
    e = drop(torch.relu(F.linear(e, P["audio_encoder.3.weight"], P["audio_encoder.3.bias"])), "enc2")
    d = e.shape[-1]
    B, T = e.shape[0], e.shape[1]
    hd = d // num_heads
    W, bi = P["attention.in_proj_weight"], P["attention.in_proj_bias"]
    q = F.linear(P["blendshape_queries"], W[:d], bi[:d])                             # (52, d): the same for every window
    k = F.linear(e, W[d:2 * d], bi[d:2 * d])
    v = F.linear(e, W[2 * d:], bi[2 * d:])
    qh = q.view(-1, num_heads, hd).permute(1, 0, 2)                                  # (H, 52, hd)
    kh = k.view(B, T, num_heads, hd).permute(0, 2, 1, 3)                             # (B, H, T, hd)
    vh = v.view(B, T, num_heads, hd).permute(0, 2, 1, 3)
    s = torch.matmul(qh.unsqueeze(0), kh.transpose(-1, -2)) / float(np.sqrt(hd))     # (B, H, 52, T)
    a = drop(torch.softmax(s, dim=-1), "attn")
    o = torch.matmul(a, vh).permute(0, 2, 1, 3).reshape(B, -1, d)                    # (B, 52, d)
    o = F.linear(o, P["attention.out_proj.weight"], P["attention.out_proj.bias"])
    h = drop(torch.relu(F.linear(o, P["decoder.0.weight"], P["decoder.0.bias"])), "dec1")
    h = drop(torch.relu(F.linear(h, P["decoder.3.weight"], P["decoder.3.bias"])), "dec2")
    y = torch.sigmoid(F.linear(h, P["decoder.6.weight"], P["decoder.6.bias"]))       # (B, 52, 52)
    return y.mean(dim=1)


def loss_and_grads(params, mel, target, loss_kw, p=0.0, masks=None, dtype=torch.float64):
    """(loss, out (B,52), {key: gradient}) of the restatement."""
    P = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True) for k, v in params.items()}
    out = forward(P, torch.as_tensor(mel).to(dtype), masks, p)
    loss = core.koemorph_loss(out, torch.as_tensor(target).to(dtype), **loss_kwargs(loss_kw))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in P.items()}
    return float(loss.detach()), out.detach().numpy(), grads


class Containers(nn.Module):
    """The containers SimplifiedKoeMorphModel.__init__ builds (simplified_model.py:44-76), state-dict keys included."""

    def __init__(self, params, dtype=torch.float64, d_model=256, num_heads=8, hidden=128, nb=52):
        super().__init__()
        self.audio_encoder = nn.Sequential(nn.Linear(80, d_model), nn.ReLU(), nn.Dropout(0.1),
                                           nn.Linear(d_model, d_model), nn.ReLU(), nn.Dropout(0.1))
        self.attention = nn.MultiheadAttention(embed_dim=d_model, num_heads=num_heads, dropout=0.1, batch_first=True)
        self.decoder = nn.Sequential(nn.Linear(d_model, hidden), nn.ReLU(), nn.Dropout(0.1),
                                     nn.Linear(hidden, hidden), nn.ReLU(), nn.Dropout(0.1),
                                     nn.Linear(hidden, nb), nn.Sigmoid())
        self.blendshape_queries = nn.Parameter(torch.zeros(nb, d_model))
        self.to(dtype)
        self.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in params.items()})

    def forward(self, mel, need_weights=False):
        """forward() of the reference behind extract_mel_features (:129-147); with need_weights also the per-head weights."""
        e = self.audio_encoder(mel)
        q = self.blendshape_queries.unsqueeze(0).repeat(mel.shape[0], 1, 1)
        a, w = self.attention(query=q, key=e, value=e, need_weights=need_weights, average_attn_weights=False)
        return self.decoder(a).mean(dim=1), w


def containers_loss_and_grads(params, mel, target, loss_kw, dtype=torch.float32):
    """Eval-mode autograd of the torch containers in `dtype`: (loss, out, grads)."""
    m = Containers(params, dtype).eval()
    out, _ = m(torch.as_tensor(mel).to(dtype))
    loss = core.koemorph_loss(out, torch.as_tensor(target).to(dtype), **loss_kwargs(loss_kw))
    loss.backward()
    grads = {k: v.grad.detach().numpy().astype(np.float64) for k, v in m.named_parameters()}
    return float(loss.detach()), out.detach().numpy().astype(np.float64), grads


def tier_a_bounds(ref_grads, split_keys=()):
    """{key: (atol, rtol)}: 1e-9 + 1e-5 max|ref|; gradients reduced over split-K partials 1e-7 + 2e-4 max|ref| with rtol 2e-4."""
    return {k: ((1e-7 + 2e-4 * np.abs(r).max(), 2e-4) if k in split_keys else (1e-9 + 1e-5 * np.abs(r).max(), 0.0))
            for k, r in ref_grads.items()}


# gradients the step reduces over split-K partials once a product runs over more than 256 rows: the B T rows of the encoder and of
# the key / value projections reach that at the two larger shapes, the B 52 rows of out_proj and the decoder from B = 5 on
SPLIT_KEYS = ("audio_encoder.0.weight", "audio_encoder.0.bias", "audio_encoder.3.weight", "audio_encoder.3.bias",
              "attention.in_proj_weight", "attention.in_proj_bias")
SPLIT_KEYS_TAIL = ("attention.out_proj.weight", "attention.out_proj.bias", "decoder.0.weight", "decoder.0.bias",
                   "decoder.3.weight", "decoder.3.bias", "decoder.6.weight", "decoder.6.bias")


def split_keys_for(B, T):
    return (SPLIT_KEYS if B * T > 256 else ()) + (SPLIT_KEYS_TAIL if B * 52 > 256 else ())
