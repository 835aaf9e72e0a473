"""The float64 restatement of SimplifiedKoeMorphModel in training mode (tests/legacy_train_cases.py) against the torch containers
the reference instantiates (nn.Sequential, nn.MultiheadAttention(dropout=0.1, batch_first=True)), both in float64: in eval mode,
and under .train() with a seeded torch RNG, where the keep masks torch drew are recovered -- the nn.Dropout masks with forward
hooks, the attention mask from the returned post-dropout weights (zeros mark the dropped entries) -- and fed to the restatement.
Output and every gradient agree to float64 rounding.  Guards the yardstick of tests/test_gpu_legacy_train.py."""
import numpy as np
import pytest
import torch

import legacy_train_cases as L
from oracle import core
from oracle.legacy import make_legacy_params


def _compare(got, want, tag):
    (l0, o0, g0), (l1, o1, g1) = got, want
    assert abs(l0 - l1) <= 1e-12 * max(1.0, abs(l1)), (tag, l0, l1)
    assert np.abs(o0 - o1).max() <= 1e-12, tag
    assert sorted(g0) == sorted(g1)
    for k in g1:
        assert np.abs(g0[k] - g1[k]).max() <= 1e-12 * max(1.0, np.abs(g1[k]).max()), (tag, k)


@pytest.mark.parametrize("B,T", [(1, 1), (3, 37)])
@pytest.mark.parametrize("loss_kw", [L.LOSS_PLAIN, L.LOSS_FULL], ids=["plain", "full"])
def test_restatement_matches_containers_in_eval_mode(B, T, loss_kw):
    params = make_legacy_params(7)
    mel, target = L.inputs(11, B, T)
    got = L.loss_and_grads(params, mel, target, loss_kw)
    want = L.containers_loss_and_grads(params, mel, target, loss_kw, dtype=torch.float64)
    _compare(got, want, f"eval {B}x{T}")


@pytest.mark.parametrize("B,T", [(3, 37), (2, 65)])
def test_restatement_matches_containers_in_train_mode_with_recovered_masks(B, T):
    params = make_legacy_params(8)
    mel, target = L.inputs(21, B, T)
    m = L.Containers(params, torch.float64).train()
    masks = {}
    def hook(site):
        def fn(mod, inp, out):
            masks[site] = (out != 0).numpy()          # where the input is 0 (ReLU) either value of the mask gives the same result
        return fn
    hs = [m.audio_encoder[2].register_forward_hook(hook("enc1")), m.audio_encoder[5].register_forward_hook(hook("enc2")),
          m.decoder[2].register_forward_hook(hook("dec1")), m.decoder[5].register_forward_hook(hook("dec2"))]
    torch.manual_seed(1234)
    out, w = m(torch.from_numpy(mel).double(), need_weights=True)
    for h in hs:
        h.remove()
    assert w.shape == (B, 8, 52, T)
    masks["attn"] = (w != 0).detach().numpy()
    for k, s in L.mask_shapes(B, T).items():
        assert masks[k].shape == s
    assert 0.85 < masks["attn"].mean() < 0.95 and 0.3 < masks["enc1"].mean() < 0.95
    loss = core.koemorph_loss(out, torch.from_numpy(target).double(), **L.loss_kwargs(L.LOSS_FULL))
    loss.backward()
    want = (float(loss.detach()), out.detach().numpy(), {k: v.grad.numpy() for k, v in m.named_parameters()})
    got = L.loss_and_grads(params, mel, target, L.LOSS_FULL, p=0.1, masks=masks)
    _compare(got, want, f"train {B}x{T}")
