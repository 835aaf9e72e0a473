"""Training step of SimplifiedKoeMorphModel on the device (km_legacy_train_*, koemorph_amd.training.LegacyTrainer) against the
float64 restatement of tests/legacy_train_cases.py (pinned to the torch containers in tests/test_legacy_train_host.py).

Bounds: the project's tier A (tests/test_gpu_train_audio.py:96-103): loss 2e-6 max(1, |loss|), out 2e-6, each gradient
1e-9 + 1e-5 max|ref|; gradients reduced over split-K partials (products over more than 256 rows: the encoder and in_proj tensors
at (2,257) and (4,301)) 1e-7 + 2e-4 max|ref| with rtol 2e-4.  D32, the distance between float32 CPU autograd of the torch
containers and the float64 restatement, was measured per tensor at each of the four shapes and both loss settings: at most 0.09
of the tensor's tier-A bound (decoder.3.weight at (1,1), 3.7e-8 against 4.0e-7), so no bound is widened.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import legacy_train_cases as L
from koemorph_amd import _lib, synth
from koemorph_amd.model.simplified_model import SimplifiedKoeMorphModel
from koemorph_amd.training import LegacyTrainer
from oracle import legacy as olegacy
from oracle.legacy import make_legacy_params

pytestmark = pytest.mark.gpu

DEV = "cuda"


def make_model(params, **kw):
    m = SimplifiedKoeMorphModel(**kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def check(tag, got, want, B, T):
    loss, out, grads = got
    la, oa, ga = want
    bounds = L.tier_a_bounds(ga, L.split_keys_for(B, T))
    e_loss, e_out = abs(loss - la), float(np.abs(out - oa).max())
    worst, worst_k = 0.0, None
    lines = []
    for k, r in ga.items():
        a, rt = bounds[k]
        err = np.abs(grads[k].astype(np.float64) - r)
        q = float((err / (a + rt * np.abs(r))).max())
        lines.append((k, float(err.max()), q))
        if q >= worst:
            worst, worst_k = q, k
    print(f"\n[{tag}] loss err {e_loss:.2e} (bound {2e-6 * max(1.0, abs(la)):.1e}), out err {e_out:.2e}, gradients at {worst:.3f} of "
          f"the bound (worst {worst_k})")
    for k, e, q in lines:
        print(f"    {k:32s} err {e:.3e}  {q:.3f} of its bound")
    assert e_loss <= 2e-6 * max(1.0, abs(la)), (tag, loss, la)
    assert e_out <= 2e-6, (tag, e_out)
    for k, e, q in lines:
        assert q <= 1.0, f"{tag}: {k} max err {e:.3e} is {q:.2f} of its bound"


def set_loss(tr, kw):
    tr.mse_weight, tr.l1_weight = kw["mse_weight"], kw["l1_weight"]
    extra = {k: v for k, v in kw.items() if k not in ("mse_weight", "l1_weight")}
    tr.set_loss_terms(**extra)


@pytest.fixture(scope="module")
def params():
    return make_legacy_params(5)


@pytest.fixture(scope="module")
def trainer(params):
    return LegacyTrainer(make_model(params), max_windows=4, max_frames=301, lr=1e-3)


def hip(tr, mel, target):
    loss = float(tr.forward_backward_mel(dev(mel), dev(target)).item())
    return loss, tr.out[:mel.shape[0]].cpu().numpy().copy(), tr.grads()


# ---- 1 ----
@pytest.mark.parametrize("B,T", L.SHAPES)
@pytest.mark.parametrize("loss_kw", [L.LOSS_PLAIN, L.LOSS_FULL], ids=["plain", "full"])
def test_gradients_in_eval_arithmetic(trainer, params, B, T, loss_kw):
    """p = 0 from mel, loss weights 1.0 / 0.1 and with perceptual 0.5, sparsity 0.01, smoothness 0.1 on.  (1,1): one key, the
    gradients of K and of the logits vanish; (3,37): odd batch, T no multiple of 4 or 16; (2,257), (4,301): split-K reductions.
    The observed errors are printed per tensor (run with -s)."""
    trainer.set_dropout(0.0)
    set_loss(trainer, loss_kw)
    mel, target = L.inputs(100 + B, B, T)
    want = L.loss_and_grads(params, mel, target, loss_kw)
    check(f"eval {B}x{T}", hip(trainer, mel, target), want, B, T)
    if T == 1:
        d = 256
        assert np.abs(want[2]["attention.in_proj_weight"][d:2 * d]).max() == 0.0


def test_gradients_with_the_query_rows_split(params):
    """(6, 5): B 52 = 312 query rows, so the out_proj and decoder gradients are sums of two split-K partials (256 + 56 rows, row
    strides 52, 128 and 256) while the B T = 30 frame rows are not split: the path the training script takes at its batch of 16.
    Those eight tensors get the split-K tier, the others 1e-9 + 1e-5 max|ref|."""
    B, T = 6, 5
    tr = LegacyTrainer(make_model(params), max_windows=B, max_frames=8, lr=1e-3)
    set_loss(tr, L.LOSS_FULL)
    assert set(L.split_keys_for(B, T)) == set(L.SPLIT_KEYS_TAIL)
    mel, target = L.inputs(150, B, T)
    check(f"eval {B}x{T}", hip(tr, mel, target), L.loss_and_grads(params, mel, target, L.LOSS_FULL), B, T)


# ---- 2 ----
@pytest.mark.parametrize("B,T", [(3, 37), (2, 257)])
def test_dropout_with_given_masks(trainer, params, B, T):
    masks = L.draw_masks(31 + B, B, T, 0.1)
    trainer.set_dropout(0.1, external_masks=True)
    trainer.set_dropout_masks(masks)
    set_loss(trainer, L.LOSS_FULL)
    mel, target = L.inputs(200 + B, B, T)
    got = hip(trainer, mel, target)
    check(f"given masks {B}x{T}", got, L.loss_and_grads(params, mel, target, L.LOSS_FULL, p=0.1, masks=masks), B, T)


# ---- 3 ----
def test_dropout_with_device_masks(trainer, params):
    B, T = 2, 257
    trainer.set_dropout(0.1, seed=77)
    set_loss(trainer, L.LOSS_PLAIN)
    mel, target = L.inputs(300, B, T)
    step0 = trainer.dropout_step()
    got = hip(trainer, mel, target)
    masks = trainer.dropout_masks()
    check("device masks", got, L.loss_and_grads(params, mel, target, L.LOSS_PLAIN, p=0.1, masks=masks), B, T)
    for k, m in masks.items():
        n = m.size
        assert abs(m.mean() - 0.9) <= 4 * np.sqrt(0.09 / n), (k, m.mean(), n)
    assert trainer.dropout_step() == step0 + 1
    got2 = hip(trainer, mel, target)
    masks2 = trainer.dropout_masks()
    assert any(not np.array_equal(masks[k], masks2[k]) for k in masks) and got2[0] != got[0]
    trainer.set_dropout_step(step0)
    got3 = hip(trainer, mel, target)
    assert got3[0] == got[0] and np.array_equal(got3[1], got[1])
    for k in got[2]:
        assert np.array_equal(got3[2][k], got[2][k]), k


# ---- 4 ----
@pytest.mark.parametrize("Ln", [37 * 533 - 1, 136448])
def test_from_audio_is_mel_batch_then_step_from_mel(trainer, Ln):
    B = 3
    trainer.set_dropout(0.0)
    set_loss(trainer, L.LOSS_PLAIN)
    audio = dev(synth.make_audio(41, B, Ln))
    target = dev(synth.uniform(42, (B, 52), 0, 1))
    la = float(trainer.forward_backward(audio, target).item())
    oa, ga = trainer.out[:B].clone(), trainer.flat_grad.clone()
    mel = trainer.model.extract_mel_features(audio)
    assert mel.shape[1] == 1 + Ln // 533
    lb = float(trainer.forward_backward_mel(mel, target).item())
    assert la == lb and torch.equal(oa, trainer.out[:B]) and torch.equal(ga, trainer.flat_grad)
    assert np.isfinite(la) and float(ga.abs().max()) > 0


# ---- 5 ----
def test_run_to_run_and_graph_replay_are_bit_identical(trainer):
    B, Ln = 3, 37 * 533 - 1
    audio = dev(synth.make_audio(51, B, Ln))
    target = dev(synth.uniform(52, (B, 52), 0, 1))
    set_loss(trainer, L.LOSS_FULL)
    for p in (0.0, 0.1):
        trainer.set_dropout(p, seed=5)
        s0 = trainer.dropout_step()
        l1 = float(trainer.forward_backward(audio, target).item())
        o1, g1 = trainer.out[:B].clone(), trainer.flat_grad.clone()
        trainer.set_dropout_step(s0)
        l2 = float(trainer.forward_backward(audio, target).item())
        assert l1 == l2 and torch.equal(o1, trainer.out[:B]) and torch.equal(g1, trainer.flat_grad)
        trainer.capture(B, Ln)
        trainer.set_dropout_step(s0)
        l3 = float(trainer.replay(audio, target).item())
        assert l1 == l3 and torch.equal(o1, trainer.out[:B]) and torch.equal(g1, trainer.flat_grad), p
    trainer.set_dropout(0.0)


# ---- 6 and 7 ----
def test_optimizer_matches_torch_adamw_then_sync(params):
    B, T = 3, 37
    model = make_model(params)
    tr = LegacyTrainer(model, max_windows=B, max_frames=64, lr=1e-3, weight_decay=1e-2, grad_clip=0.05)
    set_loss(tr, L.LOSS_PLAIN)
    P = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.AdamW(list(P.values()), lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
    for s in range(3):
        mel, target = L.inputs(400 + 7 * s, B, T)
        loss = float(tr.step_mel(dev(mel), dev(target)).item())
        opt.zero_grad()
        ref = L.core.koemorph_loss(L.forward(P, torch.from_numpy(mel).double()), torch.from_numpy(target).double(), **L.loss_kwargs(L.LOSS_PLAIN))
        ref.backward()
        torch.nn.utils.clip_grad_norm_(list(P.values()), 0.05)
        opt.step()
        print(f"\n[adamw step {s}] loss {loss:.8f} ref {float(ref):.8f}")
        assert abs(loss - float(ref)) <= 2e-6 * max(1.0, float(ref))
    got = tr.params()
    for k, v in P.items():
        r = v.detach().numpy()
        err = np.abs(got[k] - r)
        print(f"    {k:32s} param err {err.max():.3e}")
        assert np.all(err <= 2e-6 + 2e-5 * np.abs(r)), k
    # get / set round trip, with values the trainer does not already hold: perturbed moments and parameters are loaded, read
    # back exactly, and then USED: the next step follows a float64 AdamW that starts from the loaded state (updates of about
    # lr = 1e-3 per element, decided by the loaded moments, against a bound of 2e-6 + 2e-5 |ref|)
    st = tr.optimizer_state()
    assert int(st["steps"][0]) == 3 and st["step_count"] == 3
    rng = np.random.RandomState(9)
    st["exp_avg"] = {k: torch.from_numpy(rng.uniform(-1e-2, 1e-2, v.shape).astype(np.float32)) for k, v in st["exp_avg"].items()}
    st["exp_avg_sq"] = {k: torch.from_numpy(rng.uniform(1e-5, 1e-4, v.shape).astype(np.float32)) for k, v in st["exp_avg_sq"].items()}
    moved = {k: (v + rng.uniform(-1e-3, 1e-3, v.shape)).astype(np.float32) for k, v in got.items()}
    tr.load_optimizer_state(st)
    tr.load_params(moved)
    st2, got2 = tr.optimizer_state(), tr.params()
    for k in moved:
        assert torch.equal(st["exp_avg"][k], st2["exp_avg"][k]) and torch.equal(st["exp_avg_sq"][k], st2["exp_avg_sq"][k]), k
        assert np.array_equal(moved[k], got2[k]) and not np.array_equal(got[k], got2[k]), k
    assert torch.equal(st["steps"], st2["steps"]) and st2["step_count"] == 3
    P = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in moved.items()}
    opt = torch.optim.AdamW(list(P.values()), lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
    for k, v in P.items():
        opt.state[v] = {"step": torch.tensor(3.0), "exp_avg": st["exp_avg"][k].double(), "exp_avg_sq": st["exp_avg_sq"][k].double()}
    mel, target = L.inputs(450, B, T)
    loss = float(tr.step_mel(dev(mel), dev(target)).item())
    ref = L.core.koemorph_loss(L.forward(P, torch.from_numpy(mel).double()), torch.from_numpy(target).double(), **L.loss_kwargs(L.LOSS_PLAIN))
    ref.backward()
    torch.nn.utils.clip_grad_norm_(list(P.values()), 0.05)
    opt.step()
    print(f"\n[adamw step from the loaded state] loss {loss:.8f} ref {float(ref):.8f}")
    assert abs(loss - float(ref)) <= 2e-6 * max(1.0, float(ref))
    got = tr.params()
    for k, v in P.items():
        r = v.detach().numpy()
        err = np.abs(got[k] - r)
        print(f"    {k:32s} param err {err.max():.3e}, moved by {np.abs(r - moved[k]).max():.3e}")
        assert np.all(err <= 2e-6 + 2e-5 * np.abs(r)), k
    # 7: sync
    tr.sync_inference_weights()
    sd = model.state_dict()
    for k in got:
        assert np.array_equal(sd[k].cpu().numpy(), got[k]), k
    audio = synth.make_audio(61, 2, 136448)
    out = model.eval()(dev(audio)).cpu().numpy()
    ref = olegacy.legacy_forward(got, audio)
    assert out.shape == (2, 52) and np.abs(out - ref).max() < 2e-5          # the bound of tests/test_gpu_models.py::test_legacy_simplified_koemorph_model


# ---- 8 ----
def test_refusals(trainer, params):
    lib = _lib.load()
    small = make_model(make_legacy_params(3, d_model=128), d_model=128)
    _, h, _ = small._handle()
    assert lib.km_legacy_train_init(h, 2, 16, None) == _lib.KM_ERR_UNSUPPORTED
    mel, target = dev(np.zeros((5, 4, 80))), dev(np.zeros((5, 52)))
    a = (C.c_float(1.0), C.c_float(0.1), trainer.flat_grad.data_ptr(), trainer.loss.data_ptr(), None, None)
    assert lib.km_legacy_train_step_mel(trainer._h, mel.data_ptr(), 5, 4, target.data_ptr(), *a) == _lib.KM_ERR_WORKSPACE
    mel2 = dev(np.zeros((1, 302, 80)))
    assert lib.km_legacy_train_step_mel(trainer._h, mel2.data_ptr(), 1, 302, target.data_ptr(), *a) == _lib.KM_ERR_WORKSPACE
    assert lib.km_train_adamw(trainer._h, trainer.flat_grad.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, None) == _lib.KM_ERR_INVALID_ARG
    model = trainer.model.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        model(dev(np.zeros((1, 5330))))
    model.eval()
