"""Training step parity: HIP forward/backward gradients against torch.autograd on the REFERENCE
module (golden G7, tests/golden/core_*_grads.npz), and forward + clip + AdamW against torch.optim.AdamW driven by the
oracle's autograd over several steps."""
import numpy as np
import pytest
import torch

from conftest import assert_grads_match, full_loss_inputs, golden_case
from koemorph_amd import synth
from koemorph_amd.engine import Engine
from koemorph_amd.training import Trainer, cosine_warm_restarts_lr
from oracle import core

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make(params, c, **kw):
    e = Engine(d_model=c["d"], num_heads=c["H"], mel_sequence_length=c["T"])
    e.load_state_dict(params)
    e.finalize()
    return e, Trainer(e, max_windows=c["B"], use_smoothing=False, **kw)


@pytest.mark.parametrize("name", ["core_d64_T32_H4_small", "core_d256_T256_H8_grads", "core_d512_T512_H8_grads"])
def test_gradients_match_reference_autograd(name):
    c, params, (mel, short, emo), g = golden_case(name)
    target = synth.uniform(c["seed"] * 3 + 1, (c["B"], 52), 0.0, 1.0)
    e, tr = make(params, c)
    loss = tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
    assert abs(float(loss.item()) - float(g["loss"])) < 1e-6 * max(1.0, abs(float(g["loss"])))
    np.testing.assert_allclose(tr.out[:c["B"]].cpu().numpy(), g["blendshapes"], atol=2e-6)
    grads = tr.grads({k: v.shape for k, v in params.items()})
    for k, v in grads.items():
        if "grad/" + k in g:
            ref = g["grad/" + k]
            np.testing.assert_allclose(v, ref, atol=1e-7 + 2e-4 * np.abs(ref).max(), rtol=2e-4, err_msg=k)
        else:
            ref = g["gradsample/" + k]
            np.testing.assert_allclose(v.ravel()[::97], ref, atol=1e-7 + 2e-4 * np.abs(ref).max(), rtol=2e-4, err_msg=k)
            n = np.sqrt(np.sum(v.astype(np.float64) ** 2))
            assert abs(n - float(g["gradnorm/" + k])) <= 2e-4 * float(g["gradnorm/" + k]) + 1e-9, k


@pytest.mark.parametrize("name", ["core_d64_T32_H4_fullloss", "core_d256_T256_H8_fullloss"])
def test_full_koemorph_loss_gradients_match_reference(name):
    """All eight KoeMorphLoss terms (src/model/losses.py, default weights) in the HIP loss tail: loss value and the
    gradient of every parameter against the reference's own KoeMorphLoss + autograd (golden fixtures)."""
    c, params, (mel, short, emo), g = golden_case(name)
    target, prev_pred, prev_target, lw = full_loss_inputs(c["seed"], c["B"])
    e, tr = make(params, c, mse_weight=1.0, l1_weight=0.1)
    tr.set_loss_terms(perceptual_weight=0.5, temporal_weight=0.2, sparsity_weight=0.01, smoothness_weight=0.1,
                      landmark_weight=0.3, velocity_weight=0.05, prev_pred=dev(prev_pred), prev_target=dev(prev_target),
                      landmark_weights=dev(lw))
    loss = tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
    assert abs(float(loss.item()) - float(g["loss"])) < 2e-6 * max(1.0, abs(float(g["loss"])))
    assert_grads_match(tr.grads({k: v.shape for k, v in params.items()}), g, 2e-4)
    # switching the extra terms off restores the plain mse + l1 loss
    tr.set_loss_terms()
    l2 = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    want = float(g["metric/mse"]) + 0.1 * float(g["metric/l1"])
    assert abs(l2 - want) < 2e-6 * max(1.0, want)


@pytest.mark.parametrize("name", ["core_d64_T32_H4_small", "core_d256_T256_H8_grads"])
def test_dual_stream_loss_terms_match_oracle_autograd(name):
    """DualStreamLoss (src/train_dual_stream.py:434-516: L1 + 0.1 L2 + 0.05 velocity vs prev_predictions + 0.01 stream
    separation) in the HIP loss tail: loss and every parameter gradient against torch.autograd on the oracle's
    restatement.  PARITY UNPINNED: the reference module imports hydra (absent) -- the oracle restates it from the text."""
    from oracle import core as ocore
    c, params, (mel, short, emo), g = golden_case(name)
    target, prev_pred, _, _ = full_loss_inputs(c["seed"], c["B"])
    e, tr = make(params, c, mse_weight=0.1, l1_weight=1.0)
    tr.set_loss_terms(ds_velocity_weight=0.05, ds_separation_weight=0.01, ds_prev_pred=dev(prev_pred))
    loss = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    want, grads, _ = ocore.core_dual_stream_loss_and_grads(params, mel, short, emo, target, prev_pred, num_heads=c["H"],
                                                           mel_sequence_length=c["T"])
    assert abs(loss - want) < 2e-6 * max(1.0, abs(want))
    got = tr.grads({k: v.shape for k, v in params.items()})
    for k, ref in grads.items():
        np.testing.assert_allclose(got[k], ref, atol=1e-7 + 2e-4 * np.abs(ref).max(), rtol=2e-4, err_msg=k)
    # the separation term alone (large weight): its gradient is +-1/(28 B) / -+1/(24 B) per coefficient before the chain rule
    tr.set_loss_terms(ds_separation_weight=5.0)
    l2 = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    w2, g2, _ = ocore.core_dual_stream_loss_and_grads(params, mel, short, emo, target, None, num_heads=c["H"], mel_sequence_length=c["T"],
                                                       weights=dict(velocity_weight=0.0, stream_separation_weight=5.0))
    assert abs(l2 - w2) < 2e-6 * max(1.0, abs(w2))
    got = tr.grads({k: v.shape for k, v in params.items()})
    for k, ref in g2.items():
        np.testing.assert_allclose(got[k], ref, atol=1e-7 + 2e-4 * np.abs(ref).max(), rtol=2e-4, err_msg=k)


def test_training_loop_matches_torch_adamw_with_ema_and_l1():
    """4 optimisation steps, EMA inside the forward (stateful across steps like the reference), MSE + L1, global-norm
    clipping, AdamW: compared with the same loop in torch (autograd on the oracle forward, torch.optim.AdamW)."""
    c = dict(d=64, T=32, H=4, B=5)
    params = synth.make_core_params(71, 64, 32, 256, "trained")
    params_full = dict(params)
    e = Engine(d_model=64, num_heads=4, mel_sequence_length=32)
    e.load_state_dict(params)
    e.load_param("smoothing_alpha", np.float32(0.3))
    e.finalize()
    tr = Trainer(e, max_windows=5, lr=3e-3, weight_decay=1e-2, grad_clip=0.05, mse_weight=1.0, l1_weight=0.1,
                 use_smoothing=True)
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    alpha_p = torch.tensor(0.3, requires_grad=True)
    opt = torch.optim.AdamW(list(P.values()) + [alpha_p], lr=3e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
    prev = None
    for step in range(4):
        mel, short, emo = synth.make_core_inputs(300 + step, 5, 33, style="randn")
        target = synth.uniform(400 + step, (5, 52), 0, 1)
        loss_gpu = tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
        # torch side
        opt.zero_grad()
        x = core.core_forward(P, mel, short, emo, num_heads=4, mel_sequence_length=32)["blendshapes"]
        if prev is None:
            y = x
        else:
            a = torch.sigmoid(alpha_p)
            y = a * x + (1 - a) * prev
        prev = y.detach()
        t = torch.from_numpy(target)
        loss = torch.nn.functional.mse_loss(y, t) + 0.1 * torch.nn.functional.l1_loss(y, t)
        loss.backward()
        assert abs(float(loss_gpu.item()) - float(loss.item())) < 2e-6 * max(1.0, float(loss.item())), step
        if step > 0:
            ga = tr.grads({"smoothing_alpha": ()})["smoothing_alpha"]
            assert abs(float(ga) - float(alpha_p.grad)) < 1e-7 + 2e-4 * abs(float(alpha_p.grad))
        torch.nn.utils.clip_grad_norm_(list(P.values()) + [alpha_p], 0.05)
        opt.step()
        tr.optimizer_step()
    got = tr.params({**{k: v.shape for k, v in params.items()}, "smoothing_alpha": ()})
    for k, v in P.items():
        a, b = got[k], v.detach().numpy()
        if k == "mel_attention.in_proj_bias":
            # the key bias shifts every score of a query row equally, so its gradient is EXACTLY zero in exact
            # arithmetic (softmax shift invariance); both sides hold rounding noise there, which Adam's
            # m / sqrt(v) turns into +-lr-sized steps of random sign.  Compare the q and v thirds tightly and
            # bound the k third by the total step budget.
            np.testing.assert_allclose(a[:64], b[:64], atol=2e-6, rtol=2e-5, err_msg=k + "[q]")
            np.testing.assert_allclose(a[128:], b[128:], atol=2e-6, rtol=2e-5, err_msg=k + "[v]")
            assert np.abs(a[64:128] - b[64:128]).max() <= 2 * 4 * 3e-3
            continue
        # Adam divides by sqrt(v): elements whose gradient is at rounding-noise level move by lr-sized steps whose
        # sign is noise on BOTH sides, so demand tight agreement on >= 99.9 % of every tensor and bound the rest
        # well below one step (lr = 3e-3)
        bad = np.abs(a - b) > 2e-6 + 2e-5 * np.abs(b)
        assert bad.mean() <= 1e-3, (k, bad.mean())
        assert np.abs(a - b).max() < 1e-4, (k, np.abs(a - b).max())
    assert abs(float(got["smoothing_alpha"]) - float(alpha_p.detach())) < 2e-6
    # the trained weights reach the inference kernels
    tr.sync_inference_weights()
    mel, short, emo = synth.make_core_inputs(999, 3, 33, style="randn")
    want = core.core_forward_np({k: v.detach().numpy() for k, v in P.items()}, mel, short, emo, num_heads=4,
                                mel_sequence_length=32)["blendshapes"]
    inf = e.core_forward(dev(mel), dev(short), dev(emo))["blendshapes"].cpu().numpy()
    assert np.abs(inf - want).max() < 5e-6


def test_train_step_from_audio_and_schedule():
    """BASELINE config 3 shape on one rank: 8 windows of 136448 samples, window 256, d_model 256.  The first step's loss (the EMA
    starts there, so the output is the forward's) against the float64 oracle fed by the numpy front end (oracle.mel): 1e-4
    relative."""
    from oracle import mel as omel
    params = synth.make_core_params(72, style="init")
    e = Engine()
    e.load_state_dict(params)
    e.finalize()
    tr = Trainer(e, max_windows=8)
    audio_np, emo_np, target_np = synth.make_audio(73, 8, 136448), synth.normal(74, (8, 256)), synth.uniform(75, (8, 52), 0, 1)
    audio, emo, target = dev(audio_np), dev(emo_np), dev(target_np)
    losses = [float(tr.step(audio, emo, target).item()) for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]           # it learns the (fixed) batch
    long, short = omel.mel_batch(audio_np)
    want = core.core_loss_and_grads(params, long, short, emo_np, target_np, dtype=torch.float64)[0]
    assert abs(losses[0] - want) <= 1e-4 * abs(want), (losses[0], want)
    assert tr.n_params >= 837738 and tr.step_count == 6
    # CosineAnnealingWarmRestarts(T_0=10, T_mult=2, eta_min=1e-6) against torch
    p = torch.nn.Parameter(torch.zeros(1))
    o = torch.optim.AdamW([p], lr=1e-4)
    s = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(o, T_0=10, T_mult=2, eta_min=1e-6)
    for ep in range(1, 35):
        o.step(); s.step()
        assert abs(cosine_warm_restarts_lr(ep, 1e-4) - o.param_groups[0]["lr"]) < 1e-12


def test_graph_replay_of_the_train_step_matches_eager():
    params = synth.make_core_params(76, style="init")
    def run(use_graph):
        e = Engine()
        e.load_state_dict(params)
        e.finalize()
        tr = Trainer(e, max_windows=4, lr=1e-3)
        losses = []
        for i in range(5):
            audio = dev(synth.make_audio(200 + i, 4, 20000))
            emo = dev(synth.normal(210 + i, (4, 256)))
            target = dev(synth.uniform(220 + i, (4, 52), 0, 1))
            if use_graph and i == 1:
                tr.capture(4, 20000)
            if use_graph and i >= 1:
                losses.append(float(tr.step_graph(audio, emo, target).item()))
            else:
                losses.append(float(tr.step(audio, emo, target).item()))
        return losses, tr.params({k: v.shape for k, v in params.items()})
    l0, p0 = run(False)
    l1, p1 = run(True)
    assert l0 == l1
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k


# ---- training step (km_trainp.hip) against the float64 oracle; dropout; the audio-visual term -----------------------------
def test_training_step_is_reproducible_and_agrees_with_the_float64_oracle():
    """The step run twice gives the same bits (no atomics), and its loss (mse + 0.1 l1), output and every gradient agree
    with torch.autograd in FLOAT64 on the oracle's restated forward (oracle.core.core_full_loss_and_grads with the
    extra KoeMorphLoss terms weighted zero), on the same parameters, inputs and weights.  The bounds are those this test
    held against a second fp32 implementation (the launch-per-op chain, since removed): loss 1e-6 max(1, |loss|), output
    1e-6, gradients atol 1e-8 + 2e-5 max|ref| with rtol 2e-4.
    The test prints what it observes (pytest -s).  For scale: torch's own fp32 autograd on the oracle differs from the float64
    result by 2.5e-8 (loss), 5.7e-8 (output) and 2.1e-6 of a tensor's largest entry (gradients) on this fixture."""
    c, params, (mel, short, emo), g = golden_case("core_d256_T256_H8_grads")
    target = synth.uniform(c["seed"] * 3 + 1, (c["B"], 52), 0.0, 1.0)
    _, prev_pred, prev_target, lw = full_loss_inputs(c["seed"], c["B"])           # placeholders: their terms are weighted zero
    shapes = {k: v.shape for k, v in params.items()}
    e, tr = make(params, c, l1_weight=0.1)
    l_ph = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    g_ph, out_ph = tr.grads(shapes), tr.out[:c["B"]].cpu().numpy()
    again = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    assert again == l_ph and all(np.array_equal(v, tr.grads(shapes)[k]) for k, v in g_ph.items())     # no atomics: bit-reproducible
    only_mse_l1 = dict(mse_weight=1.0, l1_weight=0.1, perceptual_weight=0.0, temporal_weight=0.0, sparsity_weight=0.0,
                       smoothness_weight=0.0, landmark_weight=0.0, velocity_weight=0.0)
    l_64, g_64, out_64 = core.core_full_loss_and_grads(params, mel, short, emo, target, prev_pred, prev_target, lw, weights=only_mse_l1,
                                                       num_heads=c["H"], mel_sequence_length=c["T"], dtype=torch.float64)
    worst = max(float(np.abs(g_ph[k] - g_64[k]).max()) / max(float(np.abs(g_64[k]).max()), 1e-300) for k in g_ph)
    print(f"loss {l_ph!r} vs float64 {l_64!r} (|diff| {abs(l_ph - l_64):.3e}); output max |diff| {np.abs(out_ph - out_64).max():.3e}; "
          f"gradients: worst max |diff| / max |ref| over the tensors {worst:.3e}")
    assert abs(l_ph - l_64) < 1e-6 * max(1.0, abs(l_64)) and float(np.abs(out_ph - out_64).max()) < 1e-6
    for k in g_ph:
        np.testing.assert_allclose(g_ph[k], g_64[k], atol=1e-8 + 2e-5 * np.abs(g_64[k]).max(), rtol=2e-4, err_msg=k)


@pytest.mark.parametrize("variant,T,ED,seed", [("fast", 128, 256, 91), ("basic", 256, 9, 93)])
def test_training_step_at_the_d128_variants_agrees_with_the_float64_oracle(variant, T, ED, seed):
    """The reference's d_model 128 / 4-head variants (configs/model/dual_stream.yaml: `fast`, window 128; `basic`, window 256 and
    emotion_dim 9) in training: forward_backward_mel with B = 3 and mse + 0.1 l1 against torch.autograd in FLOAT64 on the oracle
    (core_full_loss_and_grads, the other KoeMorphLoss terms weighted zero), under the bounds of
    test_training_step_is_reproducible_and_agrees_with_the_float64_oracle, unchanged: loss 1e-6 max(1, |loss|), output 1e-6,
    gradients atol 1e-8 + 2e-5 max|ref| with rtol 2e-4.  Run twice: the same bits.  Prints what it observes (pytest -s); on the
    MI355X: `fast` loss 9.5e-9, output 9.7e-8, gradients 3.1e-6 of a tensor's largest entry; `basic` 1.0e-9, 2.8e-8, 1.2e-6."""
    d, H, B = 128, 4, 3
    params = synth.make_core_params(seed, d, T, ED, "trained")
    mel, short, emo = synth.make_core_inputs(seed + 1, B, T + 1, emotion_dim=ED)
    target, prev_pred, prev_target, lw = full_loss_inputs(seed, B)                 # all but the target: placeholders, weighted zero
    shapes = {k: v.shape for k, v in params.items()}
    e = Engine(d_model=d, num_heads=H, mel_sequence_length=T, emotion_dim=ED)
    e.load_state_dict(params)
    e.finalize()
    tr = Trainer(e, max_windows=B, use_smoothing=False, l1_weight=0.1)
    l_ph = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    g_ph, out_ph = tr.grads(shapes), tr.out[:B].cpu().numpy()
    again = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    assert again == l_ph and all(np.array_equal(v, tr.grads(shapes)[k]) for k, v in g_ph.items())     # no atomics: bit-reproducible
    only_mse_l1 = dict(mse_weight=1.0, l1_weight=0.1, perceptual_weight=0.0, temporal_weight=0.0, sparsity_weight=0.0,
                       smoothness_weight=0.0, landmark_weight=0.0, velocity_weight=0.0)
    l_64, g_64, out_64 = core.core_full_loss_and_grads(params, mel, short, emo, target, prev_pred, prev_target, lw, weights=only_mse_l1,
                                                       num_heads=H, mel_sequence_length=T, dtype=torch.float64)
    assert sorted(g_ph) == sorted(g_64)
    worst = max(float(np.abs(g_ph[k] - g_64[k]).max()) / max(float(np.abs(g_64[k]).max()), 1e-300) for k in g_ph)
    print(f"{variant}: loss {l_ph!r} vs float64 {l_64!r} (|diff| {abs(l_ph - l_64):.3e}); output max |diff| {np.abs(out_ph - out_64).max():.3e}; "
          f"gradients: worst max |diff| / max |ref| over the tensors {worst:.3e}")
    assert abs(l_ph - l_64) < 1e-6 * max(1.0, abs(l_64)) and float(np.abs(out_ph - out_64).max()) < 1e-6
    for k in g_ph:
        np.testing.assert_allclose(g_ph[k], g_64[k], atol=1e-8 + 2e-5 * np.abs(g_64[k]).max(), rtol=2e-4, err_msg=k)
    e.close()


@pytest.mark.parametrize("name", ["core_d64_T32_H4_train", "core_d256_T256_H8_train", "core_d512_T512_H8_train"])
def test_training_mode_dropout_gradients_match_reference(name):
    """model.train() with dropout 0.1: the step replays the three dropout masks of the fixture (drawn by torch in the
    reference run) and must reproduce the reference's training-mode output, loss and autograd gradients."""
    from conftest import golden_masks
    c, params, (mel, short, emo), g = golden_case(name)
    masks, p = golden_masks(g), float(g["dropout_p"])
    target = synth.uniform(c["seed"] * 3 + 1, (c["B"], 52), 0.0, 1.0)
    e, tr = make(params, c)
    tr.set_dropout(p, external_masks=True)
    tr.set_dropout_masks(masks)
    loss = tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
    np.testing.assert_allclose(tr.out[:c["B"]].cpu().numpy(), g["train_blendshapes"], atol=2e-6)
    assert abs(float(loss.item()) - float(g["loss"])) < 2e-6 * max(1.0, abs(float(g["loss"])))
    assert_grads_match(tr.grads({k: v.shape for k, v in params.items()}), g, 2e-4)
    back = tr.dropout_masks(c["B"])
    assert all(np.array_equal(back[k], masks[k]) for k in masks)


def test_philox_dropout_masks_and_oracle_parity():
    """Masks drawn on the device: keep rate 1 - p, fresh every step, reproducible for a seed; and the step that used
    them matches the oracle fed with the exported masks (gradients <= 1e-5 relative to the largest entry)."""
    c, params, (mel, short, emo), g = golden_case("core_d256_T256_H8_grads")
    target = synth.uniform(c["seed"] * 3 + 1, (c["B"], 52), 0.0, 1.0)
    shapes = {k: v.shape for k, v in params.items()}
    e, tr = make(params, c, dropout=0.1, seed=1234)
    loss = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    m1 = tr.dropout_masks(c["B"])
    grads = tr.grads(shapes)
    for k, tol in (("mel", 0.004), ("dec", 0.01), ("emo", 0.03)):
        assert abs(m1[k].mean() - 0.9) < tol, (k, m1[k].mean())
    want_loss, want_grads, want_out = core.core_loss_and_grads(params, mel, short, emo, target, num_heads=c["H"],
                                                               mel_sequence_length=c["T"], dropout_p=0.1, drop_masks=m1)
    assert abs(loss - want_loss) < 2e-6 * max(1.0, abs(want_loss))
    np.testing.assert_allclose(tr.out[:c["B"]].cpu().numpy(), want_out, atol=2e-6)
    for k in grads:
        scale = max(float(np.abs(want_grads[k]).max()), 1e-12)
        assert float(np.abs(grads[k] - want_grads[k]).max()) <= 1e-5 * scale + 1e-9, k
    tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
    m2 = tr.dropout_masks(c["B"])
    assert (m1["mel"] != m2["mel"]).mean() > 0.1                       # the next step draws different masks
    e2, tr2 = make(params, c, dropout=0.1, seed=1234)
    tr2.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
    assert all(np.array_equal(tr2.dropout_masks(c["B"])[k], m1[k]) for k in m1)        # same seed, same first step
    e3, tr3 = make(params, c, dropout=0.1, seed=99)
    tr3.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
    assert (tr3.dropout_masks(c["B"])["mel"] != m1["mel"]).mean() > 0.1


@pytest.mark.parametrize("name", ["core_d64_T32_H4_fullloss_av", "core_d256_T256_H8_train_fullloss_av"])
def test_audio_visual_term_and_full_loss_match_reference(name):
    """KoeMorphLoss with audio_features (audio-visual consistency term, losses.py:340-378), with and without dropout."""
    from conftest import golden_masks
    c, params, (mel, short, emo), g = golden_case(name)
    target, prev_pred, prev_target, lw = full_loss_inputs(c["seed"], c["B"])
    af = synth.make_av_features(c["seed"], c["B"])
    e, tr = make(params, c, mse_weight=1.0, l1_weight=0.1)
    if "dropout_p" in g:
        tr.set_dropout(float(g["dropout_p"]), external_masks=True)
        tr.set_dropout_masks(golden_masks(g))
    tr.set_loss_terms(perceptual_weight=0.5, temporal_weight=0.2, sparsity_weight=0.01, smoothness_weight=0.1,
                      landmark_weight=0.3, velocity_weight=0.05, prev_pred=dev(prev_pred), prev_target=dev(prev_target),
                      landmark_weights=dev(lw), audio_features=dev(af))
    loss = tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
    assert abs(float(loss.item()) - float(g["loss"])) < 2e-6 * max(1.0, abs(float(g["loss"])))
    assert_grads_match(tr.grads({k: v.shape for k, v in params.items()}), g, 2e-4)


def test_train_step_from_audio_leaves_clean_window_maxima():
    """The from-audio step converts the front end's power-mel inside phase 0 of the program and re-zeroes the window maxima
    in phase 1 (no memset launch): loss and gradient of a quiet batch must not depend on a loud batch run before it."""
    params = synth.make_core_params(81, style="init")
    loud = dev(synth.make_audio(82, 8, 136448))
    quiet = dev(synth.make_audio(83, 8, 136448) * 1e-3)
    emo = dev(synth.normal(84, (8, 256)))
    target = dev(synth.uniform(85, (8, 52), 0, 1))
    res = []
    for fresh in (False, True):
        e = Engine()
        e.load_state_dict(params)
        e.finalize()
        tr = Trainer(e, max_windows=8, dropout=0.0)
        if not fresh:
            tr.forward_backward(loud, emo, target)           # no optimizer step: the weights stay what they were
            tr.reset_temporal_state()                        # ... and the EMA starts over, as in the fresh trainer
        loss = float(tr.forward_backward(quiet, emo, target).item())
        res.append((loss, tr.flat_grad.clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("B,L", [(8, 136448), (5, 136000), (3, 20000), (2, 1200)])
def test_front_end_packed_input_agrees_with_the_phase_0_conversion(B, L):
    """Round 4: km_train_step_audio's front-end launch writes 10 log10(power) straight into the channel encoder's packed input
    (MelArgs::pack_*), the channel encoder's tile finishes the dB conversion on its operand fragments (DbXform) and the padded
    channel-encoder weight is kept beside the parameters by AdamW (PaddedCopy) -- phase 0 of the program is gone.  Option
    train_no_fe_pack brings the phase-0 conversion back: same power-mel, same operations in the same order, but the compiler
    contracts 10 log10(s) - ref into one fma where both sit in one function -- the two paths differ in the last bit of some
    features (observed: gradients to 3e-7 of their maximum, losses equal).  Also after three optimizer steps (PaddedCopy).
    L = 136000: 256 frames (no 257th); 20000 / 1200: fewer frames than the window -- those take the phase-0 path in both runs."""
    params = synth.make_core_params(31, style="trained")
    shapes = {k: v.shape for k, v in params.items()}
    audio = [dev(synth.make_audio(300 + i, B, L)) for i in range(3)]
    emo = dev(synth.normal(310, (B, 256)))
    target = dev(synth.uniform(311, (B, 52), 0, 1))
    res = []
    for no_pack in (0, 1):
        e = Engine()
        e.load_state_dict(params)
        e.finalize()
        e.set_option("train_no_fe_pack", no_pack)
        tr = Trainer(e, max_windows=8, lr=1e-3, dropout=0.1)
        tr.set_dropout(0.1, seed=5)
        losses = [float(tr.step(a, emo, target).item()) for a in audio]
        loss = float(tr.forward_backward(audio[0], emo, target).item())
        res.append((losses, loss, tr.flat_grad.clone(), tr.params(shapes)))
    np.testing.assert_allclose(res[0][0] + [res[0][1]], res[1][0] + [res[1][1]], rtol=2e-6)
    g0, g1 = res[0][2].cpu().numpy(), res[1][2].cpu().numpy()
    assert np.abs(g0 - g1).max() <= 2e-5 * np.abs(g1).max()
    for k in shapes:          # three AdamW steps at lr 1e-3: a sign-like update, so compare to a fraction of the step
        assert np.abs(res[0][3][k] - res[1][3][k]).max() <= 3e-4, k
    if L < 136000:
        assert torch.equal(res[0][2], res[1][2])


def test_split_k_gradient_products_agree_with_the_unsplit_step():
    """64 windows: the gradient products over all rows of the batch (K = 80 B, 28 B, 24 B > 512) are cut along K into partial
    products summed by the next phase (km_trainp.hip, Program::gemm).  Same gradients as the unsplit program (option
    train_no_split) up to summation order, bit-reproducible from run to run."""
    params = synth.make_core_params(5, style="trained")
    B = 64
    mel, short, emo = synth.make_core_inputs(77, B, 257, style="mel01")
    target = synth.uniform(78, (B, 52), 0.0, 1.0)
    c = dict(d=256, H=8, T=256, B=B)
    e, tr = make(params, c, l1_weight=0.1)
    shapes = {k: v.shape for k, v in params.items()}
    l1 = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    g1 = tr.grads(shapes)
    l1b = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    assert l1b == l1 and all(np.array_equal(v, tr.grads(shapes)[k]) for k, v in g1.items())
    e.set_option("train_no_split", 1)
    l0 = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
    g0 = tr.grads(shapes)
    e.set_option("train_no_split", 0)
    assert abs(l1 - l0) < 1e-6 * max(1.0, abs(l0))
    for k in g0:
        np.testing.assert_allclose(g1[k], g0[k], atol=1e-8 + 2e-5 * np.abs(g0[k]).max(), rtol=2e-4, err_msg=k)
    # and against autograd on the oracle for a sample of the tensors whose products are split
    from oracle import core as ocore
    _, gref, _ = ocore.core_loss_and_grads(params, mel[:B], short[:B], emo[:B], target)
    e2, tr2 = make(params, c)
    tr2.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target))
    g2 = tr2.grads(shapes)
    for k in ("mel_attention.in_proj_weight", "mel_attention.out_proj.weight", "mel_output_proj.weight", "blendshape_decoder.0.weight",
              "blendshape_decoder.3.weight", "mel_channel_encoder.weight", "mel_norm.weight", "mel_attention.in_proj_bias"):
        np.testing.assert_allclose(g2[k], gref[k], atol=1e-8 + 2e-4 * np.abs(gref[k]).max(), rtol=2e-4, err_msg=k)


@pytest.mark.parametrize("B", [8, 5])
def test_lds_dma_tiles_and_attention_blocks_agree_with_the_register_staged_ones(B):
    """Round 4: the products of the program run on the LDS-DMA tile (km_gemm_dma_dev.h), the attention blocks on LDS-DMA staged
    images (km_train_attn_dev.h).  Options train_no_dma / train_attn_regs select the register-staged code of round 3: the same
    step, dropout masks included, must give the same loss and gradients -- the tile is bit-identical per product
    (tools/micro/tile_bench.hip), the epilogue and the softmax (v_exp_f32 / v_rcp_f32) differ in the last bits.  B = 5: K = 80 B is
    not a multiple of 32, so the gradient products over the batch fall back to the register tile inside the SAME program."""
    params = synth.make_core_params(9, style="trained")
    mel, short, emo = synth.make_core_inputs(91, B, 257, style="mel01")
    target = synth.uniform(92, (B, 52), 0.0, 1.0)
    c = dict(d=256, H=8, T=256, B=B)
    e, tr = make(params, c, l1_weight=0.1, dropout=0.1, seed=3)
    shapes = {k: v.shape for k, v in params.items()}
    runs = {}
    for name, opts in (("dma", {}), ("no_dma", {"train_no_dma": 1}), ("attn_regs", {"train_attn_regs": 1}),
                       ("colsum_gemm", {"train_colsum_gemm": 1}),      # column sums as ones-vector products (before OP_COLSUM)
                       ("ln_phase", {"train_no_ln_fuse": 1}),          # a LayerNorm phase instead of LayerNorm in the readers of Y0 / E0
                       ("round3", {"train_no_dma": 1, "train_attn_regs": 1, "train_colsum_gemm": 1})):
        for k in ("train_no_dma", "train_attn_regs", "train_colsum_gemm", "train_no_ln_fuse"):
            e.set_option(k, opts.get(k, 0))
        tr.set_dropout(0.1, seed=3)                      # the same Philox masks in every run
        check_step = tr._lib.km_train_set_dropout_step(tr._h, 0)
        assert check_step == 0
        loss = float(tr.forward_backward_mel(dev(mel), dev(short), dev(emo), dev(target)).item())
        runs[name] = (loss, tr.grads(shapes))
    l0, g0 = runs["round3"]
    for name in ("dma", "no_dma", "attn_regs", "colsum_gemm", "ln_phase"):
        l, g = runs[name]
        assert abs(l - l0) < 2e-6 * max(1.0, abs(l0)), name
        for k in g0:
            np.testing.assert_allclose(g[k], g0[k], atol=1e-8 + 2e-5 * np.abs(g0[k]).max(), rtol=2e-4, err_msg=f"{name}: {k}")


@pytest.mark.parametrize("d,H,T,B", [(64, 4, 64, 3), (256, 8, 128, 5), (512, 8, 96, 2), (128, 4, 256, 4)])
def test_program_variants_agree_from_audio_at_other_shapes(d, H, T, B):
    """The round-4 forms of the training program -- front-end packing + conversion on the fragments, LayerNorm by the reader, dY in two K
    halves, OP_COLSUM, LDS-DMA tiles -- each against the register-tile program of round 3 (train_no_dma, which switches all of them but the
    column sums off), from audio, at shapes none of the goldens has: other widths, windows and odd batch sizes (d_model 128: generic
    LayerNorm rows; 512: sixteen statistic parts per row; window 96 / 128: other packed widths).  Loss after three optimizer steps and the
    gradient of a fourth step."""
    from koemorph_amd.engine import Engine
    params = synth.make_core_params(3, d, T, 256, "trained")
    L = T * 533 + 40
    audio, emo, target = dev(synth.make_audio(5, B, L)), dev(synth.normal(6, (B, 256))), dev(synth.uniform(7, (B, 52), 0, 1))
    res = {}
    for name, opts in (("default", {}), ("no_pack", {"train_no_fe_pack": 1}), ("ln_phase", {"train_no_ln_fuse": 1}), ("dy_whole", {"train_no_dy_split": 1}),
                       ("colsum_gemm", {"train_colsum_gemm": 1}), ("round3", {"train_no_dma": 1})):
        e = Engine(d_model=d, num_heads=H, mel_sequence_length=T)
        e.load_state_dict(params)
        e.finalize()
        for k, v in opts.items():
            e.set_option(k, v)
        tr = Trainer(e, max_windows=B, lr=1e-3, dropout=0.1)
        tr.set_dropout(0.1, seed=5)
        for _ in range(3):
            tr.step(audio, emo, target)
        loss = float(tr.forward_backward(audio, emo, target).item())
        res[name] = (loss, tr.flat_grad.cpu().numpy().copy())
    l0, g0 = res["round3"]
    assert np.isfinite(l0) and np.abs(g0).max() > 0
    for name, (l, g) in res.items():
        assert abs(l - l0) < 2e-5 * max(1.0, abs(l0)), name
        assert np.abs(g - g0).max() <= 2e-4 * np.abs(g0).max(), name

