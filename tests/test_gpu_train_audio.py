"""The from-audio training step (km_train_step_audio: front end + packed rows + phased program, what bench.py's C3 workload
times and SequentialTrainer runs) against the float64 oracle, loss, output and the gradient of every parameter.

Two feature sources give the oracle its input:

* Tier A (tight): ``Engine.mel_batch`` on a separate engine with the same MelConfig -- km_mel_batch, a different code path,
  pinned to ``oracle.mel`` by tests/test_gpu_mel.py.  The oracle gets every frame (257 at the C3 shape) and the short frames
  mel_batch returns, and truncates / pads itself, so this pins the training program's own row layout: T long frames, the last
  3 frames of the WHOLE clip in the short slots, the window maximum over all frames, zeros up to the packed width.
  Bounds of the mel-path tests at the same shape: loss 2e-6 relative, ``out`` 2e-6, gradients 1e-5 of each tensor's largest
  entry (2e-4 with rtol 2e-4 where split-K sums 64 windows).
* Tier B (independent): ``oracle.mel.mel_batch`` -- no HIP at all.  D = what the feature source alone moves the float64
  oracle (per tensor); the step must be within 2 D + the Tier-A bound of the oracle on these features, and ``out`` within
  1e-4 (the contractual figure for the 52 coefficients).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from koemorph_amd import synth
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.training import Trainer
from oracle import core
from oracle import mel as omel

pytestmark = pytest.mark.gpu

C3 = dict(d=256, H=8, T=256)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def engine(params, c, mel_cfg=None):
    e = Engine(d_model=c["d"], num_heads=c["H"], mel_sequence_length=c["T"], mel=mel_cfg)
    e.load_state_dict(params)
    e.finalize()
    return e


def speech(seed, B, L):
    return synth.make_audio(seed, B, L)


def burst(a, b, n=400, amp=1.0):
    """A loud 1 kHz tone in the last n samples of window b: at L = 136448 the window maximum is then in frame 257, the one the
    long rows drop (3.7 dB above any other frame)."""
    t = np.arange(n)
    a[b, -n:] += (amp * np.sin(2 * np.pi * 1000.0 * t / 16000.0)).astype(np.float32)


def hip_features(params, c, audio, mel_cfg=None):
    """Tier A: km_mel_batch (every frame + the 3 short frames) on an engine of its own."""
    long, short = engine(params, c, mel_cfg).mel_batch(dev(audio))
    torch.cuda.synchronize()
    return long.cpu().numpy(), short.cpu().numpy()


def oracle_features(audio, mel_cfg=None):
    """Tier B: the numpy front end (oracle.mel) with the MelConfig's hop and dB constants."""
    m = mel_cfg or MelConfig()
    kw = dict(hop=m.hop_length)
    if (m.top_db, m.db_add, m.db_scale) != (80.0, 80.0, 1.0 / 80.0):
        kw.update(top_db=m.top_db, db_add=m.db_add, db_scale=m.db_scale)
    return omel.mel_batch(audio, **kw)


def oracle_step(params, feats, emo, target, c, l1=0.0, p=0.0, masks=None):
    """float64 autograd on the restated forward: (loss, grads, out).  MSE alone through core_loss_and_grads; MSE + l1 as
    test_training_loop_matches_torch_adamw_with_ema_and_l1 builds it from core_forward."""
    long, short = feats
    kw = dict(num_heads=c["H"], mel_sequence_length=c["T"], dtype=torch.float64, dropout_p=p, drop_masks=masks)
    if l1 == 0.0:
        return core.core_loss_and_grads(params, long, short, emo, target, **kw)
    P = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_(True) for k, v in params.items()}
    y = core.core_forward(P, long, short, emo, **kw)["blendshapes"]
    t = torch.from_numpy(target).double()
    loss = F.mse_loss(y, t) + l1 * F.l1_loss(y, t)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}
    return float(loss.detach()), grads, y.detach().numpy()


def hip_step(params, c, audio, emo, target, mel_cfg=None, l1=0.0, **trkw):
    """One km_train_step_audio at default engine options: (loss, out[:B], grads of every parameter, trainer)."""
    B = audio.shape[0]
    e = engine(params, c, mel_cfg)
    tr = Trainer(e, max_windows=B, use_smoothing=False, l1_weight=l1, **trkw)
    loss = float(tr.forward_backward(dev(audio), dev(emo), dev(target)).item())
    return loss, tr.out[:B].cpu().numpy().copy(), tr.grads({k: v.shape for k, v in params.items()}), tr


def check(tag, got, want_a, want_b=None, split=False):
    """Tier A: loss <= 2e-6 max(1, |loss|), out <= 2e-6, each gradient <= 1e-5 of its largest entry (split: 2e-4 of it with
    rtol 2e-4).  Tier B: within 2 D + those bounds of the oracle on oracle features, D = the distance between the two oracles;
    out within 1e-4 as well.  Prints the observed figures."""
    loss, out, grads = got
    la, ga, oa = want_a
    lbound = 2e-6 * max(1.0, abs(la))
    atol = {k: (1e-7 + 2e-4 * np.abs(r).max()) if split else (1e-9 + 1e-5 * np.abs(r).max()) for k, r in ga.items()}
    rtol = 2e-4 if split else 0.0
    e_loss, e_out = abs(loss - la), float(np.abs(out - oa).max())
    worst, worst_k = 0.0, None
    for k, r in ga.items():
        err = np.abs(grads[k].astype(np.float64) - r)
        q = float((err / (atol[k] + rtol * np.abs(r))).max())
        if q > worst:
            worst, worst_k = q, k
        rel = float(err.max() / max(np.abs(r).max(), 1e-30))
        assert np.all(err <= atol[k] + rtol * np.abs(r)), f"{tag} tier A: {k} max err {err.max():.3e} ({rel:.2e} of its max)"
    print(f"\n[{tag}] tier A: loss {e_loss:.2e} (bound {lbound:.1e}), out {e_out:.2e}, gradients at {worst:.2f} of the bound "
          f"(worst {worst_k}: {float(np.abs(grads[worst_k] - ga[worst_k]).max() / np.abs(ga[worst_k]).max()):.2e} of its max)")
    assert e_loss <= lbound, (tag, "tier A loss", loss, la)
    assert e_out <= 2e-6, (tag, "tier A out", e_out)
    if want_b is None:
        return
    lb, gb, ob = want_b
    d_loss, d_out = abs(lb - la), float(np.abs(ob - oa).max())
    e_loss_b, e_out_b = abs(loss - lb), float(np.abs(out - ob).max())
    worst_b, worst_bk = 0.0, None
    for k, r in gb.items():
        D = float(np.abs(r - ga[k]).max())
        err = np.abs(grads[k].astype(np.float64) - r)
        lim = 2 * D + atol[k] + rtol * np.abs(r)
        q = float((err / lim).max())
        if q > worst_b:
            worst_b, worst_bk = q, k
        assert np.all(err <= lim), f"{tag} tier B: {k} max err {err.max():.3e}, D {D:.3e}"
    print(f"[{tag}] tier B: loss {e_loss_b:.2e} (D {d_loss:.1e}), out {e_out_b:.2e} (D {d_out:.1e}), gradients at {worst_b:.2f} "
          f"of 2 D + bound (worst {worst_bk})")
    assert e_loss_b <= 2 * d_loss + lbound, (tag, "tier B loss", loss, lb, d_loss)
    assert e_out_b <= 2 * d_out + 2e-6 and e_out_b <= 1e-4, (tag, "tier B out", e_out_b, d_out)


def both_tiers(params, c, audio, emo, target, mel_cfg=None, l1=0.0, split=False, tag="", **trkw):
    got = hip_step(params, c, audio, emo, target, mel_cfg, l1, **trkw)
    fa, fb = hip_features(params, c, audio, mel_cfg), oracle_features(audio, mel_cfg)
    masks = got[3].dropout_masks(audio.shape[0]) if trkw.get("dropout", 0.0) > 0 else None
    p = trkw.get("dropout", 0.0)
    want_a = oracle_step(params, fa, emo, target, c, l1, p, masks)
    want_b = oracle_step(params, fb, emo, target, c, l1, p, masks)
    check(tag, got[:3], want_a, want_b, split)
    return got, fa, fb


# ---- 1: the C3 shape, 257 frames: truncation, the short slots, the window maximum, silence, a quiet window --------------
def test_c3_shape_from_audio_matches_oracle_with_edge_windows():
    """B = 8, L = 136448 (257 frames), MSE + 0.1 L1, LayerNorm by the reader (R = 640).  Window 0: a loud burst in the last
    400 samples puts the window maximum into frame 257, which the long rows drop (a maximum over the kept frames alone moves
    that window's features by 3.7 dB / 80); window 1: silence (every power at the amin floor: features exactly 1); window 2:
    x 1e-3 (amin floor in the weak bins); the rest speech.  Short slots must be frames 254-256, the long rows frames 0-255.
    Observed on MI355X: tier A loss 8.7e-9, out 8.8e-8, gradients at 0.33 of the bound (mel_channel_encoder.weight, 3.8e-6 of
    its largest entry); tier B the same (D <= 2e-9)."""
    params = synth.make_core_params(101, style="trained")
    audio = speech(101, 8, 136448)
    burst(audio, 0)
    audio[1] = 0.0
    audio[2] *= 1e-3
    emo, target = synth.normal(102, (8, 256)), synth.uniform(103, (8, 52), 0, 1)
    _, fa, fb = both_tiers(params, C3, audio, emo, target, l1=0.1, tag="c3 edges")
    long_a, short_a = fa
    assert long_a.shape == (8, 257, 80) and np.array_equal(short_a, long_a[:, 254:257])
    assert long_a[0].max(axis=1).argmax() == 256 and long_a[0, :256].max() < 0.99      # the maximum lies in the dropped frame
    assert np.all(long_a[1] == 1.0)
    assert fb[0][0].max(axis=1).argmax() == 256


# ---- 2: dropout ----------------------------------------------------------------------------------------------------------
def test_c3_shape_from_audio_with_philox_dropout_matches_oracle():
    """As the C3 case with dropout 0.1: the step's own Philox masks (tr.dropout_masks) given to the oracle.
    Observed on MI355X: loss 1.2e-9, out 9.9e-8, gradients at 0.17 of the bound (2.5e-6 of the largest entry)."""
    params = synth.make_core_params(111, style="trained")
    audio = speech(111, 8, 136448)
    emo, target = synth.normal(112, (8, 256)), synth.uniform(113, (8, 52), 0, 1)
    got, _, _ = both_tiers(params, C3, audio, emo, target, l1=0.1, tag="c3 dropout", dropout=0.1, seed=4321)
    m = got[3].dropout_masks(8)
    assert abs(m["mel"].mean() - 0.9) < 0.01 and not m["mel"].all()


# ---- 3: exactly 256 frames; odd length, odd batch ------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(5, 136000), (3, 136449)])
def test_from_audio_at_256_frames_and_odd_lengths_matches_oracle(B, L):
    """L = 136000: exactly 256 frames, no truncation, short slots = frames 253-255; L = 136449: 257 frames, every window's audio
    at another alignment.  K = 80 B is not a multiple of 32: the gradient products over the batch fall back to the register tile
    inside the program.  Observed on MI355X: B 5: loss 1.6e-9, out 1.8e-8, gradients at 0.16 of the bound; B 3: loss 2.0e-8,
    out 1.6e-8, gradients at 0.20 of the bound (mel_attention.in_proj_weight, whose largest entry is so small that the 1e-9
    floor of the bound is what binds)."""
    params = synth.make_core_params(121 + B, style="trained")
    audio = speech(121 + B, B, L)
    emo, target = synth.normal(122 + B, (B, 256)), synth.uniform(123 + B, (B, 52), 0, 1)
    _, fa, _ = both_tiers(params, C3, audio, emo, target, tag=f"B{B} L{L}")
    F_ = 1 + L // 533
    assert fa[0].shape == (B, F_, 80) and np.array_equal(fa[1], fa[0][:, F_ - 3:])


# ---- 4: clips shorter than the window ------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [20000, 1100, 533])
def test_short_clips_from_audio_match_oracle(L):
    """38, 3 and 2 frames: the phase-0 conversion (OP_LOGPACK), zero padding of the long rows up to T = 256, and the short rows
    when F <= 3 (oracle.mel.mel_batch_window: the frames there are, then zeros).  Observed on MI355X: loss <= 1.3e-8, out
    <= 4.8e-8, gradients at <= 0.11 of the bound (1.2e-6 of the largest entry)."""
    params = synth.make_core_params(131, style="trained")
    audio = speech(131 + L, 3, L)
    emo, target = synth.normal(132, (3, 256)), synth.uniform(133, (3, 52), 0, 1)
    _, fa, _ = both_tiers(params, C3, audio, emo, target, tag=f"L{L}")
    if L == 533:
        assert fa[0].shape == (3, 2, 80) and np.array_equal(fa[1][:, :2], fa[0]) and not fa[1][:, 2].any()


# ---- 5: 64 windows: LayerNorm phase + split-K ----------------------------------------------------------------------------
def test_64_windows_from_audio_match_oracle():
    """The 64-window C3 config: R = 5120 > 3200 rows takes the LayerNorm phase, the gradient products over the batch are cut
    along K (split-K) -- the golden bound (2e-4 of each tensor's largest entry, rtol 2e-4) for the gradients.  Observed on
    MI355X: loss 4.2e-8, out 3.9e-7, gradients 4.1e-6 of the largest entry at worst (mel_weights)."""
    params = synth.make_core_params(141, style="trained")
    audio = speech(141, 64, 136448)
    burst(audio, 17)
    emo, target = synth.normal(142, (64, 256)), synth.uniform(143, (64, 52), 0, 1)
    both_tiers(params, C3, audio, emo, target, l1=0.1, split=True, tag="64 windows")


# ---- 6: the 60 fps training shape ----------------------------------------------------------------------------------------
def test_d512_60fps_from_audio_matches_oracle():
    """d_model 512, window 512, hop 266 (MelConfig.model_batch(target_fps=60)), 513 frames: sixteen statistic parts per row,
    another packed width.  Observed on MI355X: loss 1.8e-8, out 1.3e-7, gradients at 0.19 of the bound (2.3e-6 of the largest
    entry)."""
    c = dict(d=512, H=8, T=512)
    params = synth.make_core_params(151, 512, 512, 256, "trained")
    audio = speech(151, 4, 136448)
    emo, target = synth.normal(152, (4, 256)), synth.uniform(153, (4, 52), 0, 1)
    cfg = MelConfig.model_batch(target_fps=60)
    assert cfg.hop_length == 266
    _, fa, _ = both_tiers(params, c, audio, emo, target, mel_cfg=cfg, tag="d512 60fps")
    assert fa[0].shape == (4, 513, 80)


# ---- 7: other dB constants -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["db_scale_negative", "top_db_60"])
def test_other_db_constants_from_audio_match_oracle(which):
    """MelConfig(db_scale=-1/80): features (max(db, max - 80) + 80) (-1/80) <= 0 -- the packed front end's two-instruction
    finish max(fma(x, scale, c1), 0) is only right for a positive scale (it gave 0 for every feature).  MelConfig(top_db=60):
    top_db != db_add, the floor maps to 0.25, not 0.  Two windows get a quiet second half, so the clamp is met widely.
    Observed on MI355X: before the mel_packs fix the negative scale missed tier A by 7.4x mouth_queries' largest gradient entry;
    now both: loss <= 1.2e-8, out 6.7e-8, gradients at 0.19 of the bound (2.3e-6 of the largest entry)."""
    cfg = MelConfig(db_scale=-1.0 / 80.0) if which == "db_scale_negative" else MelConfig(top_db=60.0)
    params = synth.make_core_params(161, style="trained")
    audio = speech(161, 8, 136448)
    audio[3, 70000:] *= 1e-3
    audio[6, 30000:] *= 1e-4
    emo, target = synth.normal(162, (8, 256)), synth.uniform(163, (8, 52), 0, 1)
    _, fa, fb = both_tiers(params, C3, audio, emo, target, mel_cfg=cfg, tag=which)
    if which == "db_scale_negative":
        assert fa[0].max() <= 0.0 and fa[0].min() < -0.5 and fb[0].min() < -0.5
    else:
        assert abs(fa[0].min() - 0.25) < 1e-6 and (fa[0] < 0.25 + 1e-6).mean() > 0.01


# ---- 8: caller pointers that are not 16-byte aligned ---------------------------------------------------------------------
def test_unaligned_emotion_and_target_views_train():
    """emo and target as views at a one-float offset, through forward_backward and forward_backward_mel at 8 windows (where
    the program normalises Y0 / E0 in their readers).  E0's product reads the caller's emotion pointer: off the LDS-DMA tile
    it cannot carry the LayerNorm parts, and the step must take the LayerNorm phase instead of failing.  Same numbers as the
    aligned call within the ln_phase tolerance (2e-5 of the largest entry), and tier A against the oracle.  Observed on MI355X:
    before the fix both entry points raised "LayerNorm by the reader needs the LDS-DMA tile"; now tier A loss 3.2e-8, out
    1.5e-7, gradients at 0.16 of the bound, on both paths, aligned or not."""
    params = synth.make_core_params(171, style="trained")
    shapes = {k: v.shape for k, v in params.items()}
    audio = speech(171, 8, 136448)
    emo, target = synth.normal(172, (8, 256)), synth.uniform(173, (8, 52), 0, 1)

    def offset_view(x):
        t = torch.empty(x.size + 1, device="cuda")[1:].view(*x.shape)
        t.copy_(dev(x))
        assert t.data_ptr() % 16 != 0 and t.is_contiguous()
        return t

    e = engine(params, C3)
    tr = Trainer(e, max_windows=8, use_smoothing=False, l1_weight=0.1)
    long, short = hip_features(params, C3, audio)
    want = oracle_step(params, (long, short), emo, target, C3, l1=0.1)
    runs = {}
    for path in ("audio", "mel"):
        for aligned in (True, False):
            em, tg = (dev(emo), dev(target)) if aligned else (offset_view(emo), offset_view(target))
            if path == "audio":
                loss = tr.forward_backward(dev(audio), em, tg)
            else:
                loss = tr.forward_backward_mel(dev(long), dev(short), em, tg)
            runs[path, aligned] = (float(loss.item()), tr.out[:8].cpu().numpy().copy(), tr.grads(shapes))
    for path in ("audio", "mel"):
        la, _, ga = runs[path, True]
        lu, _, gu = runs[path, False]
        assert abs(lu - la) < 2e-6 * max(1.0, abs(la)), path
        for k in ga:
            np.testing.assert_allclose(gu[k], ga[k], atol=1e-8 + 2e-5 * np.abs(ga[k]).max(), rtol=2e-4, err_msg=f"{path}: {k}")
        check(f"unaligned {path}", runs[path, False], want)
        check(f"aligned {path}", runs[path, True], want)


# ---- 9: three optimizer steps from audio against torch.optim.AdamW -------------------------------------------------------
def test_adamw_steps_from_audio_match_torch_adamw_with_ema_and_l1():
    """3 x tr.step + a 4th forward_backward from audio, EMA inside the forward, MSE + 0.1 L1, global-norm clipping, AdamW --
    against the same loop in torch (float64 autograd on the oracle forward fed with tier-A features, torch.optim.AdamW).  The
    from-audio step reads the channel encoder through its padded copy (PaddedCopy), which AdamW must keep current: the losses
    of steps 2-4 would move otherwise.  Acceptance as in test_training_loop_matches_torch_adamw_with_ema_and_l1.  Observed on
    MI355X: losses within 1.7e-8 at every step, parameters within 1.1e-5 (k third of the key bias aside)."""
    c, B, lr = C3, 5, 3e-3
    params = synth.make_core_params(181, style="trained")
    e = Engine(d_model=c["d"], num_heads=c["H"], mel_sequence_length=c["T"])
    e.load_state_dict(params)
    e.load_param("smoothing_alpha", np.float32(0.3))
    e.finalize()
    tr = Trainer(e, max_windows=B, lr=lr, weight_decay=1e-2, grad_clip=0.05, mse_weight=1.0, l1_weight=0.1, use_smoothing=True)
    P = {k: torch.from_numpy(v.copy()).double().requires_grad_(True) for k, v in params.items()}
    alpha_p = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW(list(P.values()) + [alpha_p], lr=lr, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
    fe = engine(params, c)                    # tier-A features: the front end alone, on an engine the optimizer never touches
    prev = None
    for step in range(4):
        audio = speech(190 + step, B, 136448)
        emo, target = synth.normal(195 + step, (B, 256)), synth.uniform(199 + step, (B, 52), 0, 1)
        long, short = fe.mel_batch(dev(audio))
        long, short = long.cpu().numpy(), short.cpu().numpy()
        if step < 3:
            loss_gpu = float(tr.step(dev(audio), dev(emo), dev(target)).item())
        else:
            loss_gpu = float(tr.forward_backward(dev(audio), dev(emo), dev(target)).item())
        opt.zero_grad()
        x = core.core_forward(P, long, short, emo, num_heads=8, mel_sequence_length=256, dtype=torch.float64)["blendshapes"]
        y = x if prev is None else torch.sigmoid(alpha_p) * x + (1 - torch.sigmoid(alpha_p)) * prev
        prev = y.detach()
        t = torch.from_numpy(target).double()
        loss = F.mse_loss(y, t) + 0.1 * F.l1_loss(y, t)
        loss.backward()
        want = float(loss.item())
        print(f"\n[adamw] step {step}: loss {abs(loss_gpu - want):.2e}")
        assert abs(loss_gpu - want) < 2e-6 * max(1.0, want), step
        if step > 0:
            ga = tr.grads({"smoothing_alpha": ()})["smoothing_alpha"]
            assert abs(float(ga) - float(alpha_p.grad)) < 1e-7 + 2e-4 * abs(float(alpha_p.grad)), step
        if step < 3:
            torch.nn.utils.clip_grad_norm_(list(P.values()) + [alpha_p], 0.05)
            opt.step()
    got = tr.params({**{k: v.shape for k, v in params.items()}, "smoothing_alpha": ()})
    worst = 0.0
    for k, v in P.items():
        a, b = got[k], v.detach().numpy()
        if k == "mel_attention.in_proj_bias":
            # the key bias has an exactly-zero gradient (softmax shift invariance): Adam turns both sides' rounding noise there
            # into lr-sized steps of random sign -- q and v thirds tightly, the k third by the step budget
            np.testing.assert_allclose(a[:256], b[:256], atol=2e-6, rtol=2e-5, err_msg=k + "[q]")
            np.testing.assert_allclose(a[512:], b[512:], atol=2e-6, rtol=2e-5, err_msg=k + "[v]")
            assert np.abs(a[256:512] - b[256:512]).max() <= 2 * 3 * lr
            continue
        bad = np.abs(a - b) > 2e-6 + 2e-5 * np.abs(b)
        assert bad.mean() <= 1e-3, (k, bad.mean())
        assert np.abs(a - b).max() < 1e-4, (k, np.abs(a - b).max())
        worst = max(worst, float(np.abs(a - b).max()))
    print(f"[adamw] parameters: max |diff| {worst:.2e}")
    assert abs(float(got["smoothing_alpha"]) - float(alpha_p.detach())) < 2e-6
