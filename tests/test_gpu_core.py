"""GPU parity of the attention core (km_core_forward, HIP through the C-ABI) against the golden
outputs of the reference's own DualStreamCrossAttention and against the oracle.

Tolerance: BASELINE.json states 1e-4 abs on the 52 fp32 coefficients.  The kernel is exact-fp32
MFMA, so the expected error is summation-order noise (~1e-7); the tests assert 2e-6 (and 1e-4
as the contractual bound) so that a layout bug cannot hide inside the tolerance.
"""
import numpy as np
import pytest
import torch

from conftest import CORE_CASES_D256, CORE_CASES_OTHER, golden_case
from koemorph_amd import synth
from koemorph_amd.engine import Engine
from oracle import core

pytestmark = pytest.mark.gpu
TOL = 2e-6
CONTRACT = 1e-4


def assert_logit_bound(name, c, params, inputs, o):
    """The same outputs in the logit-space measure against the float64 oracle (tests/test_gpu_core_logit.py): the fixed
    bounds above admit ~200 times more on the decoder logit than they seem to."""
    from core_logit_cases import K
    mel, short, emo = inputs
    ref = core.logit_reference(params, mel, short, emo, num_heads=c["H"], mel_sequence_length=c["T"])
    for what, s, roundings in (("raw", o["raw"].cpu().numpy(), 1),
                               ("out/c", core.recover_sigmoid(o["blendshapes"].cpu().numpy(), params), core.OUT_OVER_C_ROUNDINGS)):
        e, ratio = core.logit_verdict(s, ref, K, roundings)
        print(f"CORELOGIT|golden|{name} {what}|{e:.3e}|{ref['yard_e']:.3e}|{ratio:.3f}")
        assert ratio <= 1.0, (name, what, e, ref["yard_e"])
    e, ratio = core.attention_verdict(o["mel_attention_weights"].cpu().numpy(), ref, K)
    print(f"CORELOGIT|golden|{name} attention|{e:.3e}|{ref['yard_a']:.3e}|{ratio:.3f}")
    assert ratio <= 1.0, (name, "attention", e, ref["yard_a"])


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def engine_for(params, **kw):
    e = Engine(**kw)
    e.load_state_dict(params)
    e.finalize()
    return e


@pytest.mark.parametrize("name", CORE_CASES_D256)
def test_core_matches_reference_golden(name):
    c, params, (mel, short, emo), g = golden_case(name)
    e = engine_for(params)
    o = e.core_forward(dev(mel), dev(short), dev(emo), return_attention=True)
    bs = o["blendshapes"].cpu().numpy()
    err = np.abs(bs - g["blendshapes"]).max()
    assert err < CONTRACT, f"contract violated: {err}"
    assert err < TOL, f"max abs err {err}"
    np.testing.assert_allclose(o["mel_attention_weights"].cpu().numpy(), g["mel_attention_weights"], atol=TOL)
    raw = o["raw"].cpu().numpy()
    mb = np.zeros_like(raw); mb[:, synth.MOUTH_INDICES] = raw[:, synth.MOUTH_INDICES]
    eb = np.zeros_like(raw); eb[:, synth.EXPRESSION_INDICES] = raw[:, synth.EXPRESSION_INDICES]
    np.testing.assert_allclose(mb, g["mel_blendshapes"], atol=2e-5)
    np.testing.assert_allclose(eb, g["emotion_blendshapes"], atol=2e-5)
    # the no-attention kernel instantiation must give the same coefficients
    o2 = e.core_forward(dev(mel), dev(short), dev(emo))
    assert torch.equal(o2["blendshapes"], o["blendshapes"])
    assert_logit_bound(name, c, params, (mel, short, emo), o)


def test_core_full_batch_against_oracle():
    """BASELINE config C2 shape: B=256 windows, plus a ragged batch that is not a multiple of anything."""
    params = synth.make_core_params(77, style="trained")
    e = engine_for(params)
    for B, t_in in ((256, 257), (37, 257), (1, 256)):
        mel, short, emo = synth.make_core_inputs(900 + B, B, t_in)
        ref = core.core_forward_np(params, mel, short, emo)["blendshapes"]
        got = e.core_forward(dev(mel), dev(short), dev(emo))["blendshapes"].cpu().numpy()
        assert np.abs(got - ref).max() < TOL


def test_core_properties_at_full_size():
    params = synth.make_core_params(78, style="trained")
    e = engine_for(params)
    mel, short, emo = synth.make_core_inputs(5, 64, 257)
    o = e.core_forward(dev(mel), dev(short), dev(emo), return_attention=True)
    a = o["mel_attention_weights"]
    assert torch.allclose(a.sum(-1), torch.ones_like(a.sum(-1)), atol=1e-5)     # rows sum to 1
    bs = o["blendshapes"]
    assert bs.min() >= 0 and bs.max() <= 1
    # windows are independent: permuting the batch permutes the output bit for bit
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0)).cuda()
    o2 = e.core_forward(dev(mel)[perm], dev(short)[perm], dev(emo)[perm])
    assert torch.equal(o2["blendshapes"], bs[perm])
    # rows beyond mel_sequence_length are ignored (truncate path) and the result is deterministic
    mel_long = np.concatenate([mel, synth.uniform(9, (64, 10, 80), 0, 1)], axis=1)
    o3 = e.core_forward(dev(mel_long), dev(short), dev(emo))
    assert torch.equal(o3["blendshapes"], bs)


def test_core_error_paths():
    from koemorph_amd._lib import KoeMorphError
    params = synth.make_core_params(1)
    e = Engine()
    e.load_state_dict(params)
    mel, short, emo = synth.make_core_inputs(1, 2, 257)
    with pytest.raises(KoeMorphError, match="km_finalize"):
        e.reserve(2)
        e.core_forward(dev(mel), dev(short), dev(emo))
    e.finalize()
    with pytest.raises(ValueError):
        e.core_forward(dev(mel)[0], dev(short), dev(emo))                       # bad rank
    with pytest.raises(ValueError):
        e.core_forward(dev(mel), dev(short), dev(emo)[:, :100])                 # bad emotion dim


@pytest.mark.parametrize("name", CORE_CASES_OTHER)
def test_generic_shapes_match_reference_golden(name):
    """BASELINE config 4 (d_model 512, window 512, 8 / 16 heads) and the small d=64 configuration run the
    shape-generic GEMM-chain path (km_generic.hip)."""
    c, params, (mel, short, emo), g = golden_case(name)
    e = engine_for(params, d_model=c["d"], num_heads=c["H"], mel_sequence_length=c["T"])
    assert not e.fused
    o = e.core_forward(dev(mel), dev(short), dev(emo), return_attention=True)
    err = np.abs(o["blendshapes"].cpu().numpy() - g["blendshapes"]).max()
    assert err < TOL, err
    np.testing.assert_allclose(o["mel_attention_weights"].cpu().numpy(), g["mel_attention_weights"], atol=TOL)
    raw = o["raw"].cpu().numpy()
    np.testing.assert_allclose(raw[:, synth.MOUTH_INDICES], g["mel_blendshapes"][:, synth.MOUTH_INDICES], atol=2e-5)
    np.testing.assert_allclose(raw[:, synth.EXPRESSION_INDICES], g["emotion_blendshapes"][:, synth.EXPRESSION_INDICES], atol=2e-5)
    assert_logit_bound(name, c, params, (mel, short, emo), o)


def test_generic_path_full_batch_against_oracle():
    """BASELINE config 4 at batch size, plus the zero-pad (T_in < T) and truncate (T_in > T) branches."""
    params = synth.make_core_params(88, 512, 512, style="trained")
    e = engine_for(params, d_model=512, num_heads=8, mel_sequence_length=512)
    for B, t_in in ((64, 513), (5, 300), (3, 600)):
        mel, short, emo = synth.make_core_inputs(700 + B, B, t_in)
        ref = core.core_forward_np(params, mel, short, emo, num_heads=8, mel_sequence_length=512)["blendshapes"]
        got = e.core_forward(dev(mel), dev(short), dev(emo))["blendshapes"].cpu().numpy()
        assert np.abs(got - ref).max() < TOL


def test_smooth_kernel_matches_oracle():
    from oracle import smoothing
    e = engine_for(synth.make_core_params(3))
    seq = synth.uniform(4, (5, 7, 52), 0, 1)
    want = smoothing.smooth_sequence(seq, 0.8)
    state = torch.zeros(7, 52, device="cuda")
    for i in range(5):
        x = dev(seq[i])
        e.smooth(x, state, first=(i == 0))
        np.testing.assert_allclose(x.cpu().numpy(), want[i], atol=1e-7)


@pytest.mark.parametrize("terms,tol", [(3, 5e-6), (6, 2e-7)])
def test_split_bf16_variant_is_opt_in_and_close(terms, tol):
    """The experimental split-bf16 form of phases 2+3 (option core_split): off by default, and when asked for it
    stays within the error study's bounds of the fp32 kernel on trained-like weights (contract: 1e-4)."""
    from koemorph_amd import synth
    from koemorph_amd.engine import Engine
    eng = Engine(); eng.load_state_dict(synth.make_core_params(12, style="trained")); eng.finalize(); eng.reserve(8, 136448)
    audio = torch.from_numpy(synth.make_audio(3, 8, 136448, "speech")).cuda()
    emo = torch.from_numpy(synth.normal(4, (8, 256))).cuda()
    eng.set_option("core_split", 0)
    ref = eng.forward_audio(audio, emo).clone()
    eng.set_option("core_split", terms)
    got = eng.forward_audio(audio, emo).clone()
    eng.set_option("core_split", 0)
    again = eng.forward_audio(audio, emo)
    assert torch.equal(again, ref)
    err = float((got - ref).abs().max())
    assert err < tol, err                          # inside the error study's bound
    if terms == 3:
        assert err > 0                             # 16 mantissa bits: a different arithmetic, visibly (six terms can round to the same floats)


def test_window_maxima_are_handed_back_clean_without_a_memset():
    """The dB reference of a window is the maximum of ITS power-mel (librosa power_to_db(ref=np.max)), collected with
    atomicMax into a per-window slot that the consumer re-zeroes (fused d=256 core, generic encoder).  A loud batch followed
    by a quiet one on the same engine must give what a fresh engine gives for the quiet one -- a stale maximum would shift
    every dB value of the second call."""
    for kw, pk in ((dict(), dict(style="init")), (dict(d_model=512, num_heads=16, mel_sequence_length=512), None)):
        if pk is None:
            params = synth.make_core_params(5, 512, 512, 256, "init")
        else:
            params = synth.make_core_params(5, **pk)
        L = 136448 if not kw else 512 * 266
        loud = dev(synth.make_audio(6, 4, L, "uniform"))
        quiet = dev(synth.make_audio(7, 4, L, "uniform") * 1e-3)
        emo = dev(synth.normal(8, (4, 256)))
        outs = []
        for fresh in (False, True):
            from koemorph_amd.engine import Engine, MelConfig
            e = Engine(**kw, **({"mel": MelConfig.model_batch(target_fps=60)} if kw else {}))
            e.load_state_dict(params)
            e.finalize()
            e.reserve(4, L)
            if not fresh:
                e.forward_audio(loud, emo)
            outs.append(e.forward_audio(quiet, emo).cpu().numpy())
        assert np.array_equal(outs[0], outs[1])


def test_generic_path_at_d256_other_window_against_oracle():
    """d_model 256 with a window other than 256 does not fit the fused kernel's constants and runs the generic chain with
    the 8-wave x 32-column instantiation of the encoder + LayerNorm kernel (the d=512 and d=64 goldens cover the others);
    16 heads of 16 columns go through the unfused output path."""
    for H, T in ((8, 128), (16, 160)):
        params = synth.make_core_params(91, 256, T, style="trained")
        e = engine_for(params, d_model=256, num_heads=H, mel_sequence_length=T)
        assert not e.fused
        for B, t_in in ((9, T + 1), (4, T - 37)):
            mel, short, emo = synth.make_core_inputs(800 + B, B, t_in)
            ref = core.core_forward_np(params, mel, short, emo, num_heads=H, mel_sequence_length=T)["blendshapes"]
            got = e.core_forward(dev(mel), dev(short), dev(emo))["blendshapes"].cpu().numpy()
            assert np.abs(got - ref).max() < TOL


@pytest.mark.parametrize("heads", [8, 16])
def test_d512_core_in_one_launch_is_the_three_kernels_bit_for_bit(heads):
    """Round 4: at d_model 512 the encoder + LayerNorm, scores + softmax and output kernels run as three stages of ONE launch
    (core512_kernel: the same three bodies, a __syncthreads() between them; option no_core_merge brings the three launches back).
    From audio (dB conversion inside the first stage, window maxima re-zeroed by it) and from caller-provided mel: identical bits."""
    from koemorph_amd.engine import Engine, MelConfig
    params = synth.make_core_params(21, 512, 512, 256, "trained")
    L = 512 * 266
    audio = dev(synth.make_audio(22, 5, L, "uniform"))
    emo = dev(synth.normal(23, (5, 256)))
    mel, short, _ = synth.make_core_inputs(24, 5, 513, style="mel01")
    res = []
    for no_merge in (0, 1):
        e = Engine(d_model=512, num_heads=heads, mel_sequence_length=512, mel=MelConfig.model_batch(target_fps=60))
        e.load_state_dict(params)
        e.finalize()
        e.set_option("no_core_merge", no_merge)
        e.reserve(5, L)
        a = [e.forward_audio(audio, emo).cpu().numpy() for _ in range(2)]          # twice: the maxima were handed back clean
        m = e.core_forward(dev(mel), dev(short), emo)["blendshapes"].cpu().numpy()
        res.append((a, m))
    assert np.array_equal(res[0][0][0], res[0][0][1]) and np.array_equal(res[1][0][0], res[1][0][1])
    assert np.array_equal(res[0][0][0], res[1][0][0])
    assert np.array_equal(res[0][1], res[1][1])

