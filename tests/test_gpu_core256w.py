"""The shape of the reference's frame_rate=60 recipe -- d_model 256, 8 heads, 80 mel channels, window 512, front end at hop
266 -- against the float64 oracle in logit space (the harness and the bound of tests/core_logit_cases.py, K = 4), on both routes:

  route 2   core256w_kernel, one launch: encoder_ln_body<8, 2> at KP = 528, scores_softmax_body<256, 2> (its first instantiation
            below d_model 512: 14 row tiles, tiles 12 and 13 split along k) and attn_out_vr32_body (km_attn256_dev.h);
  route 3   option no_core_merge: encoder_ln_kernel<8, 2> and the launch-per-product chain, which no test ran at this window.

The routes are not required to agree bit for bit; each meets the bound on its own.  A call that asks for the attention map takes
the chain on either engine, so run_core's `raw` and map lines judge the chain; `out / c noattn` and raw_without_map judge the
route under test.
"""

import numpy as np
import pytest
import torch

from core_logit_cases import engine_for, guarded, judge, make_inputs, make_params, run_core
from koemorph_amd import synth
from koemorph_amd._lib import check
from koemorph_amd.engine import MelConfig, _ptr, _stream_ptr
from oracle import core, models

pytestmark = pytest.mark.gpu
D, H, T = 256, 8, 512
SEED = 88
ROUTES = [pytest.param(0, id="core256w"), pytest.param(1, id="chain")]


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(pk, no_merge):
        if (pk, no_merge) not in cache:
            params = make_params(pk, SEED, D, T)
            e = engine_for(params, d_model=D, num_heads=H, mel_sequence_length=T, mel=MelConfig.model_batch(target_fps=60))
            e.set_option("no_core_merge", no_merge)
            assert not e.fused and e.mel.hop_length == 266
            assert e.core_route() == (3 if no_merge else 2) and e.core_route(with_attention=True) == 3
            cache[(pk, no_merge)] = (params, e)
        return cache[(pk, no_merge)]
    yield get
    for _, e in cache.values():
        e.close()


def raw_without_map(e, gm, gs, ge):
    """km_core_forward with `raw` asked for and no map: the route under test, not the chain a map request falls back to."""
    B = gm.shape[0]
    e.reserve(B, 0)
    out = torch.empty(B, 52, device="cuda")
    raw = torch.empty(B, 52, device="cuda")
    check(e._lib.km_core_forward(e._h, _ptr(gm), B, gm.shape[1], _ptr(gs), _ptr(ge), _ptr(out), _ptr(raw), None, _stream_ptr(gm.device)))
    return out, raw


def from_mel(e, params, label, inputs):
    ref, o = run_core(e, "d256w", label, params, inputs, H=H, T=T)
    gm, gs, ge = (guarded(x) for x in inputs)
    out, raw = raw_without_map(e, gm, gs, ge)
    judge("d256w", label + " raw nomap", ref, s=raw.cpu().numpy())
    assert torch.equal(out, e.core_forward(gm, gs, ge)["blendshapes"])                  # asking for raw changes no bit of out
    out2, raw2 = raw_without_map(e, gm, gs, ge)
    assert torch.equal(out, out2) and torch.equal(raw, raw2)                           # two runs, equal bits


# every parameter kind at B = 3, t_in = 513 (NaN in row 512: it must be skipped, not multiplied by zero); every input kind once
@pytest.mark.parametrize("no_merge", ROUTES)
@pytest.mark.parametrize("pk,ik", [("init", "mel01"), ("trained", "zeroch"), ("sharp", "huge"), ("bias0", "zeroch"), ("offset", "mel01")])
def test_parameter_kinds_at_t_in_513(engines, pk, ik, no_merge):
    params, e = engines(pk, no_merge)
    from_mel(e, params, f"{pk} {ik} B=3 t_in=513 route {e.core_route()}", make_inputs(ik, 700, 3, 513, T))


# batch sizes and input lengths: the full window, a short one (zero rows 100 .. 511) and a single frame
@pytest.mark.parametrize("no_merge", ROUTES)
@pytest.mark.parametrize("B,t_in,ik", [(1, 512, "mel01"), (9, 100, "huge"), (3, 1, "mel01"), (9, 513, "zeroch"), (1, 513, "huge")])
def test_batch_sizes_and_input_lengths(engines, B, t_in, ik, no_merge):
    params, e = engines("trained", no_merge)
    from_mel(e, params, f"trained {ik} B={B} t_in={t_in} route {e.core_route()}", make_inputs(ik, 710 + t_in + B, B, t_in, T))


@pytest.mark.parametrize("no_merge", ROUTES)
@pytest.mark.parametrize("pk", ["init", "trained"])
def test_forward_audio_in_logit_space(engines, pk, no_merge):
    """km_forward_audio: the dB conversion inside the first stage (encoder_ln_body<8, 2, FUSE_DB = true>).  L = 136 192 is 513
    frames (the 513th only feeds the short rows), 136 000 is 512, 5 000 is 19 (zero rows up to 512); window 1 of the first batch is
    silent (window maximum 0); every batch runs twice, and a quiet batch follows a loud one on the same engine, so a window
    maximum that was not handed back clean would move the dB reference."""
    params, e = engines(pk, no_merge)
    emo = synth.normal(81, (3, 256))
    ge = guarded(emo)
    batches = []
    for L in (136192, 136000, 5000):
        a = synth.make_audio(82 + L % 7, 3, L, "speech")
        if L == 136192:
            a = a.copy()
            a[1] = 0.0
        batches.append((f"L={L}", a))
    loud = np.clip(synth.make_audio(90, 3, 136192, "uniform") * np.float32(8.0), -1.0, 1.0).astype(np.float32)
    batches += [("loud", loud), ("quiet after loud", (synth.make_audio(91, 3, 136192, "speech") * np.float32(1e-3)).astype(np.float32))]
    for name, audio in batches:
        ga = guarded(audio)
        long, short = e.mel_batch(ga)
        ref = core.logit_reference(params, long.cpu().numpy(), short.cpu().numpy(), emo, num_heads=H, mel_sequence_length=T)
        first = None
        for call in range(2):
            out = e.forward_audio(ga, ge)
            judge("d256w", f"{pk} route {e.core_route()} audio {name} call{call}", ref, s=core.recover_sigmoid(out.cpu().numpy(), params),
                  out_over_c=True)
            first = out.clone() if first is None else first
            assert torch.equal(out, first)


@pytest.mark.parametrize("no_merge", ROUTES)
def test_whole_model_from_audio_and_sequence_mode(no_merge):
    """forward_audio and sequence_forward at stride 2 on two clips against the per-window oracle (its own float64 front end), within
    the 5e-6 the d_model 512 model test holds (tests/test_gpu_models.py, BASELINE config 4)."""
    params = synth.make_core_params(55, D, T, 256, "trained")
    e = engine_for(params, d_model=D, num_heads=H, mel_sequence_length=T, mel=MelConfig.model_batch(target_fps=60))
    e.set_option("no_core_merge", no_merge)
    assert e.core_route() == (3 if no_merge else 2)
    orc = models.SimplifiedOracle(params, num_heads=H, mel_sequence_length=T, target_fps=60)
    audio, emo = synth.make_audio(97, 2, T * 266), synth.normal(98, (2, 256))
    got = e.forward_audio(guarded(audio), guarded(emo)).cpu().numpy()
    err = float(np.abs(got - orc.forward(audio, emo)["blendshapes"]).max())
    print(f"D256W|route {e.core_route()}|forward_audio|{err:.3e}")
    assert err < 5e-6
    sorc = models.SequentialOracle(params, num_heads=H, mel_sequence_length=T, target_fps=60, stride_frames=2)
    audio, emo = synth.make_audio(99, 2, T * 266 + 266 * 6 + 50), synth.normal(100, (2, 256))
    want = sorc.forward(audio, emo)
    g = e.sequence_forward(guarded(audio), guarded(emo), stride_frames=2)
    assert g.shape == (2, 4, 52) and want["num_frames"] == 4
    err = float(np.abs(g.cpu().numpy() - want["blendshapes"]).max())
    print(f"D256W|route {e.core_route()}|sequence_forward|{err:.3e}")
    assert err < 5e-6
    assert torch.equal(g, e.sequence_forward(guarded(audio), guarded(emo), stride_frames=2))
    e.close()
