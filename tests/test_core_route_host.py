"""km_core_route / Engine.core_route names the core the forward calls run for a shape and its switches, on the host alone
(after finalize_host, no device): 0 the fused d_model 256 / window 256 core, 1 core512_kernel, 2 core256w_kernel -- d_model 256,
8 heads, 80 mel channels, window 512, the shape of the reference's frame_rate=60 recipe -- and 3 the launch-per-product chain."""
import pytest

from koemorph_amd import synth
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.engine import Engine, MelConfig


def host_engine(d, H, T, n_mels=80, **options):
    mel = MelConfig.model_batch(target_fps=60)
    mel.n_mels = n_mels
    e = Engine(d_model=d, num_heads=H, mel_sequence_length=T, num_mel_channels=n_mels, mel=mel)
    e.load_state_dict(synth.make_core_params(3, d, T, 256, "trained"))     # no parameter's shape depends on the channel count
    for name, value in options.items():
        e.set_option(name, value)
    e.finalize_host()
    return e


def route(d, H, T, with_attention=False, **kw):
    e = host_engine(d, H, T, **kw)
    try:
        return e.core_route(with_attention)
    finally:
        e.close()


def test_the_60fps_recipe_shape_takes_the_one_launch_core():
    assert route(256, 8, 512) == 2


def test_a_requested_map_and_no_core_merge_bring_the_chain_back():
    assert route(256, 8, 512, with_attention=True) == 3
    assert route(256, 8, 512, no_core_merge=1) == 3
    for name in ("no_ln_fusion", "no_score_fusion", "no_out_fusion", "no_v_fusion"):
        assert route(256, 8, 512, **{name: 1}) == 3, name


def test_the_production_shape_and_d512_keep_their_kernels():
    assert route(256, 8, 256) == 0 and route(256, 8, 256, with_attention=True) == 0
    assert route(512, 8, 512) == 1 and route(512, 16, 512) == 1
    assert route(512, 8, 512, with_attention=True) == 3 and route(512, 8, 512, no_core_merge=1) == 3


def test_every_other_d256_shape_keeps_the_chain():
    assert route(256, 8, 128) == 3
    assert route(256, 16, 512) == 3
    assert route(256, 8, 512, n_mels=64) == 3


def test_the_switch_is_read_when_the_route_is_asked_for():
    e = host_engine(256, 8, 512)
    assert e.core_route() == 2
    e.set_option("no_core_merge", 1)
    assert e.core_route() == 3
    e.set_option("no_core_merge", 0)
    assert e.core_route() == 2
    e.close()


def test_value_operand_image_of_the_one_launch_core():
    """wv_bg32[k block][wave][column tile < 2][lane 16 g + j][s] = Wv[32 wave + 16 tile + j][16 kb + 4 g + s]; packed at d_model
    256 only, and wv_bg (the d_model 512 image) keeps its meaning."""
    import numpy as np
    d = 256
    e = host_engine(d, 8, 512)
    wv = synth.make_core_params(3, d, 512, 256, "trained")["mel_attention.in_proj_weight"][2 * d:]
    img = e.debug_buffer("wv_bg32").reshape(d // 16, 8, 2, 4, 16, 4)          # kb, wave, tile, g, j, s
    want = wv.reshape(8, 2, 16, d // 16, 4, 4).transpose(3, 0, 1, 4, 2, 5)     # (wave, tile, j, kb, g, s) -> image order
    assert np.array_equal(img, want)
    with pytest.raises(KoeMorphError):
        e.debug_buffer("wv_bg")
    e.close()
    e = host_engine(512, 8, 512)
    assert e.debug_buffer("wv_bg").size == 512 * 512
    with pytest.raises(KoeMorphError):
        e.debug_buffer("wv_bg32")
    e.close()


def test_the_route_needs_the_folded_parameters():
    e = Engine(d_model=256, num_heads=8, mel_sequence_length=512, mel=MelConfig.model_batch(target_fps=60))
    with pytest.raises(KoeMorphError, match="km_finalize_host"):
        e.core_route()
    e.close()
