"""d_model 128 / 4 heads / 80 mel channels at window 128 (`fast`) and 256 (`basic`) on the host alone (after finalize_host, no device):
the route code km_core_route names -- 3, the launch-per-product chain, by default; 4, core128_kernel, under option core128 -- and the
three operand images the kernel reads (wce_pg128, wv_bg128, wf_pg128), which are packed at this shape only and under names of their
own, so that the presence of wce_pg and wv_bg32 keeps meaning what it meant."""
import numpy as np
import pytest

from koemorph_amd import synth
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.engine import Engine, MelConfig

SHAPES = [(128, 4, 128), (128, 4, 256)]
FALLBACKS = ("no_ln_fusion", "no_score_fusion", "no_out_fusion", "no_v_fusion", "no_core_merge", "no_db_fusion")


def host_engine(d, H, T, n_mels=80, **options):
    mel = MelConfig(n_mels=n_mels)
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


@pytest.mark.parametrize("d,H,T", SHAPES)
def test_the_chain_by_default_and_core128_under_the_option(d, H, T):
    assert route(d, H, T) == 3
    assert route(d, H, T, core128=1) == 4


@pytest.mark.parametrize("d,H,T", SHAPES)
def test_a_requested_map_and_the_fallback_switches_bring_the_chain_back(d, H, T):
    assert route(d, H, T, with_attention=True, core128=1) == 3
    for name in FALLBACKS:
        assert route(d, H, T, core128=1, **{name: 1}) == 3, name


def test_the_switch_is_read_when_the_route_is_asked_for():
    e = host_engine(128, 4, 128)
    assert e.core_route() == 3
    e.set_option("core128", 1)
    assert e.core_route() == 4 and e.core_route(with_attention=True) == 3
    e.set_option("no_core_merge", 1)
    assert e.core_route() == 3
    e.set_option("no_core_merge", 0)
    e.set_option("core128", 0)
    assert e.core_route() == 3
    e.close()


def test_every_other_shape_keeps_its_route_under_the_option():
    assert route(128, 4, 64, core128=1) == 3
    assert route(128, 8, 128, core128=1) == 3
    assert route(128, 4, 128, n_mels=64, core128=1) == 3
    assert route(256, 8, 128, core128=1) == 3
    assert route(256, 8, 256, core128=1) == 0 and route(256, 8, 512, core128=1) == 2 and route(512, 8, 512, core128=1) == 1


@pytest.mark.parametrize("d,H,T", SHAPES)
def test_operand_images_of_core128(d, H, T):
    """wce_pg128[k block][wave < 4][tile < 2][lane 16 g + j][s] = Wce[32 wave + 2 j + tile][16 kb + 4 g + s] (K zero-padded to KP);
    wv_bg128[k block][wave][tile][lane][s] = Wv[32 wave + 16 tile + j][16 kb + 4 g + s];
    wf_pg128[wave][k block][lane][s] = Wf[16 kb + 4 g + s][16 wave + j], Wf the folded (d, 64) decoder input matrix."""
    e = host_engine(d, H, T)
    p = synth.make_core_params(3, d, T, 256, "trained")
    KT, KP, KB = T + 3, (T + 3 + 15) // 16 * 16, d // 16
    assert KP == {128: 144, 256: 272}[T]
    wce = np.zeros((d, KP), np.float32)
    wce[:, :KT] = p["mel_channel_encoder.weight"]
    img = e.debug_buffer("wce_pg128").reshape(KP // 16, 4, 2, 4, 16, 4)              # kb, wave, tile, g, j, s
    want = wce.reshape(4, 16, 2, KP // 16, 4, 4).transpose(3, 0, 2, 4, 1, 5)          # (wave, j, tile, kb, g, s) -> image order
    assert np.array_equal(img, want)
    wv = p["mel_attention.in_proj_weight"][2 * d:]
    img = e.debug_buffer("wv_bg128").reshape(KB, 4, 2, 4, 16, 4)                     # kb, wave, tile, g, j, s
    want = wv.reshape(4, 2, 16, KB, 4, 4).transpose(3, 0, 1, 4, 2, 5)                 # (wave, tile, j, kb, g, s) -> image order
    assert np.array_equal(img, want)
    wf = e.debug_buffer("wf").reshape(d, 64)
    img = e.debug_buffer("wf_pg128").reshape(4, KB, 4, 16, 4)                        # wave, kb, g, j, s
    want = wf.reshape(KB, 4, 4, 4, 16).transpose(3, 0, 1, 4, 2)                       # (kb, g, s, wave, j) -> image order
    assert np.array_equal(img, want)
    for name in ("wce_pg", "wv_bg32", "wv_bg"):                                      # the names other predicates read stay unpacked
        with pytest.raises(KoeMorphError):
            e.debug_buffer(name)
    e.close()


@pytest.mark.parametrize("d,H,T", [(256, 8, 512), (256, 8, 256), (512, 8, 512), (128, 8, 128), (128, 4, 64)])
def test_the_images_are_packed_where_the_kernel_runs(d, H, T):
    e = host_engine(d, H, T)
    for name in ("wce_pg128", "wv_bg128", "wf_pg128"):
        if (d, H) == (128, 4):          # the images do not depend on the window; the predicate does
            assert e.debug_buffer(name).size > 0
        else:
            with pytest.raises(KoeMorphError):
                e.debug_buffer(name)
    e.close()
