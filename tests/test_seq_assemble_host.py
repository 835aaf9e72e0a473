"""km_sequence_plan / Engine.sequence_plan names the schedule a sequence call runs, on the host alone (after finalize_host, no
device), against the restatement in tests/seq_assemble_cases.py built on koemorph_amd.clip_span.edge_frames:

  route 1 (images read by the fused core) only on the fused shape with one edge frame per side and option seq_assemble off;
  route 2 (images assembled into the workspace) only with the option on, where km_forward_audio has a power path;
  route 0 (per window) everywhere else -- among them d_model 128 with attention maps asked for, which has no power path, and the
  fused shape at hop 266 with the option off: its frames 1 and T - 1 see the padding and the fused core takes only 0 and T from
  the edge image.
"""
import ctypes as C

import pytest

import seq_assemble_cases as sc
from koemorph_amd import _lib
from koemorph_amd._lib import KoeMorphError

SWITCH_SETS = [{}, {"seq_assemble": 1}, {"seq_assemble": 1, "seq_per_window": 1}, {"seq_per_window": 1},
               {"seq_assemble": 1, "generic_staged": 1}, {"seq_assemble": 1, "no_db_fusion": 1},
               {"seq_assemble": 1, "core128": 1}, {"core128": 1}, {"seq_assemble": 1, "core128": 1, "no_db_fusion": 1},
               {"seq_assemble": 1, "core128": 1, "generic_staged": 1}]


def plan(name, opts, L, stride, B, with_attention=False):
    e = sc.new_engine(name, **opts)
    e.finalize_host()
    try:
        return e.sequence_plan(L, stride, B, with_attention)
    finally:
        e.close()


@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_plan_equals_the_restatement_for_every_switch_set(name):
    L = sc.clip_length(name)
    for opts in SWITCH_SETS:
        e = sc.new_engine(name, **opts)
        e.finalize_host()
        for stride, B in ((1, 1), (3, 2)):
            for wa in (False, True):
                got = e.sequence_plan(L, stride, B, wa)
                assert got == sc.expected_plan(name, opts, L, stride, B, wa), (name, opts, stride, B, wa, got)
        e.close()


def test_edge_frames_per_side():
    assert sc.edges_per_side(533, 256) == 1 and sc.edges_per_side(266, 512) == 2 and sc.edges_per_side(256, 32) == 2
    for name in sc.SHAPES:
        p = plan(name, {}, sc.clip_length(name), 1, 1)
        assert p["edge_frames_per_side"] == (1 if sc.hop_of(name) == 533 else 2) and p["N"] == 8


def test_routes_by_shape_and_switch():
    L = {n: sc.clip_length(n) for n in sc.SHAPES}
    on = {"seq_assemble": 1}
    # option off: route 1 on the fused shape with E = 1 alone
    for name in sc.SHAPES:
        assert plan(name, {}, L[name], 1, 2)["route"] == (1 if name == "fused hop533" else 0), name
    # option on: route 2 wherever the forward call has a power path
    for name in sc.SHAPES:
        want = 0 if name in ("fast", "basic") else 2                      # d_model 128 needs option core128 for its power path
        assert plan(name, on, L[name], 1, 2)["route"] == want, name
    for name in ("fast", "basic"):
        assert plan(name, {**on, "core128": 1}, L[name], 1, 2)["route"] == 2
        assert plan(name, {**on, "core128": 1}, L[name], 1, 2, with_attention=True)["route"] == 0      # no power path with maps
        assert plan(name, {"core128": 1}, L[name], 1, 2)["route"] == 0
    # the maps of the other shapes come from the chain behind the same power-mel workspace
    for name in ("fused hop266", "d256 w512 hop266", "d512 h8", "d64 w32 hop266"):
        assert plan(name, on, L[name], 1, 2, with_attention=True)["route"] == 2, name
    # the switches that take the power path or the shared schedule away
    for name in ("d256 w512 hop266", "d512 h16", "d64 w32 hop533"):
        for off in ("seq_per_window", "generic_staged", "no_db_fusion"):
            assert plan(name, {**on, off: 1}, L[name], 1, 2)["route"] == 0, (name, off)
    assert plan("fused hop533", {**on, "seq_per_window": 1}, L["fused hop533"], 1, 2)["route"] == 0
    assert plan("fused hop533", {"seq_per_window": 1}, L["fused hop533"], 1, 2)["route"] == 0
    assert plan("fused hop266", {**on, "no_db_fusion": 1, "generic_staged": 1}, L["fused hop266"], 1, 2)["route"] == 2


def test_frames_computed():
    """B N (T + 1) per window; B (nfc + 3 E N) assembled, nfc = (N - 1) stride + T + 1."""
    name = "d256 w512 hop266"
    L = sc.clip_length(name)
    assert plan(name, {}, L, 1, 2) == {"route": 0, "N": 8, "stft_frames": 2 * 8 * 513, "edge_frames_per_side": 2}
    assert plan(name, {"seq_assemble": 1}, L, 1, 2) == {"route": 2, "N": 8, "stft_frames": 2 * (520 + 8 * 6), "edge_frames_per_side": 2}
    assert plan(name, {"seq_assemble": 1}, L, 3, 2) == {"route": 2, "N": 3, "stft_frames": 2 * (519 + 3 * 6), "edge_frames_per_side": 2}
    assert plan("fused hop533", {}, sc.clip_length("fused hop533"), 1, 3)["stft_frames"] == 3 * (264 + 2 * 8)
    assert plan("fused hop533", {"seq_assemble": 1}, sc.clip_length("fused hop533"), 1, 3)["stft_frames"] == 3 * (264 + 3 * 8)
    # 20 s at stride 1: 513 frames a window against one pass over the clip
    L20 = 20 * 16000
    a, b = plan(name, {}, L20, 1, 4), plan(name, {"seq_assemble": 1}, L20, 1, 4)
    assert a["N"] == b["N"] == 1203 - 512 + 1 and a["stft_frames"] == 4 * 692 * 513 and b["stft_frames"] == 4 * (1204 + 692 * 6)


def test_a_clip_shorter_than_a_window_is_not_assembled():
    name = "d64 w32 hop266"
    W = 32 * 266
    assert plan(name, {"seq_assemble": 1}, W, 1, 1)["route"] == 2
    assert plan(name, {"seq_assemble": 1}, W - 1, 1, 1) == {"route": 0, "N": 1, "stft_frames": 33, "edge_frames_per_side": 2}


def test_the_switch_is_read_when_the_plan_is_asked_for():
    e = sc.new_engine("d512 h8")
    e.finalize_host()
    L = sc.clip_length("d512 h8")
    assert e.sequence_plan(L)["route"] == 0
    e.set_option("seq_assemble", 1)
    assert e.sequence_plan(L)["route"] == 2
    e.set_option("seq_assemble", 0)
    assert e.sequence_plan(L)["route"] == 0
    e.close()


def test_refusals():
    lib = _lib.load()
    out = (C.c_int64 * 4)()
    e = sc.new_engine("d64 w32 hop533")
    with pytest.raises(KoeMorphError, match="km_finalize_host"):
        e.sequence_plan(20000)
    e.finalize_host()
    assert lib.km_sequence_plan(None, 1, 20000, 1, 0, out) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_sequence_plan(e._h, 1, 20000, 1, 0, None) == _lib.KM_ERR_INVALID_ARG
    for B, L, stride in ((1, 20000, 0), (1, 20000, -1), (0, 20000, 1), (1, 0, 1)):
        assert lib.km_sequence_plan(e._h, B, L, stride, 0, out) == _lib.KM_ERR_INVALID_ARG, (B, L, stride)
    assert lib.km_sequence_plan(e._h, 1, 20000, 1, 0, out) == _lib.KM_OK
    e.close()
