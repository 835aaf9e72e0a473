"""km_clip_plan / Engine.clip_plan names the schedule a resident-clip call runs, on the host alone (after finalize_host, no
device), against the restatement in tests/clip_assemble_cases.py built on koemorph_amd.clip_span.edge_frames:

  route 1 (the default shared route) wherever km_train_step_clip / km_forward_clip run by default, whatever option clip_assemble;
  route 2 (span image + two snippets of 2 E frames per window) only with the option on, on a handle route 1 does not cover, with
  zero padding, T + 1 >= 2 E and the packing front end (training) or a power path (forward);
  route 0 (refused: the wrappers gather) everywhere else.

And the snippet law the edge image rests on: the E frames at either end of a window are, sample for sample, rows of the window's
first and last Ls = (2 E - 1) hop samples cut as dense rows of 2 E frames.
"""
import ctypes as C

import numpy as np
import pytest

import clip_assemble_cases as cc
from koemorph_amd import _lib, clip_span, synth
from koemorph_amd._lib import KoeMorphError

SWITCH_SETS = [{}, {"clip_assemble": 1}, {"clip_assemble": 1, "mel_two_frame": 1}, {"mel_two_frame": 1},
               {"clip_assemble": 1, "generic_staged": 1}, {"clip_assemble": 1, "no_db_fusion": 1},
               {"clip_assemble": 1, "core128": 1}, {"core128": 1}, {"clip_assemble": 1, "core128": 1, "no_db_fusion": 1},
               {"clip_assemble": 1, "train_no_fe_pack": 1}, {"clip_assemble": 1, "train_no_dma": 1}, {"train_no_fe_pack": 1}]
ALL_SWITCHES = sorted({k for s in SWITCH_SETS for k in s})
MODES = (cc.TRAIN, cc.FORWARD, cc.FORWARD_ATTN)


def plan_of(e, B, lo, hi, mode):
    return e.clip_plan(B, lo, hi, training=mode == cc.TRAIN, forward_attention=mode == cc.FORWARD_ATTN)


def with_switches(e, opts):
    for k in ALL_SWITCHES:
        e.set_option(k, int(opts.get(k, 0)))


@pytest.mark.parametrize("hop", list(cc.HOPS))
@pytest.mark.parametrize("name", list(cc.SHAPES))
def test_plan_equals_the_restatement_for_every_switch_set(name, hop):
    e = cc.new_engine(name, hop)
    e.finalize_host()
    for opts in SWITCH_SETS:
        with_switches(e, opts)
        for B, lo, hi in ((1, 0, 0), (4, 0, 9), (9, 3, 40)):
            for mode in MODES:
                got = plan_of(e, B, lo, hi, mode)
                assert got == cc.expected_plan(name, hop, opts, B, lo, hi, mode), (name, hop, opts, B, lo, hi, mode, got)
    e.close()


def test_edges_per_side_and_the_new_helpers():
    assert [cc.edges_per_side(h, 512) for h in (533, 266, 200, 128)] == [1, 2, 3, 4]
    for hop, E in ((533, 1), (266, 2), (200, 3), (128, 4)):
        assert clip_span.edges_per_side(hop) == E and clip_span.snippet_samples(hop, E) == (2 * E - 1) * hop
        for T in (32, 2 * E - 1, 2 * E):
            edges = clip_span.edge_frames(hop, T)
            for f in range(T + 1):
                kind, row = clip_span.edge_source(f, T, E)
                assert (kind != "span") == (f in edges), (hop, T, f)
                if kind == "left":
                    assert row == f < E
                elif kind == "right":
                    assert row == 2 * E - 1 - (T - f) and E <= row < 2 * E
                else:
                    assert row == f == clip_span.frame_source(5, f, 2, T)[1] - 3
    starts = [0, 1, 2, 9]
    assert clip_span.frames_computed_edges(starts, 512, 2) == 522 + 4 * 2 * 4
    assert clip_span.frames_computed_edges([7], 32, 3) == 33 + 12
    # the existing helpers keep their meaning
    assert clip_span.frames_computed(starts, 512, True) == 522 + 8 and clip_span.frames_computed(starts, 512, False) == 4 * 513
    assert clip_span.frame_source(3, 0, 1, 8) == ("edge", 0) and clip_span.frame_source(3, 8, 1, 8) == ("edge", 1)


def test_plan_figures_agree_with_clip_span():
    for name, hop, starts in (("d256 w512", 266, [0, 1, 2, 9]), ("d64 w32", 200, [5, 3, 3, 11, 4]), ("fast", 533, list(range(8)))):
        T = cc.SHAPES[name][2]
        e = cc.new_engine(name, hop, clip_assemble=1, core128=1)
        e.finalize_host()
        E = clip_span.edges_per_side(hop)
        for mode in (cc.TRAIN, cc.FORWARD):
            p = plan_of(e, len(starts), min(starts), max(starts), mode)
            if p["route"] == 2:
                want = clip_span.frames_computed_edges(starts, T, E)
            else:
                want = clip_span.frames_computed(starts, T, p["route"] == 1)
            assert p["stft_frames"] == want and p["span_rows"] == clip_span.n_span(min(starts), max(starts), T), (name, mode, p)
            assert p["edge_frames_per_side"] == E
        e.close()
    # the 60 fps recipe: 8 and 64 stride-1 windows
    e = cc.new_engine("d256 w512", 266, clip_assemble=1)
    e.finalize_host()
    assert plan_of(e, 8, 0, 7, cc.TRAIN) == {"route": 2, "span_rows": 520, "stft_frames": 520 + 64, "edge_frames_per_side": 2}
    assert plan_of(e, 64, 0, 63, cc.FORWARD)["stft_frames"] == 576 + 512
    e.set_option("clip_assemble", 0)
    assert plan_of(e, 8, 0, 7, cc.TRAIN) == {"route": 0, "span_rows": 520, "stft_frames": 8 * 513, "edge_frames_per_side": 2}
    e.close()


def test_routes_by_shape_and_switch():
    on = {"clip_assemble": 1}

    def route(name, hop, opts, mode, reflect=False):
        e = cc.new_engine(name, hop, reflect=reflect, **opts)
        e.finalize_host()
        try:
            return plan_of(e, 4, 0, 9, mode)["route"]
        finally:
            e.close()
    # route 1 wherever the default predicates hold, whatever the option
    for opts in ({}, on):
        assert route("fused", 533, opts, cc.TRAIN) == route("fused", 533, opts, cc.FORWARD) == route("fused", 533, opts, cc.FORWARD_ATTN) == 1
        for name in ("d256 w512", "d512 h8", "fast", "basic", "d64 w32"):
            assert route(name, 533, opts, cc.TRAIN) == 1, name
    # option off: everything else is refused
    for name in cc.SHAPES:
        assert route(name, 266, {}, cc.TRAIN) == route(name, 266, {}, cc.FORWARD) == 0, name
        if name != "fused":
            assert route(name, 533, {}, cc.FORWARD) == 0, name
    # option on: training at every shape below hop n_fft / 2, forward wherever the forward call has a power path
    for name in cc.SHAPES:
        assert route(name, 266, on, cc.TRAIN) == 2, name
        power = name not in ("fast", "basic")
        for hop in (533, 266):
            if (name, hop) != ("fused", 533):
                assert route(name, hop, on, cc.FORWARD) == (2 if power else 0), (name, hop)
    for name in ("fast", "basic"):
        assert route(name, 533, {**on, "core128": 1}, cc.FORWARD) == 2
        assert route(name, 533, {**on, "core128": 1}, cc.FORWARD_ATTN) == 0            # no power path with maps
        assert route(name, 533, {"core128": 1}, cc.FORWARD) == 0
    # reflect padding
    for name, hop in (("d256 w512", 266), ("d64 w32", 533), ("fused", 266)):
        for mode in MODES:
            assert route(name, hop, on, mode, reflect=True) == 0, (name, hop, mode)
    assert route("fused", 533, on, cc.FORWARD, reflect=True) == 0
    # the switches that remove the power path or the packing front end
    for off in ("generic_staged", "no_db_fusion", "mel_two_frame"):
        assert route("d256 w512", 266, {**on, off: 1}, cc.FORWARD) == 0, off
    for off in ("train_no_fe_pack", "train_no_dma", "mel_two_frame"):
        assert route("d256 w512", 266, {**on, off: 1}, cc.TRAIN) == 0, off
        assert route("fused", 533, {**on, off: 1}, cc.TRAIN) == 0, off
    assert route("d256 w512", 266, {**on, "generic_staged": 1}, cc.TRAIN) == 2            # training has no use for the power path


def test_windows_shorter_than_their_edges_are_refused():
    """T + 1 < 2 E: the two ends of a window meet and no frame of it is a clip frame."""
    from koemorph_amd.engine import Engine
    for T, hop, want in ((8, 128, 2), (7, 128, 2), (6, 128, 0), (5, 200, 2), (4, 200, 0), (3, 266, 2), (2, 266, 0)):
        e = Engine(d_model=64, num_heads=4, mel_sequence_length=T, mel=cc.mel_config(hop))
        e.load_state_dict(synth.make_core_params(1, 64, T, 256, "trained"))
        e.set_option("clip_assemble", 1)
        e.finalize_host()
        E = clip_span.edges_per_side(hop)
        assert (T + 1 >= 2 * E) == (want == 2)
        for mode in (cc.TRAIN, cc.FORWARD):
            assert plan_of(e, 3, 0, 5, mode)["route"] == want, (T, hop, mode)
        e.close()


def test_the_switch_is_read_when_the_plan_is_asked_for():
    e = cc.new_engine("d512 h8", 266)
    e.finalize_host()
    assert plan_of(e, 4, 0, 9, cc.TRAIN)["route"] == 0
    e.set_option("clip_assemble", 1)
    assert plan_of(e, 4, 0, 9, cc.TRAIN)["route"] == 2
    e.set_option("clip_assemble", 0)
    assert plan_of(e, 4, 0, 9, cc.TRAIN)["route"] == 0
    e.close()


def test_refusals():
    lib = _lib.load()
    out = (C.c_int64 * 4)()
    e = cc.new_engine("d64 w32", 533)
    with pytest.raises(KoeMorphError, match="km_finalize_host"):
        e.clip_plan(4, 0, 9)
    e.finalize_host()
    assert lib.km_clip_plan(None, 4, 0, 9, 0, out) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_clip_plan(e._h, 4, 0, 9, 0, None) == _lib.KM_ERR_INVALID_ARG
    for B, lo, hi, mode in ((0, 0, 9, 0), (4, -1, 9, 0), (4, 5, 4, 0), (4, 0, 9, 3), (4, 0, 9, -1)):
        assert lib.km_clip_plan(e._h, B, lo, hi, mode, out) == _lib.KM_ERR_INVALID_ARG, (B, lo, hi, mode)
    assert lib.km_clip_plan(e._h, 4, 0, 9, 1, out) == _lib.KM_OK
    with pytest.raises(KoeMorphError, match="unknown option"):
        e.set_option("clip_assembled", 1)
    e.close()


@pytest.mark.parametrize("hop", list(cc.HOPS))
def test_the_snippet_law(hop):
    """Frames 0 .. E - 1 and T - E + 1 .. T of a window, cut in float64 from the window with zero padding, against the rows
    edge_source names in the two Ls-sample snippets cut the same way as dense rows of 2 E frames: the same samples, hence the
    same spectra.  Every (hop, T) of the plan test plus the smallest T (T + 1 = 2 E) and the one above."""
    E = clip_span.edges_per_side(hop)
    Ls = clip_span.snippet_samples(hop, E)
    for T in sorted({s[2] for s in cc.SHAPES.values()} | {2 * E - 1, 2 * E}):
        window = synth.make_audio(1000 + T, 1, T * hop)[0]
        assert Ls <= T * hop and 1 + Ls // hop == 2 * E
        frames = cc.centred_frames(window, hop, T + 1)
        rows = {"left": cc.centred_frames(window[:Ls], hop, 2 * E), "right": cc.centred_frames(window[T * hop - Ls:], hop, 2 * E)}
        edges = clip_span.edge_frames(hop, T)
        assert edges == list(range(E)) + list(range(T - E + 1, T + 1))
        for f in edges:
            kind, row = clip_span.edge_source(f, T, E)
            assert kind in rows
            assert np.array_equal(frames[f], rows[kind][row]), (hop, T, f)
            assert np.array_equal(cc.stft_power(frames[f]), cc.stft_power(rows[kind][row]))
        # ... and a frame that is no edge frame sees no padding: it is a frame of the clip the window was cut from
        for f in {E, T - E} - set(edges):
            assert clip_span.edge_source(f, T, E) == ("span", f)
            assert np.array_equal(frames[f], window[f * hop - 512:f * hop + 512].astype(np.float64))
