"""km_koemorph_audio_* on the host alone: km_koemorph_audio_schedule (the function the advance kernel runs) against a brute force
that walks samples through a ring, km_koemorph_audio_plan against the restatement in tests/koemorph_audio_cases.py, every refusal
that needs no device with its text, the shape errors of ``push`` and the argument parsing of scripts/rt_koemorph.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import koemorph_audio_cases as ac
import lld_cases as lc
import rollout_cases as rc
from koemorph_amd import _lib
from koemorph_amd.streaming import check_samples, koemorph_audio_plan
from oracle import koemorph_model as okm

PUSHES = (1, 159, 160, 533, 534, 1600, 0)


def schedule(lib, n0, pushed, hop, W, ring_len, origin, stream=0):
    out = (C.c_int64 * 10)()
    _lib.check(lib.km_koemorph_audio_schedule(n0, pushed, hop, W, ring_len, origin, stream, out))
    return [int(v) for v in out]


@pytest.mark.parametrize("fps", [30, 60, 25, 50])
def test_schedule_equals_the_brute_force(fps):
    """Pushes of 1, 159, 160, 533, 534, 1600 and 0 samples in turn, through a growing window, a wrapped one (three times round the
    ring) and a reset mid-way: first frame, frame count, a0, len, nf, m and the window's place in the ring."""
    lib = _lib.load()
    hop, W, M = ac.hop_of(fps), 8000, 1600
    ring_len = W + M
    assert hop == {30: 533, 60: 266, 25: 640, 50: 320}[fps]
    brute = ac.BruteStream(hop, W, ring_len)
    n, origin, k, seen = 0, 0, 0, set()
    did_reset = False
    while n < 3 * ring_len or not did_reset:
        if not did_reset and n > ring_len + 3000:                 # once, with the window wrapped and the ring's write position mid-way
            brute.reset()
            origin, n, did_reset = (origin + n) % ring_len, 0, True
            assert origin == brute.origin != 0
        p = PUSHES[k % len(PUSHES)]
        k += 1
        got = schedule(lib, n, p, hop, W, ring_len, origin, stream=5)
        first, rows, a0, length, nf, m, start = brute.push(p)
        assert got == ac.entry(n, p, hop, W, ring_len, origin, stream=5), (fps, n, p)
        assert got[0] == first and got[1] == rows and got[6] == brute.n
        if rows:
            assert got[2:6] == [a0, length, nf, m], (fps, n, p)
            assert (a0, length, m, nf) == ac.window(brute.n, W)
            if nf:
                assert got[7:] == [5, start, nf]
                seen.add("wrapped" if a0 > 0 else "growing")
                if start + length > ring_len:
                    seen.add("straddles")
                # every new row's frame coordinate lies inside the window (what the creation check on W buys)
                j = np.floor(np.arange(first, first + rows) * hop / 160.0).astype(np.int64) - m
                assert j.min() >= 0
            else:
                assert got[7:] == [-1, 0, 0] and length < 960
                seen.add("short")
        else:
            assert got[2:6] == [0, 0, 0, 0] and got[7:] == [-1, 0, 0]
            seen.add("no frame")
        n += p
    assert seen == {"wrapped", "growing", "straddles", "short", "no frame"}, seen


def test_mel_frames_of_the_brute_force_read_their_own_samples():
    """frame_samples (the restated addressing of kma_mel_rows_kernel): frame k reads samples k * hop - 256 .. k * hop + 255 of the life,
    mirrored at sample 0, and they are in the ring when the frame is due."""
    hop, W, M = 533, 8000, 1600
    b = ac.BruteStream(hop, W, W + M)
    b.push(777)
    b.reset()
    frames = 0
    for p in ac.chunks(12000, 1024):
        first, rows, *_ = b.push(p)
        for k in range(first, first + rows):
            assert [b.ring[i] for i in b.frame_samples(k)] == [(1, abs(k * hop - 256 + i)) for i in range(512)], k
            frames += 1
    assert frames == 12000 // hop


def test_shifted_grid_is_the_dense_grid_moved_by_m():
    """With hop = 16000 / fps exact (fps 25 and 50) the shifted grid at m = 0 is lld_cases.grid; any m moves j and keeps w."""
    for fps, nf in ((25, 45), (50, 45)):
        hop = ac.hop_of(fps)
        T = 10
        j0, w0, e0 = lc.grid(nf, T, fps)
        j1, w1, e1 = ac.grid(nf, np.arange(T), hop, 0)
        assert np.array_equal(j0, j1) and np.array_equal(w0, w1) and np.array_equal(e0, e1)
        j2, w2, _ = ac.grid(nf, np.arange(T) + 40, hop, 40 * hop // 160)
        assert np.array_equal(j2, j1) and np.array_equal(w2, w1)
    j, w, exact = ac.grid(45, np.arange(3, 9), 533, 5)
    assert np.array_equal(j, np.floor(np.arange(3, 9) * 533 / 160).astype(int) - 5) and not exact.any()
    j, w, exact = ac.grid(10, [0, 1, 40], 533, 2)                             # before the window: frame 0; past it: the last frame
    assert j.tolist() == [0, 1, 9] and exact.tolist() == [True, False, True]
    lld = np.arange(20.0).reshape(10, 2) + 1.0
    lld[4, 1] = 0.0
    # rows 1 and 2 at hop 533 lie at p = 3.33 and 6.66: between frames 3 | 4 and 6 | 7.  Column 1 is smoothed over non-zero values
    # and frame 4 holds a 0 there: row 1 takes the nearer frame (3), everything else blends
    rows, a, b, blend = ac.resample_columns(lld, [1, 2], 533, 0, np.array([False, True]))
    j, w, _ = ac.grid(10, [1, 2], 533, 0)
    assert j.tolist() == [3, 6] and w[0] < 0.5 < w[1]
    assert blend.tolist() == [[True, False], [True, True]] and rows[0, 1] == lld[3, 1]
    assert rows[1, 0] == lld[6, 0] + float(np.float32(w[1])) * (lld[7, 0] - lld[6, 0])


PLAN_CASES = [(1, 30, 0.5, 533), (3, 30, 0.5, 1600), (4, 60, 2.0, 1024), (2, 25, 20.0, 16000)]


@pytest.mark.parametrize("N,fps,seconds,max_samples", PLAN_CASES)
def test_plan_equals_the_restatement(N, fps, seconds, max_samples):
    h = rc.HostHandle(okm.KoeMorphConfig(emotion_dim=32))
    try:
        got = koemorph_audio_plan(h.lib, h.h, N, fps, seconds, max_samples)
        want = ac.expected_plan(N, fps, seconds, max_samples)
        assert got == want
        assert got["window_samples"] >= max_samples + got["hop"] + 1120 and got["ring_len"] >= got["window_samples"] + max_samples
        assert got["max_rows"] == max_samples // got["hop"] + 1 and got["window_frames"] <= 2048
    finally:
        h.close()
    assert ac.expected_plan(3, 30, 0.5, 1600)["window_frames"] == 45 and ac.expected_plan(4, 60, 2.0, 1024)["hop"] == 266


def _refused(lib, rcode, code, *needles):
    assert rcode == code, (rcode, lib.km_last_error())
    text = lib.km_last_error().decode()
    for n in needles:
        assert n in text, text


def test_refusals_name_the_entry_point_and_the_value():
    h = rc.HostHandle(okm.KoeMorphConfig(emotion_dim=32))
    lib = h.lib
    inv, uns, who = _lib.KM_ERR_INVALID_ARG, _lib.KM_ERR_UNSUPPORTED, "km_koemorph_audio_create"
    out8 = (C.c_int64 * 8)()
    p = C.c_void_p(64)                      # never dereferenced: every call below is refused first
    try:
        create = lambda hh=h.h, N=3, fps=30.0, win=2.0, M=1600, fs=0: lib.km_koemorph_audio_create(hh, N, fps, win, M, fs)
        plan = lambda **kw: koemorph_audio_plan(lib, h.h, kw.get("N", 3), kw.get("fps", 30.0), kw.get("win", 2.0), kw.get("M", 1600))
        _refused(lib, create(hh=None), inv, who, "NULL handle")
        _refused(lib, create(N=0), inv, who, "n_streams 0 < 1")
        _refused(lib, create(fs=2), inv, who, "feature set 2")
        _refused(lib, create(fps=62.5), uns, who, "hop 256", "fps 62.5", "at least 257")
        _refused(lib, create(fps=9.0), uns, who, "fps 9", "at least 10")
        _refused(lib, create(win=0.2, M=1600), inv, who, "3200 samples", "max_samples + hop + 1120 = 3253")
        _refused(lib, create(win=21.0, M=1600), uns, who, "2095 frames", "at most 2048")
        _refused(lib, create(M=0), inv, who, "max_samples 0")
        _refused(lib, create(fps=float("nan")), inv, who, "fps nan")
        assert plan(fps=62.5)["supported"] == 0 and b"km_koemorph_audio_plan: hop 256" in lib.km_last_error()
        assert plan(fps=9.0)["supported"] == 0 and plan(win=21.0)["supported"] == 0
        assert plan(fps=60.0, M=1024)["supported"] == 1                       # hop 266 is served
        assert plan(win=20.0)["supported"] == 1                               # 1995 frames
        _refused(lib, lib.km_koemorph_audio_plan(h.h, 0, 30.0, 2.0, 1600, 0, out8), inv, "km_koemorph_audio_plan", "n_streams 0 < 1")
        _refused(lib, lib.km_koemorph_audio_plan(h.h, 3, 30.0, 0.2, 1600, 0, out8), inv, "km_koemorph_audio_plan", "3200 samples")
        _refused(lib, lib.km_koemorph_audio_plan(h.h, 3, 30.0, 2.0, 1600, 0, None), inv, "km_koemorph_audio_plan", "out is NULL")
        # a supported shape, but nothing was uploaded: the call stops before it touches the device
        _refused(lib, create(), _lib.KM_ERR_NOT_FINALIZED, "km_finalize")
        # no engine was created on this handle
        _refused(lib, lib.km_koemorph_audio_rows(h.h, p, 533, None, p, p, p, None), inv, "km_koemorph_audio_rows", "no audio engine")
        _refused(lib, lib.km_koemorph_audio_reset(h.h, None, None), inv, "km_koemorph_audio_reset", "no audio engine")
        _refused(lib, lib.km_koemorph_audio_samples(h.h, p, None), inv, "km_koemorph_audio_samples", "no audio engine")
        assert lib.km_koemorph_audio_destroy(h.h) == _lib.KM_OK                # nothing to free
        out10 = (C.c_int64 * 10)()
        _refused(lib, lib.km_koemorph_audio_schedule(0, 533, 0, 8000, 9600, 0, 0, out10), inv, "km_koemorph_audio_schedule", "hop 0")
        _refused(lib, lib.km_koemorph_audio_schedule(-1, 533, 533, 8000, 9600, 0, 0, out10), inv, "km_koemorph_audio_schedule", "-1 samples before")
        _refused(lib, lib.km_koemorph_audio_schedule(0, 533, 533, 8000, 9600, 9600, 0, out10), inv, "km_koemorph_audio_schedule", "origin 9600")
        from koemorph_amd.engine import Engine
        e = Engine(d_model=64, num_heads=4, mel_sequence_length=32)
        try:
            _refused(lib, create(hh=e._h), inv, who, "not a KoeMorphModel handle")
            _refused(lib, lib.km_koemorph_audio_rows(e._h, p, 533, None, p, p, p, None), inv, "km_koemorph_audio_rows", "not a KoeMorphModel handle")
        finally:
            e.close()
    finally:
        h.close()
    # a model whose emotion rows cannot hold the descriptors
    h = rc.HostHandle(okm.KoeMorphConfig(emotion_dim=16))
    try:
        _refused(h.lib, h.lib.km_koemorph_audio_create(h.h, 3, 30.0, 2.0, 1600, 0), uns, who, "emotion_dim 16", "25 descriptors")
        _refused(h.lib, h.lib.km_koemorph_audio_create(h.h, 3, 30.0, 2.0, 1600, 1), uns, who, "emotion_dim 16", "18 descriptors")
    finally:
        h.close()


def test_push_shape_errors_come_before_any_device_work():
    check = lambda x, counts=None: check_samples(3, 1600, x, counts)
    check(torch.zeros(3, 1)); check(torch.zeros(3, 1600), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"expected \(3, M\) samples, got \(2, 533\)"):
        check(torch.zeros(2, 533))
    with pytest.raises(ValueError, match=r"expected \(3, M\) samples"):
        check(torch.zeros(533))
    with pytest.raises(ValueError, match="1601 samples per stream.*1 .. 1600"):
        check(torch.zeros(3, 1601))
    with pytest.raises(ValueError, match="0 samples per stream"):
        check(torch.zeros(3, 0))
    with pytest.raises(ValueError, match="int32 counts"):
        check(torch.zeros(3, 533), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="int32 counts"):
        check(torch.zeros(3, 533), torch.zeros(4, dtype=torch.int32))


def test_the_scripts_arguments_are_rt_pys():
    from koemorph_amd.scripts import rt, rt_koemorph
    mine, theirs = rt_koemorph.build_parser(), rt.build_parser()
    flags = lambda p: {s for a in p._actions for s in a.option_strings}
    assert flags(theirs) <= flags(mine) and flags(mine) - flags(theirs) == {"--emotion_window"}
    args = mine.parse_args(["--model_path", "m.pt", "--input_audio", "a.wav", "--output_json", "o.jsonl", "--target_fps", "60"])
    assert args.target_fps == 60.0 and args.chunk_size == 1024 and args.emotion_window == 2.0 and args.output_mode == "udp"
    assert args.input_audio == "a.wav" and args.output_json == "o.jsonl" and args.sample_rate == 16000
    for name in ("RingBuffer", "AudioCapture", "BlendshapeStreamer", "AudioFileReader"):
        assert getattr(rt_koemorph, name) is getattr(rt, name)
    with pytest.raises(SystemExit):
        mine.parse_args([])                                                   # --model_path is required, as in rt.py
    with pytest.raises(ValueError, match="16 kHz"):
        rt_koemorph.KoeMorphRealTime(None, sample_rate=44100, model=object())
