"""The resampler's filter, integer laws and Python state mirror, and the C side's refusals (no GPU)."""
import ctypes as C

import numpy as np
import pytest

import resample_cases as rc
from koemorph_amd import _lib
from koemorph_amd.features import resample as rs


@pytest.mark.parametrize("rate_in", (48000, 44100, 32000, 22050, 11025, 8000))
def test_filter_and_oracle_against_scipy(rate_in):
    signal = pytest.importorskip("scipy.signal")
    up, down, h, half_len = rc.plan(rate_in)
    assert half_len == 10 * max(up, down) and h.shape == (2 * half_len + 1,)
    want = signal.firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert np.abs(h - want).max() <= 1e-14
    x = rc.signal(11, 700)
    y, _ = rc.oracle(x, rate_in)
    ref = signal.resample_poly(x.astype(np.float64), up, down)
    assert y.shape == ref.shape == (rs.n_out(700, up, down),)
    assert np.abs(y - ref).max() <= 1e-14


def test_ratio_and_filter_shapes():
    assert rs.resample_ratio(48000, 16000) == (1, 3)
    assert rs.resample_ratio(44100, 16000) == (160, 441)
    assert rs.resample_ratio(11025, 16000) == (640, 441)
    assert rs.resample_ratio(8000, 16000) == (2, 1)
    assert rc.plan(48000)[2].size == 61 and rc.plan(44100)[2].size == 8821 and rc.plan(11025)[2].size == 12801
    for rate_in in rc.LAW_RATES:
        up, _, h, half_len = rc.plan(rate_in)
        assert np.array_equal(h, h[::-1]) or np.abs(h - h[::-1]).max() < 1e-15           # linear phase
        assert abs(h.sum() - up) < 1e-12


def test_clip_lengths_cross_one_output_tile():
    for rate_in in rc.CLIP_RATES:
        up, down, _, _ = rc.plan(rate_in)
        lengths = rc.clip_lengths(rate_in)
        assert lengths[0] == 1 and lengths[-1] == 5000 and len(set(lengths)) == len(lengths)
        assert any(rs.CLIP_TILE < rs.n_out(n, up, down) <= rs.CLIP_TILE + up for n in lengths)


@pytest.mark.parametrize("rate_in", (48000, 8000))
def test_vectorised_oracle_is_the_output_law(rate_in):
    up, down, h, half_len = rc.plan(rate_in)
    x = rc.signal(12, 97)
    y, bound = rc.oracle(x, rate_in)
    assert np.abs(y - rc.oracle_direct(x, up, down, h, half_len)).max() <= 1e-15
    assert np.all(bound >= 0)


@pytest.mark.parametrize("rate_in", rc.LAW_RATES)
def test_emitted_against_brute_force(rate_in):
    up, down, _, half_len = rc.plan(rate_in)
    for n in list(range(0, 200)) + [1023, 1024, 1600, 4999]:
        assert rs.emitted(n, up, down, half_len) == rc.emitted_brute(n, up, down, half_len), n
        assert rs.emitted(n, up, down, half_len) <= rs.n_out(n, up, down)


@pytest.mark.parametrize("rate_in", rc.LAW_RATES)
def test_stream_plan_chunk_by_chunk(rate_in):
    up, down, _, half_len = rc.plan(rate_in)
    p = rs.StreamPlan(up, down, half_len)
    assert p.history == -(-2 * half_len // up)
    sizes = [rc.CHUNK_SIZES[i] for i in (3, 0, 1, 2, 4, 5, 1, 1, 0, 3, 5, 4, 2, 2, 1)]
    total = out = 0
    for n in sizes:
        out += p.push(n)
        total += n
        assert out == rs.emitted(total, up, down, half_len), (n, total)
        assert p.d == out * down + half_len - total * up
        assert 0 <= p.d <= half_len + down
    out += p.flush()
    assert out == rs.n_out(total, up, down)
    assert p.d == half_len and p.push(0) == 0 and p.flush() == 0          # a flushed stream is a fresh one


def test_stream_plan_tail_is_the_last_samples():
    up, down, _, half_len = rc.plan(48000)
    p = rs.StreamPlan(up, down, half_len)
    x = rc.signal(13, 300)
    pos = 0
    for n in (7, 1, 160, 60, 72):
        p.push(n, x[pos:pos + n])
        pos += n
        want = np.concatenate([np.zeros(p.history, np.float32), x[:pos]])[-p.history:]
        assert np.array_equal(p.tail, want)


@pytest.mark.parametrize("rate_in", rc.LAW_RATES)
def test_stream_plan_over_2_to_the_40_samples(rate_in):
    """Whole periods of `down` inputs give exactly `up` outputs and leave d where it was, so the 2^40 samples are walked as a few
    thousand real pushes between jumps of many periods; d is all the state there is."""
    up, down, _, half_len = rc.plan(rate_in)
    p = rs.StreamPlan(up, down, half_len)
    total = out = 0
    sizes = (1600, 1, 7, 160, 1024, 0)
    step = 0
    while total < 2 ** 40:
        for _ in range(40):
            n = sizes[step % len(sizes)]
            step += 1
            out += p.push(n)
            total += n
            assert 0 <= p.d <= half_len + down
        before = p.d
        assert p.push(down) == up and p.d == before          # one period: the law the jump relies on
        periods = 2 ** 33 // down
        total += down * (periods + 1)
        out += up * (periods + 1)
        assert out == rs.emitted(total, up, down, half_len)
    assert total >= 2 ** 40 and p.d < 2 ** 31


def _create(n_streams, up, down, taps):
    lib = _lib.load()
    h = C.c_void_p()
    taps = np.ascontiguousarray(taps, np.float64)
    code = lib.km_resampler_create(C.byref(h), n_streams, up, down, taps.ctypes.data_as(C.POINTER(C.c_double)), taps.size)
    return lib, code, h


def test_create_refuses_bad_arguments():
    up, down, h, _ = rc.plan(48000)
    lib, code, handle = _create(1, up, down, h[:-1])                      # even n_taps
    assert code == _lib.KM_ERR_INVALID_ARG and not handle.value and b"odd" in lib.km_last_error()
    lib, code, handle = _create(1, 3, 3, h)                               # up == down
    assert code == _lib.KM_ERR_INVALID_ARG and not handle.value and b"up == down" in lib.km_last_error()
    lib, code, handle = _create(0, up, down, h)
    assert code == _lib.KM_ERR_INVALID_ARG and not handle.value
    lib, code, handle = _create(1, 0, down, h)
    assert code == _lib.KM_ERR_INVALID_ARG and not handle.value
    big_up, big_down = rs.resample_ratio(16001, 16000)                    # 16000 phases: no LDS holds that table
    taps, _ = rs.resample_filter(big_up, big_down)
    lib, code, handle = _create(1, big_up, big_down, taps)
    assert code == _lib.KM_ERR_UNSUPPORTED and not handle.value and b"LDS" in lib.km_last_error()
    lib, code, handle = _create(1, 1, 40, rs.resample_filter(1, 40)[0])   # a small table, but one tile's input span is too long
    assert code == _lib.KM_ERR_UNSUPPORTED and not handle.value
    with pytest.raises(ValueError):
        rs._check_rate_pair(16000, 16000)


def test_null_handles_are_refused():
    lib = _lib.load()
    v = C.c_int64()
    assert lib.km_resampler_out_max(None, 10, C.byref(v)) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_resampler_push(None, None, 1, None, None, 1, None, None) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_resampler_flush(None, None, None, 1, None, None) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_resampler_reset_streams(None, None, None) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_resample_clip(None, None, 1, None, 1, None) == _lib.KM_ERR_INVALID_ARG
    assert lib.km_resampler_destroy(None) == _lib.KM_OK
