"""The argument refusals of km_attn_stats_update_masked, km_attn_stats_streams_* and km_stream_tick_attn / km_stream_step_attn
that need no device, and the layout of the per-stream output.  No GPU.

Every refusal checked here is made before the accumulator is looked at or anything is allocated, so a stand-in pointer (the address
of a host buffer that is never dereferenced) is enough where the call needs a non-NULL accumulator."""
import ctypes as C
import os
import re

import numpy as np

import attn_stats_cases as ac
from koemorph_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["km_attn_stats_update_masked", "km_attn_stats_streams_create", "km_attn_stats_streams_destroy", "km_attn_stats_streams_update",
           "km_attn_stats_streams_reset", "km_attn_stats_streams_compute", "km_stream_tick_attn", "km_stream_step_attn"]


def refused(rc, text):
    return rc == _lib.KM_ERR_INVALID_ARG and text in _lib.load().km_last_error()


def test_library_exports_the_new_entry_points():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "koemorph.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES and re.search(r"\bint %s\(" % s, header), s


def test_masked_update_refusals():
    lib = _lib.load()
    stand_in = (C.c_double * 8)()                         # never dereferenced: the checks below come first
    acc, maps, mask = C.addressof(stand_in), 4096, 8192   # "pointers": only their NULL-ness and alignment are looked at
    assert refused(lib.km_attn_stats_update_masked(None, maps, mask, 4, None), b"km_attn_stats_update_masked: bad argument")
    assert refused(lib.km_attn_stats_update_masked(acc, maps, mask, -1, None), b"bad argument")
    assert refused(lib.km_attn_stats_update_masked(acc, maps, mask, 2 ** 31, None), b"bad argument")
    assert refused(lib.km_attn_stats_update_masked(acc, None, mask, 4, None), b"NULL maps or mask")
    assert refused(lib.km_attn_stats_update_masked(acc, maps, None, 4, None), b"NULL maps or mask")
    assert refused(lib.km_attn_stats_update_masked(acc, maps + 4, mask, 4, None), b"16-byte aligned")
    assert lib.km_attn_stats_update_masked(acc, None, None, 0, None) == _lib.KM_OK          # no rows: nothing to do, as update


def test_per_stream_refusals():
    lib = _lib.load()
    out = C.c_void_p()
    assert refused(lib.km_attn_stats_streams_create(None, 4, 28, 80), b"NULL argument")
    for n_streams, q, k in ((0, 28, 80), (-3, 28, 80), (65536, 28, 80)):
        assert refused(lib.km_attn_stats_streams_create(C.byref(out), n_streams, q, k), b"streams (1 .. 65535)"), n_streams
    for q, k in ((0, 80), (28, 0), (28, 78), (28, 260), (5000, 80)):                       # a bad shape, as km_attn_stats_create
        assert refused(lib.km_attn_stats_streams_create(C.byref(out), 4, q, k), b"keys: a multiple of 4 up to 256"), (q, k)
    assert not out.value
    stand_in = (C.c_double * 8)()
    acc, maps, mask = C.addressof(stand_in), 4096, 8192
    assert refused(lib.km_attn_stats_streams_update(None, maps, mask, None), b"km_attn_stats_streams_update: NULL argument")
    assert refused(lib.km_attn_stats_streams_update(acc, None, mask, None), b"NULL argument")
    assert refused(lib.km_attn_stats_streams_update(acc, maps, None, None), b"NULL argument")
    assert refused(lib.km_attn_stats_streams_update(acc, maps + 8, mask, None), b"16-byte aligned")
    assert refused(lib.km_attn_stats_streams_reset(None, None, None), b"NULL accumulator")
    assert refused(lib.km_attn_stats_streams_compute(None, maps, None), b"NULL argument")
    assert refused(lib.km_attn_stats_streams_compute(acc, None, None), b"NULL argument")
    assert lib.km_attn_stats_streams_destroy(None) == _lib.KM_OK


def test_stream_attention_calls_refuse_a_null_handle_as_tick_and_step_do():
    lib = _lib.load()
    rc_tick = lib.km_stream_tick(None, 4096, 4096, None, None)
    msg_tick = lib.km_last_error()
    assert lib.km_stream_tick_attn(None, 4096, 4096, None, 4096, 4096, None) == rc_tick != _lib.KM_OK and lib.km_last_error() == msg_tick
    rc_step = lib.km_stream_step(None, 4096, 4096, None, None, None, None)
    msg_step = lib.km_last_error()
    assert lib.km_stream_step_attn(None, 4096, 4096, None, None, None, 4096, 4096, None) == rc_step != _lib.KM_OK
    assert lib.km_last_error() == msg_step


def test_per_stream_output_layout():
    """km_attn_stats_streams_compute writes one KM_ATTN_STATS_COUNT(Q, K) vector per stream, stream-major; before any update the
    Python accumulator returns one all-zero dict per stream without touching a device."""
    text = open(os.path.join(ROOT, "include", "koemorph.h")).read()
    assert re.search(r"km_attn_stats_streams_compute\s+out_dev \(n_streams, KM_ATTN_STATS_COUNT\(Q, K\)\) float64", text)
    n = _lib.km_attn_stats_count(ac.Q, ac.K)
    assert n == ac.count() == 1 + 2 * ac.Q * ac.K + ac.Q
    per_stream = [ac.stats_f64(ac.make_maps(60 + s, s + 1)) for s in range(3)]
    flat = np.stack([ac.pack(st) for st in per_stream])                                    # what the device lays out
    assert flat.shape == (3, n)
    for s, st in enumerate(per_stream):
        got = metrics.unpack_attention_stats(flat[s], ac.Q, ac.K)
        assert got["rows"] == s + 1 and np.array_equal(got["mean_map"], st["mean_map"]) and np.array_equal(got["peak_hist"], st["peak_hist"])
    acc = metrics.StreamAttentionStats(3)
    zero = acc.compute()
    assert len(zero) == 3 and all(z["rows"] == 0 and not z["mean_map"].any() and set(z) >= {"band_mean", "band_share"} for z in zero)
    acc.reset()                                                                             # no device state yet: nothing to do
