"""The four create entry points of the emotion back ends (km_emotion_stream_create, km_emotion_stream_create_basic,
km_emotion_clip_create, km_emotion_clip_create_basic) refuse one table of bad arguments before any device call: return code, a
null handle and the whole text, with the name each entry point says (both stream entry points say km_emotion_stream_create).
No GPU.
"""
import ctypes as C

import pytest

from koemorph_amd import _lib

INVALID, UNSUPPORTED = _lib.KM_ERR_INVALID_ARG, _lib.KM_ERR_UNSUPPORTED

# entry point -> (the name its texts carry, is it the basic back end, is it a clip object)
ENTRY_POINTS = {"km_emotion_stream_create": ("km_emotion_stream_create", False, False),
                "km_emotion_stream_create_basic": ("km_emotion_stream_create", True, False),
                "km_emotion_clip_create": ("km_emotion_clip_create", False, True),
                "km_emotion_clip_create_basic": ("km_emotion_clip_create_basic", True, True)}

# (context, interval) -> refusal, whatever the object and the back end; the counts are good
TIMING = [((0.5, 0.3), INVALID, "Context window must be at least 1.0 seconds"),
          ((float("nan"), 0.3), INVALID, "Context window must be at least 1.0 seconds"),
          ((1.0, 0.05), INVALID, "Update interval must be at least 0.1 seconds"),
          ((1.0, float("nan")), INVALID, "Update interval must be at least 0.1 seconds"),
          ((1.0, 1.5), INVALID, "Update interval cannot be larger than context window"),
          ((3601.0, 0.3), UNSUPPORTED, "context window of 3601 s")]
# the frame limit of each back end: (context, interval) -> text on eGeMAPS, text on basic (None: no refusal, so not called here)
FRAMES = [((20.6, 0.3), "2055 frames per window, at most 2048 (20.5 s)", None),
          ((66.0, 0.3), "6595 frames per window, at most 2048 (20.5 s)", "a window of 1056000 samples, at most 1048576 (65.5 s)")]


def _call(lib, entry, clip, ctx, itv, counts):
    h = C.c_void_p(1)
    fn = getattr(lib, entry)
    rc = fn(C.byref(h), ctx, itv, counts[0]) if clip else fn(C.byref(h), counts[0], ctx, itv, counts[1])
    return rc, h.value, lib.km_last_error().decode()


@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_create_refuses_bad_arguments_before_any_device_call(entry):
    lib = _lib.load()
    name, basic, clip = ENTRY_POINTS[entry]
    good = (4,) if clip else (4, 2)
    fn = getattr(lib, entry)
    assert (fn(None, 1.0, 0.1, 4) if clip else fn(None, 4, 1.0, 0.1, 2)) == INVALID
    assert lib.km_last_error().decode() == f"{name}: NULL argument"
    cases = [(a, good, rc, text) for a, rc, text in TIMING]
    cases += [(a, good, UNSUPPORTED, b if basic else e) for a, e, b in FRAMES if (b if basic else e) is not None]
    # the object's own counts, and which refusal wins when two apply: the seconds' own checks come before max_slots / max_updates,
    # the limits of the kernels after them; n_streams comes first of all
    if clip:
        cases += [((1.0, 0.1), (0,), INVALID, "max_slots 0, 1 .. 65535"), ((1.0, 0.1), (65536,), INVALID, "max_slots 65536, 1 .. 65535"),
                  ((0.5, 0.3), (0,), INVALID, "Context window must be at least 1.0 seconds"),
                  ((1.0, 1.5), (0,), INVALID, "Update interval cannot be larger than context window"),
                  ((3601.0, 0.3), (0,), INVALID, "max_slots 0, 1 .. 65535"), ((66.0, 0.3), (65536,), INVALID, "max_slots 65536, 1 .. 65535")]
    else:
        cases += [((1.0, 0.1), (0, 1), INVALID, "n_streams 0, 1 .. 4096"), ((1.0, 0.1), (4097, 1), INVALID, "n_streams 4097, 1 .. 4096"),
                  ((1.0, 0.1), (4, 0), INVALID, "max_updates 0, 1 .. n_streams (4)"), ((1.0, 0.1), (4, 5), INVALID, "max_updates 5, 1 .. n_streams (4)"),
                  ((0.5, 0.3), (0, 1), INVALID, "n_streams 0, 1 .. 4096"),
                  ((0.5, 0.3), (4, 5), INVALID, "Context window must be at least 1.0 seconds"),
                  ((1.0, 1.5), (4, 0), INVALID, "Update interval cannot be larger than context window"),
                  ((3601.0, 0.3), (4, 5), INVALID, "max_updates 5, 1 .. n_streams (4)"), ((66.0, 0.3), (4, 0), INVALID, "max_updates 0, 1 .. n_streams (4)")]
    for (ctx, itv), counts, rc, text in cases:
        got = _call(lib, entry, clip, ctx, itv, counts)
        assert got == (rc, None, f"{name}: {text}"), (entry, ctx, itv, counts, got)
