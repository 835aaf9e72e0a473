"""km_koemorph_rollout on the host alone: the window law against a brute force, km_koemorph_rollout_plan against the restatement in
tests/rollout_cases.py (route by width, T, emotion_dim % 16 and option kmm_no_fuse; chunk and short-frame counts; launches;
workspace), every refusal that needs no device with its text, and the ValueErrors of KoeMorphModel.render."""
import ctypes as C

import pytest
import torch

import rollout_cases as rc
from koemorph_amd import _lib
from oracle import koemorph_model as okm


@pytest.mark.parametrize("T", [1, 3, 9, 30, 32])
def test_window_law_equals_brute_force(T):
    for F in sorted({1, 2, max(T - 1, 1), T, T + 1, 3 * T}):
        for first in sorted({0, 1, T - 2, T - 1, F - 1}):
            if not 0 <= first < F:
                continue
            law = rc.window_law(F, T, first)
            assert law == rc.window_brute(F, T, first), (F, T, first)
            assert len(law) == F - first and all(1 <= ti <= T and s >= 0 and s + ti <= F for s, ti in law)
            assert all(s + ti - 1 == first + n for n, (s, ti) in enumerate(law))        # the window ends on its own frame


CONFIGS = {
    "default": okm.KoeMorphConfig(),
    "emotion32": okm.KoeMorphConfig(emotion_dim=32),
    "emotion25": okm.KoeMorphConfig(emotion_dim=25),
    "d64": okm.KoeMorphConfig(**rc.SMALL),
    "one_layer": okm.KoeMorphConfig(num_encoder_layers=1, num_attention_layers=2, decoder_layers=1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_plan_equals_the_restatement(name):
    cfg = CONFIGS[name]
    h = rc.HostHandle(cfg)
    try:
        for no_fuse in (0, 1):
            h.set_option("kmm_no_fuse", no_fuse)
            for T in (1, 3, 30, 32, 33, 40):
                for B, F in ((1, 1), (3, 11), (2, 40), (1, 300), (5, T - 1 if T > 1 else 1), (2, T), (2, 3 * T)):
                    for first in sorted({0, 1, T - 2, T - 1, F - 1}):
                        if not 0 <= first < F:
                            continue
                        got = h.plan(B, F, T, first)
                        assert got == rc.expected_plan(cfg, B, F, T, first, no_fuse=bool(no_fuse)), (name, no_fuse, B, F, T, first, got)
        h.set_option("kmm_no_fuse", 0)
        # the routes by name: width, T, emotion_dim % 16
        want = 1 if name in ("default", "emotion32", "one_layer") else 0
        assert h.plan(2, 40, 30, 0)["route"] == want
        assert h.plan(2, 80, 40, 0)["route"] == 0
        if want:
            p = h.plan(1, 1800, 30, 0)
            assert p["short_frames"] == 29 and p["chunks"] == -(-(1800 - 29) // rc.DEFAULT_CHUNK) and p["launches"] == 4 * 29 + 3 * p["chunks"]
            assert h.plan(1, 1800, 30, 29)["short_frames"] == 0
            last = h.plan(1, 1800, 30, 1799)
            assert (last["chunks"], last["short_frames"], last["launches"]) == (1, 0, 3)
    finally:
        h.close()


def _refused(lib, rcode, code, *needles):
    assert rcode == code, (rcode, lib.km_last_error())
    text = lib.km_last_error().decode()
    for n in needles:
        assert n in text, text


def test_refusals_name_the_entry_point_and_the_value():
    h = rc.HostHandle(okm.KoeMorphConfig())
    lib = h.lib
    out5 = (C.c_int64 * 5)()
    p = C.c_void_p(64)                      # never dereferenced: every call below is refused first
    try:
        call = lambda **kw: lib.km_koemorph_rollout(kw.get("h", h.h), kw.get("mel", p), kw.get("emo", p), kw.get("B", 2), kw.get("F", 40),
                                                    kw.get("T", 30), kw.get("first", 0), None, None, 1, kw.get("out", p), None, None)
        inv = _lib.KM_ERR_INVALID_ARG
        _refused(lib, call(h=None), inv, "km_koemorph_rollout", "NULL handle")
        _refused(lib, call(mel=None), inv, "km_koemorph_rollout", "mel_dev is NULL")
        _refused(lib, call(emo=None), inv, "km_koemorph_rollout", "emotion_dev is NULL")
        _refused(lib, call(out=None), inv, "km_koemorph_rollout", "out_dev is NULL")
        _refused(lib, call(B=0), inv, "km_koemorph_rollout", "B 0 < 1")
        _refused(lib, call(F=0), inv, "km_koemorph_rollout", "F 0 < 1")
        _refused(lib, call(T=-2), inv, "km_koemorph_rollout", "T -2 < 1")
        _refused(lib, call(first=40), inv, "km_koemorph_rollout", "first_frame 40 outside 0 .. 39")
        _refused(lib, call(first=-1), inv, "km_koemorph_rollout", "first_frame -1 outside 0 .. 39")
        # valid arguments, but nothing was uploaded: the call stops before it touches the device
        _refused(lib, call(), _lib.KM_ERR_NOT_FINALIZED, "km_finalize")
        _refused(lib, lib.km_koemorph_rollout_reserve(h.h, 0, 30, 256), inv, "km_koemorph_rollout_reserve", "max_clips 0 < 1")
        _refused(lib, lib.km_koemorph_rollout_reserve(h.h, 2, 0, 256), inv, "km_koemorph_rollout_reserve", "max_context 0 < 1")
        _refused(lib, lib.km_koemorph_rollout_reserve(h.h, 2, 30, 0), inv, "km_koemorph_rollout_reserve", "chunk_frames 0 < 1")
        _refused(lib, lib.km_koemorph_rollout_reserve(None, 2, 30, 256), inv, "km_koemorph_rollout_reserve", "NULL handle")
        _refused(lib, lib.km_koemorph_rollout_plan(h.h, 2, 40, 30, 0, None), inv, "km_koemorph_rollout_plan", "NULL argument")
        _refused(lib, lib.km_koemorph_rollout_plan(h.h, 0, 40, 30, 0, out5), inv, "km_koemorph_rollout_plan", "B 0 < 1")
        _refused(lib, lib.km_koemorph_rollout_plan(h.h, 2, 0, 30, 0, out5), inv, "km_koemorph_rollout_plan", "F 0 < 1")
        _refused(lib, lib.km_koemorph_rollout_plan(h.h, 2, 40, 0, 0, out5), inv, "km_koemorph_rollout_plan", "T 0 < 1")
        _refused(lib, lib.km_koemorph_rollout_plan(h.h, 2, 40, 30, 40, out5), inv, "km_koemorph_rollout_plan", "first_frame 40 outside 0 .. 39")
        # a handle of another kind
        from koemorph_amd.engine import Engine
        e = Engine(d_model=64, num_heads=4, mel_sequence_length=32)
        try:
            _refused(lib, call(h=e._h), inv, "km_koemorph_rollout", "not a KoeMorphModel handle")
            _refused(lib, lib.km_koemorph_rollout_reserve(e._h, 2, 30, 256), inv, "km_koemorph_rollout_reserve", "not a KoeMorphModel handle")
            _refused(lib, lib.km_koemorph_rollout_plan(e._h, 2, 40, 30, 0, out5), inv, "km_koemorph_rollout_plan", "not a KoeMorphModel handle")
        finally:
            e.close()
    finally:
        h.close()


def test_plan_before_finalize_host_is_refused():
    lib = _lib.load()
    m = rc.torch_model(okm.KoeMorphConfig(**rc.SMALL))
    h = C.c_void_p()
    cfg = m._c_config()
    _lib.check(lib.km_koemorph_create(C.byref(cfg), C.byref(h)))
    try:
        _refused(lib, lib.km_koemorph_rollout_plan(h, 2, 40, 30, 0, (C.c_int64 * 5)()), _lib.KM_ERR_NOT_FINALIZED, "km_koemorph_rollout_plan")
    finally:
        lib.km_destroy(h)


def test_render_value_errors_come_before_any_device_work():
    m = rc.torch_model(okm.KoeMorphConfig(emotion_dim=32))
    audio = torch.zeros(1, 19200)                      # 1.2 s: 36 rows at 30 fps
    with pytest.raises(ValueError, match="40 wide.*emotion_dim is 32"):
        m.render(audio, emotion_rows=torch.zeros(1, 36, 40))
    with pytest.raises(ValueError, match="36 mel rows but 35 emotion rows"):
        m.render(audio, emotion_rows=torch.zeros(1, 35, 25))
    with pytest.raises(ValueError, match=r"expected emotion rows \(B, F, n\)"):
        m.render(audio, emotion_rows=torch.zeros(36, 25))
    padded = m._pad_emotion_rows(torch.ones(2, 7, 25), 32)
    assert padded.shape == (2, 7, 32) and bool((padded[..., :25] == 1).all()) and bool((padded[..., 25:] == 0).all())
    same = torch.ones(2, 7, 32)
    assert m._pad_emotion_rows(same, 32) is same
    with pytest.raises(ValueError, match="expected rows of 80 and 32 features"):
        m.rollout(torch.zeros(1, 5, 80), torch.zeros(1, 5, 25))
    with pytest.raises(ValueError, match="first_frame 5 outside 0 .. 4"):
        m.rollout(torch.zeros(1, 5, 80), torch.zeros(1, 5, 32), first_frame=5)
    m.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        m.render(audio)
    with pytest.raises(RuntimeError, match="eval-mode"):
        m.rollout(torch.zeros(1, 5, 80), torch.zeros(1, 5, 32))
