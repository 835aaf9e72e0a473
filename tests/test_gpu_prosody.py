"""The `basic` prosodic emotion features on the device (km_prosody_*, koemorph_amd.features.BasicEmotion) against the float64
restatement of tests/prosody_cases.py.  PARITY UNPINNED: the restatement has not been checked against librosa itself.

Exact: the crossing rate of every frame (a count over 2048), the index i* of every frame (tests/test_prosody_host.py asserts that
no decision behind it is within 1e-4 of flipping), max and min.  The window's zcr is a mean of exact values and may differ by the
rounding of the mean alone: F * 2^-24 * zcr.  Everything else -- C_f, the period 40 + i* + shift, f0_f, energy, mean, the two
deviations, the window means of C_f and f0_f -- is held to 8 x the largest error of the float32 NumPy evaluation of the same
restatement on the same input, floored at 2^-22 relative (``prosody_cases.bound``).  The period is read back from the record's f0
as 16000 / f0 in float64, so its figure includes the rounding of f0 to float32.
"""
import functools

import numpy as np
import pytest
import torch

import prosody_cases as pc
from koemorph_amd import _lib
from koemorph_amd.features import BasicEmotion

pytestmark = pytest.mark.gpu
PAD = 37                                   # the rows of the B = 3 calls lie in a matrix this much wider: a row stride that is not L
OUT = {name: k for k, name in enumerate(pc.FEATURE_NAMES)}


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def engine():
    return BasicEmotion("cuda")


@functools.lru_cache(maxsize=None)
def run(L: int, B: int) -> dict:
    """kind -> (out (9), frames (F, 4)).  B = 3: the three kinds as the rows of ONE call on a strided view; B = 1: a call per kind."""
    be = engine()
    rows = np.stack([pc.signal(k, L) for k in pc.KINDS])
    if B == 3:
        wide = torch.zeros(3, L + PAD, device="cuda")
        wide[:, :L] = torch.from_numpy(rows).cuda()
        view = wide[:, :L]
        assert view.stride(0) == L + PAD
        out, fr = be(view).cpu().numpy(), be.frames(view).cpu().numpy()
        return {k: (out[i], fr[i]) for i, k in enumerate(pc.KINDS)}
    res = {}
    for i, k in enumerate(pc.KINDS):
        x = torch.from_numpy(rows[i:i + 1].copy()).cuda()
        res[k] = (be(x)[0].cpu().numpy(), be.frames(x)[0].cpu().numpy())
    return res


CASES = [(L, B) for L in pc.LENGTHS for B in (1, 3)]


@pytest.mark.parametrize("L,B", CASES)
def test_exact_quantities(L, B):
    for kind in pc.KINDS:
        out, fr = run(L, B)[kind]
        o = pc.oracle(kind, L)
        F = pc.num_frames(L)
        assert fr.shape == (F, 4) and engine().num_frames(L) == F
        assert np.array_equal(bits(fr[:, 0]), bits(o["Z"].astype(np.float32))), (kind, "Z_f")
        assert np.array_equal(fr[:, 3].astype(np.int64), o["istar"]), (kind, "i*", fr[:, 3], o["istar"])
        assert out[OUT["max"]] == o["out"][OUT["max"]] and out[OUT["min"]] == o["out"][OUT["min"]], kind
        zcr = o["out"][OUT["zcr"]]
        assert abs(float(out[OUT["zcr"]]) - zcr) <= F * 2.0 ** -24 * zcr, (kind, "zcr")


@pytest.mark.parametrize("L,B", CASES)
def test_bounded_quantities(L, B):
    worst = {}
    for kind in pc.KINDS:
        out, fr = run(L, B)[kind]
        o = pc.oracle(kind, L)
        got = {"C": fr[:, 1].astype(np.float64), "f0": fr[:, 2].astype(np.float64), "period": pc.SR / fr[:, 2].astype(np.float64)}
        for key, g in got.items():
            frac = np.abs(g - o[key]) / pc.bound(kind, L, key)
            worst[key] = max(worst.get(key, 0.0), float(frac.max()))
        b = pc.bound(kind, L, "out")
        for name in ("energy", "spectral_centroid", "f0_mean", "f0_std", "mean", "std"):
            k = OUT[name]
            err = abs(float(out[k]) - o["out"][k])
            frac = err / b[k] if b[k] > 0 else (0.0 if err == 0 else float("inf"))
            worst[name] = max(worst.get(name, 0.0), frac)
    print(f"L={L} B={B}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("L", pc.LENGTHS)
def test_rows_of_one_call_are_the_rows_of_separate_calls_and_a_second_run_gives_the_same_bits(L):
    for kind in pc.KINDS:
        (o1, f1), (o3, f3) = run(L, 1)[kind], run(L, 3)[kind]
        assert np.array_equal(bits(o1), bits(o3)) and np.array_equal(bits(f1), bits(f3)), kind
    x = torch.from_numpy(np.stack([pc.signal(k, L) for k in pc.KINDS])).cuda()
    a, b = engine()(x), engine()(x)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.array_equal(bits(a.cpu().numpy()), bits(np.stack([run(L, 3)[k][0] for k in pc.KINDS])))


def test_silence_and_a_constant_row():
    """Silence reproduces the oracle's nine values and every frame record exactly.  Of a constant 0.5 row, what is exactly
    representable is reproduced exactly: energy, zcr, mean, std, max, min, the crossing rate and i* of every frame, and f0 = 400
    on the frames that hold no padding (their difference function is exactly 0).  Its centroid goes through a float32 FFT of
    0.5 x Hann and the frames at the edges through the cumulative mean of a step's difference function: those follow the bound of
    the other tests, they cannot be bit-equal to a float64 evaluation."""
    be = engine()
    z = torch.zeros(1, 3000, device="cuda")
    o = pc.analyse(np.zeros(3000, np.float32))
    assert np.array_equal(bits(be(z)[0].cpu().numpy()), bits(o["out"].astype(np.float32)))
    assert be(z)[0].tolist() == [0, 0, 0, 400, 0, 0, 0, 0, 0]
    fr = be.frames(z)[0].cpu().numpy()
    assert np.array_equal(fr, np.tile(np.float32([0, 0, 400, 0]), (6, 1)))
    L = 5000
    y = np.full(L, 0.5, np.float32)
    o, y32 = pc.analyse(y), pc.analyse(y, np.float32)
    out, fr = be(torch.from_numpy(y[None]).cuda())[0].cpu().numpy(), be.frames(torch.from_numpy(y[None]).cuda())[0].cpu().numpy()
    for name in ("energy", "zcr", "mean", "std", "max", "min"):
        assert out[OUT[name]] == np.float32(o["out"][OUT[name]]), name
    assert out[OUT["energy"]] == 0.25 and out[OUT["mean"]] == 0.5 and out[OUT["std"]] == 0 and out[OUT["zcr"]] == 0
    assert np.array_equal(fr[:, 0], o["Z"].astype(np.float32)) and np.array_equal(fr[:, 3].astype(np.int64), o["istar"])
    inner = slice(2, pc.num_frames(L) - 2)                     # frames 2 .. 7 of 10 read samples 0 .. 4607 and no padding
    assert (fr[inner, 2] == 400).all() and (o["f0"][inner] == 400).all()
    for key, col in (("C", 1), ("f0", 2)):
        b = np.maximum(8.0 * np.abs(y32[key].astype(np.float64) - o[key]).max(), 2.0 ** -22 * np.abs(o[key]))
        assert (np.abs(fr[:, col].astype(np.float64) - o[key]) <= b).all(), key


def test_windows_of_a_resident_clip():
    be = engine()
    clip_np = np.concatenate([pc.signal("chirp", 16000)[:6000], pc.signal("vibrato", 16000)[:5000]])
    n, L = len(clip_np), 5000
    clip = torch.from_numpy(clip_np.copy()).cuda()
    starts = [0, 1, 533, n - L, n - 7, n]
    got = be.windows(clip, torch.tensor(starts, dtype=torch.int32, device="cuda"), L).cpu().numpy()
    assert got.shape == (len(starts), 9)
    for w, s in enumerate(starts):
        win = clip[s:s + L]
        if win.numel() == 0:
            assert not got[w].any() and not np.signbit(got[w]).any()
            continue
        assert win.numel() == min(L, n - s)
        want = be(win[None].clone())[0].cpu().numpy()
        assert np.array_equal(bits(got[w]), bits(want)), (w, s)
    assert not np.array_equal(bits(got[0]), bits(got[1]))
    with pytest.raises(ValueError, match="int32"):
        be.windows(clip, torch.tensor(starts, device="cuda"), L)
    with pytest.raises(ValueError, match="samples"):
        be(torch.zeros(1, (1 << 20) + 1, device="cuda"))


def test_the_longest_window():
    """2^20 samples, 2049 frames: the last sample index and the last frame the entry point accepts."""
    L = 1 << 20
    x = torch.from_numpy(np.tile(pc.signal("vibrato", 16000), 66)[:L].copy()).cuda()
    fr = engine().frames(x[None])[0]
    out = engine()(x[None])[0]
    assert fr.shape == (2049, 4)
    assert torch.equal(out[7], x.max()) and torch.equal(out[8], x.min())
    assert abs(float(out[5]) - float(x.double().mean())) <= 2.0 ** -22 * abs(float(x.double().mean())) + 1e-12
    assert torch.isfinite(fr).all() and (fr[:, 2] >= 16000 / 321).all() and (fr[:, 2] <= 16000 / 39).all()


def test_device_memory_returns_to_its_baseline():
    lib = _lib.load()
    torch.cuda.synchronize()
    base = lib.km_live_device_bytes()
    be = BasicEmotion("cuda")
    assert lib.km_live_device_bytes() == base + 4 * (2048 + 2048)
    be(torch.zeros(2, 1000, device="cuda"))
    torch.cuda.synchronize()
    be.close()
    assert lib.km_live_device_bytes() == base
