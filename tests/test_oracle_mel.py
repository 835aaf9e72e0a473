"""oracle/mel.py is PARITY UNPINNED by the reference (librosa / torchaudio absent, no mel
fixtures in the reference).  These tests cross-check its building blocks against the
independent pure-numpy implementation in transformers.audio_utils, and check the
frame-count quirks SURVEY.md section 7 lists."""
import numpy as np
import pytest

from koemorph_amd import synth
from oracle import mel

au = pytest.importorskip("transformers.audio_utils")


def test_slaney_filterbank_matches_transformers():
    fb = mel.mel_filterbank_librosa(16000, 1024, 80, 80.0, 8000.0)           # (80, 513)
    ref = au.mel_filter_bank(num_frequency_bins=513, num_mel_filters=80, min_frequency=80.0,
                             max_frequency=8000.0, sampling_rate=16000, norm="slaney",
                             mel_scale="slaney").T
    np.testing.assert_allclose(fb, ref, atol=1e-7, rtol=1e-5)
    fb512 = mel.mel_filterbank_librosa(16000, 512, 80, 80.0, 8000.0)
    ref512 = au.mel_filter_bank(257, 80, 80.0, 8000.0, 16000, norm="slaney", mel_scale="slaney").T
    np.testing.assert_allclose(fb512, ref512, atol=1e-7, rtol=1e-5)


def test_htk_filterbank_matches_transformers():
    fb = mel.mel_filterbank_torchaudio(257, 80.0, 8000.0, 80, 16000)           # (257, 80)
    ref = au.mel_filter_bank(257, 80, 80.0, 8000.0, 16000, norm=None, mel_scale="htk")
    np.testing.assert_allclose(fb, ref, atol=1e-6, rtol=1e-5)


def test_power_to_db_matches_transformers():
    S = np.abs(synth.normal(3, (257, 80))).astype(np.float32) ** 2 + 1e-12
    mine = mel.power_to_db(S)
    ref = au.power_to_db(S, reference=float(S.max()), min_value=1e-10, db_range=80.0)
    np.testing.assert_allclose(mine, ref, atol=2e-4)


def test_stft_power_matches_transformers_spectrogram():
    y = synth.make_audio(5, 1, 16000)[0]
    P = mel.stft_power(y, 1024, 533, center=True, pad_mode="constant", precision="f64")
    ref = au.spectrogram(y.astype(np.float64), window=mel.hann_periodic(1024), frame_length=1024,
                         hop_length=533, fft_length=1024, power=2.0, center=True,
                         pad_mode="constant", onesided=True).T
    assert P.shape == ref.shape
    np.testing.assert_allclose(P, ref, rtol=1e-6, atol=1e-9 * ref.max())


def test_frame_count_quirks():
    # 136448-sample window -> 257 frames; the last 3 are taken BEFORE the core truncates to 256
    y = synth.make_audio(1, 1, 136448)[0]
    long, short = mel.mel_batch_window(y)
    assert long.shape == (257, 80) and short.shape == (3, 80)
    assert np.array_equal(short, long[254:257])
    assert long.max() == pytest.approx(1.0) and long.min() >= 0.0
    # real-time ring: 136000 samples, hop 532 -> 256 frames -> truncated to int(8.5/0.0333)=255
    y2 = synth.make_audio(2, 1, 136000)[0]
    db = mel.mel_sliding_window(y2)
    assert db.shape == (255, 80) and db.max() == 0.0 and db.min() >= -80.0
    # torchaudio path: 136000 samples -> 256 raw frames -> int(8.5*30) = 255 kept
    lm = mel.mel_torchaudio(y2)
    assert lm.shape == (1, 255, 80)
    # 60 fps hop is int(16000/60) = 266
    assert mel.num_frames(512 * 266, 1024, 266) == 513


def test_ref_precision_close_to_f64():
    y = synth.make_audio(7, 1, 136448)[0]
    a, _ = mel.mel_batch_window(y, precision="ref")
    b, _ = mel.mel_batch_window(y, precision="f64")
    assert np.max(np.abs(a - b)) < 5e-5


def test_batch_window_db_constants():
    """mel_batch_window's top_db / db_add / db_scale (km_mel_config's dB constants): the defaults are today's (db + 80) / 80 bit for
    bit, and other values follow (max(db, max - top_db) + db_add) * db_scale -- the oracle of the training tests' MelConfig cases."""
    y = synth.make_audio(11, 1, 136448)[0]
    y[60000:] *= 1e-3                                                      # a quiet half: more than 80 dB below the loud frames
    fb = mel.mel_filterbank_librosa(16000, 1024, 80, 80.0, 8000.0)
    P = mel.stft_power(y, 1024, 533, center=True, pad_mode="constant")
    m = (P.astype(np.float32) @ fb.T.astype(np.float32)).astype(np.float32)
    raw = mel.power_to_db(m, top_db=None)                                  # 10 log10(S / max S), no clamp
    base = (mel.power_to_db(m) + np.float32(80)) / np.float32(80)
    for kw in ({}, dict(top_db=80.0, db_add=80.0)):
        long, short = mel.mel_batch_window(y, **kw)
        assert long.dtype == np.float32 and np.array_equal(long, base) and np.array_equal(short, base[-3:])
    assert raw.min() < -80.0                                               # the clamps below are exercised
    for top_db, db_add, db_scale in ((60.0, 80.0, 1.0 / 80.0), (80.0, 80.0, -1.0 / 80.0), (60.0, 80.0, -1.0 / 80.0), (50.0, 0.0, 1.0)):
        long, short = mel.mel_batch_window(y, top_db=top_db, db_add=db_add, db_scale=db_scale)
        want = (np.maximum(raw.astype(np.float64), -top_db) + db_add) * db_scale
        np.testing.assert_allclose(long, want, rtol=1e-6, atol=1e-6 * abs(db_add * db_scale) + 1e-7)
        assert np.array_equal(short, long[-3:])
        lim = (db_add - top_db) * db_scale                                 # the clamped value: a floor for db_scale > 0, a ceiling below
        assert (long.min() if db_scale > 0 else long.max()) == pytest.approx(lim, abs=1e-6)
    # a short clip: fewer than 3 frames, the short rows are zero-filled after the frames there are (as with the defaults)
    long, short = mel.mel_batch_window(y[:533], top_db=60.0, db_scale=-1.0 / 80.0)
    assert long.shape == (2, 80) and np.array_equal(short[:2], long) and not short[2].any()
    # mel_batch passes them on
    lb, sb = mel.mel_batch(synth.make_audio(12, 2, 20000), top_db=60.0)
    assert lb.min() == pytest.approx(0.25, abs=1e-6) and sb.shape == (2, 3, 80)


# ---- mel_power / mel_power_error: the linear-power oracle of tests/test_gpu_mel_power.py -----------------------------------
# Pinned to things the helper did not compute itself (closed forms of the periodic Hann window), and shown to be the same
# oracle the dB tests use (power_to_db of its "ref" path is mel_batch_window / mel_sliding_window / mel_torchaudio, bit for bit).
MEL_VARIANTS = [dict(), dict(n_fft=512, hop=266, mel_scale="htk", slaney_norm=False, n_mels=40, f_min=0.0, f_max=8000.0)]


@pytest.mark.parametrize("kw", MEL_VARIANTS)
def test_mel_power_unit_impulse_at_a_frame_centre(kw):
    """x = delta at t0 * hop: frame t0 sees it at n_fft/2, where the periodic Hann window is exactly 1, so |X_k|^2 = 1
    for every k and the mel row is the filters' row sums."""
    n_fft, hop = kw.get("n_fft", 1024), kw.get("hop", 533)
    assert mel.hann_periodic(n_fft)[n_fft // 2] == 1.0
    y = np.zeros(12 * hop, np.float32)
    y[5 * hop] = 1.0
    P, aux = mel.mel_power(y, precision="f64", return_aux=True, **kw)
    want = aux["fb"].astype(np.float64).sum(axis=1)
    assert aux["spec_peak"][5] == pytest.approx(1.0, rel=1e-12) and want.min() > 0
    np.testing.assert_allclose(P[5], want, rtol=1e-12)
    np.testing.assert_allclose(mel.mel_power(y, precision="f32", **kw)[5], want, rtol=2e-6)
    np.testing.assert_allclose(mel.mel_power(y, precision="ref", **kw)[5], want, rtol=2e-6)


@pytest.mark.parametrize("kw", MEL_VARIANTS)
@pytest.mark.parametrize("k0,A", [(37, 1.0), (200, 0.25)])
def test_mel_power_cosine_on_an_exact_bin(kw, k0, A):
    """A cos(2 pi k0 n / N) under the periodic Hann window: P[k0] = (A N / 4)^2, P[k0 +- 1] = (A N / 8)^2, nothing else."""
    N, hop = kw.get("n_fft", 1024), kw.get("hop", 533)
    y = A * np.cos(2.0 * np.pi * k0 * np.arange(20 * hop) / N + 0.3)           # float64 samples: no input rounding
    S = mel.stft_power(y, N, hop, precision="f64")[4:12]                        # interior frames
    want_S = np.zeros(N // 2 + 1)
    want_S[k0], want_S[k0 - 1], want_S[k0 + 1] = (A * N / 4) ** 2, (A * N / 8) ** 2, (A * N / 8) ** 2
    np.testing.assert_allclose(S, np.tile(want_S, (8, 1)), rtol=1e-10, atol=1e-20 * want_S.max())
    P, aux = mel.mel_power(y, precision="f64", return_aux=True, **kw)
    want = aux["fb"].astype(np.float64) @ want_S
    assert want.max() > 0
    np.testing.assert_allclose(P[4:12], np.tile(want, (8, 1)), rtol=1e-10, atol=1e-20 * want.max())
    e, dead = mel.mel_power_error(mel.mel_power(y.astype(np.float32), precision="f32", **kw)[4:12], np.tile(want, (8, 1)),
                                  np.full(8, want_S.max()), aux["fb"])
    assert dead == 0 and e.max() < 8 * mel.MEL_POWER_U, e.max()


def test_mel_power_constant_signal():
    """x = c: bins 0 and 1 only, (c N / 2)^2 and (c N / 4)^2; f_min = 0 so that the first filters see bin 1."""
    c, N = 0.75, 1024
    y = np.full(12 * 533, c)
    P, aux = mel.mel_power(y, precision="f64", f_min=0.0, return_aux=True)
    fb = aux["fb"].astype(np.float64)
    want = fb[:, 0] * (c * N / 2) ** 2 + fb[:, 1] * (c * N / 4) ** 2
    assert want.max() > 0 and np.count_nonzero(want) < 5
    np.testing.assert_allclose(P[3:9], np.tile(want, (6, 1)), rtol=1e-10, atol=1e-18 * want.max())
    np.testing.assert_allclose(aux["spec_peak"][3:9], (c * N / 2) ** 2, rtol=1e-12)


@pytest.mark.parametrize("n_fft,window_norm", [(1024, False), (512, True)])
def test_mel_power_parseval(n_fft, window_norm):
    """One 'filter' with the weights (1, 2, ..., 2, 1) turns the mel product into the full-spectrum energy, which is
    N sum (x w)^2 (divided by sum w^2 under window normalisation)."""
    hop = 300
    y = synth.make_audio(9, 1, 9000, "uniform")[0]
    ones = np.full((1, n_fft // 2 + 1), 2.0, np.float32)
    ones[0, 0] = ones[0, -1] = 1.0
    w = mel.hann_periodic(n_fft)
    yp = np.pad(y.astype(np.float64), n_fft // 2)
    for prec, rtol in (("f64", 1e-12), ("f32", 1e-5), ("ref", 1e-5)):
        P = mel.mel_power(y, n_fft=n_fft, hop=hop, window_norm=window_norm, precision=prec, fb=ones)
        assert P.shape == (31, 1)
        for t in (0, 7, 30):
            want = n_fft * np.sum((yp[t * hop:t * hop + n_fft] * w) ** 2) / (np.sum(w * w) if window_norm else 1.0)
            assert P[t, 0] == pytest.approx(want, rel=rtol), (prec, t)


def test_mel_power_is_the_oracle_of_the_db_tests():
    y = synth.make_audio(5, 2, 30000)
    long, _ = mel.mel_batch_window(y[0])
    db = mel.power_to_db(mel.mel_power(y[0], precision="ref"))
    assert np.array_equal(long, (db + np.float32(80)) / np.float32(80))
    long64, _ = mel.mel_batch_window(y[0], precision="f64")
    assert np.array_equal(long64, (mel.power_to_db(mel.mel_power(y[0], precision="f64")) + 80.0) / 80.0)
    for kw in (dict(), dict(n_fft=1024, hop=533)):
        n_fft, hop = kw.get("n_fft", 512), kw.get("hop", 532)
        m = mel.mel_power(y[1], n_fft=n_fft, hop=hop, f_max=8000.0, pad_mode="reflect", precision="ref")
        F = m.shape[0]
        got = mel.mel_sliding_window(y[1], context_window=F * 0.0333 + 1e-6, **kw)
        assert got.shape[0] == F and np.array_equal(got, mel.power_to_db(m))
    fbt = mel.mel_filterbank_torchaudio(257, 80.0, 8000.0, 80, 16000)
    for use_fb in (fbt.T, None):           # torchaudio's own filters, and librosa's HTK ones (the same to rounding)
        m = mel.mel_power(y[1], n_fft=512, hop=533, mel_scale="htk", slaney_norm=False, pad_mode="reflect",
                          window_norm=True, precision="ref", fb=use_fb)
        want = mel.mel_torchaudio(y[1])[0]                                    # truncated to int(L / sr * fps) rows
        got = np.log(m + np.float32(1e-8))[:want.shape[0]]
        if use_fb is not None:
            assert np.array_equal(got, want)
        else:
            np.testing.assert_allclose(np.exp(got), np.exp(want), rtol=1e-5)


def test_mel_power_defaults_and_f32_pipeline():
    y = synth.make_audio(6, 1, 20000)[0]
    # the "f32" branch of stft_power is float32 throughout; the other two are untouched by it
    assert mel.stft_power(y, 1024, 533, precision="f32").dtype == np.float32
    assert mel.stft_power(y, 1024, 533).dtype == np.float32 and mel.stft_power(y, 1024, 533, precision="f64").dtype == np.float64
    assert mel.mel_power(y, precision="f32").dtype == np.float32
    P64, aux = mel.mel_power(y, precision="f64", return_aux=True)
    e, dead = mel.mel_power_error(mel.mel_power(y, precision="f32"), P64, aux["spec_peak"], aux["fb"])
    assert dead == 0 and 1e-8 < e.max() < 2e-6                                # the yardstick's scale (speech: ~2e-7)
    assert mel.mel_power_error(P64, P64, aux["spec_peak"], aux["fb"])[0].max() == 0.0
    # a 0.1 % error planted on the largest entry is three orders above the yardstick
    bad = P64.copy()
    bad[np.unravel_index(np.argmax(P64), P64.shape)] *= 1.001
    assert mel.mel_power_error(bad, P64, aux["spec_peak"], aux["fb"])[0].max() > 1e-4


def test_mel_power_error_zero_frames():
    z = np.zeros(20000, np.float32)
    z[10000] = 1.0
    P64, aux = mel.mel_power(z, precision="f64", return_aux=True)
    e, dead = mel.mel_power_error(P64, P64, aux["spec_peak"], aux["fb"])
    assert dead == 36 and P64.shape[0] == 38 and e.max() == 0.0
    bad = P64.copy()
    bad[0, 3] = 1e-30                                                          # a silent frame must be EXACTLY zero
    assert np.isinf(mel.mel_power_error(bad, P64, aux["spec_peak"], aux["fb"])[0][0, 3])
