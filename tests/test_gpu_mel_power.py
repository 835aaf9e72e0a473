"""The log-mel front end pinned in LINEAR power against the float64 oracle, on every kernel path and edge.

tests/test_gpu_mel.py compares after the logarithm (0.04 dB ~ 1 % of a bin's power, and nothing at all more than 80 dB under
the window maximum).  Here every case reads the kernels' power-mel rows themselves and compares them with
``oracle.mel.mel_power(..., precision="f64")`` by ``oracle.mel.mel_power_error``:

    S = max_k |X64[t,k]|^2 * max_k fb[m,k],  u = 2^-23,  e[t,m] = |P - P64| / (sqrt(P64 S) + u S)

THE BOUND: max e of the GPU <= 8 x max(yardstick, u), the yardstick being max e of the plain float32 pipeline
(``precision="f32"``: numpy's float32 rFFT, float32 products) on the same input and configuration, computed in the test.
Reason for 8: a radix-2 float32 FFT of 1024 points has a worst-case error of about log2(N) u ~ 10 u per bin against the 1-3 u
pocketfft shows in practice, the kernel's table twiddles and its summation order in the mel product add small constants, and
anything actually wrong (a twiddle off by 1e-4, a bin paired with the wrong partner, a weight in the wrong slot) lands at 1e-3
or worse.  The factor was fixed before the first GPU run.

HOW THE POWER IS READ.  The C ABI has no linear output; ``log_mode = KM_LOG_LN_EPS`` returns log(mel + log_eps) in float32.
``LOG_EPS = 2^-100`` (7.9e-31): a normal float32 whose logarithm is exact in the kernel (log2 = -100), so a row of zero power
comes back as exactly ``ZERO_LOG`` and is checked for that; and far below every power of interest -- the smallest scale S of any
case here is ~1e-11 (the 1e-6 tones), so log_eps changes e by less than 1e-12 (each case asserts log_eps < 1e-9 u S_min).
exp() of a float32 logarithm is NOT the power to float32 accuracy, though: a value y = ln P carries an absolute rounding
error of up to ~|y| 2^-23 (the hardware log2 is good to an ulp of ITS result, |log2 P| up to 30 here), which is a RELATIVE error
of the same size on P = exp(y): 7e-7 at P = 1e3, 1.3e-6 at P = 1e-9 -- as large as the bound itself, and nothing to do with the
FFT or the filters.  So the read-out goes through powers of two: float32 arithmetic is exactly homogeneous under them, the
kernel computes mel(2^-k x) = 4^-k mel(x) bit for bit (short of under/overflow), and for every entry the launch is repeated on
2^-k x with k = round(log2(P) / 2), which brings that entry into [1/2, 2] where |ln P| < 0.7 and the read-out error is < 1e-7
relative (below u, so it cannot eat the factor 8).  ``gpu_power`` assembles P = 4^k exp(y_k) entry by entry and asserts that each
rescaled value agrees with the direct read-out y_0 - 2 k ln 2 to the direct read-out's own rounding, so a kernel that was NOT
homogeneous would fail there.  Entries more than 1e-25 below their frame's largest are left at the direct read-out (their
contribution to e is < 1e-12) so that the rescaled launches cannot overflow, and so are entries below 1e3 log_eps (as P - log_eps).
The hop cases run on an Engine of their own: km_reserve sizes the workspace rows for the smallest hop among the plans a
handle has seen (an upper bound by design), so a hop-1 plan on the handle that also runs 1100 windows would ask for 136 449
frames per window.  That allocation failure is how test_failed_workspace_growth_leaves_other_launches_working was found.

CASES (all through ``Engine.mel_extract``; production configuration = n_fft 1024, hop 533, 80 Slaney bins 80-8000 Hz, zero padding)
  signals      B = 3, L = 136 448: speech, uniform noise, on-/off-bin tones at 1, 1e-3, 1e-6, clicks (mid-frame and on a frame
               boundary), DC 0.9 + 1e-4 tone, chirp, full-scale square wave, silence, a silent window between loud ones
  closed forms unit impulse at a frame centre (mel row = filter row sums) and an on-bin cosine ((A N/4)^2, (A N/8)^2) against the
               formulas, so a fault shared by oracle and kernel is caught too
  geometry     B in {1, 31, 32, 40, 100, 256, 511, 600, 1100} at L = 40 000 (76 frames = 4 chunks of 16 + a ragged one of 12;
               per_window = 5 (= n_chunks: one chunk each, no walk) up to B = 100, then 2, 1, 1, 1 workgroups for 5 chunks) and
               B in {32, 40, 100, 170, 256} at L = 136 448 (17 chunks for 16, 13, 5, 3, 2 workgroups: the chunk_ctr walk with
               several workgroups racing); every window compared, and bit-identical to the same window computed in a batch of 3
  loader edges hop 533 and 266, both pad modes: L = 20 hop + 512 + {-1, 0, +1} (frame 20 slow / fast / fast on the right),
               L in {1, 2, hop-1, hop, hop+1, 511, 512, 513, 1023, 1024, 1025}, 16 / 17 / 31 / 32 frames; reflect only for
               L > n_fft/2 (L = 513 included; L = 512 asserted to be KM_ERR_INVALID_ARG).  The LEFT side of the fast-loader test,
               f hop - 512 >= 0, does not depend on L, so it is walked with the hop: hop 511 / 512 / 513 (frame 1 slow / fast /
               fast) and hop 256 (frame 2 at exactly 0)
  hops         1, 64, 127, 128, 160, 532, 1024, 1025, 1600 (34 frames each; hop 1: 301 frames), both pad modes
  configs      CONFIG_SET below: a pairwise covering set of {1024-point rows-per-wave kernel, 1024-point two-frame kernel
               (option mel_two_frame), 512-point kernel} x {Slaney + norm, HTK no norm} x window_norm x n_mels {1, 40, 80, 128}
               x (f_min, f_max) x pad mode -- every value of every axis with every kernel, every pair of values at least once
  out_frames   truncation to 1 and n_frames - 1 rows and padding to n_frames + 5 by repeating the last row are bit-exact copies
  sequence     the shared-frame sequence mode (SeqFrames) inherits this pin through
               tests/test_gpu_models.py::test_shared_frame_sequence_path_is_bit_identical_to_per_window

  streaming    the ring instantiation (mel_power_rp_kernel<true>): StreamEngine.tick bit for bit against forward_audio on the
               unrolled ring, 3 and 600 streams, at the push counts that put the ring wrap on a frame's first sample, one sample
               inside it, and the frame's end exactly at / one sample past the ring's end (see ring_conditions below)
  readout      (CPU) gpu_power against a stand-in float32 front end; the covering property of CONFIG_SET; ring_conditions

Every case prints one line ``MELPOWER|case|gpu max e|f32 yardstick|bound|zero frames`` before it asserts.

OBSERVED (MI355X; GPU max e / float32 yardstick max e; bound = 8 x max(yardstick, 1.19e-7)):
  case                                                                 GPU    float32  zero frames
  signal speech                                                   4.01e-07   4.47e-07
  signal uniform                                                  5.99e-07   6.43e-07
  signal tone_on_1                                                3.44e-07   3.14e-07
  signal tone_on_1e-3                                             3.43e-07   1.52e-07
  signal tone_on_1e-6                                             2.68e-07   2.97e-07
  signal tone_off_1                                               4.27e-07   1.70e-07
  signal tone_off_1e-3                                            2.72e-07   2.34e-07
  signal tone_off_1e-6                                            3.67e-07   2.08e-07
  signal click_mid_frame                                          8.18e-07   8.27e-07  766
  signal click_frame_boundary                                     8.12e-07   1.22e-06  767
  signal dc_tone                                                  2.79e-08   1.29e-08
  signal chirp                                                    3.93e-07   3.21e-07
  signal square                                                   2.81e-07   1.65e-07
  signal silence                                                  0.00e+00   0.00e+00  771
  signal silent_between_loud                                      6.07e-07   6.66e-07  257
  closed impulse rp                                               4.53e-07   6.66e-07
  closed impulse two                                              4.53e-07   6.66e-07
  closed impulse p512                                             4.28e-07   2.90e-07
  closed cosine rp k0=37 A=1.0                                    3.01e-07   1.65e-07
  closed cosine two k0=37 A=1.0                                   2.34e-07   1.65e-07
  closed cosine p512 k0=37 A=1.0                                  2.51e-07   1.23e-07
  closed cosine rp k0=200 A=0.25                                  3.10e-07   1.82e-07
  closed cosine two k0=200 A=0.25                                 2.08e-07   1.82e-07
  closed cosine p512 k0=200 A=0.25                                1.76e-07   1.83e-07
  geometry B=1 L=40000                                            2.70e-07   1.68e-07
  geometry B=31 L=40000                                           3.99e-07   5.08e-07
  geometry B=32 L=40000                                           3.99e-07   5.08e-07
  geometry B=40 L=40000                                           4.26e-07   5.08e-07
  geometry B=100 L=40000                                          4.41e-07   5.08e-07
  geometry B=256 L=40000                                          5.10e-07   6.43e-07
  geometry B=511 L=40000                                          5.10e-07   6.43e-07
  geometry B=600 L=40000                                          5.46e-07   6.43e-07
  geometry B=1100 L=40000                                         6.86e-07   7.21e-07
  geometry B=32 L=136448                                          4.36e-07   4.83e-07
  geometry B=40 L=136448                                          5.08e-07   5.86e-07
  geometry B=100 L=136448                                         5.08e-07   6.42e-07
  geometry B=170 L=136448                                         5.08e-07   6.42e-07
  geometry B=256 L=136448                                         5.08e-07   6.42e-07
  edge hop=533 constant L=1                                       7.74e-07   3.81e-07
  edge hop=533 constant L=2                                       7.12e-07   3.44e-07
  edge hop=533 constant L=511                                     3.90e-07   1.84e-07
  edge hop=533 constant L=512                                     2.57e-07   1.71e-07
  edge hop=533 constant L=513                                     4.08e-07   1.35e-07
  edge hop=533 constant L=532                                     2.93e-07   2.19e-07
  edge hop=533 constant L=533                                     3.95e-07   1.67e-07
  edge hop=533 constant L=534                                     2.55e-07   2.22e-07
  edge hop=533 constant L=1023                                    3.79e-07   1.91e-07
  edge hop=533 constant L=1024                                    4.58e-07   1.91e-07
  edge hop=533 constant L=1025                                    3.16e-07   1.66e-07
  edge hop=533 constant L=8000                                    3.99e-07   5.22e-07
  edge hop=533 constant L=8533                                    5.54e-07   4.95e-07
  edge hop=533 constant L=11171                                   4.87e-07   5.03e-07
  edge hop=533 constant L=11172                                   4.70e-07   5.89e-07
  edge hop=533 constant L=11173                                   4.45e-07   4.69e-07
  edge hop=533 constant L=15995                                   5.33e-07   5.11e-07
  edge hop=533 constant L=16528                                   4.58e-07   4.79e-07
  edge hop=533 reflect L=513                                      3.73e-07   1.31e-07
  edge hop=533 reflect L=532                                      2.36e-07   1.66e-07
  edge hop=533 reflect L=533                                      2.31e-07   1.65e-07
  edge hop=533 reflect L=534                                      3.75e-07   1.36e-07
  edge hop=533 reflect L=1023                                     3.41e-07   2.19e-07
  edge hop=533 reflect L=1024                                     3.49e-07   2.00e-07
  edge hop=533 reflect L=1025                                     4.22e-07   2.20e-07
  edge hop=533 reflect L=8000                                     3.99e-07   5.22e-07
  edge hop=533 reflect L=8533                                     5.54e-07   4.95e-07
  edge hop=533 reflect L=11171                                    4.87e-07   5.03e-07
  edge hop=533 reflect L=11172                                    4.70e-07   5.89e-07
  edge hop=533 reflect L=11173                                    4.45e-07   4.69e-07
  edge hop=533 reflect L=15995                                    5.33e-07   5.11e-07
  edge hop=533 reflect L=16528                                    4.58e-07   4.79e-07
  edge hop=266 constant L=1                                       7.74e-07   3.81e-07
  edge hop=266 constant L=2                                       7.12e-07   3.44e-07
  edge hop=266 constant L=265                                     3.55e-07   1.54e-07
  edge hop=266 constant L=266                                     3.17e-07   2.02e-07
  edge hop=266 constant L=267                                     2.74e-07   2.18e-07
  edge hop=266 constant L=511                                     3.90e-07   2.50e-07
  edge hop=266 constant L=512                                     3.25e-07   2.17e-07
  edge hop=266 constant L=513                                     4.08e-07   2.19e-07
  edge hop=266 constant L=1023                                    3.49e-07   1.89e-07
  edge hop=266 constant L=1024                                    3.47e-07   2.72e-07
  edge hop=266 constant L=1025                                    3.86e-07   2.19e-07
  edge hop=266 constant L=3995                                    4.28e-07   4.95e-07
  edge hop=266 constant L=4261                                    4.26e-07   4.79e-07
  edge hop=266 constant L=5831                                    5.89e-07   5.34e-07
  edge hop=266 constant L=5832                                    4.16e-07   6.24e-07
  edge hop=266 constant L=5833                                    4.27e-07   5.85e-07
  edge hop=266 constant L=7985                                    4.38e-07   4.88e-07
  edge hop=266 constant L=8251                                    4.70e-07   5.16e-07
  edge hop=266 reflect L=513                                      3.73e-07   1.61e-07
  edge hop=266 reflect L=1023                                     4.21e-07   2.06e-07
  edge hop=266 reflect L=1024                                     3.49e-07   2.00e-07
  edge hop=266 reflect L=1025                                     3.86e-07   2.03e-07
  edge hop=266 reflect L=3995                                     4.28e-07   4.95e-07
  edge hop=266 reflect L=4261                                     4.26e-07   4.92e-07
  edge hop=266 reflect L=5831                                     4.06e-07   5.34e-07
  edge hop=266 reflect L=5832                                     4.16e-07   6.24e-07
  edge hop=266 reflect L=5833                                     4.07e-07   5.85e-07
  edge hop=266 reflect L=7985                                     4.38e-07   4.88e-07
  edge hop=266 reflect L=8251                                     4.70e-07   5.16e-07
  edge hop=511 constant L=10731                                   4.95e-07   5.83e-07
  edge hop=511 constant L=10732                                   4.70e-07   5.41e-07
  edge hop=511 reflect L=10731                                    4.95e-07   5.83e-07
  edge hop=511 reflect L=10732                                    4.70e-07   5.41e-07
  edge hop=512 constant L=10751                                   5.18e-07   4.62e-07
  edge hop=512 constant L=10752                                   4.42e-07   4.66e-07
  edge hop=512 reflect L=10751                                    5.18e-07   4.55e-07
  edge hop=512 reflect L=10752                                    4.42e-07   4.66e-07
  edge hop=513 constant L=10771                                   6.07e-07   5.00e-07
  edge hop=513 constant L=10772                                   4.02e-07   5.28e-07
  edge hop=513 reflect L=10771                                    6.07e-07   5.00e-07
  edge hop=513 reflect L=10772                                    3.63e-07   5.28e-07
  edge hop=256 constant L=5631                                    5.62e-07   6.00e-07
  edge hop=256 constant L=5632                                    4.96e-07   5.26e-07
  edge hop=256 reflect L=5631                                     5.62e-07   6.00e-07
  edge hop=256 reflect L=5632                                     4.96e-07   5.26e-07
  edge reflect n_fft=1024 L=n_fft/2+1                             2.31e-07   1.87e-07
  edge reflect n_fft=512 L=n_fft/2+1                              2.29e-07   1.33e-07
  hop=1 constant L=300                                            5.95e-07   6.20e-07
  hop=1 reflect L=600                                             5.17e-07   6.61e-07
  hop=64 constant L=2119                                          5.11e-07   6.20e-07
  hop=64 reflect L=2119                                           5.11e-07   6.20e-07
  hop=127 constant L=4198                                         4.14e-07   4.74e-07
  hop=127 reflect L=4198                                          4.03e-07   4.74e-07
  hop=128 constant L=4231                                         5.46e-07   4.12e-07
  hop=128 reflect L=4231                                          5.46e-07   4.12e-07
  hop=160 constant L=5287                                         5.35e-07   5.05e-07
  hop=160 reflect L=5287                                          4.58e-07   4.30e-07
  hop=532 constant L=17563                                        5.20e-07   5.61e-07
  hop=532 reflect L=17563                                         5.20e-07   5.61e-07
  hop=1024 constant L=33799                                       5.93e-07   4.64e-07
  hop=1024 reflect L=33799                                        5.93e-07   4.64e-07
  hop=1025 constant L=33832                                       4.96e-07   6.66e-07
  hop=1025 reflect L=33832                                        4.96e-07   5.37e-07
  hop=1600 constant L=52807                                       5.23e-07   4.96e-07
  hop=1600 reflect L=52807                                        5.23e-07   4.96e-07
  config rp slaney wn=0 M=1 80-8000 constant speech               7.19e-07   2.18e-07
  config rp slaney wn=0 M=1 80-8000 constant uniform              3.78e-06   1.10e-06
  config rp htk wn=1 M=40 0-8000 reflect speech                   3.15e-07   2.75e-07
  config rp htk wn=1 M=40 0-8000 reflect uniform                  6.74e-07   1.04e-06
  config two slaney wn=0 M=80 300-3400 reflect speech             2.73e-07   8.28e-08
  config two slaney wn=0 M=80 300-3400 reflect uniform            3.57e-07   2.23e-07
  config p512 htk wn=1 M=128 300-3400 constant speech             3.92e-07   1.59e-07
  config p512 htk wn=1 M=128 300-3400 constant uniform            3.54e-07   2.20e-07
  config two htk wn=1 M=1 80-8000 reflect speech                  9.15e-07   4.84e-07
  config two htk wn=1 M=1 80-8000 reflect uniform                 4.69e-06   1.47e-06
  config p512 slaney wn=0 M=40 0-8000 constant speech             8.23e-07   3.22e-07
  config p512 slaney wn=0 M=40 0-8000 constant uniform            5.21e-07   5.37e-07
  config two slaney wn=0 M=128 0-8000 constant speech             6.88e-07   2.04e-07
  config two slaney wn=0 M=128 0-8000 constant uniform            4.06e-07   4.01e-07
  config p512 slaney wn=1 M=80 80-8000 constant speech            6.66e-07   2.32e-07
  config p512 slaney wn=1 M=80 80-8000 constant uniform           3.69e-07   4.03e-07
  config rp htk wn=0 M=80 0-8000 constant speech                  3.22e-07   1.96e-07
  config rp htk wn=0 M=80 0-8000 constant uniform                 4.72e-07   5.23e-07
  config rp slaney wn=0 M=128 80-8000 reflect speech              3.21e-07   1.68e-07
  config rp slaney wn=0 M=128 80-8000 reflect uniform             3.96e-07   3.64e-07
  config p512 slaney wn=0 M=1 0-8000 reflect speech               8.41e-07   3.23e-07
  config p512 slaney wn=0 M=1 0-8000 reflect uniform              2.86e-06   7.18e-07
  config rp slaney wn=0 M=1 300-3400 constant speech              5.65e-07   1.12e-07
  config rp slaney wn=0 M=1 300-3400 constant uniform             2.35e-06   4.90e-07
  config two slaney wn=0 M=40 80-8000 constant speech             4.89e-07   2.71e-07
  config two slaney wn=0 M=40 80-8000 constant uniform            7.73e-07   9.40e-07
  config rp slaney wn=0 M=40 300-3400 constant speech             1.35e-07   9.36e-08
  config rp slaney wn=0 M=40 300-3400 constant uniform            3.30e-07   3.79e-07
  config two htk wn=0 M=80 80-8000 constant speech                7.88e-07   1.67e-07
  config two htk wn=0 M=80 80-8000 constant uniform               5.65e-07   4.57e-07
  config p512 htk wn=0 M=80 80-8000 reflect speech                8.04e-07   1.97e-07
  config p512 htk wn=0 M=80 80-8000 reflect uniform               3.40e-07   4.05e-07
  closest to its bound: config rp slaney wn=0 M=1 300-3400 constant uniform at 0.60 of it
"""
import numpy as np
import pytest
import torch

from koemorph_amd import _lib, synth
from koemorph_amd._lib import KoeMorphError
from koemorph_amd.engine import Engine, MelConfig
from oracle import mel as omel

gpu = pytest.mark.gpu          # per test: the two CPU tests at the end of the file run without a GPU

U = omel.MEL_POWER_U
FACTOR = 8.0
LOG_EPS = 2.0 ** -100
LN2_F32 = np.float32(0.693147180559945309)
ZERO_LOG = float(LN2_F32 * np.float32(-100.0))        # the kernel's ln2 * log2(0 + 2^-100), in float32
PROD = dict(n_fft=1024, hop=533, n_mels=80, f_min=80.0, f_max=8000.0, mel_scale="slaney", slaney_norm=True,
            pad_mode="constant", window_norm=False)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def mel_config(kw):
    return MelConfig(n_fft=kw["n_fft"], hop_length=kw["hop"], n_mels=kw["n_mels"], f_min=kw["f_min"], f_max=kw["f_max"],
                     mel_scale=_lib.KM_MEL_HTK if kw["mel_scale"] == "htk" else _lib.KM_MEL_SLANEY,
                     slaney_norm=1 if kw["slaney_norm"] else 0,
                     pad_mode=_lib.KM_PAD_REFLECT if kw["pad_mode"] == "reflect" else _lib.KM_PAD_CONSTANT,
                     window_norm=1 if kw["window_norm"] else 0, log_mode=_lib.KM_LOG_LN_EPS, log_eps=LOG_EPS)


def _engine(two_frame):
    e = Engine()
    e.load_state_dict(synth.make_core_params(7, style="trained"))
    e.finalize()
    if two_frame:
        e.set_option("mel_two_frame", 1)
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine(False)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_two():
    e = _engine(True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_hops():
    e = _engine(False)
    yield e
    e.close()


def gpu_power(e, cfg, audio_t):
    """(B, F, M) float64 power-mel of the kernels (see HOW THE POWER IS READ) and the direct float32 read-out y0."""
    y0 = e.mel_extract(cfg, audio_t).clone()
    assert bool(torch.isfinite(y0).all())
    zero = y0 == ZERO_LOG
    assert not bool((y0 < ZERO_LOG).any())
    P = torch.clamp(torch.exp(y0.double()) - LOG_EPS, min=0.0)           # the direct read-out: y0 = ln(P + log_eps)
    P = torch.where(zero, torch.zeros_like(P), P)
    l2 = torch.log2(torch.clamp(P, min=1e-300))
    row_top = l2.amax(dim=2, keepdim=True)
    refine = ~zero & (l2 > row_top - np.log2(1e25)) & (P > 1e3 * LOG_EPS)
    k = torch.round(l2 / 2.0).to(torch.int64)
    for kk in torch.unique(k[refine]).tolist():
        sel = refine & (k == kk)
        yk = e.mel_extract(cfg, audio_t * (2.0 ** -kk))
        got = yk[sel].double()
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) < 0.75, kk
        # homogeneity: the same value as the direct read-out, to the direct read-out's rounding (3 ulp of |y0|, |log2| <= 128)
        direct = torch.log(torch.exp(got + 2.0 * kk * np.log(2.0)) + LOG_EPS)
        slack = 3.0 * 2.0 ** -23 * torch.clamp(y0[sel].double().abs() / np.log(2.0), min=1.0) + 1e-7
        assert bool(((y0[sel].double() - direct).abs() <= slack).all()), (kk, float(((y0[sel].double() - direct).abs() / slack).max()))
        P[sel] = torch.exp(got) * 4.0 ** kk
    return P.cpu().numpy(), y0


def oracle_case(audio, kw):
    """Per window: float64 truth, its scale, and the float32 yardstick's error."""
    P64, peak, e32 = [], [], []
    fb = None
    for y in audio:
        p, aux = omel.mel_power(y, precision="f64", return_aux=True, **kw)
        fb = aux["fb"]
        P64.append(p)
        peak.append(aux["spec_peak"])
        e32.append(omel.mel_power_error(omel.mel_power(y, precision="f32", **kw), p, aux["spec_peak"], fb)[0])
    return np.stack(P64), np.stack(peak), fb, np.stack(e32)


def judge(label, P, P64, peak, fb, e32, dead_expected=0):
    e, dead = omel.mel_power_error(P, P64, peak, fb)
    S = (peak[..., None] * fb.max(axis=1).astype(np.float64))
    live = S[S > 0]
    if live.size:
        assert LOG_EPS < 1e-9 * U * live.min(), (label, live.min())
    yard = float(e32.max())
    bound = FACTOR * max(yard, U)
    worst = float(e.max())
    print(f"MELPOWER|{label}|{worst:.2e}|{yard:.2e}|{bound:.2e}|{dead}")
    if not worst <= bound:
        idx = np.argsort(e.ravel())[::-1][:6]
        for i in idx:
            w, t, m = np.unravel_index(i, e.shape)
            print(f"  worst: window {w} frame {t} filter {m}: e {e[w, t, m]:.3e} P {P[w, t, m]:.6e} P64 {P64[w, t, m]:.6e}")
    if dead_expected is not None:
        assert dead == dead_expected, (label, dead)
    # frames whose float64 spectrum is identically zero came back as exactly zero power (e is inf otherwise)
    assert worst <= bound, (label, worst, yard, bound)
    return worst


def run_case(e, label, audio, kw, dead_expected=0):
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    P, y0 = gpu_power(e, mel_config(kw), dev(audio))
    P64, peak, fb, e32 = oracle_case(audio, kw)
    assert P.shape == P64.shape, (P.shape, P64.shape)
    judge(label, P, P64, peak, fb, e32, dead_expected)
    return y0


# ---- signals ----------------------------------------------------------------------------------------------------------------
L_PROD = 136448


def _tone(k_bins, A, L=L_PROD, N=1024):
    n = np.arange(L, dtype=np.float64)
    return np.stack([A * np.cos(2.0 * np.pi * k * n / N + 0.4 * i) for i, k in enumerate(k_bins)]).astype(np.float32)


def make_signal(name):
    """(audio (3, L), expected number of all-zero frames or None = not asserted)."""
    L = L_PROD
    n = np.arange(L, dtype=np.float64)
    if name == "speech":
        return synth.make_audio(3, 3, L), 0
    if name == "uniform":
        return synth.make_audio(3, 3, L, "uniform"), 0
    if name.startswith("tone_on_"):
        return _tone((37, 200, 450), float(name[8:])), 0
    if name.startswith("tone_off_"):
        return _tone((37.37, 200.5, 449.81), float(name[9:])), 0
    if name == "click_mid_frame":                          # frame 128 is centred on 128 * 533
        z = np.zeros((3, L), np.float32)
        z[0, 128 * 533], z[1, 128 * 533 + 100], z[2, 7 * 533 - 31] = 1.0, -0.5, 0.25
        return z, None
    if name == "click_frame_boundary":                     # the first / last sample of a frame: 128 * 533 -+ 512
        z = np.zeros((3, L), np.float32)
        z[0, 128 * 533 - 512], z[1, 128 * 533 + 511], z[2, 128 * 533 + 512] = 1.0, 1.0, 1.0
        return z, None
    if name == "dc_tone":
        return np.stack([0.9 + 1e-4 * np.cos(2.0 * np.pi * k * n / 1024) for k in (100.3, 37.0, 300.7)]).astype(np.float32), 0
    if name == "chirp":                                    # 50 Hz -> 7.9 kHz across the clip
        f1 = np.array([7900.0, 4000.0, 7900.0])[:, None]
        f0 = np.array([50.0, 50.0, 3000.0])[:, None]
        ph = 2.0 * np.pi * (f0 * n + 0.5 * (f1 - f0) * n * n / L) / 16000.0
        return (0.8 * np.sin(ph)).astype(np.float32), 0
    if name == "square":                                   # full scale +-1, periods 64 / 100 / 7 samples
        return np.stack([np.where((np.arange(L) // h) % 2 == 0, 1.0, -1.0) for h in (32, 50, 7)]).astype(np.float32)[:, :L], 0
    if name == "silence":
        return np.zeros((3, L), np.float32), 3 * 257
    if name == "silent_between_loud":
        a = synth.make_audio(4, 3, L, "uniform") * 1.9
        a[1] = 0.0
        return a, 257
    raise KeyError(name)


SIGNALS = ["speech", "uniform", "tone_on_1", "tone_on_1e-3", "tone_on_1e-6", "tone_off_1", "tone_off_1e-3", "tone_off_1e-6",
           "click_mid_frame", "click_frame_boundary", "dc_tone", "chirp", "square", "silence", "silent_between_loud"]


@gpu
@pytest.mark.parametrize("name", SIGNALS)
def test_signals(eng, name):
    audio, dead = make_signal(name)
    y0 = run_case(eng, "signal " + name, audio, PROD, dead)
    if name in ("silence", "silent_between_loud"):         # exact zero rows, and no leak from the loud neighbours
        assert bool((y0[1] == ZERO_LOG).all())
    if name.startswith("click"):
        P64 = omel.mel_power(audio[0], precision="f64", **PROD)
        silent = ~P64.any(axis=1)
        assert silent.sum() >= 254 and bool((y0[0][torch.from_numpy(silent).cuda()] == ZERO_LOG).all())


# ---- closed forms on the GPU ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel", ["rp", "two", "p512"])
def test_closed_form_impulse(eng, eng_two, kernel):
    """delta at a frame centre: |X_k|^2 = w[n_fft/2]^2 = 1 for every k, the mel row is the filters' row sums."""
    kw = dict(PROD, n_fft=512 if kernel == "p512" else 1024)
    e = eng_two if kernel == "two" else eng
    y = np.zeros((3, 40 * 533), np.float32)
    frames = (0, 17, 39)
    for b, t in enumerate(frames):
        y[b, t * 533] = 1.0
    P, _ = gpu_power(e, mel_config(kw), dev(y))
    fb = omel.mel_filterbank_librosa(16000, kw["n_fft"], 80, 80.0, 8000.0)
    want = fb.astype(np.float64).sum(axis=1)
    P32 = np.stack([omel.mel_power(y[b], precision="f32", **kw)[t] for b, t in enumerate(frames)])
    got = np.stack([P[b, t] for b, t in enumerate(frames)])
    peak = np.ones(3)
    e32 = omel.mel_power_error(P32, np.tile(want, (3, 1)), peak, fb)[0]
    judge(f"closed impulse {kernel}", got, np.tile(want, (3, 1)), peak, fb, e32)


@gpu
@pytest.mark.parametrize("kernel", ["rp", "two", "p512"])
@pytest.mark.parametrize("k0,A", [(37, 1.0), (200, 0.25)])
def test_closed_form_cosine(eng, eng_two, kernel, k0, A):
    """A cos(2 pi k0 n / N) under the periodic Hann window: P[k0] = (A N/4)^2, P[k0 +- 1] = (A N/8)^2, nothing else."""
    N = 512 if kernel == "p512" else 1024
    kw = dict(PROD, n_fft=N)
    e = eng_two if kernel == "two" else eng
    y = np.stack([A * np.cos(2.0 * np.pi * k0 * np.arange(40 * 533) / N + ph) for ph in (0.0, 0.3, 1.7)]).astype(np.float32)
    P, _ = gpu_power(e, mel_config(kw), dev(y))
    fb = omel.mel_filterbank_librosa(16000, N, 80, 80.0, 8000.0)
    S = np.zeros(N // 2 + 1)
    S[k0], S[k0 - 1], S[k0 + 1] = (A * N / 4) ** 2, (A * N / 8) ** 2, (A * N / 8) ** 2
    rows = slice(2, 38)                                    # interior frames: no padding inside them
    want = np.broadcast_to(fb.astype(np.float64) @ S, P[:, rows].shape)
    peak = np.full(want.shape[:2], S.max())
    P32 = np.stack([omel.mel_power(w, precision="f32", **kw)[rows] for w in y])
    e32 = omel.mel_power_error(P32, want, peak, fb)[0]
    judge(f"closed cosine {kernel} k0={k0} A={A}", P[:, rows], want, peak, fb, e32)


# ---- launch geometry ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def speech_1100():
    return synth.make_audio(80, 1100, 40000)


def _same_as_batches_of_three(e, cfg, audio_t, y0):
    B = audio_t.shape[0]
    for lo in range(0, B, 3):
        lo = max(0, min(lo, B - 3))
        hi = min(B, lo + 3)
        assert torch.equal(e.mel_extract(cfg, audio_t[lo:hi].contiguous()), y0[lo:hi]), (B, lo)


@gpu
@pytest.mark.parametrize("B", [1, 31, 32, 40, 100, 256, 511, 600, 1100])
def test_launch_geometry(eng, speech_1100, B):
    audio = speech_1100[:B]
    y0 = run_case(eng, f"geometry B={B} L=40000", audio, PROD)
    assert y0.shape == (B, 76, 80)
    cfg = mel_config(PROD)
    if B >= 3:
        _same_as_batches_of_three(eng, cfg, dev(audio), y0)
    else:                                                  # the window alone == the window as the first of three
        assert torch.equal(eng.mel_extract(cfg, dev(speech_1100[:3]))[:B], y0)


@gpu
@pytest.mark.parametrize("B", [32, 40, 100, 170, 256])
def test_launch_geometry_production_length(eng, B):
    """17 chunks for per_window = 16, 13, 5, 3, 2 workgroups: several workgroups ask chunk_ctr for a ragged number of chunks."""
    assert [(512 + b // 2) // b for b in (32, 40, 100, 170, 256)] == [16, 13, 5, 3, 2]
    audio = synth.make_audio(81, 256, L_PROD)[:B]
    y0 = run_case(eng, f"geometry B={B} L=136448", audio, PROD)
    assert y0.shape == (B, 257, 80)
    _same_as_batches_of_three(eng, mel_config(PROD), dev(audio), y0)


# ---- loader edges ---------------------------------------------------------------------------------------------------------------
def _edge_lengths(hop):
    out = [20 * hop + 512 + d for d in (-1, 0, 1)]
    out += [1, 2, hop - 1, hop, hop + 1, 511, 512, 513, 1023, 1024, 1025]
    out += [(n - 1) * hop + 5 for n in (16, 17, 31, 32)]
    return sorted(set(out))


EDGES = [(hop, pad, L) for hop in (533, 266) for pad in ("constant", "reflect") for L in _edge_lengths(hop)
         if pad == "constant" or L > 512]
EDGES += [(hop, pad, 20 * hop + 512 + d) for hop in (511, 512, 513, 256) for pad in ("constant", "reflect") for d in (-1, 0)]


@gpu
@pytest.mark.parametrize("hop,pad,L", EDGES)
def test_loader_edges(eng, hop, pad, L):
    kw = dict(PROD, hop=hop, pad_mode=pad)
    y0 = run_case(eng, f"edge hop={hop} {pad} L={L}", synth.make_audio(1000 + L % 97, 2, L, "uniform"), kw)
    assert y0.shape[1] == 1 + L // hop
    for n in (16, 17, 31, 32):
        if L == (n - 1) * hop + 5:
            assert y0.shape[1] == n


@gpu
@pytest.mark.parametrize("n_fft", [1024, 512])
def test_reflect_padding_refuses_the_shortest_clip(eng, n_fft):
    kw = dict(PROD, n_fft=n_fft, pad_mode="reflect")
    cfg = mel_config(kw)
    with pytest.raises(KoeMorphError) as ei:
        eng.mel_extract(cfg, dev(synth.make_audio(5, 2, n_fft // 2, "uniform")))
    assert ei.value.code == _lib.KM_ERR_INVALID_ARG
    run_case(eng, f"edge reflect n_fft={n_fft} L=n_fft/2+1", synth.make_audio(5, 2, n_fft // 2 + 1, "uniform"), kw)


# ---- hops -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pad", ["constant", "reflect"])
@pytest.mark.parametrize("hop", [1, 64, 127, 128, 160, 532, 1024, 1025, 1600])
def test_hops(eng_hops, hop, pad):
    eng = eng_hops
    L = 300 if hop == 1 else 33 * hop + 7
    if pad == "reflect" and L <= 512:
        L = 600
    y0 = run_case(eng, f"hop={hop} {pad} L={L}", synth.make_audio(2000 + hop, 2, L, "uniform"), dict(PROD, hop=hop, pad_mode=pad))
    assert y0.shape[1] == 1 + L // hop >= 33


# ---- configurations x kernels ---------------------------------------------------------------------------------------------------
# (kernel, (mel scale, Slaney norm), window_norm, n_mels, (f_min, f_max), pad mode): greedy pairwise cover of the product
CONFIG_SET = [
    ("rp", ("slaney", 1), 0, 1, (80, 8000), "constant"),
    ("rp", ("htk", 0), 1, 40, (0, 8000), "reflect"),
    ("two", ("slaney", 1), 0, 80, (300, 3400), "reflect"),
    ("p512", ("htk", 0), 1, 128, (300, 3400), "constant"),
    ("two", ("htk", 0), 1, 1, (80, 8000), "reflect"),
    ("p512", ("slaney", 1), 0, 40, (0, 8000), "constant"),
    ("two", ("slaney", 1), 0, 128, (0, 8000), "constant"),
    ("p512", ("slaney", 1), 1, 80, (80, 8000), "constant"),
    ("rp", ("htk", 0), 0, 80, (0, 8000), "constant"),
    ("rp", ("slaney", 1), 0, 128, (80, 8000), "reflect"),
    ("p512", ("slaney", 1), 0, 1, (0, 8000), "reflect"),
    ("rp", ("slaney", 1), 0, 1, (300, 3400), "constant"),
    ("two", ("slaney", 1), 0, 40, (80, 8000), "constant"),
    ("rp", ("slaney", 1), 0, 40, (300, 3400), "constant"),
    ("two", ("htk", 0), 0, 80, (80, 8000), "constant"),
    ("p512", ("htk", 0), 0, 80, (80, 8000), "reflect"),
]


def test_config_set_covers_every_pair():
    import itertools
    for i, j in itertools.combinations(range(6), 2):
        vi, vj = {c[i] for c in CONFIG_SET}, {c[j] for c in CONFIG_SET}
        assert {(c[i], c[j]) for c in CONFIG_SET} == set(itertools.product(vi, vj)), (i, j)
    assert {c[3] for c in CONFIG_SET} == {1, 40, 80, 128} and {c[0] for c in CONFIG_SET} == {"rp", "two", "p512"}


@gpu
@pytest.mark.parametrize("kernel,scale,wnorm,n_mels,band,pad", CONFIG_SET)
def test_configurations(eng, eng_two, kernel, scale, wnorm, n_mels, band, pad):
    kw = dict(n_fft=512 if kernel == "p512" else 1024, hop=533, n_mels=n_mels, f_min=float(band[0]), f_max=float(band[1]),
              mel_scale=scale[0], slaney_norm=bool(scale[1]), pad_mode=pad, window_norm=bool(wnorm))
    e = eng_two if kernel == "two" else eng
    for style, L in (("speech", 40000), ("uniform", 20000)):
        run_case(e, f"config {kernel} {scale[0]} wn={wnorm} M={n_mels} {band[0]}-{band[1]} {pad} {style}",
                 synth.make_audio(90, 3, L, style), kw)


# ---- out_frames policy ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kernel", ["rp", "two", "p512"])
def test_out_frames_policy_copies_rows_bit_for_bit(eng, eng_two, kernel):
    kw = dict(PROD, n_fft=512 if kernel == "p512" else 1024)
    e = eng_two if kernel == "two" else eng
    cfg = mel_config(kw)
    a = dev(synth.make_audio(95, 3, 40000))
    full = e.mel_extract(cfg, a).clone()
    F = full.shape[1]
    assert F == 76
    for n in (1, F - 1):
        assert torch.equal(e.mel_extract(cfg, a, out_frames=n), full[:, :n])
    more = e.mel_extract(cfg, a, out_frames=F + 5)
    assert torch.equal(more[:, :F], full) and torch.equal(more[:, F:], full[:, F - 1:F].expand(-1, 5, -1))


# ---- the streaming ring (mel_power_rp_kernel<true>) -----------------------------------------------------------------------------
# km_stream_tick returns the 52 outputs, so they are compared bit for bit with km_forward_audio on the unrolled ring: same
# configuration (n_fft 1024, hop 533, reflect, dB), same EMA state and first flag on both sides.  The two are the same function
# only where the tick keeps as many rows as the STFT makes, int(context_window / update_interval) == 1 + ring_len // hop.  The
# default ring (8.5 s / 0.0333 s) keeps 255 of 256, so the case uses 8.5 s / 0.0332 s: 256 of 256 rows, ring_len 136 000, ring hop
# int(16000 * 0.0332) = 531.  After n pushes the ring starts at rs = 531 n mod 136 000 and frame f (fully inside the window:
# 0 <= 533 f - 512, 533 f + 512 <= 136 000) begins at physical sample (rs + 533 f - 512) mod 136 000.  gcd(531, 136 000) = 1, so
# every start is reachable; ring_conditions searches the first push counts at which some frame
#   (a) begins at 0 (the wrap on its first sample: fast loader),        (b) begins at ring_len - 1 (wrap one sample inside: slow),
#   (c) ends exactly at ring_len (start + 1024 == ring_len: last fast), (d) ends one sample past it (first slow)
# and finds n = 2293 (frame 13), 459 (frame 54), 2272 (frame 32), 437 (frame 74).
RING_LEN, RING_HOP, RING_CW, RING_UI = 136000, 531, 8.5, 0.0332


def ring_conditions(ring_len, ring_hop, hop, n_frames):
    want = {"a": 0, "b": ring_len - 1, "c": ring_len - 1024, "d": ring_len - 1023}
    lo = np.arange(n_frames) * hop - 512
    inside = (lo >= 0) & (lo + 1024 <= ring_len)
    found, n = {}, -(-ring_len // ring_hop)
    while len(found) < 4 and n < 100000:
        start = ((n * ring_hop) % ring_len + lo) % ring_len
        for key, v in want.items():
            hit = np.nonzero(inside & (start == v))[0]
            if key not in found and hit.size:
                found[key] = (n, int(hit[0]))
        n += 1
    return found


def test_ring_conditions_are_reachable():
    assert int(RING_CW / RING_UI) == 1 + RING_LEN // 533 == 256 and int(16000 / (1.0 / RING_UI)) == RING_HOP
    assert ring_conditions(RING_LEN, RING_HOP, 533, 256) == {"a": (2293, 13), "b": (459, 54), "c": (2272, 32), "d": (437, 74)}
    # the default ring reaches them too (385 pushes), but its tick keeps 255 rows of the 256 forward_audio uses
    assert len(ring_conditions(136000, 532, 533, 256)) == 4 and int(8.5 / 0.0333) == 255


@gpu
@pytest.mark.parametrize("S", [3, 600])
def test_streaming_ring_is_bit_identical_to_forward_audio_on_the_unrolled_ring(S):
    from koemorph_amd.streaming import StreamEngine
    cfg = MelConfig.sliding_window(n_fft=1024, hop_length=533)
    e = Engine(mel=cfg)
    e.load_state_dict(synth.make_core_params(7, style="trained"))
    e.finalize()
    se = StreamEngine(e, S, context_window=RING_CW, update_interval=RING_UI, mel=cfg)
    assert se.ring_hop == RING_HOP
    cond = ring_conditions(RING_LEN, RING_HOP, 533, 256)
    full = -(-RING_LEN // RING_HOP)
    ticks = sorted({full, full + 1} | {n for n, _ in cond.values()})          # also the first full ring and the one after
    pool = synth.make_audio(300 + S, S, RING_HOP * 67, "uniform")              # 67 pushes of distinct audio, then rescaled
    emo = dev(synth.normal(301, (S, 256)))
    ring = np.zeros((S, RING_LEN), np.float32)
    state = torch.zeros(S, 52, device="cuda")
    w, first = 0, True
    for n in range(1, ticks[-1] + 1):
        chunk = pool[:, (n % 67) * RING_HOP:(n % 67 + 1) * RING_HOP] * np.float32(0.25 + 0.125 * ((n // 67) % 7))
        se.push(dev(chunk))
        idx = (w + np.arange(RING_HOP)) % RING_LEN
        ring[:, idx] = chunk
        w = (w + RING_HOP) % RING_LEN
        if n in ticks:
            out, ready = se.tick(emo)
            assert bool(ready.all())
            unrolled = np.roll(ring, -w, axis=1)                             # chronological order starts at the write pointer
            lo = np.arange(256) * 533 - 512
            start = (w + lo) % RING_LEN
            for key, (cn, cf) in cond.items():                               # the condition really is met at this tick
                if cn == n:
                    assert start[cf] == {"a": 0, "b": RING_LEN - 1, "c": RING_LEN - 1024, "d": RING_LEN - 1023}[key]
            want = e.forward_audio(dev(unrolled), emo, state=state, first=first)
            assert torch.equal(out, want), (S, n, float((out - want).abs().max()))
            assert float(want.std()) > 1e-3
            first = False
    e.close()


# ---- a failed allocation must not poison later launches -----------------------------------------------------------------------
@gpu
def test_failed_workspace_growth_leaves_other_launches_working(eng):
    """km_reserve for a workspace no device holds fails with KM_ERR_HIP (an allocation refused by the runtime, nothing is
    launched); the runtime keeps such a failure as its 'last error', which the launch checks of every handle used to pick
    up: the next mel_extract of ANOTHER engine failed with 'out of memory'.  Both engines must work afterwards."""
    cfg = mel_config(PROD)
    a = dev(synth.make_audio(96, 3, 20000))
    before = eng.mel_extract(cfg, a).clone()
    other = _engine(False)
    with pytest.raises(KoeMorphError) as ei:
        other.reserve(1 << 22, 1 << 28)                    # 4 Mi windows x 503 k frames x 80 bins: ~7e14 bytes
    assert ei.value.code == _lib.KM_ERR_HIP
    assert torch.equal(eng.mel_extract(cfg, a), before)    # the other handle's failure is not ours
    assert torch.equal(other.mel_extract(cfg, a), before)  # and the failed handle reserves again from nothing
    other.close()


# ---- CPU: the read-out logic of gpu_power against a stand-in front end ----------------------------------------------------------
class _FloatLogFrontEnd:
    """mel_extract of a float32 front end that is NOT the kernel: oracle mel_power('f32') and a float32 ln2 * log2(P + eps)."""

    def mel_extract(self, cfg, audio_t):
        rows = []
        for y in audio_t.numpy():
            P = omel.mel_power(y, precision="f32", **PROD)
            rows.append(LN2_F32 * np.log2(P + np.float32(LOG_EPS), dtype=np.float32))
        return torch.from_numpy(np.stack(rows).astype(np.float32))


def test_gpu_power_readout_recovers_the_power_to_under_u():
    a = synth.make_audio(3, 2, 20000)
    a[1, :8000] = 0.0                                                          # some all-zero frames
    a[1, 8000:] *= 1e-6                                                        # and a quiet window: |log2 P| ~ 30
    P, y0 = gpu_power(_FloatLogFrontEnd(), None, torch.from_numpy(a))
    want = np.stack([omel.mel_power(y, precision="f32", **PROD) for y in a]).astype(np.float64)
    assert np.array_equal(P == 0.0, want == 0.0) and (want == 0.0).any()
    live = want > 0
    rel = np.abs(P - want)[live] / want[live]
    direct = np.abs(np.exp(y0.numpy().astype(np.float64)) - want)[live] / want[live]
    assert rel.max() < U, rel.max()                                            # the rescaled read-out
    assert direct.max() > 4 * U                                                # against exp() of the float32 logarithm
