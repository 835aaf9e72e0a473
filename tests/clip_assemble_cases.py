"""Shapes, hops, switches and the host restatement of km_clip_plan shared by tests/test_clip_assemble_host.py and
tests/test_gpu_clip_assemble.py.  Not a test module.

The windows of a batch start at start[b] hop inside one clip.  A window of T hop samples has STFT frames f = 0 .. T; the E =
ceil((n_fft / 2) / hop) frames at either end see its zero padding (koemorph_amd.clip_span.edge_frames), every other frame is a
frame of the clip.  The three schedules of a resident-clip call:

  route 0   refused: the wrappers gather the windows and every window's T + 1 frames are computed, B (T + 1)
  route 1   the default shared route: the span + frames 0 and T of every window, span + 2 B; hop >= n_fft / 2, and the packing
            front end (training) or the fused core (forward); whatever option clip_assemble says
  route 2   option clip_assemble where route 1 does not hold: the span + two snippets of 2 E frames per window, span + 4 E B

with span = max_start - min_start + T + 1 rows.
"""
import numpy as np

import seq_assemble_cases as sc
from koemorph_amd import _lib, synth
from koemorph_amd.clip_span import edge_frames
from koemorph_amd.engine import Engine, MelConfig

N_FFT = 1024
HOPS = {533: 30, 266: 60, 200: 80, 128: 125}          # hop: the target fps MelConfig.model_batch turns into it (E = 1, 2, 3, 4)
# the (d_model, heads, window, emotion_dim) of tests/seq_assemble_cases.py, each once
SHAPES = {"fused": (256, 8, 256, 256), "d256 w512": (256, 8, 512, 256), "d512 h8": (512, 8, 512, 256), "d512 h16": (512, 16, 512, 256),
          "fast": (128, 4, 128, 256), "basic": (128, 4, 256, 9), "d64 w32": (64, 4, 32, 256)}
SEQ_NAME = {"fused": "fused hop533", "d256 w512": "d256 w512 hop266", "d512 h8": "d512 h8", "d512 h16": "d512 h16", "fast": "fast",
            "basic": "basic", "d64 w32": "d64 w32 hop533"}          # the entry of sc.SHAPES with the same d_model, heads and window
assert all(sc.SHAPES[SEQ_NAME[k]][:4] == v for k, v in SHAPES.items())
TRAIN, FORWARD, FORWARD_ATTN = 1, 0, 2


def mel_config(hop, reflect=False):
    m = MelConfig.model_batch(target_fps=HOPS[hop])
    assert m.hop_length == hop
    if reflect:
        m.pad_mode = _lib.KM_PAD_REFLECT
    return m


def params_for(name, seed=sc.PARAM_SEED):
    d, _, T, ED = SHAPES[name]
    return synth.make_core_params(seed, d, T, ED, "trained")


def new_engine(name, hop, reflect=False, params=None, **options):
    """An engine of the shape at the hop with its parameters loaded and the switches set; the caller finalizes it."""
    d, H, T, ED = SHAPES[name]
    e = Engine(d_model=d, num_heads=H, mel_sequence_length=T, emotion_dim=ED, mel=mel_config(hop, reflect))
    e.load_state_dict(params if params is not None else params_for(name))
    e.set_option("core_split", 0)
    for k, v in options.items():
        e.set_option(k, v)
    return e


def edges_per_side(hop, T):
    """E, from the list of edge frames itself: they are 0 .. E - 1 and T - E + 1 .. T (where the two ends do not meet)."""
    E = -(-(N_FFT // 2) // hop)
    if T + 1 >= 2 * E:
        assert edge_frames(hop, T, N_FFT) == list(range(E)) + list(range(T - E + 1, T + 1))
    return E


def expected_plan(name, hop, opts, B, lo, hi, mode, reflect=False):
    d, H, T, _ = SHAPES[name]
    o = lambda k: bool(opts.get(k, 0))
    E = edges_per_side(hop, T)
    span = hi - lo + T + 1
    rp = not o("mel_two_frame")
    only_0_and_T = edge_frames(hop, T, N_FFT) == [0, T] and not reflect          # clip_frames_shared
    packs = rp and not o("train_no_fe_pack") and not o("train_no_dma")            # the front end writes the packed training input
    fused = (d, H, T) == (256, 8, 256)
    if mode == TRAIN:
        today, base = only_0_and_T and packs, packs
    else:
        today = fused and rp and only_0_and_T
        base = rp and sc.has_power_path(SEQ_NAME[name], opts, mode == FORWARD_ATTN)
    if today:
        route, frames = 1, span + 2 * B
    elif o("clip_assemble") and base and not reflect and T + 1 >= 2 * E:
        route, frames = 2, span + 4 * E * B
    else:
        route, frames = 0, B * (T + 1)
    return {"route": route, "span_rows": span, "stft_frames": frames, "edge_frames_per_side": E}


def stft_power(frame):
    """float64 power spectrum of one n_fft-sample frame under a periodic Hann window."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    return np.abs(np.fft.rfft(frame.astype(np.float64) * w)) ** 2


def centred_frames(samples, hop, n_frames):
    """Frames 0 .. n_frames - 1 of `samples` as the front end cuts them: centred at f hop, zeros on either side."""
    padded = np.concatenate([np.zeros(N_FFT // 2), samples.astype(np.float64), np.zeros(N_FFT // 2 + hop)])
    return [padded[f * hop:f * hop + N_FFT] for f in range(n_frames)]
