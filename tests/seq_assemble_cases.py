"""Shapes, switches and the host restatement of km_sequence_plan shared by tests/test_seq_assemble_host.py and
tests/test_gpu_seq_assemble.py.  Not a test module.

A window of T hop samples has STFT frames f = 0 .. T, frame f covering its samples [f hop - n_fft / 2, f hop + n_fft / 2).  The
frames that leave the window see its zero padding and belong to it alone (koemorph_amd.clip_span.edge_frames): E = ceil((n_fft / 2) /
hop) at either end.  Every other frame is a frame of the clip.  The three schedules of sequence mode differ in what they compute:

  route 0   per window: B N (T + 1) frames
  route 1   the clip once + frames 0 and T of every window, read by the fused core: B (nfc + 2 N), right only where E = 1
  route 2   option seq_assemble: the clip once + E left-edge rows and E launches of two rows per window (row 0 of each is frame 0
            again and is discarded), assembled into the front end's workspace: B (nfc + 3 E N)

with nfc = (N - 1) stride + T + 1 clip frames.
"""
from koemorph_amd import synth
from koemorph_amd.clip_span import edge_frames
from koemorph_amd.engine import Engine, MelConfig

N_FFT = 1024
# name: (d_model, heads, window T, emotion_dim, target fps of the front end)
SHAPES = {
    "fused hop533": (256, 8, 256, 256, 30), "fused hop266": (256, 8, 256, 256, 60),
    "d256 w512 hop266": (256, 8, 512, 256, 60),
    "d512 h8": (512, 8, 512, 256, 60), "d512 h16": (512, 16, 512, 256, 60),
    "fast": (128, 4, 128, 256, 30), "basic": (128, 4, 256, 9, 30),
    "d64 w32 hop533": (64, 4, 32, 256, 30), "d64 w32 hop266": (64, 4, 32, 256, 60),
}
PARAM_SEED = 55


def hop_of(name):
    return int(16000 / SHAPES[name][4])


def params_for(name):
    d, _, T, ED, _ = SHAPES[name]
    return synth.make_core_params(PARAM_SEED, d, T, ED, "trained")


def new_engine(name, **options):
    """An engine of the shape with its parameters loaded and the switches set; the caller finalizes it (host or device)."""
    d, H, T, ED, fps = SHAPES[name]
    e = Engine(d_model=d, num_heads=H, mel_sequence_length=T, emotion_dim=ED, mel=MelConfig.model_batch(target_fps=fps))
    e.load_state_dict(params_for(name))
    e.set_option("core_split", 0)
    for k, v in options.items():
        e.set_option(k, v)
    return e


def clip_length(name, extra_frames=7):
    """T hop + 7 hop + 50 samples: 8 window positions at stride 1, 4 at stride 2, 3 at stride 3."""
    _, _, T, _, _ = SHAPES[name]
    hop = hop_of(name)
    return T * hop + extra_frames * hop + 50


def edges_per_side(hop, T):
    """E, from the list of edge frames itself: they are 0 .. E - 1 and T - E + 1 .. T."""
    edges = edge_frames(hop, T, N_FFT)
    E = sum(1 for f in edges if 2 * f < T)
    assert edges == list(range(E)) + list(range(T - E + 1, T + 1)) and E == -(-(N_FFT // 2) // hop)
    return E


def num_outputs(L, hop, T, stride):
    return max(1, (L // hop - T) // stride + 1)


def has_power_path(name, opts, with_attention):
    """km_forward_audio goes power-mel -> core with the dB conversion inside: the fused core, or a generic core that converts."""
    d, H, T, _, _ = SHAPES[name]
    o = lambda k: bool(opts.get(k, 0))
    if (d, H, T) == (256, 8, 256):
        return True
    takes_power = d in (512, 256, 64) and not o("no_ln_fusion") and not o("no_db_fusion")
    core128 = (d == 128 and H == 4 and T in (128, 256) and o("core128") and not with_attention and
               not any(o(k) for k in ("no_ln_fusion", "no_score_fusion", "no_out_fusion", "no_v_fusion", "no_core_merge", "no_db_fusion")))
    return (takes_power or core128) and not o("generic_staged")


def expected_plan(name, opts, L, stride, B, with_attention=False):
    d, H, T, _, _ = SHAPES[name]
    hop = hop_of(name)
    E = edges_per_side(hop, T)
    N = num_outputs(L, hop, T, stride)
    nfc = (N - 1) * stride + T + 1
    o = lambda k: bool(opts.get(k, 0))
    fused = (d, H, T) == (256, 8, 256)
    shared_ok = not o("seq_per_window") and not o("mel_two_frame")
    if o("seq_assemble") and shared_ok and has_power_path(name, opts, with_attention) and T + 1 >= 2 * E and L >= T * hop:
        route, frames = 2, B * (nfc + N * 3 * E)
    elif fused and shared_ok and 2 * hop >= N_FFT:
        route, frames = 1, B * (nfc + 2 * N)
    else:
        route, frames = 0, B * N * (T + 1)
    return {"route": route, "N": N, "stft_frames": frames, "edge_frames_per_side": E}
