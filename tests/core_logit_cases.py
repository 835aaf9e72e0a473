"""Parameter sets, inputs, planted faults and the judging harness shared by tests/test_gpu_core_logit.py and
tests/test_gpu_generic_shapes.py (the kernels against the float64 oracle in logit space) and tests/test_oracle_core.py (the same
measure on a stand-in kernel, without a GPU).  Not a test module."""
import numpy as np

from koemorph_amd import synth
from oracle import core

K = 4.0          # the factor of the bound; how it was chosen: the docstring of tests/test_gpu_core_logit.py


# ---- parameter sets ------------------------------------------------------------------------------------------------------------
def make_params(kind, seed, d=256, T=256, emotion_dim=256):
    """init: synth's style.  trained: synth's style with the decoder's output weight halved -- as synth scales it, the logit of
    some seeds and shapes reaches 13, and the measure wants |z| <= 8 (every case asserts it).  The others start from `trained`:
    sharp    mouth queries x 6 and the key projection x 6: the largest score of a row leads the next by tens of units, rows are
             close to one-hot, most exponentials of the base-2 softmax underflow and the max subtraction carries the result
    bias0    mel_channel_encoder.bias = 0: a mel channel that is zero in every frame encodes to exactly 0, variance exactly 0,
             and LayerNorm must return beta
    offset   mel_channel_encoder.bias += 40: mean >> standard deviation in the LayerNorm input, where E[y^2] - E[y]^2 cancels"""
    base = "init" if kind == "init" else "trained"
    p = synth.make_core_params(seed, d, T, emotion_dim, style=base)
    if kind != "init":
        p["blendshape_decoder.3.weight"] = (p["blendshape_decoder.3.weight"] * np.float32(0.5)).astype(np.float32)
    if kind == "sharp":
        p["mouth_queries"] = (p["mouth_queries"] * np.float32(6.0)).astype(np.float32)
        w = p["mel_attention.in_proj_weight"].copy()
        w[d:2 * d] *= np.float32(6.0)
        p["mel_attention.in_proj_weight"] = w
    elif kind == "bias0":
        p["mel_channel_encoder.bias"] = np.zeros_like(p["mel_channel_encoder.bias"])
    elif kind == "offset":
        p["mel_channel_encoder.bias"] = (p["mel_channel_encoder.bias"] + np.float32(40.0)).astype(np.float32)
    elif kind not in ("init", "trained"):
        raise KeyError(kind)
    return p


PARAM_KINDS = ("init", "trained", "sharp", "bias0", "offset")


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def make_inputs(kind, seed, B, t_in, T=256, n_mels=80, emotion_dim=256):
    """(mel (B, t_in, n_mels), short (B, 3, n_mels), emotion (B, emotion_dim)).  Rows of `mel` from T on are NaN: the core truncates
    to T rows, and a kernel that multiplied the surplus rows by zero instead of skipping them would turn NaN.
    mel01 / randn  synth's styles
    const          every frame of a window is the same row (and the three short frames another one)
    zeroch         mel01 with channels 0, 37 n_mels / 80 and n_mels - 1 zero in every frame, short ones included (with `bias0`: zero
                   variance); 0, 37 and 79 of 80 channels
    huge           mel01 with one entry of 1e4 in one frame of every window, and one in a short frame of window 0
    denorm         mel01 x 1e-39: float32 subnormals"""
    style = "randn" if kind == "randn" else "mel01"
    mel, short, emo = synth.make_core_inputs(seed, B, t_in, n_mels=n_mels, emotion_dim=emotion_dim, style=style)
    mel, short = mel.copy(), short.copy()
    zero = sorted({0, 37 * n_mels // 80, n_mels - 1})
    if kind == "const":
        mel[:] = mel[:, :1]
        short[:] = short[:, :1]
    elif kind == "zeroch":
        mel[:, :, zero] = 0.0
        short[:, :, zero] = 0.0
    elif kind == "huge":
        for b in range(B):
            mel[b, (17 * b + min(t_in, T) - 1) % min(t_in, T), (29 * b + 5) % n_mels] = 1e4
        short[0, 1, 63 % n_mels] = 1e4
    elif kind == "denorm":
        mel = (mel.astype(np.float64) * 1e-39).astype(np.float32)
        short = (short.astype(np.float64) * 1e-39).astype(np.float32)
    elif kind not in ("mel01", "randn"):
        raise KeyError(kind)
    if t_in > T:
        mel[:, T:] = np.nan
    return mel, short, emo


INPUT_KINDS = ("mel01", "randn", "const", "zeroch", "huge", "denorm")


# ---- planted faults, as the float32 oracle would compute them (a stand-in for a kernel that has the fault) -------------------------
def _scale_rows(p, key, rows, f, bias_key=None):
    q = dict(p)
    w = q[key].copy()
    w[rows] *= np.float32(f)
    q[key] = w
    if bias_key is not None:
        b = q[bias_key].copy()
        b[rows] *= np.float32(f)
        q[bias_key] = b
    return q


def apply_fault(name, params, mel, short, emo, T=256):
    """(params, mel, short, emo, core_forward keywords) with the fault planted."""
    d = params["mel_channel_encoder.weight"].shape[0]
    kw = {}
    if name == "none":
        pass
    elif name == "short_reversed":                       # short-term frames staged in reverse order
        short = short[:, ::-1].copy()
    elif name == "last_long_row":                        # row T-1 replaced by row T-2
        mel = mel.copy()
        mel[:, T - 1] = mel[:, T - 2]
    elif name == "ln_eps":                               # LayerNorm epsilon 1e-5 -> 1e-6
        kw["ln_eps"] = 1e-6
    elif name == "softmax_scale":                        # the scale of q k^T x 1.0005 (= the query projection x 1.0005)
        params = _scale_rows(params, "mel_attention.in_proj_weight", slice(0, d), 1.0005, "mel_attention.in_proj_bias")
    elif name == "value_column":                         # one output column of the value projection x 1.001
        params = _scale_rows(params, "mel_attention.in_proj_weight", 2 * d + 5, 1.001, "mel_attention.in_proj_bias")
    elif name == "emotion_last_column":                  # the emotion encoder's last input column dropped
        params = dict(params)
        w = params["emotion_encoder.weight"].copy()
        w[:, -1] = 0.0
        params["emotion_encoder.weight"] = w
    elif name == "one_query":                            # one mouth query x 1.001 (the smallest fault of the sensitivity table)
        params = _scale_rows(params, "mouth_queries", 3, 1.001)
    else:
        raise KeyError(name)
    return params, mel, short, emo, kw


FAULTS = ("short_reversed", "last_long_row", "ln_eps", "softmax_scale", "value_column", "emotion_last_column")


# ---- guarded device views ------------------------------------------------------------------------------------------------------
def guarded(x, guard=1280, n_mels=None):
    """x on the device as a view into a larger NaN-filled allocation: `guard` floats of NaN (16 rows of 80) before the first
    element and after the last, so a read outside the tensor meets NaN.  The default keeps the 16-byte alignment of the rows
    (the kernels read them as float4); guard = 1281 puts the view 4 bytes off it (the emotion vectors are read word by word).
    With n_mels the guard is 16 rows of n_mels channels: 16 n_mels floats, a multiple of 4 floats for any channel count."""
    import torch
    if n_mels is not None:
        guard = 16 * n_mels
    x = np.ascontiguousarray(x, dtype=np.float32)
    buf = torch.full((x.size + 2 * guard,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[guard:guard + x.size].view(*x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * guard
    return view


# ---- engines and the judge (the bound: the docstring of tests/test_gpu_core_logit.py) --------------------------------------------------
EMA_ROUNDINGS = 5.0


def engine_for(params, **kw):
    from koemorph_amd.engine import Engine
    e = Engine(**kw)
    e.load_state_dict(params)
    e.finalize()
    e.set_option("core_split", 0)          # the split-bf16 images are opt-in and no case here opts in
    return e


def judge(group, label, ref, s=None, a=None, extra=None, out_over_c=False):
    """Assert the bound on the sigmoid values `s` (B, 52) and / or the attention map `a` (B, 28, 80).  out_over_c: `s` was recovered
    as out / c_i and the bound holds three storage terms instead of one (core.logit_bound); `extra` is a derived per-entry term
    added to the bound (the EMA recovery)."""
    zmax = float(np.abs(ref["z64"]).max())
    assert zmax <= core.LOGIT_Z_MAX, f"{group} {label}: |z64| reaches {zmax}, choose other parameters"
    e_max = e_ratio = a_max = a_ratio = float("nan")
    if s is not None:
        e_max, e_ratio = core.logit_verdict(s, ref, K, core.OUT_OVER_C_ROUNDINGS if out_over_c else 1, extra)
    if a is not None:
        a_max, a_ratio = core.attention_verdict(a, ref, K)
    print(f"CORELOGIT|{group}|{label}|{e_max:.3e}|{ref['yard_e']:.3e}|{e_ratio:.3f}|{a_max:.3e}|{ref['yard_a']:.3e}|{a_ratio:.3f}")
    if s is not None:
        assert e_ratio <= 1.0, f"{group} {label}: logit error {e_max:.3e} is {e_ratio:.2f} x its bound (float32 yardstick {ref['yard_e']:.3e})"
    if a is not None:
        assert a_ratio <= 1.0, f"{group} {label}: attention error {a_max:.3e} is {a_ratio:.2f} x its bound (yardstick {ref['yard_a']:.3e})"


def ema_term(x64, prev, params):
    """The rounding of the float32 EMA as seen through undo_ema, in the units of logit_error (see the module docstring)."""
    alpha = 1.0 / (1.0 + np.exp(-0.8))
    c = core.stream_coefficients(params)
    s64 = x64 / c
    return EMA_ROUNDINGS * core.LOGIT_U * np.maximum(x64, prev) / (alpha * c * s64 * (1.0 - s64))


def run_core(e, group, label, params, inputs, H=8, T=256):
    """core_forward with and without the attention outputs on guarded views; `raw`, out / c_i of both calls and the map judged."""
    mel, short, emo = inputs
    ref = core.logit_reference(params, mel, short, emo, num_heads=H, mel_sequence_length=T)
    gm, gs, ge = guarded(mel), guarded(short), guarded(emo)
    o = e.core_forward(gm, gs, ge, return_attention=True)
    o2 = e.core_forward(gm, gs, ge)
    judge(group, label + " raw", ref, s=o["raw"].cpu().numpy(), a=o["mel_attention_weights"].cpu().numpy())
    judge(group, label + " out/c", ref, s=core.recover_sigmoid(o["blendshapes"].cpu().numpy(), params), out_over_c=True)
    judge(group, label + " out/c noattn", ref, s=core.recover_sigmoid(o2["blendshapes"].cpu().numpy(), params), out_over_c=True)
    # raw and the recovery agree to the storage of both (c_i s is one more float32 product)
    d = np.abs(core.recover_sigmoid(o["blendshapes"].cpu().numpy(), params) - o["raw"].cpu().numpy().astype(np.float64))
    assert (d <= 3 * core.LOGIT_U * ref["s64"] + 1e-45).all(), (group, label, float(d.max()))
    return ref, o
