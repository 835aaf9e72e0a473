"""Sequence mode with option seq_assemble (km_sequence_plan route 2): each clip's STFT once, the E frames at either end of every
window that see its zero padding from small launches of the unchanged front end, and seq_assemble_kernel (km_seq_assemble.hip)
writing every tile of windows into the front end's own workspace, behind which runs the core km_forward_audio runs on its power
path.  So a window's output is, bit for bit, what km_forward_audio gives on the window's samples: the same rows, the same window
maximum, the same core, the same emotion logit (the engines compute it in its own kernel, emotion_separate, on both calls).

Clips are T hop + 7 hop + 50 samples (8 window positions at stride 1, 4 at stride 2, 3 at stride 3), two clips a call.  On the
fused shape at hop 266 the yardstick is the per-window schedule (seq_per_window) of the same engine.
"""
import numpy as np
import pytest
import torch

import seq_assemble_cases as sc
from core_logit_cases import guarded
from koemorph_amd import _lib, parallel, synth
from koemorph_amd._lib import check
from koemorph_amd.engine import _ptr, _stream_ptr
from oracle import models

pytestmark = pytest.mark.gpu
B = 2
# the shapes whose forward call has a power path, with the switch that opens it at d_model 128
ASSEMBLED = {"d256 w512 hop266": {}, "d512 h8": {}, "fast": {"core128": 1}, "basic": {"core128": 1}, "d64 w32 hop533": {},
             "d64 w32 hop266": {}}

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def make_engine(name, **options):
    e = sc.new_engine(name, emotion_separate=1, **{**ASSEMBLED.get(name, {}), **options})
    e.finalize()
    return e


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = make_engine(name, seq_assemble=1)
        return cache[name]
    yield get
    for e in cache.values():
        e.close()


def clip_audio(name, seed=99):
    return synth.make_audio(seed, B, sc.clip_length(name))


def emotion(name, seed=100):
    return synth.normal(seed, (B, sc.SHAPES[name][3]))


def forward_audio_on_the_windows(e, name, audio, emo, stride):
    """forward_audio on the windows sliced in torch, (B, N, 52): the yardstick of the assembled route."""
    T, hop = sc.SHAPES[name][2], sc.hop_of(name)
    N = sc.num_outputs(audio.shape[1], hop, T, stride)
    wins = torch.stack([audio[b, i * stride * hop:i * stride * hop + T * hop] for b in range(audio.shape[0]) for i in range(N)])
    rows = emo.repeat_interleave(N, dim=0)
    return e.forward_audio(wins.contiguous(), rows.contiguous()).view(audio.shape[0], N, 52)


def route(e, L, stride=1, **kw):
    return e.sequence_plan(L, stride, B, **kw)["route"]


# ---- 1: equal bits with the forward call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("name", list(ASSEMBLED))
def test_equal_bits_with_forward_audio_on_the_windows(engines, name, stride):
    e = engines(name)
    audio, emo = guarded(clip_audio(name)), guarded(emotion(name))
    assert route(e, audio.shape[1], stride) == 2
    got = e.sequence_forward(audio, emo, stride, smooth=False)
    want = forward_audio_on_the_windows(e, name, audio, emo, stride)
    assert got.shape == want.shape == (B, 8 if stride == 1 else 3, 52)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert len({got[0, i].cpu().numpy().tobytes() for i in range(got.shape[1])}) == got.shape[1]      # the windows differ


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("name", ["fused hop266", "fused hop533"])
def test_fused_shape_equals_the_per_window_schedule(name, stride):
    e = make_engine(name, seq_assemble=1)
    audio, emo = guarded(clip_audio(name)), guarded(emotion(name))
    assert route(e, audio.shape[1], stride) == 2
    got = e.sequence_forward(audio, emo, stride, smooth=False)
    smoothed = e.sequence_forward(audio, emo, stride)
    e.set_option("seq_per_window", 1)
    assert route(e, audio.shape[1], stride) == 0
    assert torch.equal(got, e.sequence_forward(audio, emo, stride, smooth=False))
    assert torch.equal(smoothed, e.sequence_forward(audio, emo, stride))
    e.set_option("seq_per_window", 0)
    assert torch.equal(got, forward_audio_on_the_windows(e, name, audio, emo, stride))
    e.close()


@pytest.mark.parametrize("name", ["d64 w32 hop266", "d256 w512 hop266", "fused hop266"])
def test_maps_equal_forward_audio_on_the_windows(name):
    """km_sequence_forward_attn on the assembled route: the chain (or the fused core's ATTN form) behind the same workspace."""
    e = make_engine(name, seq_assemble=1)
    T, hop = sc.SHAPES[name][2], sc.hop_of(name)
    audio, emo = guarded(clip_audio(name)), guarded(emotion(name))
    assert route(e, audio.shape[1], 3, with_attention=True) == 2
    got = e.sequence_forward(audio, emo, 3, smooth=False, return_attention=True)
    wins = torch.stack([audio[b, i * 3 * hop:i * 3 * hop + T * hop] for b in range(B) for i in range(3)]).contiguous()
    want = e.forward_audio(wins, emo.repeat_interleave(3, dim=0).contiguous(), return_attention=True)
    for key in ("blendshapes", "raw", "mel_attention_weights"):
        assert torch.equal(got[key].reshape(want[key].shape), want[key]), key
    e.close()


# ---- 2: schedules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d256 w512 hop266", "fast", "d64 w32 hop266", "fused hop266"])
def test_tiles_track_chunks_second_call_and_graph_replay(name):
    e = make_engine(name, seq_assemble=1)                  # its own engine: the workspace only grows, and tiles of 4 come first
    ED = sc.SHAPES[name][3]
    T, hop = sc.SHAPES[name][2], sc.hop_of(name)
    audio, emo = dev(clip_audio(name)), dev(emotion(name))
    L = audio.shape[1]
    tiles4 = e.sequence_forward(audio, emo, 1, max_tile=4)             # 16 windows: 4 + 4 + 4 + 4
    tiles5 = e.sequence_forward(audio, emo, 1, max_tile=5)             # 5 + 5 + 5 + 1
    one = e.sequence_forward(audio, emo, 1)
    assert torch.equal(tiles4, one) and torch.equal(tiles5, one)
    assert torch.equal(e.sequence_forward(audio, emo, 1), one)         # a second identical call
    # a constant track is one vector per clip (rows: the first window's end, then one every two hops -- four rows for eight windows)
    FIRST, INTERVAL = T * hop, 2 * hop
    K = 1 + (L - FIRST) // INTERVAL
    assert K == 4
    const = emo[:, None, :].expand(B, K, ED).contiguous()
    assert torch.equal(e.sequence_forward_track(audio, const, FIRST, INTERVAL, 1), one)
    # a chunk placed by sample_offset / clip_len equals the matching slice of the whole clip
    trk = dev(synth.normal(193, (B, K, ED)))
    whole = e.sequence_forward_track(audio, trk, FIRST, INTERVAL, 1, smooth=False)
    assert route(e, L) == 2
    differs = False
    for rank in range(2):
        lo, hi, s0, s1 = parallel.sequence_chunk(L, hop, T, 1, whole.shape[1], rank, 2)
        chunk = audio[:, s0:s1].contiguous()
        assert route(e, chunk.shape[1]) == 2
        part = e.sequence_forward_track(chunk, trk, FIRST, INTERVAL, 1, smooth=False, sample_offset=s0, clip_len=L)
        assert part.shape[1] == hi - lo and torch.equal(part, whole[:, lo:hi]), rank
        if rank:
            differs = not torch.equal(e.sequence_forward_track(chunk, trk, FIRST, INTERVAL, 1, smooth=False), whole[:, lo:hi])
    assert differs                                                    # the offsets are what makes them equal
    # the call captured after one eager call, replayed on other samples
    buf = audio.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e.sequence_forward(buf, emo, 1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = e.sequence_forward(buf, emo, 1)
    other = dev(clip_audio(name, seed=123))
    for samples in (other, audio):
        buf.copy_(samples)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, e.sequence_forward(samples, emo, 1))
    assert torch.equal(captured, one)
    del graph
    e.close()


# ---- 3: the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d256 w512 hop266", "fast", "basic"])
def test_sequential_oracle_at_stride_2(engines, name):
    """models.SequentialOracle (its own float64 front end per window) within the 5e-6 that tests/test_gpu_core256w.py and
    tests/test_gpu_core128.py hold for sequence_forward at these shapes."""
    _, H, T, _, fps = sc.SHAPES[name]
    e = engines(name)
    audio, emo = clip_audio(name), emotion(name)
    want = models.SequentialOracle(sc.params_for(name), num_heads=H, mel_sequence_length=T, target_fps=fps, stride_frames=2).forward(audio, emo)
    assert route(e, audio.shape[1], 2) == 2
    got = e.sequence_forward(guarded(audio), guarded(emo), stride_frames=2)
    assert got.shape == (B, 4, 52) and want["num_frames"] == 4
    err = float(np.abs(got.cpu().numpy() - want["blendshapes"]).max())
    print(f"SEQASM|{name}|sequence_forward against the oracle|{err:.3e}")
    assert err < 5e-6


# ---- 4: the dB reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d256 w512 hop266", "basic", "d64 w32 hop266", "fused hop266"])
def test_silent_first_window_and_quiet_after_loud(name):
    e = make_engine(name, seq_assemble=1)
    T, hop = sc.SHAPES[name][2], sc.hop_of(name)
    emo = guarded(emotion(name))
    silent = clip_audio(name, seed=131).copy()
    silent[:, :T * hop + 512] = 0.0                        # window 0 is zeros (window maximum 0), and so is the left edge of window 1
    loud = np.clip(synth.make_audio(132, B, sc.clip_length(name), "uniform") * np.float32(8.0), -1.0, 1.0).astype(np.float32)
    quiet = (clip_audio(name, seed=133) * np.float32(1e-3)).astype(np.float32)
    results = {}
    for label, a in (("silent", silent), ("loud", loud), ("quiet", quiet)):      # a maximum not stored cleanly would move `quiet`
        results[label] = e.sequence_forward(guarded(a), emo, 1, smooth=False)
    f = make_engine(name)                                  # the yardstick on an engine no sequence call has touched
    for label, a in (("silent", silent), ("loud", loud), ("quiet", quiet)):
        ga = guarded(a)
        want = forward_audio_on_the_windows(f, name, ga, emo, 1)
        assert torch.equal(results[label], want), label
        assert torch.equal(forward_audio_on_the_windows(e, name, ga, emo, 1), want), label      # ... and left the workspace clean
    assert not torch.equal(results["quiet"], results["loud"])
    e.close()
    f.close()


# ---- 5: guard regions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d512 h8", "fast", "d64 w32 hop533"])
def test_nothing_outside_out_is_written(engines, name):
    e = engines(name)
    audio, emo = guarded(clip_audio(name)), guarded(emotion(name))
    want = e.sequence_forward(audio, emo, 1)
    out = guarded(np.zeros((B, 8, 52), np.float32))
    check(e._lib.km_sequence_forward(e._h, _ptr(audio), B, audio.shape[1], _ptr(emo), 1, 1, _ptr(out), _stream_ptr(audio.device)))
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    base = out._base
    assert base.numel() == out.numel() + 2 * 1280
    assert torch.isnan(base[:1280]).all() and torch.isnan(base[-1280:]).all()
    for t in (audio, emo):
        assert torch.isnan(t._base[:1280]).all() and torch.isnan(t._base[-1280:]).all() and not torch.isnan(t).any()


# ---- 6, 7: with the option off -------------------------------------------------------------------------------------------------
def test_fused_shape_at_hop_266_runs_per_window_by_default():
    """Frames 1 and T - 1 of a window see its padding at hop 266 and the fused core takes only frames 0 and T from the edge image: the
    images-read-by-the-core schedule is for hop >= n_fft / 2 alone (clip_frames_shared).  Before the guard this shape took it and
    differed from the per-window schedule by up to 4.4e-5 on these clips (measured with the library of the commit before)."""
    name = "fused hop266"
    e = make_engine(name)
    audio, emo = guarded(clip_audio(name)), guarded(emotion(name))
    assert route(e, audio.shape[1]) == 0
    got = e.sequence_forward(audio, emo, 1, smooth=False)
    e.set_option("seq_per_window", 1)
    want = e.sequence_forward(audio, emo, 1, smooth=False)
    print(f"SEQASM|{name}|default against per-window|{float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want)
    assert torch.equal(got, forward_audio_on_the_windows(e, name, audio, emo, 1))
    e.close()


@pytest.mark.parametrize("name", ["d256 w512 hop266", "fused hop533"])
def test_the_default_route_is_untouched(name):
    e = make_engine(name)
    audio, emo = guarded(clip_audio(name)), guarded(emotion(name))
    assert route(e, audio.shape[1]) == (1 if name == "fused hop533" else 0)
    got = e.sequence_forward(audio, emo, 1)
    e.set_option("seq_per_window", 1)
    assert route(e, audio.shape[1]) == 0
    assert torch.equal(got, e.sequence_forward(audio, emo, 1))
    e.close()


# ---- 8: memory ------------------------------------------------------------------------------------------------------------------
def test_the_images_go_with_the_engine():
    live = _lib.load().km_live_device_bytes
    base = live()
    e = make_engine("d64 w32 hop266", seq_assemble=1)
    held = live()
    e.sequence_forward(dev(clip_audio("d64 w32 hop266")), dev(emotion("d64 w32 hop266")), 1)
    torch.cuda.synchronize()
    assert live() > held > base                            # the workspace and the clip / edge images
    e.close()
    assert live() == base


def test_model_option_sets_the_engine_switch():
    from koemorph_amd.model import SequentialDualStreamModel
    torch.manual_seed(0)
    m = SequentialDualStreamModel(d_model=64, num_heads=4, mel_sequence_length=32, target_fps=60, share_frames=True).cuda().eval()
    plain = SequentialDualStreamModel(d_model=64, num_heads=4, mel_sequence_length=32, target_fps=60).cuda().eval()
    plain.load_state_dict(m.state_dict())
    audio, emo = dev(clip_audio("d64 w32 hop266")), dev(emotion("d64 w32 hop266"))
    with torch.no_grad():
        got = m(audio, emotion_features=emo)["blendshapes"]
        want = plain(audio, emotion_features=emo)["blendshapes"]
    L = audio.shape[1]
    eng = m.dual_stream_attention.engine()
    assert eng.sequence_plan(L)["route"] == 2
    assert plain.dual_stream_attention.engine().sequence_plan(L)["route"] == 0
    assert got.shape == want.shape == (B, 8, 52)
    assert torch.equal(got, eng.sequence_forward(audio, emo, 1, smooth=m.use_temporal_smoothing))
    print(f"SEQASM|model share_frames against the default schedule|{float((got - want).abs().max()):.3e}")
    m.share_frames = False                                 # ... and the switch follows the attribute back
    with torch.no_grad():
        assert torch.equal(m(audio, emotion_features=emo)["blendshapes"], want)
    assert eng.sequence_plan(L)["route"] == 0
