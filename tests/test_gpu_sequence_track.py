"""Sequence mode with a per-window emotion input from each clip's emotion track (km_sequence_forward_track,
``Engine.sequence_forward_track``, ``SequentialDualStreamModel(clip_emotion=...)``, ``scripts.render_sequential``).

Which row a window takes is pinned on the host (tests/test_seq_track_host.py).  Here: the values against the per-window float64
oracle of tests/seq_track_cases.py at the bound tests/test_gpu_models.py holds sequence mode to (5e-6), and bit for bit against
every other way of computing the same thing -- the per-window schedule, another tile size, one vector per clip when the track is
constant, ``forward_clip`` on the rows ``ClipEmotion.rows`` gathers, and the chunks ``parallel.sequence_chunk`` hands the ranks.
"""
import functools
import json
import logging

import numpy as np
import pytest
import torch

import seq_track_cases as sc
from koemorph_amd import parallel, synth
from koemorph_amd._lib import KM_ERR_INVALID_ARG
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.features import ClipEmotion
from koemorph_amd.model import DualStreamCrossAttention, SequentialDualStreamModel
from koemorph_amd.scripts import render_sequential

pytestmark = pytest.mark.gpu

HOP, T = sc.HOP, sc.T
CASES = [(20, 1), (9, 2), (-40, 1)]


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def full_state(params, alpha=0.8):
    sd = {"dual_stream_attention." + k: torch.from_numpy(v) for k, v in params.items()}
    sd["smoothing_alpha"] = torch.tensor(alpha)
    return sd


@functools.lru_cache(maxsize=None)
def engine():
    m = DualStreamCrossAttention().cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sc.params().items()})
    return m, m.engine()


@functools.lru_cache(maxsize=None)
def layer():
    torch.manual_seed(4321)
    return torch.nn.Linear(264, 256)


@functools.lru_cache(maxsize=None)
def clip_emotion():
    return ClipEmotion(compression_layer=layer())


@functools.lru_cache(maxsize=None)
def built_track(extra):
    """The emotion tracks of the test clips, built once: (B, K, 256) on the device."""
    emotion, _ = clip_emotion().build_batch(dev(sc.audio(extra)))
    return emotion


# ---- 1: against the per-window float64 oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", ["track", "identity"])
@pytest.mark.parametrize("extra,stride", CASES)
def test_sequence_with_a_track_matches_the_per_window_oracle(extra, stride, mapping):
    L = sc.clip_length(extra)
    N = sc.num_outputs(L, stride)
    if mapping == "track":
        K, first, interval = sc.num_rows(L), sc.FIRST, sc.INTERVAL
    else:
        K, first, interval = N, T * HOP, stride * HOP
    rows = sc.window_rows(L, stride, K, first, interval)
    if mapping == "identity":
        assert rows == list(range(N))
    elif (extra, stride) == (20, 1):
        assert K == 30 and rows == [26] * 3 + [27] * 9 + [28] * 9
    elif extra == -40:
        assert N == 1 and K == 23 and rows == [22]                                # the clamp to K - 1
    trk = sc.track(K)
    orc = sc.production_oracle()
    want = sc.sequence_with_rows(orc, sc.audio(extra), trk, stride, rows, smooth=True)
    _, eng = engine()
    got = eng.sequence_forward_track(dev(sc.audio(extra)), dev(trk), first, interval, stride).cpu().numpy()
    assert got.shape == want.shape == (sc.CLIPS, N, 52)
    err = float(np.abs(got - want).max())
    print(f"extra {extra} stride {stride} {mapping}: K {K}, N {N}, max |got - oracle| = {err:.3g}")
    if rows != [0] * N:
        # a wrong row cannot pass: the oracle with row 0 alone is somewhere else (a single window on row 0 has no other row to take)
        row0 = sc.sequence_with_rows(orc, sc.audio(extra), trk, stride, [0] * N, smooth=True)
        assert np.abs(want - row0).max() > 1e-3
    assert err < 5e-6


# ---- 2: schedules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,stride", CASES)
def test_shared_frame_per_window_and_tiles_are_bit_identical_with_a_track(extra, stride):
    L = sc.clip_length(extra)
    trk = dev(sc.track(sc.num_rows(L)))
    audio = dev(sc.audio(extra))
    _, eng = engine()
    shared = eng.sequence_forward_track(audio, trk, sc.FIRST, sc.INTERVAL, stride, max_tile=4096)
    tiled = eng.sequence_forward_track(audio, trk, sc.FIRST, sc.INTERVAL, stride, max_tile=7)
    eng.set_option("seq_per_window", 1)
    try:
        per_window = eng.sequence_forward_track(audio, trk, sc.FIRST, sc.INTERVAL, stride, max_tile=7)
    finally:
        eng.set_option("seq_per_window", 0)
    assert torch.equal(shared, per_window) and torch.equal(shared, tiled)


# ---- 3: a constant track is one vector per clip ------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,stride", CASES)
def test_constant_track_equals_one_vector_per_clip(extra, stride):
    L = sc.clip_length(extra)
    K = sc.num_rows(L)
    v = dev(synth.normal(192, (sc.CLIPS, 256)))
    trk = v[:, None, :].expand(sc.CLIPS, K, 256).contiguous()
    audio = dev(sc.audio(extra))
    _, eng = engine()
    before = eng.sequence_forward(audio, v, stride, True)
    got = eng.sequence_forward_track(audio, trk, sc.FIRST, sc.INTERVAL, stride, True)
    after = eng.sequence_forward(audio, v, stride, True)                          # ... and the track call leaves that path as it was
    assert torch.equal(got, before) and torch.equal(after, before)


# ---- 4: a built track, against forward_clip on the rows ClipEmotion.rows gathers ----------------------------------------------------
@pytest.mark.parametrize("extra,stride", [(20, 1), (9, 2)])
def test_built_track_equals_forward_clip_on_the_gathered_rows(extra, stride):
    L = sc.clip_length(extra)
    N = sc.num_outputs(L, stride)
    audio = dev(sc.audio(extra))
    ce, trk = clip_emotion(), built_track(extra)
    assert trk.shape == (sc.CLIPS, sc.num_rows(L), 256)
    _, eng = engine()
    got = eng.sequence_forward_track(audio, trk, ce.shape["min_samples"], ce.shape["update_samples"], stride, smooth=False)
    starts = np.arange(N, dtype=np.int32) * stride
    for c in range(sc.CLIPS):
        rows = ce.rows(trk[c], L, dev(starts), HOP, T)
        want = eng.forward_clip(audio[c], starts, rows)
        assert torch.equal(got[c], want), (c, float((got[c] - want).abs().max()))
        assert len({rows[i].cpu().numpy().tobytes() for i in range(N)}) > 1      # the windows do not all use one row


# ---- 5: chunks of a clip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("extra,stride", [(20, 1), (9, 2)])
def test_chunks_with_offsets_equal_the_whole_call(extra, stride, world):
    L = sc.clip_length(extra)
    N = sc.num_outputs(L, stride)
    audio, trk = dev(sc.audio(extra)), dev(sc.track(sc.num_rows(L)))
    _, eng = engine()
    whole = eng.sequence_forward_track(audio, trk, sc.FIRST, sc.INTERVAL, stride, smooth=False)
    differs = False
    for rank in range(world):
        lo, hi, s0, s1 = parallel.sequence_chunk(L, HOP, T, stride, N, rank, world)
        assert hi > lo
        chunk = audio[:, s0:s1].contiguous()
        part = eng.sequence_forward_track(chunk, trk, sc.FIRST, sc.INTERVAL, stride, smooth=False, sample_offset=s0, clip_len=L)
        assert part.shape[1] == hi - lo and torch.equal(part, whole[:, lo:hi]), rank
        if rank:
            alone = eng.sequence_forward_track(chunk, trk, sc.FIRST, sc.INTERVAL, stride, smooth=False)
            differs = differs or not torch.equal(alone, whole[:, lo:hi])
    assert differs                                                                # the offsets are what makes them equal


def test_sequence_apply_without_a_process_group_takes_the_track():
    L = sc.clip_length(9)
    audio, trk = dev(sc.audio(9)), dev(sc.track(sc.num_rows(L)))
    _, eng = engine()
    a = parallel.sequence_apply(eng, audio, None, 2, emotion_track=trk, track_shape=(sc.FIRST, sc.INTERVAL))
    assert torch.equal(a, eng.sequence_forward_track(audio, trk, sc.FIRST, sc.INTERVAL, 2))


# ---- 6: the generic path --------------------------------------------------------------------------------------------------------
def test_generic_path_small_shape_matches_the_per_window_oracle():
    d, Tw, H, seed = 64, 32, 4, 56
    params = synth.make_core_params(seed, d, Tw, 256, "trained")
    eng = Engine(d_model=d, num_heads=H, mel_sequence_length=Tw, mel=MelConfig.model_batch(target_fps=30))
    eng.load_state_dict(params)
    eng.finalize()
    L = Tw * HOP + 4 * HOP + 50
    for stride in (1, 2):
        N = sc.num_outputs(L, stride, HOP, Tw)
        assert N == (5 if stride == 1 else 3)
        clips = synth.make_audio(103, 3, L)
        trk = synth.normal(104, (3, N, 256))
        rows = sc.window_rows(L, stride, N, Tw * HOP, stride * HOP, HOP, Tw)
        assert rows == list(range(N))
        orc = sc.WindowOracle(params, num_heads=H, mel_sequence_length=Tw)
        want = sc.sequence_with_rows(orc, clips, trk, stride, rows, smooth=True)
        got = eng.sequence_forward_track(dev(clips), dev(trk), Tw * HOP, stride * HOP, stride, max_tile=4).cpu().numpy()
        err = float(np.abs(got - want).max())
        print(f"generic d{d} T{Tw} stride {stride}: max |got - oracle| = {err:.3g}")
        assert np.abs(want - sc.sequence_with_rows(orc, clips, trk, stride, [0] * N, smooth=True)).max() > 1e-3
        assert err < 5e-6
    eng.close()


# ---- 7: the model ---------------------------------------------------------------------------------------------------------------
def test_model_with_clip_emotion_builds_the_track_itself(caplog):
    extra, stride = 9, 2
    audio = dev(sc.audio(extra))
    ce = clip_emotion()
    m = SequentialDualStreamModel(stride_frames=stride, clip_emotion=ce).cuda().eval()
    m.load_state_dict(full_state(sc.params()))
    builds = ce.builds
    with caplog.at_level(logging.WARNING):
        auto = m(audio)
    assert ce.builds == builds + 1
    assert not [r for r in caplog.records if "dummy features" in r.getMessage()]
    assert auto["emotion_backend"] == "egemaps_track" and auto["num_frames"] == sc.num_outputs(sc.clip_length(extra), stride)
    explicit = m(audio, emotion_track=ce.build_batch(audio)[0])
    assert torch.equal(auto["blendshapes"], explicit["blendshapes"])
    _, eng = engine()
    sh = ce.shape
    assert torch.equal(auto["blendshapes"], eng.sequence_forward_track(audio, built_track(extra), sh["min_samples"], sh["update_samples"], stride))
    ga = m(audio, return_attention=True)
    assert torch.allclose(ga["blendshapes"], auto["blendshapes"], atol=1e-6)
    assert ga["mel_attention_weights"].shape == (sc.CLIPS, auto["num_frames"], 28, 80)
    with pytest.raises(ValueError, match="pass one of them"):
        m(audio, emotion_features=dev(synth.normal(1, (sc.CLIPS, 256))), emotion_track=built_track(extra))
    # an explicit vector per clip still takes the old path
    v = dev(synth.normal(193, (sc.CLIPS, 256)))
    assert torch.equal(m(audio, emotion_features=v)["blendshapes"], eng.sequence_forward(audio, v, stride))


def test_track_without_rows_is_a_zero_row():
    """K = 0 (a clip shorter than the first update) stands for one zero row per clip, what ClipEmotion.rows gives such clips."""
    audio = dev(sc.audio(-40))
    _, eng = engine()
    got = eng.sequence_forward_track(audio, torch.empty(sc.CLIPS, 0, 256, device="cuda"), sc.FIRST, sc.INTERVAL)
    assert torch.equal(got, eng.sequence_forward(audio, torch.zeros(sc.CLIPS, 256, device="cuda")))


def test_refusals_on_a_finalized_handle():
    _, eng = engine()
    audio = dev(sc.audio(-40))
    L = audio.shape[1]
    out = torch.empty(sc.CLIPS, 1, 52, device="cuda")
    trk = dev(sc.track(3))

    def call(K=3, first=8000, interval=4800, offset=0, clip_len=L):
        return eng._lib.km_sequence_forward_track(eng._h, audio.data_ptr(), sc.CLIPS, L, trk.data_ptr(), K, first, interval, offset,
                                                  clip_len, 1, 1, out.data_ptr(), torch.cuda.current_stream().cuda_stream)

    for kw in (dict(K=0), dict(interval=0), dict(first=-1), dict(offset=-1), dict(clip_len=L - 1), dict(offset=5), dict(K=2 ** 31)):
        assert call(**kw) == KM_ERR_INVALID_ARG, kw
    with pytest.raises(ValueError):
        eng.sequence_forward_track(audio, trk[:1], 8000, 4800)
    with pytest.raises(ValueError):
        eng.sequence_forward_track(audio, trk[:, :, :100].contiguous(), 8000, 4800)


# ---- 8: the command-line tool ---------------------------------------------------------------------------------------------------
def test_render_sequential_writes_the_models_frames(tmp_path):
    from scipy.io import wavfile
    L = sc.clip_length(20)                                                        # 9.2 s
    pcm = np.round(sc.audio(20)[0] * 32767.0).astype(np.int16)                    # what a 16-bit WAV holds
    wav, ckpt, out = tmp_path / "a.wav", tmp_path / "ckpt.pth", tmp_path / "out.jsonl"
    wavfile.write(str(wav), 16000, pcm)
    torch.save({"epoch": 0, "global_step": 0, "model_state_dict": full_state(sc.params()),
                "model_config": {"d_model": 256, "num_heads": 8, "mel_sequence_length": 256}}, ckpt)
    assert render_sequential.main(["--model_path", str(ckpt), "--input_audio", str(wav), "--output_json", str(out), "--stride", "2"]) == 0
    lines = out.read_text().splitlines()
    N = sc.num_outputs(L, 2)
    assert len(lines) == N
    # the same model, built by hand: the layer of a checkpoint without one is torch's default under the tool's seed
    layer, source = render_sequential.compression_layer({})
    assert "seed" in source
    ce = ClipEmotion(compression_layer=layer)
    m = SequentialDualStreamModel(stride_frames=2, clip_emotion=ce).cuda().eval()
    m.load_state_dict(full_state(sc.params()))
    samples = pcm.astype(np.float32) / 32768.0
    want = m(dev(samples)[None])["blendshapes"][0].cpu().numpy()
    for i, line in enumerate(lines):
        rec = json.loads(line)
        assert set(rec) == {"timestamp", "blendshapes"}
        assert rec["timestamp"] == min(L, (i * 2 + T) * HOP) / 16000.0            # the window's end
        assert np.array_equal(np.asarray(rec["blendshapes"], np.float32), want[i]), i
    ce.close()
    # a checkpoint that carries the layer is rendered with it
    got_layer, source = render_sequential.compression_layer({"emotion_compression": {"weight": layer.weight.detach() * 2, "bias": layer.bias.detach()}})
    assert source == "checkpoint" and torch.equal(got_layer.weight.detach(), layer.weight.detach() * 2)
