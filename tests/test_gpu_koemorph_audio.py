"""AudioRowStreams and KoeMorphAudioStreams (km_koemorph_audio_*) on the device, at the small shape: a fused-width model with one encoder
and one attention layer and emotion_dim 32, three streams, an emotion window of 0.5 s (8000 samples, 45 frames; the ring of 9600
samples wraps twice) and 1.2 s of the speech-like synthetic audio per stream.

1. MEL ROWS are a function of the stream's samples alone: equal bits whether the audio comes in chunks of 160, 533, 534, 1024 or 1600
   samples or ragged, wherever the life starts in the ring (a frame whose first sample sits on ring index 0, a frame that straddles the
   ring's end); against oracle.mel.mel_torchaudio and the dense MelSpectrogramExtractor within the tolerance of
   tests/test_gpu_mel.py::test_torchaudio_front_end (exp() of both, rtol 2e-3, atol 2e-8).
2. EMOTION ROWS on every push against the dense llds(audio[a0:n], fps=None) through the shifted grid of koemorph_audio_cases: rows
   that are no blend have equal bits, blends lie within 2^-22 (|a| + |b|) of the blend of the GPU's own native rows.
3. END TO END: KoeMorphAudioStreams.push against a twin model's KoeMorphStreams.step on the rows of an AudioRowStreams, bit for bit.
4. CONTRACT: capture and replay, guard regions, clamped counts, reset, changed weights, device memory.  5. The script."""
import ctypes as C
import gc
import json

import numpy as np
import pytest
import torch

import egemaps_cases as ec
import koemorph_audio_cases as ac
import rollout_cases as rc
from koemorph_amd import _lib
from koemorph_amd.egemaps_names import GEMAPS_LLD_COLUMNS
from koemorph_amd.features.opensmile_extractor import EGeMAPSEngine
from koemorph_amd.features.stft import MelSpectrogramExtractor
from koemorph_amd.streaming import AudioRowStreams, KoeMorphAudioStreams, KoeMorphStreams
from oracle import koemorph_model as okm
from oracle import mel as omel

pytestmark = pytest.mark.gpu

N, WINDOW, MAX_SAMPLES = 3, 0.5, 1600
W = ac.window_samples(WINDOW)
RING = W + MAX_SAMPLES

_models = {}


def models(mel_dim=80, smoothing="exponential"):
    """(engine model, twin model, cfg): two models of one configuration and one set of weights, made once per module."""
    key = (mel_dim, smoothing)
    if key not in _models:
        cfg = okm.KoeMorphConfig(mel_dim=mel_dim, emotion_dim=32, num_encoder_layers=1, num_attention_layers=1, smoothing_method=smoothing)
        params = okm.make_koemorph_params(29, cfg)
        _models[key] = (rc.build(cfg, params), rc.build(cfg, params), cfg)
    return _models[key]


_audio = {}


def audio():
    """(N, L) float32 on the host, L = 19200: 1.2 s of another speech-like voice per stream."""
    if "x" not in _audio:
        rows = [ec.speechlike(60 + 3 * s, 1.2) for s in range(N)]
        L = min(len(r) for r in rows)
        x = np.stack([r[:L] for r in rows]).astype(np.float32)
        x.setflags(write=False)
        _audio["x"] = x
    return _audio["x"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b, what):
    a, b = a.detach().cpu().numpy() if torch.is_tensor(a) else a, b.detach().cpu().numpy() if torch.is_tensor(b) else b
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), (what, float(np.nanmax(np.abs(a - b))))


def batch(x, used, counts, M):
    """The (N, M) samples of a push: stream s brings counts[s] samples from x[s, used[s]:]."""
    buf = np.zeros((N, M), np.float32)
    for s in range(N):
        c = max(0, min(counts[s], M))
        buf[s, :c] = x[s, used[s]:used[s] + c]
    return torch.from_numpy(buf).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda")


def even_steps(L, M):
    return [([c] * N, None) for c in ac.chunks(L, M)]


def walk_rows(eng, x, steps, M):
    """Drive an AudioRowStreams through ``steps``.  -> per stream the mel rows of its life (K, mel_dim), and the pushes
    [(stream, samples after, first frame, rows, emotion rows (rows, emotion_dim))]."""
    hop = eng.hop
    used = [0] * N
    mel = [[] for _ in range(N)]
    pushes = []
    for counts, _ in steps:
        xb, cnt = batch(x, used, counts, M)
        mrows, erows, rcount = eng.push(xb, cnt)
        rcount = rcount.tolist()
        for s in range(N):
            first = used[s] // hop
            used[s] += max(0, min(counts[s], M))
            assert rcount[s] == used[s] // hop - first, (s, used[s], rcount)
            if rcount[s]:
                mel[s].append(mrows[s, :rcount[s]].cpu().numpy().copy())
                pushes.append((s, used[s], first, rcount[s], erows[s, :rcount[s]].cpu().numpy().copy()))
    assert eng.samples().tolist() == used
    return [np.concatenate(m) if m else np.zeros((0, eng.mel_rows.shape[2]), np.float32) for m in mel], pushes


# ---- 1. mel rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps,mel_dim", [(30, 80), (60, 64)])
def test_mel_rows_are_a_function_of_the_samples_alone(fps, mel_dim):
    m, _, cfg = models(mel_dim)
    x = audio()
    L = x.shape[1]
    hop = ac.hop_of(fps)
    K = L // hop
    eng = AudioRowStreams(m, N, fps=fps, emotion_window=WINDOW, max_samples=MAX_SAMPLES)
    try:
        assert eng.plan == ac.expected_plan(N, fps, WINDOW, MAX_SAMPLES) and eng.hop == hop and eng.plan["ring_len"] == RING
        origin = [0] * N                                                   # the lives' origins, by the law of the reset
        seen = set()
        runs = []
        for M in (160, 533, 534, 1024, 1600, None):
            if M == 1024:
                # the next lives start where frame 2's first sample (2 hop - 256) falls on ring index 0: push what is missing, reset
                want_origin = (RING - (2 * hop - 256)) % RING
                pre = [(want_origin - o) % RING for o in origin]
                assert len(set(pre)) == 1
                used = [0] * N
                for c in ac.chunks(pre[0], MAX_SAMPLES):
                    eng.push(*batch(x, used, [c] * N, MAX_SAMPLES))
                eng.reset()
                origin = [want_origin] * N
            steps = ac.ragged_schedule(L, 1024) if M is None else even_steps(L, M)
            for k in range(K):                                             # where the frames of this life lie in the ring
                p = (origin[0] + k * hop - 256) % RING
                if k * hop >= 256 and p == 0:
                    seen.add("index 0")
                if k * hop >= 256 and p + 512 > RING:
                    seen.add("straddles")
            mel, _ = walk_rows(eng, x, steps, 1024 if M is None else M)
            runs.append((M, mel))
            totals = eng.samples().tolist()
            eng.reset()
            origin = [(o + t) % RING for o, t in zip(origin, totals)]
        assert seen == {"index 0", "straddles"}, seen
        first = runs[0][1]
        assert all(first[s].shape == (K, mel_dim) for s in range(N))
        for M, mel in runs[1:]:
            for s in range(N):
                k = len(mel[s])
                assert k == K if M is not None or s == 0 else 0 < k < K, (M, s, k)
                same_bits(mel[s], first[s][:k], f"chunks of {M}, stream {s}")
        # against the float64-backed oracle and the dense extractor, on the audio extended by zeros (no row below K sees them)
        ext = np.concatenate([x, np.zeros((N, 2 * hop + 512), np.float32)], axis=1)
        want = omel.mel_torchaudio(ext, target_fps=fps, n_mels=mel_dim, f_max=8000)
        dense = MelSpectrogramExtractor(target_fps=fps, n_mels=mel_dim)(torch.from_numpy(ext).cuda()).cpu().numpy()
        assert want.shape[1] >= K and dense.shape[1] >= K
        got = np.stack(first)
        assert np.isfinite(got).all()
        rel = lambda a, b: float((np.abs(np.exp(a) - np.exp(b)) / (2e-8 / 2e-3 + np.exp(b))).max())
        print(f"MELROWS|fps {fps}|mel_dim {mel_dim}|worst relative difference of exp(): oracle {rel(got, want[:, :K]):.3e}, "
              f"dense extractor {rel(got, dense[:, :K]):.3e}|rtol 2e-3")
        np.testing.assert_allclose(np.exp(got), np.exp(want[:, :K]), rtol=2e-3, atol=2e-8)
        np.testing.assert_allclose(np.exp(got), np.exp(dense[:, :K]), rtol=2e-3, atol=2e-8)
    finally:
        eng.close()


# ---- 2. emotion rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps,feature_set", [(30, "eGeMAPSv02"), (25, "eGeMAPSv02"), (30, "GeMAPS")])
def test_emotion_rows_against_the_dense_descriptors_of_the_window(fps, feature_set):
    m, _, cfg = models()
    x = audio()
    xd = torch.from_numpy(x.copy()).cuda()
    L = x.shape[1]
    hop = ac.hop_of(fps)
    Wd = ac.LLD_WIDTH[feature_set]
    nz = (np.arange(25) if feature_set == "eGeMAPSv02" else np.array(GEMAPS_LLD_COLUMNS)) >= 10
    semitone = int(np.argmax(nz)) if feature_set == "eGeMAPSv02" else list(GEMAPS_LLD_COLUMNS).index(10)
    dense = EGeMAPSEngine("cuda")
    eng = AudioRowStreams(m, N, fps=fps, emotion_window=WINDOW, max_samples=MAX_SAMPLES, feature_set=feature_set)
    seen = set()
    try:
        _, pushes = walk_rows(eng, x, ac.ragged_schedule(L, 1024), 1024)
        for s, n, first, rows, got in pushes:
            a0, length, mm, nf = ac.window(n, W)
            assert got.shape == (rows, 32) and not got[:, Wd:].any(), (s, n)             # zeros to the right
            if nf == 0:
                assert length < 960 and not got.any()
                seen.add("short window")
                continue
            native = dense.llds(xd[s:s + 1, a0:n].contiguous(), feature_set=feature_set)[0].cpu().numpy()
            assert native.shape == (nf, Wd)
            ks = np.arange(first, first + rows)
            want, a, b, blend = ac.resample_columns(native.astype(np.float64), ks, hop, mm, nz)
            j, w, exact = ac.grid(nf, ks, hop, mm)
            assert (np.floor(ks * hop / 160.0) - mm >= 0).all()
            picked = np.where(exact[:, None] | (w <= 0.5)[:, None], native[j], native[np.minimum(j + 1, nf - 1)])
            g = got[:, :Wd]
            assert np.array_equal(bits(g)[~blend], bits(picked)[~blend]), (fps, feature_set, s, n)
            err = np.abs(g.astype(np.float64) - want)
            bound = 2.0 ** -22 * (np.abs(a) + np.abs(b))
            bad = np.argwhere(blend & (err > bound))
            assert len(bad) == 0, [(s, n, int(ks[r]), int(c), g[r, c], want[r, c], bound[r, c]) for r, c in bad[:5]]
            assert np.isfinite(g).all()
            seen.add("wrapped window" if mm > 0 else "growing window")
            if blend.any():
                seen.add("blended")
            if (~blend & ~exact[:, None]).any():
                seen.add("nearer frame")
            if (np.floor(ks * hop / 160.0) - mm >= nf - 1).any():
                seen.add("last frame")
            if (native[j][:, semitone] != 0).any():
                seen.add("voiced")
            if (native[j][:, semitone] == 0).any():
                seen.add("unvoiced")
            if fps == 25:
                assert exact.all() and not blend.any()                                  # hop 640: every row is a frame
        want_seen = {"short window", "growing window", "wrapped window", "last frame", "voiced", "unvoiced"}
        if fps != 25:
            want_seen |= {"blended", "nearer frame"}
        assert seen == want_seen, (seen, want_seen)
    finally:
        eng.close()
        dense.close()


# ---- 3. end to end -------------------------------------------------------------------------------------------------------
def e2e_steps(L, M):
    """ac.ragged_schedule with stream 0 reset ahead of the ninth push."""
    steps = ac.ragged_schedule(L, M)
    return [(c, [s == 0 for s in range(N)] if k == 8 else None) for k, (c, _) in enumerate(steps)]


def walk_frames(push, reset_streams, x, steps, M, hop, from_step=0, only=None):
    """-> [(rendered list, blendshapes clone, raw clone)] per step; stream s takes its samples in order, stream 0 again from the
    reset's position on (a reset does not rewind the audio)."""
    used = [0] * N
    out = []
    for k, (counts, mask) in enumerate(steps):
        if only is not None:
            counts = [c if s == only else 0 for s, c in enumerate(counts)]
        if k >= from_step:
            if mask is not None and k > from_step:
                reset_streams(torch.tensor(mask, dtype=torch.bool, device="cuda"))
            xb, cnt = batch(x, used, counts, M)
            res = push(xb, cnt)
            out.append((res["rendered"].tolist(), res["blendshapes"].clone(), res["raw_blendshapes"].clone()))
        for s in range(N):
            used[s] += max(0, min(counts[s], M))
    return out


@pytest.mark.parametrize("smoothing", ["exponential", "off"])
def test_push_is_the_step_on_the_rows_bit_for_bit(smoothing):
    m, ref, cfg = models()
    x = audio()
    L, M, T = x.shape[1], 1024, 9
    steps = e2e_steps(L, M)
    kw = dict(fps=30.0, emotion_window=WINDOW, max_samples=MAX_SAMPLES)
    a = KoeMorphAudioStreams(m, N, context_frames=T, apply_smoothing=smoothing != "off", **kw)
    rows = AudioRowStreams(ref, N, **kw)
    b = KoeMorphStreams(ref, N, context_frames=T, max_rows=rows.max_rows, apply_smoothing=smoothing != "off")
    try:
        assert a.max_rows == rows.max_rows == MAX_SAMPLES // 533 + 1 and a.hop == 533
        got = walk_frames(a.push, a.reset_streams, x, steps, M, 533)

        def twin_push(xb, cnt):
            mel, emo, rcount = rows.push(xb, cnt)
            return b.step(mel, emo, rcount)

        def twin_reset(mask):
            rows.reset_streams(mask)
            b.reset_streams(mask)

        want = walk_frames(twin_push, twin_reset, x, steps, M, 533)
        total = [0] * N
        for k, ((rg, og, wg), (rw, ow, ww)) in enumerate(zip(got, want)):
            assert rg == rw
            for s in range(N):
                same_bits(og[s, :rg[s]], ow[s, :rg[s]], f"step {k} stream {s} out")
                same_bits(wg[s, :rg[s]], ww[s, :rg[s]], f"step {k} stream {s} raw")
                assert bool(torch.isfinite(og[s, :rg[s]]).all())
                total[s] += rg[s]
        assert total[0] > 20 and 0 < total[1] < total[0] and 0 < total[2] < total[0]
        if smoothing == "off":
            assert a.smoother_state() is None
        else:
            same_bits(a.smoother_state(), b.smoother_state(), "smoother state")
        assert a.frames().tolist() == b.frames().tolist()
        # from its reset on, stream 0 is a fresh engine's stream 0 on the same pushes
        a.close()
        fresh = KoeMorphAudioStreams(m, N, context_frames=T, apply_smoothing=smoothing != "off", **kw)
        try:
            again = walk_frames(fresh.push, fresh.reset_streams, x, steps, M, 533, from_step=8, only=0)
            assert len(again) == len(got) - 8 and sum(r[0] for r, _, _ in again) > 8
            for k, ((rg, og, _), (rf, of, _)) in enumerate(zip(got[8:], again)):
                assert rg[0] == rf[0]
                same_bits(og[0, :rg[0]], of[0, :rf[0]], f"stream 0, push {k} after its reset")
        finally:
            fresh.close()
    finally:
        a.close()
        b.close()
        rows.close()


# ---- 4. contract ---------------------------------------------------------------------------------------------------------
def test_a_captured_push_replays_on_other_samples_and_counts():
    m, ref, cfg = models()
    x = audio()
    L, M, T = x.shape[1], 1024, 9
    steps = e2e_steps(L, M)
    kw = dict(fps=30.0, context_frames=T, emotion_window=WINDOW, max_samples=MAX_SAMPLES)
    a, b = KoeMorphAudioStreams(m, N, **kw), KoeMorphAudioStreams(ref, N, **kw)
    try:
        a.push(torch.from_numpy(x[:, :M].copy()).cuda())                   # the captured phase: every stream at M samples
        a.capture(M)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        scratch = torch.zeros(8, device="cuda")
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            with pytest.raises(_lib.KoeMorphError, match="km_koemorph_audio_create.*stream capture") as ei:
                KoeMorphAudioStreams(ref, N, **kw)
            assert ei.value.code == _lib.KM_ERR_WORKSPACE
            scratch.add_(1.0)
        torch.cuda.current_stream().wait_stream(side)
        a.reset()
        got = walk_frames(a.replay, a.reset_streams, x, steps, M, 533)
        want = walk_frames(b.push, b.reset_streams, x, steps, M, 533)
        for k, ((rg, og, wg), (rw, ow, ww)) in enumerate(zip(got, want)):
            assert rg == rw
            for s in range(N):
                same_bits(og[s, :rg[s]], ow[s, :rg[s]], f"replay {k} stream {s} out")
                same_bits(wg[s, :rg[s]], ww[s, :rg[s]], f"replay {k} stream {s} raw")
        same_bits(a.smoother_state(), b.smoother_state(), "replay state")
        assert a.frames().tolist() == b.frames().tolist() and a.rows.samples().tolist() == b.rows.samples().tolist()
        ra = a.replay(torch.from_numpy(x[:, :600].copy()).cuda())          # fewer samples than were captured, without counts
        rb = b.push(torch.from_numpy(x[:, :600].copy()).cuda())
        assert ra["rendered"].tolist() == rb["rendered"].tolist()
        same_bits(ra["blendshapes"][:, :1], rb["blendshapes"][:, :1], "narrow replay")
    finally:
        a.close()
        b.close()


def test_guard_regions_untouched_rows_and_clamped_counts():
    """km_koemorph_audio_rows and the step behind it on padded buffers: the floats around the rows, out, raw and rendered, and the
    rows past a stream's count, keep their pattern; counts are clamped to 0 .. M."""
    m, ref, cfg = models()
    x = audio()
    M, G, T = 1024, 64, 9
    kw = dict(fps=30.0, context_frames=T, emotion_window=WINDOW, max_samples=MAX_SAMPLES)
    a, b = KoeMorphAudioStreams(m, N, **kw), KoeMorphAudioStreams(ref, N, **kw)
    try:
        lib, h, R = a.rows._lib, a.rows._h, a.max_rows
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        used = [0] * N
        for turn, counts in enumerate(([M, 0, 700], [5000, 533, -4], [M, M, M])):
            n = [max(0, min(c, M)) for c in counts]
            xb, cnt = batch(x, used, n, M)
            cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
            mel = torch.full((G + N * R * 80 + G,), -7.0, device="cuda")
            emo = torch.full((G + N * R * 32 + G,), -7.0, device="cuda")
            rc_ = torch.full((G + N + G,), -7, dtype=torch.int32, device="cuda")
            outs = [torch.full((G + N * R * 52 + G,), -7.0, device="cuda") for _ in range(2)]
            rend = torch.full((G + N + G,), -7, dtype=torch.int32, device="cuda")
            at = lambda t: C.c_void_p(t.data_ptr() + 4 * G)
            _lib.check(lib.km_koemorph_audio_rows(h, C.c_void_p(xb.data_ptr()), M, C.c_void_p(cnt.data_ptr()), at(mel), at(emo), at(rc_), st))
            _lib.check(lib.km_koemorph_stream_step(h, at(mel), at(emo), at(rc_), at(outs[0]), at(outs[1]), at(rend), st))
            want = b.push(xb, torch.tensor(n, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            rows = [(used[s] + n[s]) // 533 - used[s] // 533 for s in range(N)]
            used = [u + c for u, c in zip(used, n)]
            assert a.rows.samples().tolist() == used                       # the clamp
            for t in (rc_, rend):
                assert bool((t[:G] == -7).all()) and bool((t[G + N:] == -7).all()) and t[G:G + N].tolist() == rows
            for t, width, ref_t in ((mel, 80, b.rows.mel_rows), (emo, 32, b.rows.emotion_rows), (outs[0], 52, want["blendshapes"]),
                                    (outs[1], 52, want["raw_blendshapes"])):
                assert bool((t[:G] == -7.0).all()) and bool((t[G + N * R * width:] == -7.0).all()), (turn, width)
                body = t[G:G + N * R * width].view(N, R, width)
                for s in range(N):
                    assert bool((body[s, rows[s]:] == -7.0).all()), (turn, width, s)
                    same_bits(body[s, :rows[s]], ref_t[s, :rows[s]], f"turn {turn} width {width} stream {s}")
            assert sum(rows) > 0
        rcode = lib.km_koemorph_audio_rows(h, C.c_void_p(xb.data_ptr()), MAX_SAMPLES + 1, None, at(mel), at(emo), at(rc_), st)
        assert rcode == _lib.KM_ERR_INVALID_ARG and b"km_koemorph_audio_rows: 1601 samples per stream" in lib.km_last_error()
    finally:
        a.close()
        b.close()


def test_reset_reproduces_and_changed_weights_are_picked_up():
    """reset() plus the same schedule gives the same bits; a parameter changed between two pushes is used by the next push with every
    stream's samples, rows, counter and state kept -- a twin with the same change at the same push gives the same bits."""
    cfg = okm.KoeMorphConfig(emotion_dim=32, num_encoder_layers=1, num_attention_layers=1)
    params = okm.make_koemorph_params(23, cfg)
    m, ref = rc.build(cfg, params), rc.build(cfg, params)
    x = audio()
    L, M = x.shape[1], 1024
    steps = ac.ragged_schedule(L, M)
    kw = dict(fps=30.0, context_frames=9, emotion_window=WINDOW, max_samples=MAX_SAMPLES)
    a, b = KoeMorphAudioStreams(m, N, **kw), KoeMorphAudioStreams(ref, N, **kw)
    try:
        first = walk_frames(a.push, a.reset_streams, x, steps, M, 533)
        state1, frames1 = a.smoother_state().clone(), a.frames().tolist()
        a.reset()
        assert a.frames().tolist() == [0] * N and a.rows.samples().tolist() == [0] * N
        second = walk_frames(a.push, a.reset_streams, x, steps, M, 533)
        for k, ((r1, o1, _), (r2, o2, _)) in enumerate(zip(first, second)):
            assert r1 == r2
            for s in range(N):
                same_bits(o1[s, :r1[s]], o2[s, :r2[s]], f"after reset, step {k} stream {s}")
        same_bits(a.smoother_state(), state1, "state after reset")
        assert a.frames().tolist() == frames1
        # the changed weight
        a.reset()
        new = ref.decoder.output_proj.bias.detach().clone() + 0.25
        half = len(steps) // 2
        outs = {}
        for name, eng, mod in (("a", a, m), ("b", b, ref)):
            res = walk_frames(eng.push, eng.reset_streams, x, steps[:half], M, 533)
            with torch.no_grad():
                mod.decoder.output_proj.bias.copy_(new)
            used = [sum(max(0, min(c[s], M)) for c, _ in steps[:half]) for s in range(N)]
            for counts, _ in steps[half:]:
                xb, cnt = batch(x, used, counts, M)
                r = eng.push(xb, cnt)
                res.append((r["rendered"].tolist(), r["blendshapes"].clone(), r["raw_blendshapes"].clone()))
                used = [u + max(0, min(c, M)) for u, c in zip(used, counts)]
            outs[name] = res
        assert a.frames().tolist() == frames1 == b.frames().tolist()
        changed = False
        for k, ((ra, oa, _), (rb, ob, _), (r1, o1, _)) in enumerate(zip(outs["a"], outs["b"], first)):
            assert ra == rb == r1
            for s in range(N):
                same_bits(oa[s, :ra[s]], ob[s, :ra[s]], f"changed weight, step {k} stream {s}")
                if k < half:
                    same_bits(oa[s, :ra[s]], o1[s, :ra[s]], f"before the change, step {k} stream {s}")
                elif ra[s]:
                    changed |= not torch.equal(oa[s, :ra[s]], o1[s, :ra[s]])
        assert changed
    finally:
        a.close()
        b.close()


def test_memory_returns_to_its_baseline():
    lib = _lib.load()
    cfg = okm.KoeMorphConfig(emotion_dim=32, num_encoder_layers=1, num_attention_layers=1)
    gc.collect()
    torch.cuda.synchronize()
    base0 = lib.km_live_device_bytes()
    m = rc.build(cfg, okm.make_koemorph_params(19, cfg))
    m._handle()
    torch.cuda.synchronize()
    base = lib.km_live_device_bytes()
    eng = AudioRowStreams(m, N, fps=30.0, emotion_window=WINDOW, max_samples=MAX_SAMPLES)
    with_engine = lib.km_live_device_bytes()
    assert eng.plan["device_bytes"] == ac.expected_plan(N, 30.0, WINDOW, MAX_SAMPLES)["device_bytes"]
    assert with_engine > base + eng.plan["device_bytes"]                  # the state, and the mel and eGeMAPS plans on top
    second = AudioRowStreams(m, N, fps=30.0, emotion_window=WINDOW, max_samples=MAX_SAMPLES)    # replaces the first
    assert lib.km_live_device_bytes() == with_engine
    with pytest.raises(RuntimeError, match="replaced"):
        eng.push(torch.zeros(N, 533, device="cuda"))
    eng.close()                                                            # a replaced engine frees nothing
    assert lib.km_live_device_bytes() == with_engine
    second.push(torch.zeros(N, 533, device="cuda"))
    second.close()
    assert lib.km_live_device_bytes() == base
    with pytest.raises(RuntimeError, match="closed"):
        second.samples()
    both = KoeMorphAudioStreams(m, N, fps=30.0, context_frames=9, emotion_window=WINDOW, max_samples=MAX_SAMPLES)
    both.push(torch.zeros(N, 1600, device="cuda"))
    torch.cuda.synchronize()
    assert lib.km_live_device_bytes() > with_engine
    both.rows._open = both.frames_engine._open = False                     # km_destroy frees both groups: nothing is left to close
    _lib.check(lib.km_destroy(m._h))
    m._h = None
    assert lib.km_live_device_bytes() == base0
    del both, m
    gc.collect()


# ---- 5. the script -------------------------------------------------------------------------------------------------------
def test_the_script_converts_a_file(tmp_path):
    from scipy.io import wavfile
    from koemorph_amd.scripts import rt_koemorph
    config = dict(emotion_dim=32, d_query=256, num_encoder_layers=1, num_attention_layers=1)
    torch.manual_seed(3)
    from koemorph_amd.model import create_koemorph_model
    model = create_koemorph_model(config).eval()
    ckpt, wav, out = tmp_path / "m.pt", tmp_path / "a.wav", tmp_path / "o.jsonl"
    torch.save({"model_state_dict": model.state_dict(), "config": {"model": config}}, ckpt)
    x = ec.speechlike(9, 1.6)[:24000]                                     # 1.5 s
    assert len(x) == 24000
    wavfile.write(wav, 16000, x)
    rt_koemorph.main(["--model_path", str(ckpt), "--input_audio", str(wav), "--output_json", str(out)])
    lines = [json.loads(line) for line in open(out)]
    assert len(lines) == 24000 // 533 == 45
    assert [line["timestamp"] for line in lines] == pytest.approx([k / 30.0 for k in range(45)], abs=1e-9)
    got = np.array([line["blendshapes"] for line in lines], np.float32)
    eng = KoeMorphAudioStreams(rt_koemorph.load_model(str(ckpt)), 1, fps=30.0, max_samples=1024)
    try:
        frames = []
        for c0 in range(0, 24000, 1024):
            res = eng.push(torch.from_numpy(x[None, c0:c0 + 1024].copy()).cuda())
            frames.append(res["blendshapes"][0, :int(res["rendered"][0])].cpu().numpy())
        same_bits(got, np.concatenate(frames), "the script's frames")
    finally:
        eng.close()
    # a checkpoint outside the fused width gets the engine's own refusal
    small = create_koemorph_model(dict(rc.SMALL, d_query=64, emotion_dim=32)).eval()
    torch.save({"model_state_dict": small.state_dict(), "config": {"model": dict(rc.SMALL, d_query=64, emotion_dim=32)}}, ckpt)
    with pytest.raises(_lib.KoeMorphError, match="km_koemorph_stream_create: d_model 64") as ei:
        rt_koemorph.main(["--model_path", str(ckpt), "--input_audio", str(wav), "--output_json", str(out)])
    assert ei.value.code == _lib.KM_ERR_UNSUPPORTED
