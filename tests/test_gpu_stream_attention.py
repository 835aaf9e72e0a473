"""Attention maps and `raw` from the live ticks (km_stream_tick_attn / km_stream_step_attn; ``StreamEngine.tick`` and
``ChunkedStreamEngine.step`` with ``return_attention=True``, ``capture(..., return_attention=True, stats=acc)``), at both streaming
shapes: Schedule A of tests/stream_chunked_cases.py (d_model 512, 8 heads, and 16 heads for the first 90 steps) and Schedule B
(d_model 256), the short ring of tests/stream_d512_cases.py and 260 lockstep ticks of the 8.5 s ring.

What is asserted:
  * asking for the two outputs changes no bit of out / fired / ready / backlog, step by step, against a twin engine that does not;
  * rows of `raw` and of the map belong to the streams the call computed: every other row keeps the step's sentinel, and nothing
    is written around the two tensors (they are views into NaN-filled allocations);
  * the k-th fired `raw` / map of a stream are the lockstep engine's at that stream's k-th frame, bit for bit;
  * the values, at the six oracle pairs of each schedule: the float64 oracle on the DEVICE's own features of the ring content
    (``Engine.mel_extract`` with the stream's front end), ``core.logit_verdict`` on `raw` and ``core.attention_verdict`` on the map at
    K = core_logit_cases.K, ratio <= 1 (the bound of tests/test_gpu_core_logit.py).  Every pair prints
    `STREAMATTN|case|e max|e / bound|a max|a / bound` before it asserts;
  * at d_model 512 the map against ``km_core_forward(return_attention)`` on the same features, whose chain ends in
    head_mean_kernel over its per-head probabilities (no entry point returns those per head), to the same bound;
  * a captured step with the masked statistics update in the graph against an eager twin: identical bits, accumulators included.
One pass per schedule and engine set is computed once and shared by the tests (``functools.lru_cache``); nothing modifies it."""
import functools

import numpy as np
import pytest
import torch

import attn_stats_cases as ac
import stream_chunked_cases as cc
import stream_d512_cases as sc
from core_logit_cases import K, make_params
from koemorph_amd import _lib, synth
from koemorph_amd._lib import KM_ERR_UNSUPPORTED, KoeMorphError
from koemorph_amd.engine import Engine, MelConfig
from koemorph_amd.metrics import AttentionStats, StreamAttentionStats
from koemorph_amd.streaming import ChunkedStreamEngine, StreamEngine
from oracle import core

pytestmark = pytest.mark.gpu
GUARD = 1280                      # floats of NaN on either side of `raw` and of the map (keeps the 16-byte alignment)
GRAPH_FROM = {"A": 100, "B": 280}


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the cases' arrays are read-only


def sentinel(t):
    return 1000.0 + t


# ---- engines ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params_of(variant):
    """variant: 8 / 16 (heads, Schedule A, the parameters of stream_d512_cases) or "init" / "trained" (Schedule B)."""
    return sc.params() if isinstance(variant, int) else make_params(variant, 77)


def engine_of(variant):
    if isinstance(variant, int):
        e = Engine(d_model=512, num_heads=variant, mel_sequence_length=512, mel=MelConfig.model_batch(target_fps=60))
    else:
        e = Engine()
    e.load_state_dict(params_of(variant))
    e.finalize()
    e.set_option("core_split", 0)
    return e


def chunked(name, variant):
    c = cc.SCHEDULES[name]
    if name == "A":
        return ChunkedStreamEngine(engine_of(variant), c["n_streams"], context_window=c["context_window"],
                                   update_interval=c["update_interval"], buffer_duration=c["fifo_samples"] / cc.SR)
    return ChunkedStreamEngine(engine_of(variant), c["n_streams"])


class Guarded:
    """`raw` and the map of an engine as views into NaN-filled allocations, installed before the engine's first use of them."""

    def __init__(self, se):
        S = se.n_streams
        self.bufs = [torch.full((S * 52 + 2 * GUARD,), float("nan"), device="cuda"),
                     torch.full((S * 28 * 80 + 2 * GUARD,), float("nan"), device="cuda")]
        se.raw = self.bufs[0][GUARD:-GUARD].view(S, 52)
        se.attention = self.bufs[1][GUARD:-GUARD].view(S, 28, 80)
        se.raw.zero_()
        se.attention.zero_()
        assert se.attention.data_ptr() % 16 == 0

    def intact(self):
        return all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all()) for b in self.bufs)


# ---- one pass over a schedule ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run(name, variant, steps, twins=True):
    """Engines on the same feeds: `a` asks for the outputs on every step (out, raw and the map set to the step's sentinel first);
    with `twins`, `p` never asks, and `g` asks eagerly up to GRAPH_FROM and from there replays a capture made with
    return_attention=True, stats=acc while `a` is followed by acc2.update(maps, mask=fired).  Records per step what `a` returned,
    and whether p and g agreed with it bit for bit."""
    c = cc.SCHEDULES[name]
    S = c["n_streams"]
    a = chunked(name, variant)
    guard = Guarded(a)
    p, g = (chunked(name, variant), chunked(name, variant)) if twins else (None, None)
    emo = dev(cc.emotion(name))
    cnt, x = cc.counts_table(name, steps), cc.chunks(name, steps)
    rec = dict(out=np.zeros((steps, S, 52), np.float32), raw=np.zeros((steps, S, 52), np.float32),
               attn=np.zeros((steps, S, 28, 80), np.float32), fired=np.zeros((steps, S), bool), ready=np.zeros((steps, S), bool),
               backlog=np.zeros((steps, S), np.int32), plain_differs=[], graph_differs=[], after_reset={}, graph=None)
    acc = acc2 = None
    gfrom = GRAPH_FROM[name]
    for t in range(steps):
        if t in c["resets"]:
            mask = torch.zeros(S, dtype=torch.bool, device="cuda")
            mask[list(c["resets"][t])] = True
            for se in (a, p, g):
                if se is not None:
                    se.reset_streams(mask)
            rec["after_reset"][t] = (a.raw.cpu().numpy().copy(), a.attention.cpu().numpy().copy())
        xd, cd = dev(x[t]), dev(cnt[t])
        for se in (a, g):
            if se is not None:
                se.out.fill_(sentinel(t))
                se.attention_outputs()
                se.raw.fill_(sentinel(t))
                se.attention.fill_(sentinel(t))
        a.feed(xd, cd)
        out, fired, extra = a.step(emo, return_attention=True)
        assert set(extra) == {"raw", "mel_attention_weights"} and extra["raw"] is a.raw and extra["mel_attention_weights"] is a.attention
        if twins:
            p.out.fill_(sentinel(t))
            p.feed(xd, cd)
            out_p, fired_p = p.step(emo)
            if not (torch.equal(out, out_p) and torch.equal(fired, fired_p) and torch.equal(a.ready, p.ready) and
                    torch.equal(a.backlog, p.backlog)):
                rec["plain_differs"].append(t)
            if t == gfrom:
                acc, acc2 = AttentionStats(), AttentionStats()
                g.capture(c["n_max"], return_attention=True, stats=acc)
            if t >= gfrom:
                res = g.replay(xd, cd, emo)
                assert len(res) == 3 and res[2]["mel_attention_weights"] is g.attention
                acc2.update(a.attention, mask=fired)
            else:
                g.feed(xd, cd)
                g.step(emo, return_attention=True)
            if not (torch.equal(out, g.out) and torch.equal(fired, g.fired) and torch.equal(a.ready, g.ready) and
                    torch.equal(a.backlog, g.backlog) and torch.equal(a.raw, g.raw) and torch.equal(a.attention, g.attention)):
                rec["graph_differs"].append(t)
        rec["out"][t], rec["raw"][t], rec["attn"][t] = out.cpu().numpy(), a.raw.cpu().numpy(), a.attention.cpu().numpy()
        rec["fired"][t], rec["ready"][t] = fired.cpu().numpy().astype(bool), a.ready.cpu().numpy().astype(bool)
        rec["backlog"][t] = a.backlog.cpu().numpy()
    rec["guards_intact"] = guard.intact()
    if acc is not None:
        rec["graph"] = (ac.pack(acc.compute()), ac.pack(acc2.compute()))
        acc.close()
        acc2.close()
    g = None
    return rec


SCHEDULE_RUNS = [("A", 8, 152), ("A", 16, 90), ("B", "trained", 300)]


# ---- 1 + 2: the plain outputs do not move, and only computed rows are written ------------------------------------------------------------
@pytest.mark.parametrize("name,variant,steps", SCHEDULE_RUNS)
def test_chunked_twin_is_bit_identical_and_only_fired_rows_are_written(name, variant, steps):
    sim, got = cc.simulate(name, steps), run(name, variant, steps)
    assert got["plain_differs"] == [], got["plain_differs"][:5]
    assert np.array_equal(got["fired"], sim["fired"]) and np.array_equal(got["ready"], sim["ready"])
    assert np.array_equal(got["backlog"], sim["backlog"])
    fired_rows = 0
    for t in range(steps):
        for s in range(cc.SCHEDULES[name]["n_streams"]):
            raw, attn = got["raw"][t, s], got["attn"][t, s]
            if sim["fired"][t, s]:
                fired_rows += 1
                assert (raw > 0).all() and (raw < 1).all(), (t, s)                        # sigmoid values, not the sentinel
                assert (attn >= 0).all() and (attn <= 1).all(), (t, s)
                assert np.abs(attn.astype(np.float64).sum(-1) - 1.0).max() < 1e-5, (t, s)
            else:
                assert (raw == sentinel(t)).all() and (attn == sentinel(t)).all(), (t, s)
    assert fired_rows == int(sim["fired"].sum()) and fired_rows >= 5
    assert got["guards_intact"]


def lockstep_pair(se_p, se_a, frames, emo):
    """Lockstep twins on the same frames; -> (steps on which a plain output differed, per tick raw / map / ready of the asking one)."""
    guard = Guarded(se_a)
    differs, raws, maps, readies = [], [], [], []
    for t, f in enumerate(frames):
        fd = dev(f)
        for se in (se_p, se_a):
            se.out.fill_(sentinel(t))
            se.push(fd)
        se_a.raw.fill_(sentinel(t))
        se_a.attention.fill_(sentinel(t))
        out_p, ready_p = se_p.tick(emo)
        out, ready, extra = se_a.tick(emo, return_attention=True)
        if not (torch.equal(out, out_p) and torch.equal(ready, ready_p)):
            differs.append(t)
        raws.append(extra["raw"].cpu().numpy())
        maps.append(extra["mel_attention_weights"].cpu().numpy())
        readies.append(ready.cpu().numpy().astype(bool))
    return differs, np.stack(raws), np.stack(maps), np.stack(readies), guard.intact()


def check_lockstep(differs, raws, maps, readies, intact, first_ready):
    assert differs == [] and intact
    assert not readies[:first_ready].any() and readies[first_ready:].all()
    for t in range(raws.shape[0]):
        if readies[t].all():
            assert (raws[t] > 0).all() and (raws[t] < 1).all(), t
            assert np.abs(maps[t].astype(np.float64).sum(-1) - 1.0).max() < 1e-5, t
        else:
            assert (raws[t] == sentinel(t)).all() and (maps[t] == sentinel(t)).all(), t


@pytest.mark.parametrize("heads", [8, 16])
def test_lockstep_twin_on_the_short_ring_d512(heads):
    mk = lambda: StreamEngine(engine_of(heads), sc.SHORT_S, context_window=sc.SHORT_CW, update_interval=sc.UI60)
    check_lockstep(*lockstep_pair(mk(), mk(), sc.short_frames(), dev(sc.short_emotion())), sc.SHORT_FIRST_READY)


def test_lockstep_twin_260_ticks_d256():
    S, ticks = 2, 260
    audio = synth.make_audio(521, S, ticks * 533)
    frames = [audio[:, t * 533:(t + 1) * 533] for t in range(ticks)]
    mk = lambda: StreamEngine(engine_of("trained"), S)
    check_lockstep(*lockstep_pair(mk(), mk(), frames, dev(synth.normal(522, (S, 256)))), 255)


# ---- 3: chunked against lockstep ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lockstep_a(heads, steps):
    """run_twin_a of tests/test_gpu_stream_chunked.py with the two outputs: tick k of life l pushes every stream's k-th popped
    frame of that life.  -> {life: (raw (n, S, 52), maps (n, S, 28, 80), ready (n, S))}."""
    c, sim = cc.SCHEDULES["A"], cc.simulate("A", steps)
    S = c["n_streams"]
    se = StreamEngine(engine_of(heads), S, context_window=c["context_window"], update_interval=c["update_interval"])
    emo = dev(cc.emotion("A"))
    res = {}
    for life in range(int(sim["life"].max()) + 1):
        seqs = [[f for _, l, f in sim["pops"][s] if l == life] for s in range(S)]
        n = max(len(q) for q in seqs)
        if life:
            se.reset()
            assert not se.raw.any() and not se.attention.any()                           # reset() zeroes every row of both
        raws, maps, ready = np.zeros((n, S, 52), np.float32), np.zeros((n, S, 28, 80), np.float32), np.zeros((n, S), bool)
        for k in range(n):
            frame = np.zeros((S, c["frame_samples"]), np.float32)
            for s in range(S):
                if k < len(seqs[s]):
                    frame[s] = seqs[s][k]
            se.push(dev(frame))
            _, r, extra = se.tick(emo, return_attention=True)
            raws[k], maps[k], ready[k] = extra["raw"].cpu().numpy(), extra["mel_attention_weights"].cpu().numpy(), r.cpu().numpy().astype(bool)
        res[life] = (raws, maps, ready)
    return res


@pytest.mark.parametrize("heads,steps", [(8, 152), (16, 90)])
def test_kth_fired_row_is_the_lockstep_engines_kth_frame(heads, steps):
    sim, got, twin = cc.simulate("A", steps), run("A", heads, steps), lockstep_a(heads, steps)
    compared = 0
    for s in range(cc.SCHEDULES["A"]["n_streams"]):
        k_of_life = {}
        for t, life, _ in sim["pops"][s]:
            k = k_of_life.get(life, 0)
            k_of_life[life] = k + 1
            raws, maps, ready = twin[life]
            assert got["fired"][t, s] == ready[k, s], (t, s, k)
            if ready[k, s]:
                assert np.array_equal(got["raw"][t, s], raws[k, s]), (t, s, k)
                assert np.array_equal(got["attn"][t, s], maps[k, s]), (t, s, k)
                compared += 1
    assert compared == int(sim["fired"].sum()) and compared >= 5


# ---- 4 + 5: the values -----------------------------------------------------------------------------------------------------------------
def judge(label, ref, raw, attn):
    zmax = float(np.abs(ref["z64"]).max())
    assert zmax <= core.LOGIT_Z_MAX, f"{label}: |z64| reaches {zmax}, choose other parameters"
    e_max, e_ratio = core.logit_verdict(raw, ref, K)
    a_max, a_ratio = core.attention_verdict(attn, ref, K)
    print(f"STREAMATTN|{label}|{e_max:.3e}|{e_ratio:.3f}|{a_max:.3e}|{a_ratio:.3f}|zmax {zmax:.2f}")
    assert e_ratio <= 1.0, f"{label}: logit error of raw {e_max:.3e} is {e_ratio:.2f} x its bound (yardstick {ref['yard_e']:.3e})"
    assert a_ratio <= 1.0, f"{label}: attention error {a_max:.3e} is {a_ratio:.2f} x its bound (yardstick {ref['yard_a']:.3e})"
    assert np.abs(attn.astype(np.float64).sum(-1) - 1.0).max() < 1e-5


def check_values(name, variant, got, against_core_forward=False):
    c, sim = cc.SCHEDULES[name], cc.simulate(name)
    params, emo = params_of(variant), np.array(cc.emotion(name))
    fe = engine_of(variant)                                                               # the front end (and km_core_forward) on a handle of its own
    probe = chunked(name, variant)
    front, out_frames = probe.mel, probe.shape["stream_out_frames"]
    heads, T = (variant, 512) if name == "A" else (8, 256)
    assert len(sim["windows"]) == 6
    for (t, s), win in sorted(sim["windows"].items()):
        feats_d = fe.mel_extract(front, dev(win[None]), out_frames=out_frames)
        feats = feats_d.cpu().numpy()
        ref = core.logit_reference(params, feats, feats[:, -3:], emo[s:s + 1], num_heads=heads, mel_sequence_length=T)
        judge(f"{name} {variant} step {t} stream {s}", ref, got["raw"][t, s][None], got["attn"][t, s][None])
        if against_core_forward:
            o = fe.core_forward(feats_d, feats_d[:, -3:].contiguous(), dev(emo[s:s + 1]), return_attention=True)
            chain = o["mel_attention_weights"].cpu().numpy()
            err = float(core.attention_error(got["attn"][t, s][None], chain).max())
            bound = core.attention_bound(ref, K)
            print(f"STREAMATTN|{name} {variant} step {t} stream {s} vs km_core_forward|{err:.3e}|{err / bound:.3f}")
            assert err <= bound, (t, s, err, bound)
    fe.close()


def test_values_schedule_a_and_the_head_mean_of_the_generic_chain():
    check_values("A", 8, run("A", 8, 152), against_core_forward=True)
    # the heads are averaged, not picked: the same step at 8 and at 16 heads gives other maps (and other coefficients)
    h8, h16 = run("A", 8, 152), run("A", 16, 90)
    t, s = 60, 3
    assert h8["fired"][t, s] and h16["fired"][t, s]
    assert not np.array_equal(h8["attn"][t, s], h16["attn"][t, s]) and not np.array_equal(h8["raw"][t, s], h16["raw"][t, s])


@pytest.mark.parametrize("pk", ["trained", "init"])
def test_values_schedule_b(pk):
    check_values("B", pk, run("B", "trained", 300) if pk == "trained" else run("B", "init", 300, False))


# ---- 6: graph ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,steps", [("A", 8, 152), ("B", "trained", 300)])
def test_captured_step_with_the_masked_update_in_the_graph(name, variant, steps):
    sim, got = cc.simulate(name, steps), run(name, variant, steps)
    assert got["graph_differs"] == [], got["graph_differs"][:5]                         # out, flags, raw and the maps, on every step
    replayed, eager = got["graph"]
    assert np.array_equal(replayed, eager)
    rows = int(sim["fired"][GRAPH_FROM[name]:].sum())
    assert replayed[0] == rows and rows >= 5
    st = ac.stats_f64(got["attn"][GRAPH_FROM[name]:][sim["fired"][GRAPH_FROM[name]:]])
    first_count = 1 + ac.Q * ac.K + ac.Q
    assert np.array_equal(replayed[first_count:], ac.pack(st)[first_count:])               # the peak counts, against the host restatement


def test_per_stream_statistics_from_a_captured_lockstep_tick():
    """StreamEngine.capture with a StreamAttentionStats: every stream's slice is a plain accumulator fed that stream's maps."""
    heads = 8
    se = StreamEngine(engine_of(heads), sc.SHORT_S, context_window=sc.SHORT_CW, update_interval=sc.UI60)
    emo, frames = dev(sc.short_emotion()), sc.short_frames()
    per = StreamAttentionStats(sc.SHORT_S)
    plain = [AttentionStats() for _ in range(sc.SHORT_S)]
    n0 = sc.SHORT_FIRST_READY - 2
    for t in range(n0):
        se.push(dev(frames[t]))
        se.tick(emo, return_attention=True)
    # every later frame is padded to 267 samples for the captured push (push truncates to the ring hop)
    se.capture(267, return_attention=True, stats=per)
    fed = 0
    for t in range(n0, sc.SHORT_TICKS):
        f = np.zeros((sc.SHORT_S, 267), np.float32)
        f[:, :frames[t].shape[1]] = frames[t]
        out, ready, extra = se.replay(dev(f), emo)
        for s in range(sc.SHORT_S):
            if bool(ready[s]):
                plain[s].update(extra["mel_attention_weights"][s:s + 1])
                fed += 1
    got = per.compute()
    assert fed == sc.SHORT_S * (sc.SHORT_TICKS - sc.SHORT_FIRST_READY)
    for s in range(sc.SHORT_S):
        assert got[s]["rows"] == sc.SHORT_TICKS - sc.SHORT_FIRST_READY
        assert np.array_equal(ac.pack(got[s]), ac.pack(plain[s].compute())), s
        plain[s].close()
    per.close()


# ---- 7: resets and refusals ------------------------------------------------------------------------------------------------------------
def test_reset_streams_zeroes_the_masked_rows_only():
    got = run("A", 8, 152)
    raw, attn = got["after_reset"][85]                         # stream 2 was reset before step 85's feed
    assert not raw[2].any() and not attn[2].any()
    for s in (0, 1, 3):                                        # the others hold what step 84 left (its sentinel, or its fired row)
        assert np.array_equal(raw[s], got["raw"][84, s]) and np.array_equal(attn[s], got["attn"][84, s])
    assert got["fired"][84, 0] and got["raw"][84, 0].any()


@pytest.mark.parametrize("name,variant", [("A", 8), ("B", "trained")])
def test_maps_under_core_split_3_are_refused_and_pop_nothing(name, variant):
    c = cc.SCHEDULES[name]
    a, b = chunked(name, variant), chunked(name, variant)
    emo = dev(cc.emotion(name))
    x = cc.chunks(name, 3)
    full = torch.full((c["n_streams"],), c["n_max"], dtype=torch.int32, device="cuda")
    for se in (a, b):
        se.feed(dev(x[0]), full)
        se.feed(dev(x[0]), full)                               # every FIFO holds more than two whole frames
        se.step(emo)
    before = a.backlog.clone()
    assert int(before.min()) >= 1
    a.engine.set_option("core_split", 3)
    a.out.fill_(7.0)
    for call in (lambda: a.step(emo, return_attention=True), lambda: a.tick(emo, return_attention=True)):
        with pytest.raises(KoeMorphError, match="split-bf16") as err:
            call()
        assert err.value.code == KM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(a.backlog, before) and float(a.out.min()) == 7.0 == float(a.out.max())
    assert not a.raw.any() and not a.attention.any()
    a.engine.set_option("core_split", 0)
    a.out.copy_(b.out)
    # nothing was popped: the next step of both engines pops the same frame
    for se in (a, b):
        se.step(emo)
    assert torch.equal(a.backlog, b.backlog) and torch.equal(a.fired, b.fired) and torch.equal(a.ready, b.ready)
    assert torch.equal(a.backlog, before - 1)
    # reset() zeroes every row of both outputs, whatever they held
    a.raw.fill_(5.0)
    a.attention.fill_(5.0)
    a.reset()
    assert not a.raw.any() and not a.attention.any() and not a.out.any() and not a.backlog.any()


def test_legacy_and_generic_shape_handles_keep_the_messages_of_tick_and_step():
    from koemorph_amd.model import SimplifiedKoeMorphModel
    import legacy_stream_cases as lc
    m = SimplifiedKoeMorphModel().cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in lc.params().items()})
    lib, h, _ = m._handle()
    buf = torch.zeros(2, 28 * 80, device="cuda")
    for rc in (lib.km_stream_tick_attn(h, buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), None),
               lib.km_stream_step_attn(h, buf.data_ptr(), buf.data_ptr(), None, None, None, buf.data_ptr(), buf.data_ptr(), None)):
        assert rc == _lib.KM_ERR_INVALID_ARG and b"dual-stream handle" in lib.km_last_error()
    e = Engine(d_model=128, num_heads=4, mel_sequence_length=64)
    e.load_state_dict(synth.make_core_params(5, 128, 64, 256, "trained"))
    e.finalize()
    se = ChunkedStreamEngine(e, 2, context_window=1.0)
    se.feed(torch.zeros(2, 1024, device="cuda"))
    for call in (lambda: se.step(torch.zeros(2, 256, device="cuda"), return_attention=True),
                 lambda: se.tick(torch.zeros(2, 256, device="cuda"), return_attention=True)):
        with pytest.raises(KoeMorphError, match="no kernel for d_model=128, mel_sequence_length=64, heads=4"):
            call()
    # a step before km_stream_fifo_create, and a misaligned map
    e2 = engine_of("trained")
    s2 = StreamEngine(e2, 2)
    emo, out = torch.zeros(2, 256, device="cuda"), torch.zeros(2, 52, device="cuda")
    maps = torch.zeros(2 * 28 * 80 + 4, device="cuda")
    assert lib.km_stream_step_attn(e2._h, emo.data_ptr(), out.data_ptr(), None, None, None, None, maps.data_ptr(), None) == _lib.KM_ERR_INVALID_ARG
    assert b"km_stream_fifo_create first" in lib.km_last_error()
    assert lib.km_stream_tick_attn(e2._h, emo.data_ptr(), out.data_ptr(), None, None, maps.data_ptr() + 4, None) == _lib.KM_ERR_INVALID_ARG
    assert b"16-byte aligned" in lib.km_last_error()
    with pytest.raises(ValueError):
        s2.capture(stats=AttentionStats())                     # an accumulator without return_attention
    torch.cuda.synchronize()
