"""SequentialTrainer.validate(components=True): the validation forward from the resident clip (Engine.forward_clip) and the
loss summed by component on the device (LossTerms), against the default call and against a replay done here.

Data: two synthetic clips of 267 and 264 frames at batch 4 -> 12 and 9 windows, i.e. batches of 4, 4, 4 and 4, 4, 1: a file
change in between and a short last batch (the EMA state and prev_pred / prev_target restart on both).
"""
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from koemorph_amd import synth
from koemorph_amd._lib import KM_LOSS_TERM_NAMES
from koemorph_amd.data import SequentialKoeMorphDataset
from koemorph_amd.engine import Engine
from koemorph_amd.metrics import LossTerms
from koemorph_amd.scripts import train_sequential as ts

pytestmark = pytest.mark.gpu

BATCH = 4
EXTRA = dict(perceptual_weight=0.5, temporal_weight=0.2, sparsity_weight=0.01, smoothness_weight=0.1, velocity_weight=0.05)
# the default call reduces each batch's n <= BATCH * 52 squared errors with torch in float32: at worst n roundings of 2^-24 in
# the sum + the square's, the division's and .item()'s; the component call sums in float64 and rounds the mean once to float32
TOTAL_RTOL = (BATCH * 52 + 4) * 2.0 ** -24


def write_pair(d, name, seconds, seed):
    n = int(seconds * 16000)
    wavfile.write(d / f"{name}.wav", 16000, synth.uniform(seed, (n,), -0.5, 0.5).astype(np.float32))
    F = int(seconds * 30)
    labels = synth.uniform(seed + 1, (F, 52), 0, 1).astype(np.float32)
    with open(d / f"{name}.jsonl", "w") as f:
        for i in range(F):
            f.write(json.dumps({"timestamp": i / 30.0, "blendshapes": labels[i].tolist()}) + "\n")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("val")
    write_pair(d, "a", 8.9, 40)
    write_pair(d, "b", 8.8, 50)
    kw = dict(shuffle_files=False, loop_dataset=False, batch_size=BATCH)
    eng = Engine()
    eng.load_state_dict(synth.make_core_params(3, style="trained"))
    eng.finalize()
    resident = SequentialKoeMorphDataset(d, resident_windows=True, **kw)
    st = ts.SequentialTrainer(eng, resident, resident, from_clip=True, dropout=0.0, l1_weight=0.1, extra_loss_terms=dict(EXTRA))
    return eng, st, SequentialKoeMorphDataset(d, **kw)


def replay(eng, st, gathered):
    """The pass done by hand on gathered windows: forward_audio with the carried state, torch MSE per batch (the default
    call's total), and one LossTerms over all batches + one per file (the component call's terms)."""
    st.trainer.sync_inference_weights()
    weights = dict(mse_weight=1.0, l1_weight=0.1, **EXTRA)
    lt, per_file, mse = LossTerms(**weights), {}, []
    state = prev_pred = prev_target = None
    current = None
    for batch in gathered:
        f, B = int(batch["file_indices"][0]), batch["audio"].shape[0]
        first = current != f or state is None or state.shape[0] != B
        if first:
            current, state, prev_pred, prev_target = f, torch.zeros(B, 52, device="cuda"), None, None
        pred = eng.forward_audio(batch["audio"], st._emotion(batch), state=state, first=first)
        mse.append(float(torch.nn.functional.mse_loss(pred, batch["target"]).item()))
        name = batch["file_names"][0]
        per_file.setdefault(name, LossTerms(**weights))
        for acc in (lt, per_file[name]):
            acc.update(pred, batch["target"], prev_pred=prev_pred, prev_target=prev_target)
        prev_pred, prev_target = pred, batch["target"]
    m = lt.compute()
    stats = {k: v.compute() for k, v in per_file.items()}
    return sum(mse) / len(mse), len(mse), m, stats


def test_default_validate_is_what_it_was(setup):
    eng, st, gathered = setup
    total, n, _, _ = replay(eng, st, gathered)
    v = st.validate()
    assert v == {"total": total, "batches": n} and n == 6


def test_components_from_the_resident_clip(setup, monkeypatch):
    eng, st, gathered = setup
    total, n, m, stats = replay(eng, st, gathered)
    calls = []
    orig = Engine.forward_clip
    monkeypatch.setattr(Engine, "forward_clip", lambda self, *a, **k: calls.append(int(a[1].numel())) or orig(self, *a, **k))
    v = st.validate(components=True)
    assert calls == [4, 4, 4, 4, 4, 1]                      # every batch went through km_forward_clip
    assert v["batches"] == n
    print(f"total: default {total!r}, components {v['total']!r}, relative {abs(v['total'] - total) / total:.3e}, allowed {TOTAL_RTOL:.3e}")
    assert abs(v["total"] - total) <= TOTAL_RTOL * total
    # forward_clip is bit-identical to the gathered forward, LossTerms is deterministic: the replay's values exactly
    for k in KM_LOSS_TERM_NAMES:
        assert v["weighted_total" if k == "total" else k] == m[k], k
    assert v["total"] == m["mse"] and v["landmark"] == 0.0 and v["ds_velocity"] == 0.0 and v["temporal"] > 0.0
    assert list(v["sequence_stats"]) == ["a", "b"]
    for name, batches in (("a", 3), ("b", 3)):
        s = v["sequence_stats"][name]
        assert s == {"loss": stats[name]["total"], "smoothness": stats[name]["row_smoothness"], "batches": batches}
    # metrics ride along unchanged
    vm = st.validate(metrics=True, components=True)
    assert vm["total"] == v["total"] and "mae" in vm and vm["sequence_stats"] == v["sequence_stats"]


def test_emotion_provider_falls_back_to_the_gathered_path(setup, monkeypatch):
    """With an emotion provider the trainer gathers (the provider reads window audio): no km_forward_clip call, and with a
    provider that returns, batch by batch, what the built-in fallback returns, the same numbers."""
    eng, st, gathered = setup
    v = st.validate(components=True)
    vectors = iter([st._emotion(batch) for batch in gathered])          # the built-in per-window vectors, in batch order
    seen = []

    def provider(audio):
        seen.append(tuple(audio.shape))
        return next(vectors)
    calls = []
    orig = Engine.forward_clip
    monkeypatch.setattr(Engine, "forward_clip", lambda self, *a, **k: calls.append(1) or orig(self, *a, **k))
    monkeypatch.setattr(st, "emotion_provider", provider)
    v2 = st.validate(components=True)
    assert not calls and seen == [(b, 256 * 533) for b in (4, 4, 4, 4, 4, 1)]
    assert v2 == v
