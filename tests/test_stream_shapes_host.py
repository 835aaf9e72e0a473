"""Host side of the 60 fps streaming shape (no GPU): the ring / frame arithmetic of km_stream_create as the package restates it
against MelAudioBufferOracle, the oracle's extractor and the values the reference formulas give, and the float64-oracle pipeline of tests/test_gpu_streaming_d512.py on
that test's own inputs -- so that its expected values do not rest on oracle arguments nothing else has exercised."""
import numpy as np
import pytest

import stream_d512_cases as sc
from koemorph_amd.streaming import stream_shape
from oracle import buffers, mel as omel


@pytest.mark.parametrize("cw,ui,mel_hop,want", [
    (8.5, 1.0 / 30.0, 533, dict(ring_len=136000, ring_hop=533, n_frames=256, stream_out_frames=255)),
    (8.5, 1.0 / 60.0, 266, dict(ring_len=136000, ring_hop=266, n_frames=512, stream_out_frames=510)),
    (1.0, 1.0 / 60.0, 266, dict(ring_len=16000, ring_hop=266, n_frames=61, stream_out_frames=60)),
])
def test_stream_shape_matches_the_ring_oracle_and_the_reference_formulas(cw, ui, mel_hop, want):
    got = stream_shape(cw, ui, mel_hop)
    ring = buffers.MelAudioBufferOracle(cw, 16000, ui)
    assert (got["ring_len"], got["ring_hop"]) == (ring.buffer_size, ring.hop_length)
    # the rows the oracle's extractor returns for a full ring, and the frames it computed before truncating
    win = np.zeros(ring.buffer_size, np.float32)
    win[::7] = 0.1
    assert omel.mel_sliding_window(win, n_fft=1024, hop=mel_hop, context_window=cw, update_interval=ui).shape == (got["stream_out_frames"], 80)
    assert omel.stft_power(win, 1024, mel_hop, center=True, pad_mode="reflect").shape[0] == got["n_frames"]
    assert got == want


def test_oracle_pipeline_of_the_short_ring_case():
    wins, first = sc.short_windows()
    assert first == sc.SHORT_FIRST_READY and sorted(wins) == list(sc.SHORT_CHECKED)
    shape = stream_shape(sc.SHORT_CW, sc.UI60, sc.MEL_HOP)
    U, F = shape["stream_out_frames"], shape["n_frames"]
    assert U < F < 512
    for t in sc.SHORT_CHECKED:
        # every frame the front end computes (expected == F: nothing truncated): the loud stream's dB reference lies past row U
        full = omel.mel_sliding_window(wins[t][sc.LOUD_STREAM], n_fft=1024, hop=sc.MEL_HOP, context_window=float(F), update_interval=1.0)
        assert full.shape == (F, 80)
        peak_rows = np.nonzero(full.max(axis=1) == 0.0)[0]
        assert peak_rows.min() >= U, (t, peak_rows)
        kept = sc.stream_features(wins[t][sc.LOUD_STREAM], sc.SHORT_CW)
        assert kept.shape == (U, 80) and np.array_equal(kept, full[:U]) and kept.max() < 0.0
    for heads in (8, 16):
        first, last = sc.short_expected(heads, 60), sc.short_expected(heads, 70)
        for e in (first, last):
            assert e.shape == (sc.SHORT_S, 52) and np.isfinite(e).all() and e.min() >= 0.0 and e.max() <= 1.0
        # the inputs move the output: streams differ, ticks differ, head counts differ
        assert np.abs(first[0] - first[1]).max() > 1e-4 and np.abs(first[0] - last[0]).max() > 1e-4
    assert np.abs(sc.short_expected(8, 60) - sc.short_expected(16, 60)).max() > 1e-5
