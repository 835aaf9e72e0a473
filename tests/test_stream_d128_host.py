"""The oracle side of tests/test_gpu_streaming_d128.py on the host: the 30 fps stream shapes at the three ring lengths it uses, and the
loud-burst construction of tests/stream_d128_cases.py -- the loud stream's dB reference must lie in the frame that truncation drops."""
import numpy as np
import pytest

import stream_d128_cases as dc
from koemorph_amd.streaming import chunked_stream_shape, stream_shape
from oracle import mel as omel


@pytest.mark.parametrize("cw,want", [(1.0, dict(ring_len=16000, ring_hop=532, n_frames=31, stream_out_frames=30)),
                                     (4.4, dict(ring_len=70400, ring_hop=532, n_frames=133, stream_out_frames=132)),
                                     (8.5, dict(ring_len=136000, ring_hop=532, n_frames=256, stream_out_frames=255))])
def test_stream_shapes_at_30_fps(cw, want):
    got = stream_shape(cw, dc.UI30, dc.MEL_HOP)
    ring = dc.ring(cw)
    assert got == want and (got["ring_len"], got["ring_hop"]) == (ring.buffer_size, ring.hop_length)
    win = np.zeros(ring.buffer_size, np.float32)
    win[::7] = 0.1
    assert dc.stream_features(win, cw).shape == (got["stream_out_frames"], 80)
    assert omel.stft_power(win, 1024, dc.MEL_HOP, center=True, pad_mode="reflect").shape[0] == got["n_frames"]
    assert chunked_stream_shape(cw, dc.UI30) == dict(fifo_samples=32000, frame_samples=533, ring_hop=532)


def test_oracle_pipeline_of_the_short_ring_case():
    wins, first = dc.short_windows()
    assert first == dc.SHORT_FIRST_READY and sorted(wins) == list(dc.SHORT_CHECKED)
    U, F = 30, 31
    for t in dc.SHORT_CHECKED:
        # every frame the front end computes (expected == F: nothing truncated): the loud stream's dB reference lies past row U
        full = omel.mel_sliding_window(wins[t][dc.LOUD_STREAM], n_fft=1024, hop=dc.MEL_HOP, context_window=float(F), update_interval=1.0)
        assert full.shape == (F, 80)
        peak_rows = np.nonzero(full.max(axis=1) == 0.0)[0]
        assert peak_rows.min() >= U, (t, peak_rows)
        kept = dc.stream_features(wins[t][dc.LOUD_STREAM], dc.SHORT_CW)
        assert kept.shape == (U, 80) and np.array_equal(kept, full[:U]) and kept.max() < 0.0
    for name in dc.VARIANTS:
        first, last = dc.short_expected(name, 30), dc.short_expected(name, 40)
        for e in (first, last):
            assert e.shape == (dc.SHORT_S, 52) and np.isfinite(e).all() and e.min() >= 0.0 and e.max() <= 1.0
        # the inputs move the output: streams differ, ticks differ
        assert np.abs(first[0] - first[1]).max() > 1e-4 and np.abs(first[0] - last[0]).max() > 1e-4
