"""Schedules and host oracle of the streams out of phase (km_stream_fifo_create / _feed / _step / _reset_streams,
ChunkedStreamEngine), shared by tests/test_stream_chunked_host.py (no GPU) and tests/test_gpu_stream_chunked.py.

A schedule is a table counts[step][stream]: on every step stream s is fed the next counts[step][s] samples of its own audio
source (what the FIFO drops is lost, as on a sound card), then every stream steps once.  ``resets`` maps a step to the streams
reset before that step's feed.

simulate() is the reference loop per stream, composed from what oracle/ has: RingBufferOracle (scripts/rt.py:48-99) ->
read(frame_samples) -> MelAudioBufferOracle.add_audio_frame (mel_sliding_window.py:70-116); fired = popped and is_full.  It
records, per step and stream, the flags, the backlog, the popped frame and -- at the (step, stream) pairs a schedule names in
``oracle_pairs`` -- the ring content the float64 model oracle is run on.  Everything is computed once and shared; callers must
not modify it.

  Schedule A   d_model 512, 8 (or 16) heads, 60 fps, 1.0 s ring of 16000 samples at hop 266 (full after 61 frames), 4 streams,
               FIFOs of 1600 samples, frames of 266, 152 steps.
  Schedule B   d_model 256, 8 heads, 30 fps, the 8.5 s ring of 136000 samples at hop 532 (full after 256 frames), 3 streams,
               FIFOs of 32000 samples, frames of 533 (every popped frame loses its 533rd sample), 300 steps.
"""
from __future__ import annotations

import functools

import numpy as np

from koemorph_amd import synth
from oracle import buffers

SR = 16000
UI60 = 1.0 / 60.0


def _counts_a(t, s):
    if s == 0:
        return 0 if 100 <= t <= 109 else 266                  # a pause with a full ring
    if s == 1:
        return 1024 if t % 5 == 0 else 0                      # sound-card chunks, slower than real time
    if s == 2:
        return 0 if t < 20 else (267 if (t - 20) % 2 == 0 else 266)      # joins late
    return 1500 if t % 5 == 0 else 0                          # more than the FIFO drains: overflow


def _counts_b(t, s):
    if s == 0:
        return 533
    if s == 1:
        return 533 if t <= 255 else (1024 if t % 3 == 0 else 0)          # full at step 255, then chunks with idle steps between
    return 0 if t < 20 else 533                               # joins late


SCHEDULES = {
    "A": dict(n_streams=4, steps=152, context_window=1.0, update_interval=UI60, fifo_samples=1600, frame_samples=266, ring_hop=266,
              ring_len=16000, n_max=1500, audio_seed=501, emotion_seed=502, counts=_counts_a, resets={85: (2,)},
              # first fire of streams 1, 3 and 2; stream 0's first row after its pause; stream 2's first two rows after the reset
              oracle_pairs=((60, 3), (78, 1), (80, 2), (110, 0), (145, 2), (146, 2))),
    "B": dict(n_streams=3, steps=300, context_window=8.5, update_interval=0.0333, fifo_samples=32000, frame_samples=533, ring_hop=532,
              ring_len=136000, n_max=1024, audio_seed=511, emotion_seed=512, counts=_counts_b, resets={},
              # first fire of every stream; a smoothed row; stream 1's first row after an idle step; a replayed step
              oracle_pairs=((255, 0), (255, 1), (256, 0), (261, 1), (275, 2), (282, 2))),
}


def counts_table(name: str, steps=None) -> np.ndarray:
    c = SCHEDULES[name]
    steps = c["steps"] if steps is None else steps
    return np.array([[c["counts"](t, s) for s in range(c["n_streams"])] for t in range(steps)], np.int32)


@functools.lru_cache(maxsize=None)
def sources(name: str) -> np.ndarray:
    """(n_streams, total) float32: every stream's own audio; a step takes the next counts[step][s] samples of row s."""
    c = SCHEDULES[name]
    total = int(counts_table(name).sum(axis=0).max())
    x = synth.make_audio(c["audio_seed"], c["n_streams"], total)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def emotion(name: str) -> np.ndarray:
    c = SCHEDULES[name]
    e = synth.normal(c["emotion_seed"], (c["n_streams"], 256))
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def chunks(name: str, steps=None):
    """[step] -> (n_streams, n_max) float32: the feed tensor of the step (row s holds counts[step][s] samples, then zeros)."""
    c = SCHEDULES[name]
    cnt, src = counts_table(name, steps), sources(name)
    pos = np.zeros(c["n_streams"], np.int64)
    out = []
    for t in range(cnt.shape[0]):
        x = np.zeros((c["n_streams"], c["n_max"]), np.float32)
        for s in range(c["n_streams"]):
            n = int(cnt[t, s])
            x[s, :n] = src[s, pos[s]:pos[s] + n]
            pos[s] += n
        x.setflags(write=False)
        out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def simulate(name: str, steps=None, with_resets: bool = True) -> dict:
    """The reference loop of every stream.  (steps, n_streams) arrays popped / ready / fired (bool), backlog, dropped (samples the
    FIFO refused on that step) and life (resets of the stream so far); pops[s] = [(step, life, frame)] in order; windows[(step,
    stream)] = the ring content at the schedule's oracle pairs; truncated[s] = popped frames whose tail the ring dropped."""
    c = SCHEDULES[name]
    S, frame = c["n_streams"], c["frame_samples"]
    cnt, x = counts_table(name, steps), chunks(name, steps)
    T = cnt.shape[0]
    fifos = [buffers.RingBufferOracle(c["fifo_samples"]) for _ in range(S)]
    rings = [buffers.MelAudioBufferOracle(c["context_window"], SR, c["update_interval"]) for _ in range(S)]
    assert rings[0].hop_length == c["ring_hop"] and rings[0].buffer_size == c["ring_len"]
    popped, ready, fired = (np.zeros((T, S), bool) for _ in range(3))
    backlog, dropped, life = (np.zeros((T, S), np.int32) for _ in range(3))
    pops = [[] for _ in range(S)]
    windows, lives, truncated = {}, [0] * S, [0] * S
    for t in range(T):
        if with_resets:
            for s in c["resets"].get(t, ()):
                fifos[s] = buffers.RingBufferOracle(c["fifo_samples"])
                rings[s] = buffers.MelAudioBufferOracle(c["context_window"], SR, c["update_interval"])
                lives[s] += 1
        for s in range(S):
            n = int(cnt[t, s])
            dropped[t, s] = max(0, n - (fifos[s].size - fifos[s].available))
            fifos[s].write(x[t][s, :n])
            f = fifos[s].read(frame)
            if f is not None:
                popped[t, s] = True
                before = rings[s].write_ptr
                assert rings[s].add_audio_frame(f)
                kept = rings[s].audio_buffer[(before + np.arange(rings[s].hop_length)) % rings[s].buffer_size]
                assert np.array_equal(kept[:min(frame, len(kept))], f[:len(kept)])
                truncated[s] += int(len(f) == len(kept) + 1)
                pops[s].append((t, lives[s], f))
            ready[t, s] = rings[s].is_full
            fired[t, s] = popped[t, s] and rings[s].is_full
            backlog[t, s] = fifos[s].available // frame
            life[t, s] = lives[s]
            if (t, s) in c["oracle_pairs"]:
                assert fired[t, s], (t, s)
                windows[(t, s)] = rings[s].get_current_audio()
    for a in (popped, ready, fired, backlog, dropped, life):
        a.setflags(write=False)
    return dict(popped=popped, ready=ready, fired=fired, backlog=backlog, dropped=dropped, life=life, pops=pops, windows=windows,
                truncated=truncated)


def previous_fire(sim: dict, t: int, s: int):
    """The last step before t on which stream s fired in the same life, or None: where the EMA history of row (t, s) comes from."""
    for u in range(t - 1, -1, -1):
        if sim["life"][u, s] != sim["life"][t, s]:
            return None
        if sim["fired"][u, s]:
            return u
    return None
