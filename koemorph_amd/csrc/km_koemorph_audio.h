// Audio front of the KoeMorphModel stream engine (km_koemorph_audio_*, km_koemorph_audio.hip): the clock and window arithmetic of a
// push, one function for the device (kma_advance_kernel) and the host (km_koemorph_audio_schedule, the tests).  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_egemaps_ragged.h"

namespace km {

// One stream's entry of a push's table.  Frame k of a stream is due once (k + 1) * hop samples have arrived; a push that takes the
// stream from n0 to n samples renders frames n0 / hop .. n / hop - 1.  The emotion window of a push that leaves new frames starts at
// a0, the smallest multiple of 160 that is >= n - W (0 while n <= W), and ends at n: len = n - a0 samples, m = a0 / 160 frames in
// front of it, nf = 10 ms frames of len samples (0 below 960).
struct KmaEntry {
    long long first;    // first new frame
    long long a0, m;    // the window's first sample and its frame offset
    long long total;    // samples after the push
    int32_t rows;       // new frames
    int32_t len, nf;    // the window (0, 0 where the push leaves no new frame)
    int32_t origin;     // ring index of the life's sample 0
};

// n0 samples so far, `pushed` more (already clamped to 0 .. max_samples).  Sample i of a life sits at (origin + i) mod ring_len: a
// reset leaves the ring's write position where it stands and makes it the new life's origin.  *slot: where the ragged eGeMAPS kernels
// find the window in the stream's ring; stream -1 where there is nothing to compute.
__host__ __device__ inline KmaEntry kma_schedule(long long n0, int pushed, int hop, int W, int ring_len, int origin, int stream, EgmSlot* slot) {
    KmaEntry e{};
    const long long n = n0 + pushed;
    e.total = n;
    e.origin = origin;
    e.first = n0 / hop;
    e.rows = (int32_t)(n / hop - e.first);
    *slot = EgmSlot{-1, 0, 0, 0};
    if (e.rows < 1) return e;
    e.a0 = n <= W ? 0 : (n - W + 159) / 160 * 160;
    e.m = e.a0 / 160;
    e.len = (int32_t)(n - e.a0);
    e.nf = e.len < 960 ? 0 : (e.len - 960) / 160 + 1;
    if (e.nf > 0) *slot = EgmSlot{stream, (int32_t)((origin + e.a0) % ring_len), e.len, e.nf};
    return e;
}

}  // namespace km
