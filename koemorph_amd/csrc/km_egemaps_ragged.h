// eGeMAPS functionals of ragged windows read in place from stream rings: the interface between km_emotion_stream.hip (which
// writes the slot table on the device) and km_egemaps.hip (which launches the five kernels' ragged instantiations).  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace km {

// One window of an update.  stream < 0: the slot is empty and every block that belongs to it exits at once.
struct EgmSlot {
    int32_t stream;   // row of the ring array
    int32_t start;    // ring index of the window's first sample, 0 <= start < ring_len
    int32_t len;      // samples, <= ring_len; sample i is ring[(start + i) mod ring_len]
    int32_t nf;       // 10 ms frames of a window of len samples (km_egemaps_num_frames), 1 <= nf <= max_nf
};

// peak, frame, pitch-track, voiced and functional kernels for n_slots slots: grids of max_nf x n_slots (per frame) and n_slots (per
// window) whatever the table holds.  scale_dev (n_slots), rec_dev (n_slots, max_nf, 36), out_dev (n_slots, 88): rows of empty slots
// are not written.  No allocation, no synchronisation.  max_nf <= 2048; with long_windows max_nf <= 6548 and the two per-window kernels
// (km_egemaps_window.hip) run at their long tier for every slot (equal bits on equal records up to 2048 frames).  feature_set 1 (GeMAPS,
// km_egemaps_dev.h): the frame and functional kernels' GeMAPS instantiations, out_dev is (n_slots, 62).
int egm_ragged_functionals(void* plan, const float* rings_dev, int64_t ring_len, const EgmSlot* slots_dev, int n_slots, int max_nf,
                           float* scale_dev, float* rec_dev, float* out_dev, hipStream_t st, bool long_windows = false, int feature_set = 0);

// Its first four launches alone (peak, frame, pitch track, voiced): the frame records of every slot's window in rec_dev, for a caller
// that reduces them itself (km_koemorph_audio.hip writes descriptor rows).  egm_ragged_functionals is this call plus the functional kernel.
int egm_ragged_records(void* plan, const float* rings_dev, int64_t ring_len, const EgmSlot* slots_dev, int n_slots, int max_nf, float* scale_dev,
                       float* rec_dev, hipStream_t st, bool long_windows = false, int feature_set = 0);

}  // namespace km
