// The nine prosodic features of ragged windows read in place from stream rings: the interface between km_emotion_stream.hip
// (whose plan kernel writes the slot table on the device) and km_prosody.hip.  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_egemaps_ragged.h"

namespace km {

// Frame and window kernel for n_slots slots: grids of max_frames x n_slots and n_slots whatever the table holds; a slot's `nf`
// (eGeMAPS frames) is not read, the 32 ms frames follow from its `len`.  rec_dev (n_slots, max_frames, 4), out_dev (n_slots, 9):
// rows of empty slots are not written.  No allocation, no synchronisation.
int prosody_ragged(void* plan, const float* rings_dev, int64_t ring_len, const EgmSlot* slots_dev, int n_slots, int max_frames,
                   float* rec_dev, float* out_dev, hipStream_t st);

}  // namespace km
