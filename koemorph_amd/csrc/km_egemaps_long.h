// The two per-window eGeMAPS kernels for windows beyond the 2048 frames the kernels of km_egemaps.hip hold in static LDS
// (km_egemaps_long.hip): the interface between that file, km_egemaps.hip (which launches them between its per-frame kernels)
// and the emotion objects.  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_egemaps_ragged.h"

namespace km {

namespace egml {
constexpr int REC = 36;                          // floats per frame record: egm::REC (km_egemaps.hip asserts the equality)
constexpr int MAXF_SHORT = 2048;                 // egm::MAXF: up to here the kernels of km_egemaps.hip run
constexpr int64_t MAX_WINDOW = (int64_t)1 << 20; // samples per window: the `basic` back end's limit (emo::BASIC_MAX_WINDOW)
constexpr int MAXF = (int)((MAX_WINDOW - 960) / 160 + 1);   // 6548 frames of 10 ms
constexpr int SORT_MAX = 8192;                   // MAXF padded to a power of two for the bitonic sort
constexpr int CHUNK = 4096;                      // frames of pitch-track inputs staged in LDS at a time
}  // namespace egml

// hipFuncAttributeMaxDynamicSharedMemorySize of the four instantiations on the current device (once per device).  The launchers call
// it themselves; the objects call it at creation so that nothing but launches is left for a stream capture.
int egm_long_prepare();

// egm_viterbi_kernel / egm_functional_kernel of km_egemaps.hip for 1 <= nf <= 6548 frames: n windows, dense (slots null: every
// window has nf frames, records rec_frames apart) or ragged (the frame count of window i is slots[i].nf, empty slots are skipped).
int egm_long_track(float* rec_dev, int nf, int rec_frames, const EgmSlot* slots_dev, int n, hipStream_t st);
int egm_long_functional(const float* rec_dev, int nf, int rec_frames, const EgmSlot* slots_dev, int n, float* out_dev, hipStream_t st);

}  // namespace km
