// The two per-window eGeMAPS kernels, pitch track and functionals (km_egemaps_window.hip): one source each, compiled for two
// capacity tiers.  The interface between that file, km_egemaps.hip (which launches them between its per-frame kernels) and the
// emotion objects.  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_egemaps_dev.h"
#include "km_egemaps_ragged.h"

namespace km {

namespace egm {
constexpr int64_t MAX_WINDOW = (int64_t)1 << 20;   // samples per window: the `basic` back end's limit (emo::BASIC_MAX_WINDOW)

// How much of a window the two kernels hold in LDS.  Every plain entry point and object runs the short tier; the `_long` ones run
// the long tier beyond 2048 frames (objects: for every slot), which gives the short tier's bits up to there.
struct ShortTier {
    static constexpr int MAXF = 2048;              // frames per window (20.5 s)
    static constexpr int CHUNK = 2048;             // frames of pitch-track inputs staged in LDS at a time: the window in a single pass
    static constexpr int SORT_MAX = 2048;          // MAXF padded to a power of two for the bitonic sort
};
struct LongTier {
    static constexpr int MAXF = (int)((MAX_WINDOW - 960) / 160 + 1);   // 6548 frames of 10 ms (65.5 s)
    static constexpr int CHUNK = 4096;
    static constexpr int SORT_MAX = 8192;
};
// dynamic LDS of a launch: the track's [7][CHUNK] inputs and a back pointer per frame; the functionals' two contours and sort buffer
template <class Tier> constexpr int track_lds() { return 7 * Tier::CHUNK * (int)sizeof(float) + (Tier::MAXF + 15) / 16 * 16; }
template <class Tier> constexpr int func_lds() { return (2 * Tier::MAXF + Tier::SORT_MAX) * (int)sizeof(float); }
}  // namespace egm

// hipFuncAttributeMaxDynamicSharedMemorySize of the long tier's four instantiations on the current device (once per device; the short
// tier stays below 64 KB and needs none).  The launchers call it themselves for the long tier; the long objects call it at creation
// so that nothing but launches is left for a stream capture.
int egm_window_prepare();

// Pitch track (writes the F0 column of the records) and functionals (88 floats per window, 62 for the GeMAPS feature set) of n windows, dense (slots null: every
// window has nf frames, records rec_frames apart) or ragged (the frame count of window i is slots[i].nf, empty slots are skipped).
// rec_frames is at most the tier's MAXF.  One launch of n workgroups of 256 threads each.
int egm_track(float* rec_dev, int nf, int rec_frames, const EgmSlot* slots_dev, int n, bool long_tier, hipStream_t st);
int egm_functional(const float* rec_dev, int nf, int rec_frames, const EgmSlot* slots_dev, int n, float* out_dev, bool long_tier, hipStream_t st,
                   int feature_set = egm::SET_EGEMAPS);

}  // namespace km
