// The eGeMAPS low-level descriptors per frame (km_egemaps_lld.hip): the smoothed contours behind the functionals, written out as rows
// instead of reduced.  The interface between that file and km_egemaps.hip, which launches it behind its per-frame kernels.  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_egemaps_dev.h"

namespace km {

namespace egm {
constexpr int NLLD_EGEMAPS = 25, NLLD_GEMAPS = 18;     // descriptors per frame: GeMAPS is the 25 without flux, MFCC 1-4, the bandwidths of F2 and F3
constexpr int lld_width(int set) { return set == SET_EGEMAPS ? NLLD_EGEMAPS : set == SET_GEMAPS ? NLLD_GEMAPS : -1; }
constexpr double LLD_FPS_MIN = 1.0, LLD_FPS_MAX = 400.0;
constexpr int64_t MAX_LLD_GRID = (int64_t)1 << 20;   // samples a frame grid is laid over: the longest window (65.5 s)
constexpr int LLD_MAXF =(int)((((int64_t)1 << 20) - 960) / 160 + 1);   // 6548 frames: the longest window any eGeMAPS call takes

constexpr int LLD_CORE = 128;                 // frames a tile smooths
constexpr int LLD_STAGE = LLD_CORE + 4;       // ... and stages: two frames of halo a side
constexpr int LLD_FIRST_NZ = 10;              // eGeMAPS columns 0-9: plain average; 10: semitone of the smoothed F0; 11-24: masked non-zero average

// eGeMAPS column of column c of the set, and the record field an eGeMAPS column is smoothed from (10: the F0 itself)
template <int SET> __host__ __device__ constexpr int lld_ecol(int c) {
    return SET == SET_EGEMAPS ? c : c < 5 ? c : c < 15 ? c + 5 : c == 15 ? 21 : c == 16 ? 22 : 24;
}
__host__ __device__ constexpr int lld_field(int e) {
    return e < LLD_FIRST_NZ ? e : e == 10 ? (int)R_F0 : e < 16 ? R_JIT + (e - 11) : ((e - 16) % 3 == 0 ? R_F : (e - 16) % 3 == 1 ? R_BW : R_FAMP) + (e - 16) / 3;
}
}  // namespace egm

// rows of the frame grid: fps == 0 -> the native 10 ms frames of a window of L samples; otherwise int(L / 16000 * fps) in float64, in
// that order; -1 for an fps that is not finite or outside 1 .. 400
int64_t egm_lld_frames(int64_t L, double fps);

// Descriptor rows of n windows whose records lie rec_frames * 36 floats apart, nf frames each: out_dev (n, T_out, lld_width) row-major.
// fps == 0: T_out == nf and row k is frame k; otherwise row k sits at frame coordinate k * 100.0 / fps.  One launch, nothing else.
int egm_lld(const float* rec_dev, int nf, int rec_frames, int n, int64_t T_out, double fps, float* out_dev, hipStream_t st, int feature_set);

}  // namespace km
