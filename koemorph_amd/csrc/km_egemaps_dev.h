// What the eGeMAPS kernel files share on the device: the frame record's layout, the few constants both km_egemaps.hip (peak, frame and
// voiced kernels) and km_egemaps_window.hip (pitch track and functionals) need, and the block-wide sum.  Internal, device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace km {

namespace egm {
constexpr int SR = 16000, HOP = 160;
constexpr int REC = 36;                 // floats per frame record (layout below)
enum Rec { R_LOUD = 0, R_ALPHA, R_HAMM, R_SL0, R_SL1, R_FLUX, R_MFCC, R_RMS = 10, R_CF = 11, R_CS = 14, R_VOI = 17, R_F = 18, R_BW = 21,
           R_F0 = 24, R_JIT, R_SHIM, R_HNR, R_H1H2, R_H1A3, R_FAMP = 30 };
constexpr float VOICING_CUTOFF = 0.55f, RMS_FLOOR = 0.001f;   // on the autocorrelation measure (oracle/egemaps.py acf_strength)

// The feature set a call or an object produces (KM_FEATURE_SET_*): the 88 functionals of eGeMAPSv02, or the 62 of GeMAPS v01b -- the
// 88 without the spectral flux (5), MFCC 1-4 (16), the bandwidths of F2 and F3 (4) and the equivalent sound level (1), in the order
// the 88 have.  The frame and functional kernels take it as a template parameter; gemaps_col is where an eGeMAPS column lands.
constexpr int SET_EGEMAPS = 0, SET_GEMAPS = 1;
constexpr int NFEAT_EGEMAPS = 88, NFEAT_GEMAPS = 62;
constexpr bool set_known(int set) { return set == SET_EGEMAPS || set == SET_GEMAPS; }
constexpr int set_width(int set) { return set == SET_EGEMAPS ? NFEAT_EGEMAPS : set == SET_GEMAPS ? NFEAT_GEMAPS : -1; }
constexpr bool gemaps_keeps(int col) {
    return !((col >= 20 && col <= 29) || col == 48 || col == 49 || col == 54 || col == 55 || (col >= 66 && col <= 75) || col == 80 || col == 87);
}
constexpr int gemaps_col(int col) {                // position of eGeMAPS column `col` among the 62, or -1 where GeMAPS has none
    if (!gemaps_keeps(col)) return -1;
    int n = 0;
    for (int i = 0; i < col; ++i) n += gemaps_keeps(i) ? 1 : 0;
    return n;
}
constexpr int gemaps_pos(int col) {                // the same for a column that is kept, as the kernel computes it: the removed ones below it
    return col - (col < 30 ? 0 : col < 50 ? 10 : col < 56 ? 12 : col < 76 ? 14 : col < 81 ? 24 : 25);
}
constexpr bool gemaps_pos_agrees() {
    for (int c = 0; c < NFEAT_EGEMAPS; ++c) if (gemaps_keeps(c) && gemaps_pos(c) != gemaps_col(c)) return false;
    return true;
}
static_assert(gemaps_col(87) == -1 && gemaps_col(86) == NFEAT_GEMAPS - 1 && gemaps_pos_agrees(), "62 of the 88 columns are kept");
}  // namespace egm

// block-wide sum (256 threads = 4 waves), fixed order: an xor butterfly inside each wave, then the four wave results
// in wave order through 4 floats of LDS scratch -- two barriers instead of the ten of a 256-element LDS tree
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace km
