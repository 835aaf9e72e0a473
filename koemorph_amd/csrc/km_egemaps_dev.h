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
