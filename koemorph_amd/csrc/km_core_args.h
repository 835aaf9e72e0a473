// Kernel arguments of the one-launch generic cores (core512_kernel in km_generic.hip, core256w_kernel in km_core256w.hip, core128_kernel
// in km_core128.hip) and the launchers of the latter two (core512's are in km_generic.hip, beside the table of the three).  Internal: not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_encoder_dev.h"

namespace km {

struct Core512Args {
    const float* xp; const float* wce_pg; const float* bce; const float* ln_g; const float* ln_b; float* Y; int KP; EncSrc src;
    const float* qk_pg; float* S; int rows;
    const float* wv_bg; const float* wf_pg; const float* bf; const float* w2; const float* b2; const float* zemo; const float* wsum;
    float* out; float* raw;
};
struct Core512StreamArgs { Core512Args c; StreamSrc st; };

// A one-launch core's two launchers, as the table in km_generic.hip holds them: B windows (fuse_db: rows from the power-mel of a.src
// instead of the packed image a.xp) and S streams.  The launch only: what follows it (window maxima, maps) is the caller's
using CoreLaunch = int (*)(const Core512Args& a, bool fuse_db, int64_t B, int device, hipStream_t st);
using CoreStreamLaunch = int (*)(const Core512StreamArgs& sa, int64_t S, int device, hipStream_t st);

// km_core256w.hip: one 512-thread workgroup per window / stream; a.wv_bg holds the wv_bg32 image
int launch_core256w_kernel(const Core512Args& a, bool fuse_db, int64_t B, int device, hipStream_t st);
int launch_core256w_stream_kernel(const Core512StreamArgs& sa, int64_t S, int device, hipStream_t st);

// km_core128.hip: one 256-thread workgroup per window / stream at d_model 128 / 4 heads; a.wce_pg, a.wv_bg and a.wf_pg hold the
// wce_pg128, wv_bg128 and wf_pg128 images
int launch_core128_kernel(const Core512Args& a, bool fuse_db, int64_t B, int device, hipStream_t st);
int launch_core128_stream_kernel(const Core512StreamArgs& sa, int64_t S, int device, hipStream_t st);

}  // namespace km
