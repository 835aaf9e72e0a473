// The one-launch core of d_model 256 / 8 heads / 80 mel channels / decoder hidden 128 at window 512 (kernels and their launches; the
// dispatch is km_generic.hip's: its row of kOneLaunchCores, launch_core_generic_packed / _power, launch_core_stream).  A
// translation unit of its own: the kernels of km_generic.hip are compiled exactly as before.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_context.h"
#include "km_device.h"
#include "km_core_args.h"
#include "km_attn256_dev.h"

namespace km {

// ---------------------------------------------------------------------------------------------------------
// core256w_kernel: core512_kernel's counterpart for d_model 256 / 8 heads / decoder hidden 128 at window 512 -- the shape the
// reference's frame_rate=60 recipe trains (dual_stream.yaml + dual_stream_60fps.yaml).  The same three stages in one 512-thread
// workgroup per window: encoder_ln_body<8, 2> (KP = 528), scores_softmax_body<256, 2> (14 row tiles), attn_out_vr32_body
// (km_attn256_dev.h), with Y_b and the softmaxed scores through the workgroup's own L2 lines.  Core512Args carries the arguments
// (its wv_bg member holds wv_bg32 here).  LDS: the encoder's 26 KB static + kCore256wLds dynamic.
// ---------------------------------------------------------------------------------------------------------
template <bool FUSE_DB>
__global__ __launch_bounds__(512) void core256w_kernel(Core512Args a) {
    __shared__ EncLds<8> el;
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const int b = (int)blockIdx.x;
    encoder_ln_body<8, 2, FUSE_DB>(a.xp, a.wce_pg, a.bce, a.ln_g, a.ln_b, a.Y, a.KP, a.src, b, el);
    __syncthreads();          // Y_b is in memory for every wave of this workgroup
    scores_softmax_body<256, 2>(a.Y, a.qk_pg, a.S, a.rows, b, *reinterpret_cast<float (*)[2][kScoresYsFloats]>(gsm));
    __syncthreads();          // ... and the window's attention weights
    attn_out_vr32_body<>(a.S, a.Y, a.wv_bg, a.wf_pg, a.bf, a.w2, a.b2, a.zemo, a.wsum, a.out, a.raw, b, gsm);
}

// the streaming instantiation, as core512_stream_kernel: window b is stream b, a stream whose gate byte is zero returns at once
__global__ __launch_bounds__(512) void core256w_stream_kernel(Core512StreamArgs sa) {
    __shared__ EncLds<8> el;
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const Core512Args& a = sa.c;
    const int b = (int)blockIdx.x;
    if (!sa.st.ready[b]) return;     // workgroup-uniform
    encoder_ln_body<8, 2, true, true>(a.xp, a.wce_pg, a.bce, a.ln_g, a.ln_b, a.Y, a.KP, a.src, b, el, sa.st);
    __syncthreads();
    scores_softmax_body<256, 2>(a.Y, a.qk_pg, a.S, a.rows, b, *reinterpret_cast<float (*)[2][kScoresYsFloats]>(gsm));
    __syncthreads();
    attn_out_vr32_body<true>(a.S, a.Y, a.wv_bg, a.wf_pg, a.bf, a.w2, a.b2, a.zemo, a.wsum, a.out, a.raw, b, gsm, sa.st);
}

template <bool FUSE_DB>
static int launch_core256w_t(const Core512Args& a, int64_t B, int device, hipStream_t st) {
    static PerDeviceOnce once;
    if (once.first(device))
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&core256w_kernel<FUSE_DB>), hipFuncAttributeMaxDynamicSharedMemorySize, kCore256wLds));
    hipLaunchKernelGGL((core256w_kernel<FUSE_DB>), dim3((unsigned)B), dim3(512), kCore256wLds, st, a);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int launch_core256w_kernel(const Core512Args& a, bool fuse_db, int64_t B, int device, hipStream_t st) {
    return fuse_db ? launch_core256w_t<true>(a, B, device, st) : launch_core256w_t<false>(a, B, device, st);
}

int launch_core256w_stream_kernel(const Core512StreamArgs& sa, int64_t S, int device, hipStream_t st) {
    static PerDeviceOnce once;
    if (once.first(device))
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&core256w_stream_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kCore256wLds));
    hipLaunchKernelGGL(core256w_stream_kernel, dim3((unsigned)S), dim3(512), kCore256wLds, st, sa);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km
