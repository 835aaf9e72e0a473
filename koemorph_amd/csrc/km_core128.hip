// The one-launch core of d_model 128 / 4 heads / 80 mel channels / decoder hidden 64 at window 128 or 256 -- the reference's `fast`
// and `basic` variants (kernels and their launches; the dispatch is km_generic.hip's: its row of kOneLaunchCores,
// launch_core_generic_packed / _power, launch_core_stream).  A translation unit of its own: the kernels of every other unit are
// compiled exactly as before.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_context.h"
#include "km_device.h"
#include "km_core_args.h"
#include "km_core128_dev.h"

namespace km {

// ---------------------------------------------------------------------------------------------------------
// core128_kernel: core256w_kernel's counterpart at d_model 128.  One 256-thread workgroup per window, one wave per SIMD, three
// barrier-separated stages: encoder_ln_body<4, 2> (KP = 144 / 272), then scores + softmax and value projection + P V + fold + tail in
// attn128_body (km_core128_dev.h), which stages Y_b into LDS once for both.  Core512Args carries the arguments (its wce_pg, wv_bg
// and wf_pg members hold the wce_pg128, wv_bg128 and wf_pg128 images).  LDS: the encoder's 23 KB static, reused by the last stage,
// + kCore128Lds (41 KB) dynamic: two workgroups per CU.
// ---------------------------------------------------------------------------------------------------------
static_assert(kCore128OsFloats <= (int)(sizeof(EncLds<4>::As) / sizeof(float)) && 4 * 32 <= 80 * 4, "the last stage's O and partial sums fit the encoder's tiles");

template <bool FUSE_DB>
__global__ __launch_bounds__(256) void core128_kernel(Core512Args a) {
    __shared__ EncLds<4> el;
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const int b = (int)blockIdx.x;
    encoder_ln_body<4, 2, FUSE_DB>(a.xp, a.wce_pg, a.bce, a.ln_g, a.ln_b, a.Y, a.KP, a.src, b, el);
    __syncthreads();          // Y_b is in memory for every wave of this workgroup, and the encoder's LDS is free
    attn128_body<>(a.Y, a.qk_pg, a.S, a.wv_bg, a.wf_pg, a.bf, a.w2, a.b2, a.zemo, a.wsum, a.out, a.raw, b, gsm, el.As, el.Ps[0]);
}

// the streaming instantiation, as core256w_stream_kernel: window b is stream b, a stream whose gate byte is zero returns at once
__global__ __launch_bounds__(256) void core128_stream_kernel(Core512StreamArgs sa) {
    __shared__ EncLds<4> el;
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const Core512Args& a = sa.c;
    const int b = (int)blockIdx.x;
    if (!sa.st.ready[b]) return;     // workgroup-uniform
    encoder_ln_body<4, 2, true, true>(a.xp, a.wce_pg, a.bce, a.ln_g, a.ln_b, a.Y, a.KP, a.src, b, el, sa.st);
    __syncthreads();
    attn128_body<true>(a.Y, a.qk_pg, a.S, a.wv_bg, a.wf_pg, a.bf, a.w2, a.b2, a.zemo, a.wsum, a.out, a.raw, b, gsm, el.As, el.Ps[0], sa.st);
}

template <bool FUSE_DB>
static int launch_core128_t(const Core512Args& a, int64_t B, int device, hipStream_t st) {
    static PerDeviceOnce once;
    if (once.first(device))
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&core128_kernel<FUSE_DB>), hipFuncAttributeMaxDynamicSharedMemorySize, kCore128Lds));
    hipLaunchKernelGGL((core128_kernel<FUSE_DB>), dim3((unsigned)B), dim3(256), kCore128Lds, st, a);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

int launch_core128_kernel(const Core512Args& a, bool fuse_db, int64_t B, int device, hipStream_t st) {
    return fuse_db ? launch_core128_t<true>(a, B, device, st) : launch_core128_t<false>(a, B, device, st);
}

int launch_core128_stream_kernel(const Core512StreamArgs& sa, int64_t S, int device, hipStream_t st) {
    static PerDeviceOnce once;
    if (once.first(device))
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&core128_stream_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kCore128Lds));
    hipLaunchKernelGGL(core128_stream_kernel, dim3((unsigned)S), dim3(256), kCore128Lds, st, sa);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km
