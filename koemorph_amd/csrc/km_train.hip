// Optimizer of the training step for gfx950: global-norm clipping and fused AdamW over the flat parameter bucket, and
// the padded copy of the channel encoder weight that is kept beside the master parameters.
//
// Replaces, per rank, the tail of SequentialTrainer.train_epoch (reference src/train_sequential.py:158-181):
//   clip_grad_norm_(params, 1.0); AdamW.step()
// for the 28 tensors of DualStreamCrossAttention + smoothing_alpha (837 738 fp32 at d=256/T=256).  The gradients arrive
// in ONE flat caller-owned bucket in state-dict order -- written by the training step itself (km_trainp.hip), and what
// the data-parallel build all-reduces over RCCL (koemorph_amd/parallel.py) before km_train_adamw.  train_adamw is two
// launches: partial sums of squares (which also advance the device-side step counters), then norm + clip + AdamW.
#include <hip/hip_runtime.h>

#include "km_context.h"

namespace km {


// sum of squares of the flat gradient, deterministic two-stage reduction
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part,
                                                            int* __restrict__ steps, int alpha_live) {
    __shared__ float sh[256];
    // the 1-based AdamW step counters live on the device (graph replay): advanced here, one kernel ahead of their readers
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        steps[0] += 1;
        if (alpha_live) steps[1] += 1;
    }
    float a = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a += g[i] * g[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// The channel encoder weight is read by the training program as rows of KP floats (16-byte rows for the LDS-DMA tile, zeros
// beyond the KT = T + 3 columns).  The copy is kept beside the master parameters -- rewritten wherever they are: here, and by
// train_refresh_padded_weights after an upload -- instead of being rebuilt by an operation of every step.
struct PaddedCopy {
    float* dst; int64_t off; int64_t n; int kt, kp;      // parameters [off, off + n) are (n / kt) rows of kt floats
    __device__ __forceinline__ void put(int64_t i, float v) const {
        const int64_t j = i - off;
        if (dst && j >= 0 && j < n) { const int64_t r = j / kt; dst[r * kp + (j - r * kt)] = v; }
    }
};

// 1 - beta^t of step t without the cancellation of 1.0f - powf(beta, t): while beta^t is close to 1 (beta2 = 0.999 up to
// t ~ 100) rounding it to float32 costs 2^-24 / (1 - beta^t) of the correction, 500 ulp at t = 2
__device__ __forceinline__ float bias_correction(float beta, int t) { return -expm1f((float)t * logf(beta)); }

// torch.nn.utils.clip_grad_norm_(max_norm) + torch.optim.AdamW (decoupled weight decay, bias correction).
// smoothing_alpha is outside the autograd graph whenever the EMA passes its input through (first call / batch-size
// change / smoothing off): torch leaves its .grad as None and AdamW then skips it entirely (no decay, no moment
// update, its own step counter).  alpha_idx / alpha_live / (abc1, abc2) reproduce that.
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                    const float* __restrict__ g, int64_t n, const float* __restrict__ part,
                                                    float* __restrict__ gnorm_out, float max_norm, float lr, float b1, float b2,
                                                    float eps, float wd, const int* __restrict__ steps, int64_t alpha_idx,
                                                    int alpha_live, PaddedCopy pc) {
    // global gradient norm from the 256 partial sums: every block runs the same fixed-order tree (a butterfly inside each
    // wave, then the four wave sums in wave order), so all blocks agree bit for bit
    __shared__ float sh[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // One group of four consecutive parameters per thread (818 workgroups for the 837 744 parameters: 8.3 us; four groups per thread --
    // 205 workgroups, one round of the chip -- measured 11.1 us: the kernel is bound by the square root + two divisions per parameter,
    // not by its workgroup count).  Parameters, moments and gradients are requested FIRST: their round trip runs beside the norm's
    // (partials -> butterfly -> barrier) instead of behind it.
    constexpr int GR = 1;
    int64_t i0[GR];
    bool whole[GR];
    float4 p4[GR], m4[GR], v4[GR], g4[GR];
#pragma unroll
    for (int u = 0; u < GR; ++u) {
        i0[u] = ((int64_t)blockIdx.x * (256 * GR) + u * 256 + tid) * 4;
        whole[u] = i0[u] + 3 < n && (alpha_idx < i0[u] || alpha_idx > i0[u] + 3) && (reinterpret_cast<uintptr_t>(g) & 15) == 0;
        p4[u] = m4[u] = v4[u] = g4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (whole[u]) {
            p4[u] = *reinterpret_cast<const float4*>(p + i0[u]); m4[u] = *reinterpret_cast<const float4*>(m + i0[u]);
            v4[u] = *reinterpret_cast<const float4*>(v + i0[u]); g4[u] = *reinterpret_cast<const float4*>(g + i0[u]);
        }
    }
    float s = part[tid];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sh[wave] = s;
    // the 1-based step counters live on the device (advanced by sumsq_partial_kernel) so that the launch can be replayed
    // from a hipGraph: steps[0] = optimizer step, steps[1] = number of updates smoothing_alpha has received.  The bias
    // corrections are the same for every element but smoothing_alpha: one thread computes them for the block.
    if (tid == 0) {
        const int t = steps[0];
        sh[4] = bias_correction(b1, t);
        sh[5] = bias_correction(b2, t);
    }
    __syncthreads();
    const float gnorm = sqrtf((sh[0] + sh[1]) + (sh[2] + sh[3]));
    if (blockIdx.x == 0 && tid == 0) gnorm_out[0] = gnorm;
    float scale = 1.f;
    if (max_norm > 0.f) {
        // clip_coef, clamped to 1 the way torch.clamp(max=1) does it: a NaN norm (one NaN gradient, error_if_nonfinite=False)
        // stays a NaN scale and reaches every parameter
        const float c = max_norm / (gnorm + 1e-6f);
        scale = !(c >= 1.f) ? c : 1.f;
    }
    const float bc1_all = sh[4], bc2_all = sh[5];
    // The fused multiply-adds are spelled out: left to the compiler's contraction, the float4 path and the element path below
    // were fused differently (fma(1 - b1, g, b1 m) against fma(b1, m, (1 - b1) g), likewise v), so smoothing_alpha's neighbours,
    // and every element of a bucket that is not 16-byte aligned, were rounded unlike the rest.  These are the float4 path's forms.
    const float decay = fmaf(-lr, wd, 1.0f);
    auto update = [&](float& pi, float& mi, float& vi, float gi, float bc1, float bc2) {
        gi *= scale;
        mi = fmaf(1.0f - b1, gi, b1 * mi);
        vi = fmaf(gi, (1.0f - b2) * gi, b2 * vi);
        const float denom = sqrtf(vi) / sqrtf(bc2) + eps;
        pi = fmaf(pi, decay, -((lr / bc1) * mi / denom));
    };
#pragma unroll
    for (int u = 0; u < GR; ++u) {
        if (i0[u] >= n) continue;
        if (whole[u]) {
            update(p4[u].x, m4[u].x, v4[u].x, g4[u].x, bc1_all, bc2_all);
            update(p4[u].y, m4[u].y, v4[u].y, g4[u].y, bc1_all, bc2_all);
            update(p4[u].z, m4[u].z, v4[u].z, g4[u].z, bc1_all, bc2_all);
            update(p4[u].w, m4[u].w, v4[u].w, g4[u].w, bc1_all, bc2_all);
            *reinterpret_cast<float4*>(p + i0[u]) = p4[u];
            *reinterpret_cast<float4*>(m + i0[u]) = m4[u];
            *reinterpret_cast<float4*>(v + i0[u]) = v4[u];
            pc.put(i0[u], p4[u].x); pc.put(i0[u] + 1, p4[u].y); pc.put(i0[u] + 2, p4[u].z); pc.put(i0[u] + 3, p4[u].w);
            continue;
        }
        for (int64_t i = i0[u]; i < n && i < i0[u] + 4; ++i) {
            float bc1 = bc1_all, bc2 = bc2_all;
            if (i == alpha_idx) {
                // smoothing_alpha is outside the autograd graph whenever the EMA passes its input through: no decay, no moment
                // update, its own step counter
                if (!alpha_live) continue;
                const int t = steps[1];
                bc1 = bias_correction(b1, t); bc2 = bias_correction(b2, t);
            }
            float pi = p[i], mi = m[i], vi = v[i];
            update(pi, mi, vi, g[i], bc1, bc2);
            p[i] = pi; m[i] = mi; v[i] = vi;
            pc.put(i, pi);
        }
    }
}

// dst (rows x kp) <- src (rows x kt), columns kt .. kp zero: the padded copy from scratch (parameter upload)
__global__ __launch_bounds__(256) void pad_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows, int kt, int kp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * kp) return;
    const int64_t r = i / kp; const int t = (int)(i - r * kp);
    dst[i] = t < kt ? src[r * kt + t] : 0.f;
}

// ---- host side --------------------------------------------------------------------------------------------------------------

int train_adamw(Context* c, const float* flat_grad, float lr, float b1, float b2, float eps, float wd, float max_norm,
                int64_t step, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = c->tr.nparams;
    const int nb = 256;
    // two launches: partial sums of squares (+ the step counters), then norm + clip + AdamW in one kernel
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, st, flat_grad, n, c->tr.part, c->tr.steps, c->tr_alpha_live ? 1 : 0);
    (void)step;
    // the legacy model (km_legacy_train_*) has neither a smoothing_alpha nor a padded channel-encoder copy
    const auto alpha_it = c->tr.offset.find("smoothing_alpha");
    const int64_t alpha_idx = alpha_it == c->tr.offset.end() ? -1 : alpha_it->second;
    const PaddedCopy pc = c->tr.wcep ? PaddedCopy{c->tr.wcep, c->tr.offset.at("mel_channel_encoder.weight"), (int64_t)c->d * c->KT, (int)c->KT, (int)trainp_kp(c)}
                                      : PaddedCopy{nullptr, 0, 0, 1, 1};
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, st, c->tr.params, c->tr.m, c->tr.v, flat_grad, n,
                       c->tr.part, c->tr.gnorm, max_norm, lr, b1, b2, eps, wd, c->tr.steps, alpha_idx, c->tr_alpha_live ? 1 : 0, pc);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

// after the master parameters were written from outside (km_train_init, km_train_set_params): the padded copy from scratch
int train_refresh_padded_weights(Context* c, void* stream) {
    if (!c->tr.wcep) return KM_OK;
    const int64_t KP = trainp_kp(c);
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((c->d * KP + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       c->tr.params + c->tr.offset.at("mel_channel_encoder.weight"), c->tr.wcep, (int64_t)c->d, (int)c->KT, (int)KP);
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km
