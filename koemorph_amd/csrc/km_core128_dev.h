// Device code behind the encoder of the one-launch d_model 128 core (core128_kernel, km_core128.hip): scores, softmax, value
// projection, P V, the decoder fold and the tail for one window per 256-thread workgroup -- the counterpart of scores_softmax_body +
// attn_out_vr32_body (km_attn_dev.h, km_attn256_dev.h) for 4 heads of 32 columns and four waves.  Kernels only, as km_attn_dev.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_attn_dev.h"

namespace km {

// ---------------------------------------------------------------------------------------------------------
// attn128_body: d_model 128, 4 heads, 80 keys, decoder hidden 64 (= d_model / 2), 4 waves, one per SIMD.  At this width Y_b (80 x 128,
// 40 KB) fits in LDS whole, so it is staged ONCE, as [k / 4][row, padded to 81][k % 4] with the rows unpermuted, and one sweep over its
// 8 k blocks feeds both products that read it -- a fragment of Y rows 16 i .. 16 i + 15 is the B operand of the scores (keys) and the A
// operand of the value projection (rows), the same four registers:
//   1. scores: wave w owns row tiles 2 w and 2 w + 1 of the 7 (112 stacked rows; wave 3 owns tile 6 alone), A = qk_pg;
//      V[:, 32 w ..] (80 x 32, head w, two column tiles) = Y Wv^T, B = wv_bg128 [k block][wave][column tile < 2][lane][4] (km_host.cpp).
//      Both operand images of all 8 k blocks are requested before Y is staged.  80 MFMAs per k block and wave (60 on wave 3).
//   2. softmax over a row's 80 keys: 5 tiles in one wave, in-lane + DPP over the 16 key lanes; the weights of all heads go to the
//      workspace, H x 28 x 80 per window (what stream_head_mean_kernel averages), and come back after a barrier as the A fragments of
//   3. O_w = P_w V_w with the accumulators of step 1 as the B operand (the C/D layout of the 16 x 16 x 4 MFMA is its own B layout when
//      the contraction runs over the row index, the key).
//   4. O -> LDS [32 q][128 + 8], hidden^T = Wf^T O^T with wf_pg128 ([wave][k block][lane][4], one row tile of 16 units per wave,
//      requested before the barrier of step 2), ReLU . w2, cross-wave sum in wave order, sigmoid, stream weights, clamp; STREAM: the
//      per-stream EMA of attn_out_vr_body<..., true>.
// LDS: Ys = kCore128Lds bytes (the kernel's dynamic LDS); Os (32 x 136 floats) and R2 (4 x 32) reuse what the encoder stage is done
// with (EncLds<4>::As, ::Ps).  Every reduction has a fixed order; no atomics.
// ---------------------------------------------------------------------------------------------------------
constexpr int kCore128YsFloats = (128 / 4) * (80 + 1) * 4;
constexpr int kCore128Lds = kCore128YsFloats * (int)sizeof(float);
constexpr int kCore128OsFloats = 32 * (128 + 8);

// window b of the launch
template <bool STREAM = false>
__device__ __forceinline__ void attn128_body(const float* __restrict__ Y, const float* __restrict__ qk_pg, float* __restrict__ S,
                                             const float* __restrict__ wv_bg128, const float* __restrict__ wf_pg128,
                                             const float* __restrict__ bf, const float* __restrict__ w2, const float* __restrict__ b2,
                                             const float* __restrict__ zemo, const float* __restrict__ wsum, float* __restrict__ out,
                                             float* __restrict__ raw, int b, float* Ys, float* Os, float* R2,
                                             const StreamSrc& ss = StreamSrc{}) {
    constexpr int D = 128, NKc = 80, KB = D / 16, QS = NKc + 1, OS = D + 8, NWv = 4, H = NWv, CTW = 2, ROWS = H * 28, MT = ROWS / 16;
    static_assert(D == 32 * NWv && ROWS == 16 * MT, "one wave per head of 32 columns; the stacked rows are whole tiles");
    static_assert((D / 4) * QS * 4 == kCore128YsFloats && 32 * OS == kCore128OsFloats, "LDS images");
    static_assert(NKc * (D / 4) == 10 * 256, "Y_b is ten 16-byte vectors per thread");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lg = lane >> 4, lj = lane & 15;
    const float* Yb = Y + (int64_t)b * NKc * D;
    float* Sb = S + (int64_t)b * ROWS * NKc;
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Yb), 0, (unsigned)(NKc * D * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t ar = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(qk_pg), 0, (unsigned)(MT * KB * 1024), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wv_bg128), 0, (unsigned)(D * D * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(Sb, 0, (unsigned)(ROWS * NKc * 4), 0x00020000);
    constexpr unsigned OOB = 0x7fffffffu;
    // ---- operand images of the whole sweep: qk_pg is [k block][row tile][lane][4], wv_bg128 [k block][wave][column tile][lane][4] ----
    const int mt0 = 2 * wave, cnt = wave < 3 ? 2 : 1;                       // this wave's row tiles (wave-uniform)
    f32x4 av[KB][2], bw[KB][CTW];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
            av[kb][t] = as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(ar, t < cnt ? (unsigned)(((kb * MT + mt0 + t) * 64 + lane) * 16) : OOB, 0, 0));
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct)
            bw[kb][ct] = as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)((((kb * NWv + wave) * CTW + ct) * 64 + lane) * 16), 0, 0));
    }
    // ---- Y_b -> LDS, once ----
    {
        u32x4 yst[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const int idx = tid + 256 * j, row = idx >> 5, q = idx & 31;
            yst[j] = __builtin_amdgcn_raw_buffer_load_b128(yr, (unsigned)((row * D + 4 * q) * 4), 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const int idx = tid + 256 * j, row = idx >> 5, q = idx & 31;
            *reinterpret_cast<u32x4*>(&Ys[(q * QS + row) * 4]) = yst[j];
        }
    }
    __syncthreads();
    // ---- one sweep: scores (this wave's row tiles x 80 keys) and V[:, 32 w ..] ----
    f32x4 sc[2][5], v[5][CTW];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sc[0][i] = f32x4{0, 0, 0, 0}; sc[1][i] = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) v[i][ct] = f32x4{0, 0, 0, 0};
    }
    f32x4 yb[2][5];
    auto ldy = [&](int kb, int slot) {
#pragma unroll
        for (int i = 0; i < 5; ++i) yb[slot][i] = *reinterpret_cast<const f32x4*>(&Ys[((4 * kb + lg) * QS + 16 * i + lj) * 4]);
    };
    ldy(0, 0);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        const int cur = kb & 1;
        if (kb + 1 < KB) ldy(kb + 1, cur ^ 1);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                sc[0][i] = KM_MFMA(av[kb][0][s], yb[cur][i][s], sc[0][i]);
                if (cnt > 1) sc[1][i] = KM_MFMA(av[kb][1][s], yb[cur][i][s], sc[1][i]);      // wave-uniform
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) v[i][ct] = KM_MFMA(yb[cur][i][s], bw[kb][ct][s], v[i][ct]);
            }
    }
    // ---- softmax: row 4 lg + r of a tile sits in lanes lj = 0..15 x 5 accumulators, key 16 i + lj ----
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (t >= cnt) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = sc[t][0][r];
#pragma unroll
            for (int i = 1; i < 5; ++i) m = fmaxf(m, sc[t][i][r]);
            m = row16_max(m);
            float e[5], sum = 0.f;
#pragma unroll
            for (int i = 0; i < 5; ++i) { e[i] = __builtin_amdgcn_exp2f((sc[t][i][r] - m) * 1.44269504088896341f); sum += e[i]; }
            sum = row16_sum(sum);
            const float inv = 1.0f / sum;
            float* dst = Sb + (16 * (mt0 + t) + 4 * lg + r) * NKc + lj;
#pragma unroll
            for (int i = 0; i < 5; ++i) dst[16 * i] = e[i] * inv;
        }
    }
    // the fold weights are requested before the barrier that publishes the attention weights
    const f32x4* fp = reinterpret_cast<const f32x4*>(wf_pg128) + (size_t)wave * KB * 64 + lane;
    f32x4 wq[KB];
#pragma unroll
    for (int j = 0; j < KB; ++j) wq[j] = fp[(size_t)j * 64];
    __syncthreads();
    // ---- O[:, 32 w ..] = P_w V_w: A = ap[mt][i] = P_w[q = 16 mt + lj][keys 16 i + 4 lg .. + 3], B = the accumulators of the sweep ----
    {
        f32x4 ap[2][5];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int q = 16 * mt + lj;
#pragma unroll
            for (int i = 0; i < 5; ++i)
                ap[mt][i] = as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(pr, q < 28 ? (unsigned)(((wave * 28 + q) * NKc + 16 * i + 4 * lg) * 4) : OOB, 0, 0));
        }
        f32x4 o[2][CTW];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) o[mt][ct] = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) {
                    o[0][ct] = KM_MFMA(ap[0][i][s], v[i][ct][s], o[0][ct]);
                    o[1][ct] = KM_MFMA(ap[1][i][s], v[i][ct][s], o[1][ct]);
                }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) Os[(16 * mt + 4 * lg + r) * OS + 32 * wave + 16 * ct + lj] = o[mt][ct][r];
    }
    __syncthreads();
    // ---- hidden^T (64 x 32 q) = Wf^T O^T; wave w owns hidden units 16 w .. 16 w + 15 ----
    f32x4 Z[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        const f32x4 o0 = *reinterpret_cast<const f32x4*>(Os + lj * OS + 16 * kb + 4 * lg);
        const f32x4 o1 = *reinterpret_cast<const f32x4*>(Os + (16 + lj) * OS + 16 * kb + 4 * lg);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            Z[0] = KM_MFMA(wq[kb][s], o0[s], Z[0]);
            Z[1] = KM_MFMA(wq[kb][s], o1[s], Z[1]);
        }
    }
    {
        float zp[2] = {0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int hid = 16 * wave + 4 * lg + r;
            const float bfv = bf[hid], w2v = w2[hid];
            zp[0] += fmaxf(Z[0][r] + bfv, 0.f) * w2v;
            zp[1] += fmaxf(Z[1][r] + bfv, 0.f) * w2v;
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            zp[qt] += __shfl_xor(zp[qt], 16);
            zp[qt] += __shfl_xor(zp[qt], 32);
        }
        if (lg == 0) { R2[wave * 32 + lj] = zp[0]; R2[wave * 32 + 16 + lj] = zp[1]; }
    }
    __syncthreads();
    if (tid < 52) {
        const int slot = gen_mouth_slot(tid);
        float z;
        if (slot >= 0) {
            z = b2[0];
#pragma unroll
            for (int w = 0; w < NWv; ++w) z += R2[w * 32 + slot];
        } else {
            z = zemo[b];
        }
        const float bs = 1.0f / (1.0f + expf(-z));
        if (raw) raw[(int64_t)b * 52 + tid] = bs;
        float val = fminf(fmaxf(wsum[tid] * bs, 0.f), 1.f);
        if constexpr (STREAM) {                                         // EMA (simplified_dual_stream_model.py:357-366)
            float* st = ss.state + (int64_t)b * 52 + tid;
            if (ss.started[b]) val = ss.alpha * val + (1.0f - ss.alpha) * (*st);
            *st = val;
        }
        out[(int64_t)b * 52 + tid] = val;
    }
    if constexpr (STREAM) {
        __syncthreads();                                                // the 52 threads above have read started[b]
        if (tid == 0) ss.started[b] = 1;
    }
}

}  // namespace km
