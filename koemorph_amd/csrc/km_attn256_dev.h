// Device code of the last stage of the one-launch d_model 256 core (core256w_kernel, km_generic.hip): value projection, P V,
// the decoder fold and the tail for one window per workgroup -- the counterpart of attn_out_vr_body (km_attn_dev.h) for
// 8 heads of 32 columns.  Kernels only, as km_attn_dev.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "km_attn_dev.h"

namespace km {

// ---------------------------------------------------------------------------------------------------------
// attn_out_vr32_body: d_model 256, 8 heads, 80 keys, decoder hidden 128 (= d_model / 2), 8 waves.  Wave w owns value columns
// 32 w .. 32 w + 31, which is exactly head w (two column tiles), and hidden units 16 w .. 16 w + 15:
//   1. V[:, 32 w ..] (80 x 32, 10 accumulators) = Y Wv^T: A = Y through LDS in chunks of 64 k (the image of
//      scores_softmax_body, unpermuted rows), fragments read one k block ahead; B = wv_bg32, the MFMA operand image
//      [k block][wave][column tile < 2][lane][4] (km_host.cpp), one coalesced KiB per wave and tile, one k block ahead.
//   2. O_w = P_w V_w with the accumulators of step 1 as the B operand (the C/D layout of the 16 x 16 x 4 MFMA is its own B
//      layout when the contraction runs over the row index, the key); A = the softmaxed scores of head w, requested
//      before step 1.
//   3. O -> LDS [32 q][256 + 8], hidden^T = Wf^T O^T with wf_pg (one row tile of 16 units per wave, 16 k blocks in two groups
//      of eight requested a group ahead), ReLU . w2, cross-wave sum in wave order, sigmoid, stream weights, clamp;
//      STREAM: the per-stream EMA of attn_out_vr_body<..., true>.
// 848 MFMAs per wave (640 + 80 + 128).  Dynamic LDS: kCore256wLds bytes.
// ---------------------------------------------------------------------------------------------------------
constexpr int kCore256wLds = (2 * 16 * 81 * 4 + 32 * (256 + 8) + 8 * 32) * (int)sizeof(float);

// window b of the launch; gsm: the workgroup's dynamic LDS
template <bool STREAM = false>
__device__ __forceinline__ void attn_out_vr32_body(const float* __restrict__ S, const float* __restrict__ Y,
                                                   const float* __restrict__ wv_bg32, const float* __restrict__ wf_pg,
                                                   const float* __restrict__ bf, const float* __restrict__ w2,
                                                   const float* __restrict__ b2, const float* __restrict__ zemo,
                                                   const float* __restrict__ wsum, float* __restrict__ out,
                                                   float* __restrict__ raw, int b, float* gsm, const StreamSrc& ss = StreamSrc{}) {
    constexpr int D = 256, NKc = 80, KB = D / 16, CH = 4, NCH = KB / CH, QS = NKc + 1, OS = D + 8, NWv = 8, H = NWv, CTW = 2;
    static_assert(D == 32 * NWv && KB % CH == 0, "one wave per head of 32 columns; k blocks in chunks of four");
    static_assert((2 * 16 * QS * 4 + 32 * OS + NWv * 32) * (int)sizeof(float) == kCore256wLds, "LDS image");
    float* Ys = gsm;                                           // [2][16 * QS * 4]  Y chunk image [k / 4][row, padded][k % 4]
    float* Os = Ys + 2 * 16 * QS * 4;                          // [32][OS]
    float* R2 = Os + 32 * OS;                                  // [NWv][32]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lg = lane >> 4, lj = lane & 15;
    const float* Yb = Y + (int64_t)b * NKc * D;
    const float* Pb = S + (int64_t)b * H * 28 * NKc;
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Yb), 0, (unsigned)(NKc * D * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wv_bg32), 0, (unsigned)(D * D * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Pb), 0, (unsigned)(H * 28 * NKc * 4), 0x00020000);
    constexpr unsigned OOB = 0x7fffffffu;
    u32x4 yst[3];
    auto ystage = [&](int ch) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int idx = tid + 512 * j, row = idx >> 4, q = idx & 15;
            yst[j] = __builtin_amdgcn_raw_buffer_load_b128(yr, idx < NKc * 16 ? (unsigned)((row * D + 64 * ch + 4 * q) * 4) : OOB, 0, 0);
        }
    };
    auto ycommit = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int idx = tid + 512 * j, row = idx >> 4, q = idx & 15;
            asm volatile("" ::"v"(yst[j]));     // unconditional use: the load stays out of the branch
            if (idx < NKc * 16) *reinterpret_cast<u32x4*>(&Ys[buf * (16 * QS * 4) + (q * QS + row) * 4]) = yst[j];
        }
    };
    // the attention weights of this wave's head as A fragments: ap[mt][i] = P_w[q = 16 mt + lj][keys 16 i + 4 lg .. + 3]
    f32x4 ap[2][5];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int q = 16 * mt + lj;
#pragma unroll
        for (int i = 0; i < 5; ++i)
            ap[mt][i] = as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(pr, q < 28 ? (unsigned)(((wave * 28 + q) * NKc + 16 * i + 4 * lg) * 4) : OOB, 0, 0));
    }
    f32x4 acc[5][CTW];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) acc[i][ct] = f32x4{0, 0, 0, 0};
    f32x4 ay[2][5], bw[2][CTW];
    const unsigned wo = (unsigned)((wave * CTW * 64 + lane) * 16);
    auto ldw = [&](int kb, int slot) {
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct)
            bw[slot][ct] = as_f32x4(__builtin_amdgcn_raw_buffer_load_b128(wr, kb < KB ? wo + (unsigned)(kb * NWv * CTW + ct) * 1024u : OOB, 0, 0));
    };
    auto ldy = [&](int buf, int kk, int slot) {
#pragma unroll
        for (int i = 0; i < 5; ++i)
            ay[slot][i] = *reinterpret_cast<const f32x4*>(&Ys[buf * (16 * QS * 4) + ((4 * kk + lg) * QS + 16 * i + lj) * 4]);
    };
    ystage(0);
    ldw(0, 0);
    ycommit(0);
    __syncthreads();
    ldy(0, 0, 0);
    for (int ch = 0; ch < NCH; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < NCH;
        if (more) ystage(ch + 1);
#pragma unroll
        for (int kk = 0; kk < CH; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            ldw(CH * ch + kk + 1, nxt);
            if (kk + 1 < CH) ldy(buf, kk + 1, nxt);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < 5; ++i)
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct) acc[i][ct] = KM_MFMA(ay[cur][i][s], bw[cur][ct][s], acc[i][ct]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) ycommit(buf ^ 1);
        __syncthreads();
        if (more) ldy(buf ^ 1, 0, 0);
    }
    // ---- O[:, 32 w ..] = P_w V_w: B operand = the accumulators ----
    {
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
                    o[0][ct] = KM_MFMA(ap[0][i][s], acc[i][ct][s], o[0][ct]);
                    o[1][ct] = KM_MFMA(ap[1][i][s], acc[i][ct][s], o[1][ct]);
                }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) Os[(16 * mt + 4 * lg + r) * OS + 32 * wave + 16 * ct + lj] = o[mt][ct][r];
    }
    // the first group of fold weights is requested before the barrier that publishes O.  wf_pg is [hidden / 32][row tile < 2][k block]
    // [lane][4] (km_host.cpp): the 16 hidden units of wave w are row tile w & 1 of group w >> 1, i.e. image w of KB KiB
    const f32x4* fp = reinterpret_cast<const f32x4*>(wf_pg) + (size_t)wave * KB * 64 + lane;
    constexpr int FS = 8;
    static_assert(KB % FS == 0, "fold k blocks come in groups of eight");
    f32x4 wq[2][FS];
#pragma unroll
    for (int j = 0; j < FS; ++j) wq[0][j] = fp[(size_t)j * 64];
    __syncthreads();
    // ---- hidden^T (128 x 32 q) = Wf^T O^T; wave w owns hidden units 16 w .. 16 w + 15 ----
    f32x4 Z[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
#pragma unroll
    for (int st = 0; st < KB / FS; ++st) {
        const int cur = st & 1, nxt = cur ^ 1;
        if (st + 1 < KB / FS) {
#pragma unroll
            for (int j = 0; j < FS; ++j) wq[nxt][j] = fp[(size_t)(FS * (st + 1) + j) * 64];
        }
#pragma unroll
        for (int j = 0; j < FS; ++j) {
            const int kb = FS * st + j;
            const f32x4 o0 = *reinterpret_cast<const f32x4*>(Os + lj * OS + 16 * kb + 4 * lg);
            const f32x4 o1 = *reinterpret_cast<const f32x4*>(Os + (16 + lj) * OS + 16 * kb + 4 * lg);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                Z[0] = KM_MFMA(wq[cur][j][s], o0[s], Z[0]);
                Z[1] = KM_MFMA(wq[cur][j][s], o1[s], Z[1]);
            }
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
