// Training step of the legacy SimplifiedKoeMorphModel for gfx950 (km_legacy_train_*): forward in training mode, the
// KoeMorphLoss terms and the backward pass, into ONE flat gradient in state-dict order.
//
// Replaces the body of the reference trainer's loop (src/train.py:165-249: model(audio), criterion, loss.backward()) for the 15
// tensors of src/model/simplified_model.py:44-76.  Default width only (d_model 256, 8 heads, decoder hidden 128, 52 queries,
// 80 mel bins; any number of frames T).  R = B T frame rows, R2 = B 52 query rows.
//
//   forward   masks (Philox, one launch)                                   mask_gen_kernel
//             E1 = drop(relu(mel W0^T + b0)), E2 = drop(relu(E1 W3^T + b3)) launch_gemm + drop_rows_kernel
//             KV = E2 Wkv^T + bkv   (R, 512): keys | values                 launch_gemm
//             Q  = queries Wq^T + bq (52, 256), once per step                launch_gemm
//             O  = drop(softmax(Q K^T / sqrt 32)) V, one wave per (b, h)     ltr_attn_fwd_kernel (saves row maximum and 1 / row sum)
//             A1 = O Wo^T + bo, D1, D2 (dropout), Z3                         launch_gemm + drop_rows_kernel
//             y = sigmoid(Z3), out = mean over the 52 rows, loss, dZ3        ltr_loss_kernel
//   backward  per linear layer: dW = dY^T X as split-K partials + a fixed-order sum, db = column sums the same way,
//             dX = dY W, ReLU / dropout through the sign of the stored (post-mask) activation
//             attention: S and P recomputed per (b, h) from Q, K and the saved row statistics  ltr_attn_bwd_kernel
//             dQ = sum over the windows of the per-window parts, in window order
// No floating-point atomics: every sum has a fixed order, so two runs of a step give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "km_context.h"
#include "km_device.h"
#include "km_gemm.h"

namespace km {


#include "km_philox.h"
#include "km_train_tail.h"

#ifndef KM_MFMA
#define KM_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#endif

namespace ltr {
constexpr int D = 256, H = 8, HD = 32, NQ = 52, HID = 128, NK = 80;
constexpr int MAX_PARTS = 17;           // split-K: up to 16 whole chunks of rows + a remainder
typedef float f32x4 __attribute__((ext_vector_type(4)));
}

// ---- dropout masks -------------------------------------------------------------------------------------------------------------
// keep flags (1 = kept) with probability 1 - p: counter = (byte index / 4, 0, step), key = seed -- the generator of the
// dual-stream step (km_trainp.hip OP_MASKGEN), over the five sites of the model as one run of bytes
__global__ __launch_bounds__(256) void ltr_mask_gen_kernel(unsigned char* __restrict__ mask, int64_t n, const int* __restrict__ step_p,
                                                           unsigned k0, unsigned k1, unsigned thr) {
    const int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i4 * 4 >= n) return;
    unsigned r[4];
    philox4x32_10((unsigned)i4, (unsigned)(i4 >> 32), 0u, (unsigned)step_p[0], k0, k1, r);
    unsigned char k4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) k4[k] = r[k] >= thr ? 1 : 0;
    if (i4 * 4 + 3 < n) *reinterpret_cast<uchar4*>(mask + i4 * 4) = make_uchar4(k4[0], k4[1], k4[2], k4[3]);
    else for (int k = 0; i4 * 4 + k < n; ++k) mask[i4 * 4 + k] = k4[k];
}

// x[i] = keep[i] ? x[i] * scale : 0   (nn.Dropout behind a ReLU; n a multiple of 4)
__global__ __launch_bounds__(256) void ltr_drop_rows_kernel(float* __restrict__ x, const unsigned char* __restrict__ keep, int64_t n, float scale) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    float4 v = *reinterpret_cast<float4*>(x + i);
    const uchar4 k = *reinterpret_cast<const uchar4*>(keep + i);
    v.x = k.x ? v.x * scale : 0.f; v.y = k.y ? v.y * scale : 0.f; v.z = k.z ? v.z * scale : 0.f; v.w = k.w ? v.w * scale : 0.f;
    *reinterpret_cast<float4*>(x + i) = v;
}

// g[i] = y[i] > 0 ? g[i] * scale : 0: backward of Dropout(ReLU(.)) from the stored post-mask activation y (y > 0 <=> active and kept)
__global__ __launch_bounds__(256) void ltr_relu_bwd_kernel(float* __restrict__ g, const float* __restrict__ y, int64_t n, float scale) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    float4 v = *reinterpret_cast<float4*>(g + i);
    const float4 a = *reinterpret_cast<const float4*>(y + i);
    v.x = a.x > 0.f ? v.x * scale : 0.f; v.y = a.y > 0.f ? v.y * scale : 0.f; v.z = a.z > 0.f ? v.z * scale : 0.f; v.w = a.w > 0.f ? v.w * scale : 0.f;
    *reinterpret_cast<float4*>(g + i) = v;
}

// ---- fixed-order reductions ----------------------------------------------------------------------------------------------------
// out[i] = part[i] + part[n + i] + ... (count terms, in index order)
__global__ __launch_bounds__(256) void ltr_sum_parts_kernel(const float* __restrict__ part, int64_t n, int count, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    int y = 0;
    for (; y + 8 <= count; y += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = part[(int64_t)(y + u) * n + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; y < count; ++y) s += part[(int64_t)y * n + i];
    out[i] = s;
}

// column sums of rows [chunk z, chunk (z + 1)) of x (rows, n; row stride ld) -> part[z][n]: thread (rg, c) adds rows rg, rg + 4, ...
// of column c in order, the four row groups are added in index order
__global__ __launch_bounds__(256) void ltr_colsum_kernel(const float* __restrict__ x, int64_t rows, int n, int64_t ld, int64_t chunk,
                                                         float* __restrict__ part) {
    __shared__ float sh[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    float s = 0.f;
    if (c < n)
        for (int64_t r = r0 + rg; r < r1; r += 4) s += x[r * ld + c];
    sh[rg][threadIdx.x & 63] = s;
    __syncthreads();
    if (rg == 0 && c < n) part[(int64_t)blockIdx.y * n + c] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// ---- attention -----------------------------------------------------------------------------------------------------------------
// Forward: legacy_attention_body (km_legacy_attn_dev.h) in training mode.  One WAVE per (window, head), hd = 32, nothing in LDS.
// Differences: Q is this step's projection (unscaled: log2 e / sqrt 32 goes in at the load), the keep mask of the attention
// dropout multiplies the exponentials that go INTO the P V product while the row sum stays that of the unmasked softmax (the
// mask acts on the softmaxed weights, as nn.MultiheadAttention applies it), and the row maximum (base-2 domain) and 1 / row sum
// are saved for the backward pass, which recomputes P from them.
// mfma_f32_16x16x4f32(a, b, c) in step s: lane (g, j) gives a = A[row j][k 4 g + s], b = B[k 4 g + s][col j]; c[r] = C[row 4 g + r][col j].
__global__ __launch_bounds__(64) void ltr_attn_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ KV, float* __restrict__ O,
                                                          float* __restrict__ stat_m, float* __restrict__ stat_il,
                                                          const unsigned char* __restrict__ keep, float keep_scale, int Tm) {
    using namespace ltr;
    const int64_t bh = blockIdx.x;
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int64_t b = bh / H;
    const int h = (int)(bh - b * H);
    const float qscale = 1.4426950408889634f * 0.17677669529663687f;       // log2 e / sqrt 32
    float qT[2][4][4];                          // [dim tile][query tile][s]: Q[16 qt + j][16 dt + 4 g + s]
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            const int q = 16 * qt + j;
            const float4 v = q < NQ ? *reinterpret_cast<const float4*>(Q + (int64_t)q * D + HD * h + 16 * dt + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
            qT[dt][qt][0] = v.x * qscale; qT[dt][qt][1] = v.y * qscale; qT[dt][qt][2] = v.z * qscale; qT[dt][qt][3] = v.w * qscale;
        }
    f32x4 oT[2][4];
    float m[4], l[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        m[qt] = -INFINITY; l[qt] = 0.f;
        oT[0][qt] = f32x4{0, 0, 0, 0}; oT[1][qt] = f32x4{0, 0, 0, 0};
    }
    const float* Kb = KV + (b * Tm) * (int64_t)(2 * D) + HD * h;
    const float* Vb = Kb + D;
    const int nkt = (Tm + 15) / 16;
    for (int kt = 0; kt < nkt; ++kt) {
        float4 ka[2];
        float va[2][4];
        {
            const int kr = 16 * kt + j < Tm ? 16 * kt + j : Tm - 1;          // keys past Tm: the last row again, masked below
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) ka[dt] = *reinterpret_cast<const float4*>(Kb + (int64_t)kr * (2 * D) + 16 * dt + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kt + 4 * g + r < Tm ? 16 * kt + 4 * g + r : Tm - 1;
                va[0][r] = Vb[(int64_t)key * (2 * D) + j];
                va[1][r] = Vb[(int64_t)key * (2 * D) + 16 + j];
            }
        }
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            f32x4 S = f32x4{0, 0, 0, 0};                                     // S^T[key 4 g + r][query j], base-2 domain
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const float kv[4] = {ka[dt].x, ka[dt].y, ka[dt].z, ka[dt].w};
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) S = KM_MFMA(kv[s_], qT[dt][qt][s_], S);
            }
            float tm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (16 * kt + 4 * g + r >= Tm) S[r] = -INFINITY;
                tm = fmaxf(tm, S[r]);
            }
            tm = fmaxf(tm, __shfl_xor(tm, 16));
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const float mn = fmaxf(m[qt], tm);
            const float alpha = mn == -INFINITY ? 1.0f : __builtin_amdgcn_exp2f(m[qt] - mn);
            float ps = 0.f;
            const int q = 16 * qt + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float e = mn == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(S[r] - mn);
                ps += e;
                const int key = 16 * kt + 4 * g + r;
                if (keep && q < NQ && key < Tm) e = keep[((int64_t)bh * NQ + q) * Tm + key] ? e * keep_scale : 0.f;
                S[r] = e;
            }
            l[qt] = l[qt] * alpha + ps;
            m[qt] = mn;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                f32x4 o = oT[dt][qt];
                o[0] *= alpha; o[1] *= alpha; o[2] *= alpha; o[3] *= alpha;
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) o = KM_MFMA(va[dt][s_], S[s_], o);      // O^T[dim][query]
                oT[dt][qt] = o;
            }
        }
    }
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        float ls = l[qt];
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        const float inv = 1.0f / ls;
        const int q = 16 * qt + j;
        if (q < NQ) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const f32x4 o = oT[dt][qt];
                *reinterpret_cast<float4*>(O + (b * NQ + q) * (int64_t)D + HD * h + 16 * dt + 4 * g) =
                    make_float4(o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv);
            }
            if (g == 0) { stat_m[bh * NQ + q] = m[qt]; stat_il[bh * NQ + q] = inv; }
        }
    }
}

// Backward: one WAVE per (window, head).  Per tile of 16 keys the scores are recomputed in BOTH orientations of the MFMA C layout,
// because a C-layout tile can only be contracted over its rows:
//   rows = keys    S^T, dPd^T = V dO^T -> dS^T -> dQ^T += K^T dS^T                         (contracts over the keys)
//   rows = queries S, dPd = dO V^T -> Pd, dS -> dV^T = dO^T Pd, dK^T = Q^T dS / sqrt 32    (contracts over the queries)
// with P = 2^(S - m) / l from the saved statistics, dP = dPd keep / (1 - p), dS = P (dP - D), D[q] = sum_t dP P = dO[q] . O[q]
// (O = Pd V).  dK | dV go to dKV (R, 512); dQpart (B, 52, 256) holds this window's part of dQ (summed over the windows afterwards,
// in window order).
__global__ __launch_bounds__(64) void ltr_attn_bwd_kernel(const float* __restrict__ Q, const float* __restrict__ KV, const float* __restrict__ O,
                                                          const float* __restrict__ dO, const float* __restrict__ stat_m,
                                                          const float* __restrict__ stat_il, const unsigned char* __restrict__ keep,
                                                          float keep_scale, int Tm, float* __restrict__ dKV, float* __restrict__ dQpart) {
    using namespace ltr;
    const int64_t bh = blockIdx.x;
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int64_t b = bh / H;
    const int h = (int)(bh - b * H);
    const float rs32 = 0.17677669529663687f, qscale = 1.4426950408889634f * rs32;
    const float* Qh = Q + HD * h;
    const float* Oh = O + (b * NQ) * (int64_t)D + HD * h;
    const float* dOh = dO + (b * NQ) * (int64_t)D + HD * h;
    float qS[2][4][4], dOB[2][4][4];            // Q log2 e / sqrt 32 and dO at [16 qt + j][16 dt + 4 g + s]: B operand with rows = keys, A operand with rows = queries
    float qA[2][4][4], dOA[2][4][4];            // Q / sqrt 32 and dO at [16 qt + 4 g + s][16 dt + j]: A operands of dK^T and dV^T
    float m1[4], il1[4], D1[4];                 // statistics of query 16 qt + j
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const int q = 16 * qt + j;
        float dsum = 0.f;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f), w = v, o = v;
            if (q < NQ) {
                v = *reinterpret_cast<const float4*>(Qh + (int64_t)q * D + 16 * dt + 4 * g);
                w = *reinterpret_cast<const float4*>(dOh + (int64_t)q * D + 16 * dt + 4 * g);
                o = *reinterpret_cast<const float4*>(Oh + (int64_t)q * D + 16 * dt + 4 * g);
            }
            qS[dt][qt][0] = v.x * qscale; qS[dt][qt][1] = v.y * qscale; qS[dt][qt][2] = v.z * qscale; qS[dt][qt][3] = v.w * qscale;
            dOB[dt][qt][0] = w.x; dOB[dt][qt][1] = w.y; dOB[dt][qt][2] = w.z; dOB[dt][qt][3] = w.w;
            dsum += (w.x * o.x + w.y * o.y) + (w.z * o.z + w.w * o.w);
#pragma unroll
            for (int s_ = 0; s_ < 4; ++s_) {
                const int q2 = 16 * qt + 4 * g + s_;
                qA[dt][qt][s_] = q2 < NQ ? Qh[(int64_t)q2 * D + 16 * dt + j] * rs32 : 0.f;
                dOA[dt][qt][s_] = q2 < NQ ? dOh[(int64_t)q2 * D + 16 * dt + j] : 0.f;
            }
        }
        dsum += __shfl_xor(dsum, 16);
        dsum += __shfl_xor(dsum, 32);
        D1[qt] = dsum;
        m1[qt] = q < NQ ? stat_m[bh * NQ + q] : 0.f;
        il1[qt] = q < NQ ? stat_il[bh * NQ + q] : 0.f;
    }
    float m2[4][4], il2[4][4], D2[4][4];        // the same of query 16 qt + 4 g + r
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            m2[qt][r] = __shfl(m1[qt], 4 * g + r);
            il2[qt][r] = __shfl(il1[qt], 4 * g + r);
            D2[qt][r] = __shfl(D1[qt], 4 * g + r);
        }
    f32x4 dQT[2][4];                            // dQ^T[dim 16 dt + 4 g + r][query 16 qt + j]
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) { dQT[0][qt] = f32x4{0, 0, 0, 0}; dQT[1][qt] = f32x4{0, 0, 0, 0}; }
    const float* Kb = KV + (b * Tm) * (int64_t)(2 * D) + HD * h;
    const float* Vb = Kb + D;
    float* dKb = dKV + (b * Tm) * (int64_t)(2 * D) + HD * h;
    const unsigned char* kp = keep ? keep + (int64_t)bh * NQ * Tm : nullptr;
    const int nkt = (Tm + 15) / 16;
    for (int kt = 0; kt < nkt; ++kt) {
        float kr4[2][4], vr4[2][4], kc[2][4];   // K, V rows of key 16 kt + j at dims 16 dt + 4 g + s; K of key 16 kt + 4 g + s at dim 16 dt + j
        {
            const int kr = 16 * kt + j < Tm ? 16 * kt + j : Tm - 1;          // keys past Tm: the last row again; their P is zero below
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const float4 a = *reinterpret_cast<const float4*>(Kb + (int64_t)kr * (2 * D) + 16 * dt + 4 * g);
                const float4 v = *reinterpret_cast<const float4*>(Vb + (int64_t)kr * (2 * D) + 16 * dt + 4 * g);
                kr4[dt][0] = a.x; kr4[dt][1] = a.y; kr4[dt][2] = a.z; kr4[dt][3] = a.w;
                vr4[dt][0] = v.x; vr4[dt][1] = v.y; vr4[dt][2] = v.z; vr4[dt][3] = v.w;
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) {
                    const int key = 16 * kt + 4 * g + s_ < Tm ? 16 * kt + 4 * g + s_ : Tm - 1;
                    kc[dt][s_] = Kb[(int64_t)key * (2 * D) + 16 * dt + j];
                }
            }
        }
        // ---- rows = keys: dQ^T ----
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            f32x4 S = f32x4{0, 0, 0, 0}, dP = f32x4{0, 0, 0, 0};
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) {
                    S = KM_MFMA(kr4[dt][s_], qS[dt][qt][s_], S);             // S^T[key][query]
                    dP = KM_MFMA(vr4[dt][s_], dOB[dt][qt][s_], dP);          // dPd^T[key][query]
                }
            const int q = 16 * qt + j;
            f32x4 dS;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kt + 4 * g + r;
                const bool ok = key < Tm && q < NQ;
                const float p = ok ? __builtin_amdgcn_exp2f(S[r] - m1[qt]) * il1[qt] : 0.f;
                float ks = 1.f;
                if (kp && ok) ks = kp[(int64_t)q * Tm + key] ? keep_scale : 0.f;
                dS[r] = p * (dP[r] * ks - D1[qt]);
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) dQT[dt][qt] = KM_MFMA(kc[dt][s_], dS[s_], dQT[dt][qt]);      // A = K^T[dim j][key 4 g + s]
        }
        // ---- rows = queries: dV^T and dK^T of this key tile ----
        f32x4 dVT[2], dKT[2];
        dVT[0] = dVT[1] = dKT[0] = dKT[1] = f32x4{0, 0, 0, 0};
        const int keyc = 16 * kt + j;
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            f32x4 S = f32x4{0, 0, 0, 0}, dP = f32x4{0, 0, 0, 0};
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) {
                    S = KM_MFMA(qS[dt][qt][s_], kr4[dt][s_], S);             // S[query][key]
                    dP = KM_MFMA(dOB[dt][qt][s_], vr4[dt][s_], dP);          // dPd[query][key]
                }
            f32x4 Pd, dS;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * qt + 4 * g + r;
                const bool ok = keyc < Tm && q < NQ;
                const float p = ok ? __builtin_amdgcn_exp2f(S[r] - m2[qt][r]) * il2[qt][r] : 0.f;
                float ks = 1.f;
                if (kp && ok) ks = kp[(int64_t)q * Tm + keyc] ? keep_scale : 0.f;
                Pd[r] = p * ks;
                dS[r] = p * (dP[r] * ks - D2[qt][r]);
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) {
                    dVT[dt] = KM_MFMA(dOA[dt][qt][s_], Pd[s_], dVT[dt]);     // dV^T[dim j][key] += dO^T[dim][query 4 g + s] Pd[query][key]
                    dKT[dt] = KM_MFMA(qA[dt][qt][s_], dS[s_], dKT[dt]);
                }
        }
        if (keyc < Tm) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {                                  // C layout: dim 16 dt + 4 g + r, key 16 kt + j
                float* p = dKb + (int64_t)keyc * (2 * D) + 16 * dt + 4 * g;
                *reinterpret_cast<float4*>(p) = make_float4(dKT[dt][0], dKT[dt][1], dKT[dt][2], dKT[dt][3]);
                *reinterpret_cast<float4*>(p + D) = make_float4(dVT[dt][0], dVT[dt][1], dVT[dt][2], dVT[dt][3]);
            }
        }
    }
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
        const int q = 16 * qt + j;
        if (q < NQ) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const f32x4 v = dQT[dt][qt];
                *reinterpret_cast<float4*>(dQpart + (b * NQ + q) * (int64_t)D + HD * h + 16 * dt + 4 * g) =
                    make_float4(v[0] * rs32, v[1] * rs32, v[2] * rs32, v[3] * rs32);
            }
        }
    }
}

// ---- prediction, loss, dL/dZ3 ---------------------------------------------------------------------------------------------------
// One workgroup of four waves: wave w owns windows w, w + 4, ...; lane i < 52 owns coefficient i.  out[b][i] = mean over the 52
// query rows of sigmoid(Z3[b][q][i]) (simplified_model.py:144-147); then the terms of KoeMorphLoss by the dual-stream tail's own
// functions (km_train_tail.h: tail_coef_terms, tail_landmark_term); then dZ3[b][q][i] = dL/dout[b][i] / 52 * y (1 - y).
// Sums: per thread over its windows in order, a butterfly over the lanes, the waves in index order.

__global__ __launch_bounds__(256) void ltr_loss_kernel(const float* __restrict__ Z3, const float* __restrict__ target, int B, float mse_w,
                                                       float l1_w, km_loss_config lc, float* __restrict__ out, float* __restrict__ out2,
                                                       float* __restrict__ dZ3, float* __restrict__ loss, int* __restrict__ drop_ctr) {
    constexpr int NW = 4, NQ = ltr::NQ;
    __shared__ float red[NW], e_s[NW][52], u_s[NW][136];
    const int i = threadIdx.x & 63, w = threadIdx.x >> 6;
    auto sigm = [](float z) { return 1.0f / (1.0f + expf(-z)); };
    if (i < 52)
        for (int b = w; b < B; b += NW) {
            const float* z = Z3 + (int64_t)b * NQ * NQ + i;
            float s = 0.f;
            for (int q = 0; q < NQ; ++q) s += sigm(z[q * NQ]);
            const float y = s * (1.0f / 52.0f);
            out[(int64_t)b * 52 + i] = y;
            if (out2) out2[(int64_t)b * 52 + i] = y;
        }
    __threadfence_block();
    __syncthreads();
    const bool have_prev = lc.prev_pred_dev && lc.prev_target_dev;
    const bool t_on = lc.temporal_weight > 0.f && have_prev, v_on = lc.velocity_weight > 0.f && have_prev;
    const bool lm_on = lc.landmark_weight > 0.f && lc.landmark_w_dev;
    float loss_acc = 0.f;
    for (int b = w; b < B; b += NW) {
        float e = 0.f, dy = 0.f;
        if (i < 52) {
            const int64_t o = (int64_t)b * 52 + i;
            TailCoef tc{};
            tc.y = out[o]; tc.tgt = target[o];
            if (lc.smoothness_weight > 0.f) { tc.y_left = i > 0 ? out[o - 1] : 0.f; tc.y_right = i < 51 ? out[o + 1] : 0.f; }
            tc.t_on = t_on; tc.v_on = v_on;
            if (t_on || v_on) { tc.pp_t = lc.prev_pred_dev[o]; tc.pt_t = lc.prev_target_dev[o]; }
            dy = tail_coef_terms(lc, mse_w, l1_w, B, i, tc, e, loss_acc);
            e_s[w][i] = e;
        }
        if (lm_on) tail_landmark_term(lc, B, i, e_s[w], u_s[w], dy, loss_acc);
        if (i < 52) {
            const float dm = dy * (1.0f / 52.0f);
            const float* z = Z3 + (int64_t)b * NQ * NQ + i;
            float* dz = dZ3 + (int64_t)b * NQ * NQ + i;
            for (int q = 0; q < NQ; ++q) { const float s = sigm(z[q * NQ]); dz[q * NQ] = dm * s * (1.0f - s); }
        }
    }
    float t = i < 52 ? loss_acc : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (i == 0) red[w] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        loss[0] = ((red[0] + red[1]) + red[2]) + red[3];
        drop_ctr[0] += 1;                        // the next step draws fresh dropout masks
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

static GemmArgs lin(const float* A, int64_t a_rs, const float* W, int K, float* C, int64_t rows, int N, const float* bias, int relu) {
    GemmArgs g{};      // C (rows x N) = A (rows x K) W^T (+ bias) with W stored (N x K) like nn.Linear
    g.alpha = 1.f; g.batch2 = 1;
    g.A = A; g.a_rs = a_rs; g.a_cs = 1;
    g.B = W; g.b_rs = 1; g.b_cs = K;
    g.C = C; g.c_rs = N; g.M = (int)rows; g.N = N; g.K = K; g.bias = bias; g.bias_mode = bias ? 1 : 0; g.relu = relu;
    return g;
}

// dX (rows x K) = dY (rows x N) W, W stored (N x K)
static GemmArgs dgrad(const float* dY, const float* W, float* dX, int64_t rows, int N, int K) {
    GemmArgs g{};
    g.alpha = 1.f; g.batch2 = 1;
    g.A = dY; g.a_rs = N; g.a_cs = 1;
    g.B = W; g.b_rs = K; g.b_cs = 1;
    g.C = dX; g.c_rs = K; g.M = (int)rows; g.N = K; g.K = N;
    return g;
}

// rows of a product over the batch are cut into at most 16 whole chunks of `chunk` rows (a multiple of 32, at least 256) and a remainder
static void split_rows(int64_t rows, int64_t* chunk, int* whole, int64_t* rem) {
    int64_t c = ((rows + 15) / 16 + 31) / 32 * 32;
    if (c < 256) c = 256;
    *chunk = c; *whole = (int)(rows / c); *rem = rows - (int64_t)*whole * c;
}

// dW (N x K) = dY^T X over `rows` rows (dY: rows x N with row stride ldy; X: rows x K with row stride ldx): one partial product per
// chunk of rows, added in chunk order; db (N) = the column sums of dY the same way
static int wgrad(Context* c, const float* dY, int64_t ldy, int N, const float* X, int64_t ldx, int K, int64_t rows, float* dW, float* db,
                 void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int64_t chunk, rem; int whole;
    split_rows(rows, &chunk, &whole, &rem);
    const int parts = whole + (rem > 0 ? 1 : 0);
    const int64_t mn = (int64_t)N * K;
    float* part = parts > 1 ? c->tr.l_part : dW;
    GemmArgs g{};
    g.alpha = 1.f; g.batch2 = 1;
    g.a_rs = 1; g.a_cs = ldy; g.b_rs = ldx; g.b_cs = 1; g.c_rs = K; g.M = N; g.N = K;
    if (whole > 0) {
        g.A = dY; g.B = X; g.C = part; g.K = (int)chunk;
        g.a_bs1 = chunk * ldy; g.b_bs1 = chunk * ldx; g.c_bs1 = mn;
        if (int rc = launch_gemm(g, whole, stream)) return rc;
    }
    if (rem > 0) {
        g.A = dY + (int64_t)whole * chunk * ldy; g.B = X + (int64_t)whole * chunk * ldx; g.C = part + (int64_t)whole * mn; g.K = (int)rem;
        g.a_bs1 = g.b_bs1 = g.c_bs1 = 0;
        if (int rc = launch_gemm(g, 1, stream)) return rc;
    }
    if (parts > 1) hipLaunchKernelGGL(ltr_sum_parts_kernel, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, st, part, mn, parts, dW);
    if (db) {
        float* bpart = parts > 1 ? c->tr.l_part + (int64_t)ltr::MAX_PARTS * 512 * 256 : db;
        hipLaunchKernelGGL(ltr_colsum_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)parts), dim3(256), 0, st, dY, rows, N, ldy, chunk, bpart);
        if (parts > 1) hipLaunchKernelGGL(ltr_sum_parts_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, bpart, (int64_t)N, parts, db);
    }
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

bool legacy_train_supported(Context* c) {
    using namespace ltr;
    return c->kind == 1 && c->legacy_fused && c->legacy_tail_fused && c->d == D && c->H == H && c->hd == HD && c->NB == NQ &&
           c->NK == NK && c->legacy_hidden == HID;
}

// byte offsets of the five dropout sites for a (B, T) step: enc1 (B,T,d) | enc2 (B,T,d) | attn (B,H,52,T) | dec1 (B,52,hid) | dec2 (B,52,hid)
void legacy_train_mask_layout(int64_t B, int64_t T, int64_t off[6]) {
    using namespace ltr;
    off[0] = 0; off[1] = B * T * D; off[2] = 2 * B * T * D; off[3] = off[2] + B * H * NQ * T; off[4] = off[3] + B * NQ * HID; off[5] = off[4] + B * NQ * HID;
}

struct LtrWs {
    float *mel, *E1, *E2, *KV, *dKV, *dE2, *dE1, *Q, *dQ, *O, *A1, *dA1, *dO, *D1, *D2, *dD1, *dD2, *Z3, *dZ3, *dQpart, *out, *stat_m, *stat_il;
};

// the workspace is carved for (max_windows, max_frames): the offsets do not depend on the step's (B, T)
static int64_t carve(float* base, int64_t windows, int64_t frames, LtrWs* q) {
    using namespace ltr;
    const int64_t Rm = windows * frames, R2 = windows * NQ;
    int64_t off = 0;
    auto take = [&](float** p, int64_t n) { *p = base ? base + off : nullptr; off += (n + 3) / 4 * 4; };
    take(&q->mel, Rm * NK); take(&q->E1, Rm * D); take(&q->E2, Rm * D); take(&q->KV, Rm * 2 * D); take(&q->dKV, Rm * 2 * D);
    take(&q->dE2, Rm * D); take(&q->dE1, Rm * D); take(&q->Q, NQ * D); take(&q->dQ, NQ * D);
    take(&q->O, R2 * D); take(&q->A1, R2 * D); take(&q->dA1, R2 * D); take(&q->dO, R2 * D);
    take(&q->D1, R2 * HID); take(&q->D2, R2 * HID); take(&q->dD1, R2 * HID); take(&q->dD2, R2 * HID);
    take(&q->Z3, R2 * NQ); take(&q->dZ3, R2 * NQ); take(&q->dQpart, R2 * D); take(&q->out, windows * NQ);
    take(&q->stat_m, windows * H * NQ); take(&q->stat_il, windows * H * NQ);
    return off;
}

int legacy_train_init(Context* c, int64_t max_windows, int64_t max_frames, void* stream) {
    using namespace ltr;
    hipStream_t st = (hipStream_t)stream;
    c->tr.offset.clear();
    int64_t off = 0;
    for (const auto& k : c->param_order) {      // state-dict order, every offset a multiple of 4 floats (16 B)
        c->tr.offset[k] = off;
        off += ((int64_t)c->params.at(k).data.size() + 3) / 4 * 4;
    }
    c->tr.nparams = off; c->tr.early = off;
    const size_t nb = (size_t)off * sizeof(float);
    const char* what = "km_legacy_train_init";
    if (int rc = c->tr.params.alloc(off, what)) return rc;
    if (int rc = c->tr.m.alloc(off, what)) return rc;
    if (int rc = c->tr.v.alloc(off, what)) return rc;
    HIP_TRY(hipMemsetAsync(c->tr.m, 0, nb, st));
    HIP_TRY(hipMemsetAsync(c->tr.v, 0, nb, st));
    if (int rc = c->tr.part.alloc(256, what)) return rc;
    if (int rc = c->tr.gnorm.alloc(1, what)) return rc;
    if (int rc = c->tr.loss.alloc(1, what)) return rc;
    if (int rc = c->tr.steps.alloc(2, what)) return rc;
    HIP_TRY(hipMemsetAsync(c->tr.steps, 0, 2 * sizeof(int), st));
    if (int rc = c->tr.drop_ctr.alloc(1, what)) return rc;
    HIP_TRY(hipMemsetAsync(c->tr.drop_ctr, 0, sizeof(int), st));
    c->tr_dropout_p = 0.f; c->tr_dropout_mode = 0; c->tr_dropout_seed = 0; c->tr_loss_cfg = km_loss_config{};
    LtrWs tmp{};
    if (int rc = c->tr.l_ws.alloc(carve(nullptr, max_windows, max_frames, &tmp), what)) return rc;
    HIP_TRY(hipMemsetAsync(c->tr.l_ws, 0, (size_t)c->tr.l_ws.bytes(), st));
    if (int rc = c->tr.l_part.alloc((int64_t)MAX_PARTS * (512 * 256 + 512), what)) return rc;
    int64_t mo[6];
    legacy_train_mask_layout(max_windows, max_frames, mo);
    if (int rc = c->tr.l_masks.alloc(mo[5], what)) return rc;
    HIP_TRY(hipMemsetAsync(c->tr.l_masks, 1, (size_t)c->tr.l_masks.n, st));
    std::vector<float> flat((size_t)off, 0.f);
    for (const auto& k : c->param_order) {
        const HostParam& hp = c->params.at(k);
        std::memcpy(flat.data() + c->tr.offset.at(k), hp.data.data(), hp.data.size() * sizeof(float));
    }
    HIP_TRY(hipMemcpyAsync(c->tr.params, flat.data(), nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->tr.windows = max_windows; c->tr.l_frames = max_frames;     // the step's guards: written when everything above exists
    return KM_OK;
}

int legacy_train_copy_masks(Context* c, int64_t B, int64_t T, unsigned char* const host[5], int to_device, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int64_t mo[6];
    legacy_train_mask_layout(B, T, mo);
    if (!to_device && (B != c->tr.l_mask_B || T != c->tr.l_mask_T))
        return fail(KM_ERR_INVALID_ARG, "the masks on the device are those of a (%lld, %lld) step, not (%lld, %lld)", (long long)c->tr.l_mask_B,
                    (long long)c->tr.l_mask_T, (long long)B, (long long)T);
    HIP_TRY(hipStreamSynchronize(st));
    for (int s = 0; s < 5; ++s) {
        if (to_device) HIP_TRY(hipMemcpy(c->tr.l_masks + mo[s], host[s], (size_t)(mo[s + 1] - mo[s]), hipMemcpyHostToDevice));
        else HIP_TRY(hipMemcpy(host[s], c->tr.l_masks + mo[s], (size_t)(mo[s + 1] - mo[s]), hipMemcpyDeviceToHost));
    }
    if (to_device) { c->tr.l_mask_B = B; c->tr.l_mask_T = T; }
    return KM_OK;
}

float* legacy_train_mel_buffer(Context* c) {
    LtrWs w{};
    carve(c->tr.l_ws, c->tr.windows, c->tr.l_frames, &w);
    return w.mel;
}

int legacy_train_step(Context* c, const float* mel, int64_t B, int64_t T, const float* target, float mse_w, float l1_w, float* grad,
                      float* loss_dev, float* out_dev, void* stream) {
    using namespace ltr;
    hipStream_t st = (hipStream_t)stream;
    LtrWs w{};
    carve(c->tr.l_ws, c->tr.windows, c->tr.l_frames, &w);
    const int64_t R = B * T, R2 = B * NQ;
    const float* P = c->tr.params;
    auto par = [&](const char* k) { return P + c->tr.offset.at(k); };
    auto gr = [&](const char* k) { return grad + c->tr.offset.at(k); };
    const float *W0 = par("audio_encoder.0.weight"), *b0 = par("audio_encoder.0.bias"), *W3 = par("audio_encoder.3.weight"),
                *b3 = par("audio_encoder.3.bias"), *Win = par("attention.in_proj_weight"), *bin = par("attention.in_proj_bias"),
                *Wo = par("attention.out_proj.weight"), *bo = par("attention.out_proj.bias"), *Wd0 = par("decoder.0.weight"),
                *bd0 = par("decoder.0.bias"), *Wd3 = par("decoder.3.weight"), *bd3 = par("decoder.3.bias"), *Wd6 = par("decoder.6.weight"),
                *bd6 = par("decoder.6.bias"), *queries = par("blendshape_queries");
    const float p = c->tr_dropout_p;
    const bool drop = p > 0.f;
    const float sc = drop ? 1.0f / (1.0f - p) : 1.0f;
    int64_t mo[6];
    legacy_train_mask_layout(B, T, mo);
    unsigned char* M = c->tr.l_masks;
    if (drop && c->tr_dropout_mode == 1 && (c->tr.l_mask_B != B || c->tr.l_mask_T != T))
        return fail(KM_ERR_INVALID_ARG, "external dropout masks were set for a (%lld, %lld) step, this one is (%lld, %lld)",
                    (long long)c->tr.l_mask_B, (long long)c->tr.l_mask_T, (long long)B, (long long)T);
    if (drop && c->tr_dropout_mode == 0) {
        double t = (double)p * 4294967296.0;
        const unsigned thr = t >= 4294967295.0 ? 4294967295u : (unsigned)t;
        hipLaunchKernelGGL(ltr_mask_gen_kernel, dim3((unsigned)((mo[5] / 4 + 255) / 256)), dim3(256), 0, st, M, mo[5], c->tr.drop_ctr,
                           (unsigned)c->tr_dropout_seed, (unsigned)(c->tr_dropout_seed >> 32), thr);
        c->tr.l_mask_B = B; c->tr.l_mask_T = T;
    }
    auto drop_rows = [&](float* x, int site, int64_t n) {
        if (drop) hipLaunchKernelGGL(ltr_drop_rows_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, x, M + mo[site], n, sc);
    };
    auto relu_bwd = [&](float* g, const float* y, int64_t n) {
        hipLaunchKernelGGL(ltr_relu_bwd_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, g, y, n, sc);
    };
    // ---- forward ----
    if (int rc = launch_gemm(lin(mel, NK, W0, NK, w.E1, R, D, b0, 1), 1, stream)) return rc;
    drop_rows(w.E1, 0, R * D);
    if (int rc = launch_gemm(lin(w.E1, D, W3, D, w.E2, R, D, b3, 1), 1, stream)) return rc;
    drop_rows(w.E2, 1, R * D);
    if (int rc = launch_gemm(lin(w.E2, D, Win + D * D, D, w.KV, R, 2 * D, bin + D, 0), 1, stream)) return rc;
    if (int rc = launch_gemm(lin(queries, D, Win, D, w.Q, NQ, D, bin, 0), 1, stream)) return rc;
    hipLaunchKernelGGL(ltr_attn_fwd_kernel, dim3((unsigned)(B * H)), dim3(64), 0, st, w.Q, w.KV, w.O, w.stat_m, w.stat_il,
                       drop ? M + mo[2] : nullptr, sc, (int)T);
    if (int rc = launch_gemm(lin(w.O, D, Wo, D, w.A1, R2, D, bo, 0), 1, stream)) return rc;
    if (int rc = launch_gemm(lin(w.A1, D, Wd0, D, w.D1, R2, HID, bd0, 1), 1, stream)) return rc;
    drop_rows(w.D1, 3, R2 * HID);
    if (int rc = launch_gemm(lin(w.D1, HID, Wd3, HID, w.D2, R2, HID, bd3, 1), 1, stream)) return rc;
    drop_rows(w.D2, 4, R2 * HID);
    if (int rc = launch_gemm(lin(w.D2, HID, Wd6, HID, w.Z3, R2, NQ, bd6, 0), 1, stream)) return rc;
    hipLaunchKernelGGL(ltr_loss_kernel, dim3(1), dim3(256), 0, st, w.Z3, target, (int)B, mse_w, l1_w, c->tr_loss_cfg, w.out, out_dev, w.dZ3,
                       loss_dev, c->tr.drop_ctr);
    HIP_TRY(hipGetLastError());
    // ---- backward: decoder and out_proj on the B 52 rows ----
    if (int rc = wgrad(c, w.dZ3, NQ, NQ, w.D2, HID, HID, R2, gr("decoder.6.weight"), gr("decoder.6.bias"), stream)) return rc;
    if (int rc = launch_gemm(dgrad(w.dZ3, Wd6, w.dD2, R2, NQ, HID), 1, stream)) return rc;
    relu_bwd(w.dD2, w.D2, R2 * HID);
    if (int rc = wgrad(c, w.dD2, HID, HID, w.D1, HID, HID, R2, gr("decoder.3.weight"), gr("decoder.3.bias"), stream)) return rc;
    if (int rc = launch_gemm(dgrad(w.dD2, Wd3, w.dD1, R2, HID, HID), 1, stream)) return rc;
    relu_bwd(w.dD1, w.D1, R2 * HID);
    if (int rc = wgrad(c, w.dD1, HID, HID, w.A1, D, D, R2, gr("decoder.0.weight"), gr("decoder.0.bias"), stream)) return rc;
    if (int rc = launch_gemm(dgrad(w.dD1, Wd0, w.dA1, R2, HID, D), 1, stream)) return rc;
    if (int rc = wgrad(c, w.dA1, D, D, w.O, D, D, R2, gr("attention.out_proj.weight"), gr("attention.out_proj.bias"), stream)) return rc;
    if (int rc = launch_gemm(dgrad(w.dA1, Wo, w.dO, R2, D, D), 1, stream)) return rc;
    // ---- attention ----
    hipLaunchKernelGGL(ltr_attn_bwd_kernel, dim3((unsigned)(B * H)), dim3(64), 0, st, w.Q, w.KV, w.O, w.dO, w.stat_m, w.stat_il,
                       drop ? M + mo[2] : nullptr, sc, (int)T, w.dKV, w.dQpart);
    hipLaunchKernelGGL(ltr_sum_parts_kernel, dim3((unsigned)((NQ * D + 255) / 256)), dim3(256), 0, st, w.dQpart, (int64_t)NQ * D, (int)B, w.dQ);
    HIP_TRY(hipGetLastError());
    float* gWin = gr("attention.in_proj_weight");
    float* gbin = gr("attention.in_proj_bias");
    if (int rc = wgrad(c, w.dQ, D, D, queries, D, D, NQ, gWin, gbin, stream)) return rc;                      // query third
    if (int rc = launch_gemm(dgrad(w.dQ, Win, gr("blendshape_queries"), NQ, D, D), 1, stream)) return rc;
    if (int rc = wgrad(c, w.dKV, 2 * D, 2 * D, w.E2, D, D, R, gWin + D * D, gbin + D, stream)) return rc;     // key and value thirds
    // ---- encoder on the B T rows ----
    if (int rc = launch_gemm(dgrad(w.dKV, Win + D * D, w.dE2, R, 2 * D, D), 1, stream)) return rc;
    relu_bwd(w.dE2, w.E2, R * D);
    if (int rc = wgrad(c, w.dE2, D, D, w.E1, D, D, R, gr("audio_encoder.3.weight"), gr("audio_encoder.3.bias"), stream)) return rc;
    if (int rc = launch_gemm(dgrad(w.dE2, W3, w.dE1, R, D, D), 1, stream)) return rc;
    relu_bwd(w.dE1, w.E1, R * D);
    if (int rc = wgrad(c, w.dE1, D, D, mel, NK, NK, R, gr("audio_encoder.0.weight"), gr("audio_encoder.0.bias"), stream)) return rc;
    HIP_TRY(hipGetLastError());
    return KM_OK;
}

}  // namespace km
