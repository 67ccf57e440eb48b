// One linear layer of an MLP for a 16-row tile on v_mfma_f32_16x16x4_f32, activations in LDS, weights streamed from global memory:
// shared by the resident rollout kernel (env_resident.hip) and the fused MLP minibatch pass (mlp_fused.hip).  Device code only; the
// limits RES_R / RES_MAX_LAYERS / RES_MAX_WIDTH are in engine_ctx.h.  gfx950 only.
#pragma once
#include "common.h"

#define RES_THREADS 512                  // 8 waves: a 256-wide layer is 16 column tiles, two per wave, two waves per SIMD
#define RES_LD (RES_MAX_WIDTH + 4)       // LDS row stride in floats: + 4 puts the 16 rows of a 16-byte column read on 16 distinct bank quads
#define RES_ZLD 17

// Y[16][N] = act(X[16][K] W^T + b): W [N][K] row-major in global memory, X / Y in LDS (row stride RES_LD; X's columns K .. Kp - 1 are
// zero, Kp = K rounded up to 16).  Column tile n0 .. n0 + 15 belongs to wave (n0 / 16) % waves.  One 16-wide K chunk is four MFMAs: lane
// (i = lane & 15, q = lane >> 4) holds A[i][kk + 4 q + m] and B[kk + 4 q + m][n0 + i] for MFMA m -- the instruction's k index q stands for
// column kk + 4 q + m in both operands, so each lane fetches its four values of a chunk as ONE 16-byte read of an activation row and ONE
// 16-byte load of a weight row.  A layer whose K is not a multiple of 16 (the first: obs_dim 9 / 5), or whose weights are not 16-byte
// aligned, loads its weights one by one under k < K: nothing is read past a row.  Columns >= N of the last tile (the heads: A + 1 <= 16) load
// zeros and store nothing.  D: column lane & 15, rows 4 q + r.
__device__ __forceinline__ void res_layer(const float* __restrict__ W, const float* __restrict__ b, int K, int N, bool vec, bool relu,
                                          const float* X, float* Y, int ldy, int wave, int lane) {
    const int i = lane & 15, q = lane >> 4;
    const int Kp = (K + 15) & ~15;
    for (int n0 = wave * 16; n0 < N; n0 += (RES_THREADS / 64) * 16) {
        const bool col_on = n0 + i < N;
        const float* wrow = W + (size_t)(col_on ? n0 + i : 0) * (size_t)K + 4 * q;
        const float* xrow = X + i * RES_LD + 4 * q;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        auto chunk = [&](const f32x4 a, const f32x4 w) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w.w, acc1, 0, 0, 0);
        };
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        if (vec && (K & 63) == 0) {
            // K in groups of 64: the weights of group g + 1 are in flight while the 16 MFMAs of group g issue (an L2 hit is several
            // hundred cycles, a group's MFMAs 512)
            f32x4 wc[4], wn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) wc[u] = *(const f32x4*)(wrow + 16 * u);      // (a column >= N reads row 0 and drops it)
            for (int kk = 0; kk < K; kk += 64) {
                const bool more = kk + 64 < K;
#pragma unroll
                for (int u = 0; u < 4; ++u) wn[u] = more ? *(const f32x4*)(wrow + kk + 64 + 16 * u) : zero4;
#pragma unroll
                for (int u = 0; u < 4; ++u) chunk(*(const f32x4*)(xrow + kk + 16 * u), col_on ? wc[u] : zero4);
#pragma unroll
                for (int u = 0; u < 4; ++u) wc[u] = wn[u];
            }
        } else if (vec) {
            for (int kk = 0; kk < Kp; kk += 16) {
                const f32x4 w = *(const f32x4*)(wrow + kk);
                chunk(*(const f32x4*)(xrow + kk), col_on ? w : zero4);
            }
        } else {
            for (int kk = 0; kk < Kp; kk += 16) {
                const f32x4 a = *(const f32x4*)(xrow + kk);
                const int k = kk + 4 * q;
                const float w0 = (col_on && k + 0 < K) ? wrow[kk + 0] : 0.f, w1 = (col_on && k + 1 < K) ? wrow[kk + 1] : 0.f;
                const float w2 = (col_on && k + 2 < K) ? wrow[kk + 2] : 0.f, w3 = (col_on && k + 3 < K) ? wrow[kk + 3] : 0.f;
                chunk(a, (f32x4){w0, w1, w2, w3});
            }
        }
        if (col_on) {
            const float bias = b[n0 + i];
            const float y[4] = {acc0.x + acc1.x + bias, acc0.y + acc1.y + bias, acc0.z + acc1.z + bias, acc0.w + acc1.w + bias};
#pragma unroll
            for (int r = 0; r < 4; ++r) Y[(4 * q + r) * ldy + n0 + i] = relu ? fmaxf(y[r], 0.f) : y[r];
        }
    }
}
