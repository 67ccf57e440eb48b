// GRU over a whole trajectory, forward and backward through time: the sequential part of a recurrent minibatch of algo: ppo-pure
// (the training branch of GRU.forward, common/model.py:226-277, and its autograd).  gfx950 only (64-lane waves).
//
// Rows are time-major: row t*n + i is step t of env i.  The input products gi = W_ih x + b_ih of all T*n rows come from ONE GEMM
// in front of the forward kernel, and dX / dW_ih / db_ih / dW_hh / db_hh are GEMMs / column sums over all T*n rows behind the
// backward kernel (engine.hip); only what depends on h_{t-1} runs here:
//   forward   hm_t = h_{t-1} m[t];  gh = W_hh hm_t + b_hh;  r = s(gi_r + gh_r)  z = s(gi_z + gh_z)  n = tanh(gi_n + r gh_n)
//             h_t = (1 - z) n + z hm_t
//   backward  g = dL/dh_t + carry;  dn = g (1 - z)  dz = g (hm - n);  da_n = dn (1 - n^2)  da_z = dz z (1 - z)
//             da_r = da_n gh_n r (1 - r);  dgi = [da_r, da_z, da_n]  dgh = [da_r, da_z, da_n r];  carry = (g z + dgh W_hh) m[t]
// m[t, i] multiplies the state that ENTERS step t.  The reference's segment loop over has_zeros (model.py:239-270) is this product
// with the mask at every step: inside a segment every mask is 1.
//
// Envs never interact, so a workgroup owns 16 rows (one MFMA tile) for all T steps and there is nothing to wait for but the
// workgroup's own barrier: no grid-wide wait, no flag between workgroups, any grid size runs.  The h tile (forward) / the carry and
// the dgh tile (backward) stay in LDS; the four waves split the gate columns (forward: hidden units, each wave all three gates of
// its units, so the gates need no exchange; backward: the H output columns of dgh W_hh) and run the recurrent product on
// v_mfma_f32_16x16x4_f32 with W_hh streamed from L2 every step (it is read by every workgroup and never leaves L2 at 3 H^2 floats).
// A row's numbers depend on that row's inputs only -- every output element is one lane's accumulator over a fixed k order -- so they
// do not change with n, with the row's tile or with its neighbours.
#include "common.h"
#include "device_util.h"
#include <mutex>


__device__ __forceinline__ float gru_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// sv (saved for the backward pass, may be null): [T*n][4][H] = r, z, n, gh_n.  hm is not stored: it is h_{t-1} m[t] of out_h / h0.
template <int NT>      // H = 64 NT; wave w owns hidden units [16 NT w, 16 NT (w + 1)): NT tiles of 16 units x 3 gates
__global__ __launch_bounds__(256) void gru_seq_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ h0, const float* __restrict__ mask,
                                                          const float* __restrict__ w_hh, const float* __restrict__ b_hh, float* __restrict__ out_h,
                                                          float* __restrict__ sv, int T, int n) {
    constexpr int H = 64 * NT, LD = H + 4;              // LD / 4 odd: the 16 rows of a b128 read fall on 16 different slots
    extern __shared__ __attribute__((aligned(16))) float gru_seq_lds[];       // two h tiles [16][LD]: step t reads one, writes the other
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, q = lane >> 4;
    const int row0 = blockIdx.x * 16;
    for (int e = tid; e < 16 * H; e += 256) {
        const int rr = e / H, j = e - rr * H, row = row0 + rr;
        gru_seq_lds[rr * LD + j] = row < n ? h0[(size_t)row * H + j] * mask[row] : 0.f;
    }
    float bh[NT][3];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int g = 0; g < 3; ++g) bh[tt][g] = b_hh[g * H + w * 16 * NT + tt * 16 + i];
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const float* cur = gru_seq_lds + (t & 1) * 16 * LD;
        float* nxt = gru_seq_lds + ((t + 1) & 1) * 16 * LD;
        f32x4 acc[NT][3];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[tt][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // gh[row][unit] = sum_k hm[row][k] W_hh[unit][k]: A = the hm tile (row i, k = 16 kk + 4 q + e), B = W_hh rows (unit i, same k)
#pragma unroll 2
        for (int kk = 0; kk < H / 16; ++kk) {
            const f32x4 a = *(const f32x4*)(cur + i * LD + kk * 16 + q * 4);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const f32x4 b = *(const f32x4*)(w_hh + (size_t)(g * H + w * 16 * NT + tt * 16 + i) * H + kk * 16 + q * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[tt][g] = MFMA16(a[e], b[e], acc[tt][g]);
                }
        }
        // lane (i, q) holds rows 4 q + r (r = 0..3) of unit column i of each tile
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            const int j = w * 16 * NT + tt * 16 + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = q * 4 + r, row = row0 + rr;
                float keep = 0.f;
                if (row < n) {
                    const size_t s = (size_t)t * n + row;
                    const float* a = gi + s * 3 * H;
                    const float ghn = acc[tt][2][r] + bh[tt][2];
                    const float rg = gru_sigmoid(a[j] + (acc[tt][0][r] + bh[tt][0]));
                    const float zg = gru_sigmoid(a[H + j] + (acc[tt][1][r] + bh[tt][1]));
                    const float ng = tanhf(a[2 * H + j] + rg * ghn);
                    const float hn = (1.f - zg) * ng + zg * cur[rr * LD + j];
                    out_h[s * H + j] = hn;
                    if (sv) { float* v = sv + s * 4 * H; v[j] = rg; v[H + j] = zg; v[2 * H + j] = ng; v[3 * H + j] = ghn; }
                    if (t + 1 < T) keep = hn * mask[s + n];
                }
                nxt[rr * LD + j] = keep;            // h_t m[t + 1]: the state that enters the next step
            }
        }
        __syncthreads();
    }
}

// Writes dgi, dgh ([T*n][3H] each) and hm ([T*n][H], the masked input states: the B operand of dW_hh = dGH^T HM).
template <int NT>      // wave w owns the output columns k = 16 NT w + NT i + e' (tile e', lane column i) of dgh W_hh: NT contiguous floats of a W_hh row per lane
__global__ __launch_bounds__(256) void gru_seq_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out_h, const float* __restrict__ h0,
                                                          const float* __restrict__ mask, const float* __restrict__ sv, const float* __restrict__ w_hh,
                                                          float* __restrict__ dgi, float* __restrict__ dgh, float* __restrict__ hm_out, int T, int n) {
    constexpr int H = 64 * NT, LDG = 3 * H + 4, LDC = H + 4;
    extern __shared__ __attribute__((aligned(16))) float gru_seq_lds[];       // dgh tile [16][LDG], then the carry / g z tile [16][LDC]
    float* G = gru_seq_lds;
    float* C = gru_seq_lds + 16 * LDG;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, q = lane >> 4;
    const int row0 = blockIdx.x * 16;
    for (int e = tid; e < 16 * LDC; e += 256) C[e] = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t) {
        for (int e = tid; e < 16 * H; e += 256) {
            const int rr = e / H, j = e - rr * H, row = row0 + rr;
            float dar = 0.f, daz = 0.f, danr = 0.f, gz = 0.f;
            if (row < n) {
                const size_t s = (size_t)t * n + row;
                const float hp = t > 0 ? out_h[(s - n) * H + j] : h0[(size_t)row * H + j];
                const float hm = hp * mask[s];
                const float g = dout[s * H + j] + C[rr * LDC + j];
                const float* v = sv + s * 4 * H;
                const float rg = v[j], zg = v[H + j], ng = v[2 * H + j], ghn = v[3 * H + j];
                const float dan = g * (1.f - zg) * (1.f - ng * ng);
                daz = g * (hm - ng) * zg * (1.f - zg);
                dar = dan * ghn * rg * (1.f - rg);
                danr = dan * rg;
                gz = g * zg;
                float* a = dgi + s * 3 * H;
                a[j] = dar; a[H + j] = daz; a[2 * H + j] = dan;
                float* b = dgh + s * 3 * H;
                b[j] = dar; b[H + j] = daz; b[2 * H + j] = danr;
                hm_out[s * H + j] = hm;
            }
            G[rr * LDG + j] = dar; G[rr * LDG + H + j] = daz; G[rr * LDG + 2 * H + j] = danr;
            C[rr * LDC + j] = gz;
        }
        if (t == 0) break;                          // h0 receives no gradient
        __syncthreads();
        // (dgh W_hh)[row][k] = sum_c dgh[row][c] W_hh[c][k], c over the 3H gate columns: A = the dgh tile (row i, c = 16 cb + 4 q + s),
        // B = W_hh row c, columns k of this lane's NT tiles
        f32x4 acc[NT];
#pragma unroll
        for (int e = 0; e < NT; ++e) acc[e] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* wk = w_hh + w * 16 * NT + NT * i;
#pragma unroll 2
        for (int cb = 0; cb < 3 * H / 16; ++cb) {
            const f32x4 a = *(const f32x4*)(G + i * LDG + cb * 16 + q * 4);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float b[NT];
                const float* wr = wk + (size_t)(cb * 16 + q * 4 + s) * H;
#pragma unroll
                for (int e = 0; e < NT; ++e) b[e] = wr[e];
#pragma unroll
                for (int e = 0; e < NT; ++e) acc[e] = MFMA16(a[s], b[e], acc[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < NT; ++e)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = q * 4 + r, row = row0 + rr, k = w * 16 * NT + NT * i + e;
                const float m = row < n ? mask[(size_t)t * n + row] : 0.f;
                C[rr * LDC + k] = (C[rr * LDC + k] + acc[e][r]) * m;           // the carry into step t - 1
            }
        __syncthreads();
    }
}

template <int H> struct GruSeqFwd {
    static void run(const float* gi, const float* h0, const float* mask, const float* w_hh, const float* b_hh, float* out_h, float* sv, int T, int n, hipStream_t st) {
        constexpr int NT = H / 64;
        constexpr int LDS = 2 * 16 * (H + 4) * 4;
        static std::once_flag attr;
        std::call_once(attr, [] { hipFuncSetAttribute((const void*)gru_seq_fwd_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS); });
        hipLaunchKernelGGL(gru_seq_fwd_kernel<NT>, dim3((n + 15) / 16), dim3(256), LDS, st, gi, h0, mask, w_hh, b_hh, out_h, sv, T, n);
    }
};
template <int H> struct GruSeqBwd {
    static void run(const float* dout, const float* out_h, const float* h0, const float* mask, const float* sv, const float* w_hh, float* dgi, float* dgh,
                    float* hm_out, int T, int n, hipStream_t st) {
        constexpr int NT = H / 64;
        constexpr int LDS = 16 * (3 * H + 4 + H + 4) * 4;
        static std::once_flag attr;
        std::call_once(attr, [] { hipFuncSetAttribute((const void*)gru_seq_bwd_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS); });
        hipLaunchKernelGGL(gru_seq_bwd_kernel<NT>, dim3((n + 15) / 16), dim3(256), LDS, st, dout, out_h, h0, mask, sv, w_hh, dgi, dgh, hm_out, T, n);
    }
};

// mask[k] = 1 - done[idx[k]]: the training masks of a recurrent minibatch, gathered by flat index t*E + e from the (T, E) rollout array
__global__ void gru_seq_mask_kernel(const float* __restrict__ done, const int32_t* __restrict__ idx, float* __restrict__ mask, int N) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < N) mask[k] = 1.f - done[idx[k]];
}
void launch_gru_seq_mask(const float* done, const int32_t* idx, float* mask, int N, hipStream_t st) {
    if (N <= 0) return;
    hipLaunchKernelGGL(gru_seq_mask_kernel, dim3((N + 255) / 256), dim3(256), 0, st, done, idx, mask, N);
}

bool gru_seq_width_ok(int H) { return H >= 64 && H <= 512 && H % 64 == 0; }
void launch_gru_seq_fwd(const float* gi, const float* h0, const float* mask, const float* w_hh, const float* b_hh, float* out_h, float* sv, int T, int n, int H,
                        hipStream_t st) {
    if (T <= 0 || n <= 0) return;
    if (!fc_dispatch_width<GruSeqFwd>(H, gi, h0, mask, w_hh, b_hh, out_h, sv, T, n, st)) mi_launch_fail("GRU sequence forward: H must be a multiple of 64 in [64, 512]");
}
void launch_gru_seq_bwd(const float* dout, const float* out_h, const float* h0, const float* mask, const float* sv, const float* w_hh, float* dgi, float* dgh,
                        float* hm_out, int T, int n, int H, hipStream_t st) {
    if (T <= 0 || n <= 0) return;
    if (!fc_dispatch_width<GruSeqBwd>(H, dout, out_h, h0, mask, sv, w_hh, dgi, dgh, hm_out, T, n, st)) mi_launch_fail("GRU sequence backward: H must be a multiple of 64 in [64, 512]");
}
