// The generic fp32 MFMA GEMM of the linear layers (nn.Linear in common/model.py and common/policy.py) with its split-K reduce.
// gfx950 only.  Split-K slabs are summed in a fixed order: results are bitwise reproducible run to run.
#include "common.h"
#include "device_util.h"
#include <math.h>

// ------------------------------------------------------------------------------------------ GEMM
// 64x64 output tile per workgroup, K tile 16, four waves as 2x2 of 32x32; K permuted so that lane
// quarter q owns k = 4q..4q+3 of the K tile (one ds_read_b128 per operand per 4 MFMAs).
// Used for: embedder.fc, the policy/value heads and the MLP embedder (forward, dgrad, wgrad) --
// nn.Linear in common/model.py:176,199 / :966-971 and common/policy.py:39-40,75,80.
__device__ __forceinline__ float gemm_ld(const float* p, long long o, int bf16) {
    return bf16 ? __uint_as_float(((unsigned)((const unsigned short*)p)[o]) << 16) : p[o];
}
// K tile 32; the next tile's global loads are issued into registers before the MFMAs of the current one.
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g, int k_chunk, float* ws) {
    __shared__ __attribute__((aligned(16))) float As[64 * 36];
    __shared__ __attribute__((aligned(16))) float Bs[64 * 36];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4, wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int kbeg = blockIdx.z * k_chunk, kend = min(g.K, kbeg + k_chunk);
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool a_kc = (g.sak == 1), b_kc = (g.sbk == 1);
    float ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int l = tid + e * 256;
            int m, k;
            if (a_kc) { m = l >> 5; k = l & 31; } else { m = l & 63; k = l >> 6; }
            float v = 0.f;
            if (m0 + m < g.M && k0 + k < kend) v = gemm_ld(g.A, (long long)(m0 + m) * g.sam + (long long)(k0 + k) * g.sak, g.a_bf16);
            ra[e] = v;
            int n;
            if (b_kc) { n = l >> 5; k = l & 31; } else { n = l & 63; k = l >> 6; }
            v = 0.f;
            if (n0 + n < g.N && k0 + k < kend) v = gemm_ld(g.B, (long long)(k0 + k) * g.sbk + (long long)(n0 + n) * g.sbn, g.b_bf16);
            rb[e] = v;
        }
    };
    if (kbeg < kend) fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int l = tid + e * 256;
            int m, k;
            if (a_kc) { m = l >> 5; k = l & 31; } else { m = l & 63; k = l >> 6; }
            As[m * 36 + k] = g.relu_a ? fmaxf(ra[e], 0.f) : ra[e];
            int n;
            if (b_kc) { n = l >> 5; k = l & 31; } else { n = l & 63; k = l >> 6; }
            Bs[n * 36 + k] = g.relu_b ? fmaxf(rb[e], 0.f) : rb[e];
        }
        __syncthreads();
        if (k0 + 32 < kend) fetch(k0 + 32);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = *(const f32x4*)(As + (wm * 32 + a * 16 + i) * 36 + q * 4 + h * 16);
#pragma unroll
            for (int b = 0; b < 2; ++b) bv[b] = *(const f32x4*)(Bs + (wn * 32 + b * 16 + i) * 36 + q * 4 + h * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = MFMA16(av[a][e], bv[b][e], acc[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * 32 + a * 16 + q * 4 + r, n = n0 + wn * 32 + b * 16 + i;
                if (m < g.M && n < g.N) {
                    float v = acc[a][b][r];
                    if (ws) { ws[((long long)blockIdx.z * g.M + m) * g.N + n] = v; continue; }
                    const long long o = (long long)m * g.ldc + n;
                    if (g.bias) v += g.bias[n];
                    if (g.relu_out) v = fmaxf(v, 0.f);
                    if (g.mask) v = gemm_ld(g.mask, o, g.mask_bf16) > 0.f ? v : 0.f;
                    if (g.c_bf16) { ((unsigned short*)g.C)[o] = f2bf(v); continue; }
                    if (g.accumulate) v += g.C[o];
                    g.C[o] = v;
                }
            }
}

__global__ void gemm_splitk_reduce(const float* ws, int split, GemmArgs g) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)g.M * g.N) return;
    float v = 0.f;
    {   // 8 loads in flight, adds in split order (a plain run-time loop waited for every load before issuing the next: 21 us for 64 splits)
        const long long mn = (long long)g.M * g.N;
        int z = 0;
        for (; z + 8 <= split; z += 8) {
            float t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = ws[(long long)(z + q) * mn + e];
#pragma unroll
            for (int q = 0; q < 8; ++q) v += t[q];
        }
        for (; z < split; ++z) v += ws[(long long)z * mn + e];
    }
    const int n = (int)(e % g.N);
    const long long o = (e / g.N) * g.ldc + n;
    if (g.bias) v += g.bias[n];
    if (g.relu_out) v = fmaxf(v, 0.f);
    if (g.mask) {
        const float mv = g.mask_bf16 ? __uint_as_float(((unsigned)((const unsigned short*)g.mask)[o]) << 16) : g.mask[o];
        v = mv > 0.f ? v : 0.f;
    }
    if (g.c_bf16) { ((unsigned short*)g.C)[o] = f2bf(v); return; }
    if (g.accumulate) v += g.C[o];
    g.C[o] = v;
}

// The split plan of one call, from the sizes and the workspace alone (launch_gemm and the op-level hook mi_op_linear both take it from
// here).  Few output tiles and a long K (weight gradients: K = batch; rollout-sized forward GEMMs: M = n_envs): K is split over
// workgroups, slabs summed in a fixed order by the reduce kernel (which carries the epilogue).  split = min(512 / tiles, K / 128), lowered
// until the slabs fit the workspace; k_chunk is rounded up to the K tile, so the run can have fewer slabs than first planned.
GemmPlan gemm_plan(const GemmArgs& g) {
    const int tm = (g.M + 63) / 64, tn = (g.N + 63) / 64;
    int split = 1;
    if (g.K >= 512 && tm * tn < 192 && g.ws) {
        split = 512 / (tm * tn);
        if (split > g.K / 128) split = g.K / 128;
        if (split < 1) split = 1;
        while (split > 1 && (size_t)split * g.M * g.N > g.ws_floats) --split;
    }
    const int k_chunk = ((g.K + split - 1) / split + 31) / 32 * 32;
    if (split > 1) split = (g.K + k_chunk - 1) / k_chunk;
    return GemmPlan{split, k_chunk};
}

// split-K slabs live in the caller's workspace (GemmArgs.ws, one per context: two contexts on two streams must not share it)
void launch_gemm(const GemmArgs& g, hipStream_t st) {
    if (g.M <= 0 || g.N <= 0) return;
    const int tm = (g.M + 63) / 64, tn = (g.N + 63) / 64;
    const GemmPlan p = gemm_plan(g);
    if (p.split == 1) {
        hipLaunchKernelGGL(gemm_kernel, dim3(tn, tm, 1), dim3(256), 0, st, g, p.k_chunk, (float*)nullptr);
    } else {
        hipLaunchKernelGGL(gemm_kernel, dim3(tn, tm, p.split), dim3(256), 0, st, g, p.k_chunk, g.ws);
        const long long tot = (long long)g.M * g.N;
        hipLaunchKernelGGL(gemm_splitk_reduce, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st,
                           (const float*)g.ws, p.split, g);
    }
}
