// Fixed-order sums of per-workgroup gradient slabs (the conv / heads weight gradients) and the column sum behind the linear layers'
// bias gradients -- the tail of every loss.backward() of agents/ppo.py.  No float atomics: results are bitwise reproducible run to run.
// gfx950 only.
#include "common.h"

// ------------------------------------------------------------------------------------------ slab / column reductions
__global__ __launch_bounds__(1024) void reduce_slabs_kernel(const float* __restrict__ partial, int nslab, int slab_len,
                                                            float* dst_w, int n_w, float* dst_b, int n_b) {
    __shared__ float sh[32][33];
    const int ex = threadIdx.x & 31, g = threadIdx.x >> 5;        // 32 elements x 32 slab groups
    const int e = blockIdx.x * 32 + ex;
    float s = 0.f;
    if (e < slab_len)
        for (int b = g; b < nslab; b += 32) s += partial[(long long)b * slab_len + e];
    sh[g][ex] = s;
    __syncthreads();
    if (g == 0 && e < slab_len) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 32; ++k) t += sh[k][ex];
        if (e < n_w) dst_w[e] += t;
        else if (e - n_w < n_b) dst_b[e - n_w] += t;
    }
}
// All conv layers of one backward pass in ONE launch (blockIdx.y = layer): each layer's workgroups left their slabs in
// its own region of the workspace.  Same per-element summation order as reduce_slabs_kernel.
__global__ __launch_bounds__(1024) void reduce_all_slabs_kernel(const float* __restrict__ ws, float* __restrict__ grads, const SlabDesc* __restrict__ desc) {
    __shared__ f32x4 sh[32][33];
    const SlabDesc d = desc[blockIdx.y];
    const int ex = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int e = (blockIdx.x * 32 + ex) * 4;                     // 4 consecutive elements per thread (slab lengths, offsets and the
    if (blockIdx.x * 128 >= d.slab_len) return;                   // weight / bias boundary are multiples of 4): 512-byte rows per half-wave
    const float* partial = ws + d.src_off;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (e < d.slab_len) {
        int b = g;
        for (; b + 96 < d.nslab; b += 128) {                      // 4 loads in flight; adds stay in slab order
            const f32x4 v0 = *(const f32x4*)(partial + (long long)b * d.slab_len + e), v1 = *(const f32x4*)(partial + (long long)(b + 32) * d.slab_len + e);
            const f32x4 v2 = *(const f32x4*)(partial + (long long)(b + 64) * d.slab_len + e), v3 = *(const f32x4*)(partial + (long long)(b + 96) * d.slab_len + e);
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; b < d.nslab; b += 32) s += *(const f32x4*)(partial + (long long)b * d.slab_len + e);
    }
    sh[g][ex] = s;
    __syncthreads();
    if (g == 0 && e < d.slab_len) {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8                                                   // (all 32 reads in flight spilled 8 registers to scratch memory)
        for (int k = 0; k < 32; ++k) t += sh[k][ex];
        float* dst = (e < d.n_w) ? grads + d.w_off + e : grads + d.b_off + e - d.n_w;
        dst[0] += t.x; dst[1] += t.y; dst[2] += t.z; dst[3] += t.w;
    }
}
void launch_reduce_all_slabs(const float* ws, float* grads, const SlabDesc* d_desc, int n_desc, int max_slab_len, hipStream_t st) {
    if (n_desc <= 0) return;
    hipLaunchKernelGGL(reduce_all_slabs_kernel, dim3((max_slab_len + 127) / 128, n_desc), dim3(1024), 0, st, ws, grads, d_desc);
}
void launch_reduce_slabs(const float* partial, int nslab, int slab_len, float* dst_w, int n_w, float* dst_b, int n_b, hipStream_t st) {
    if (nslab <= 0) return;
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3((slab_len + 31) / 32), dim3(1024), 0, st, partial, nslab, slab_len, dst_w, n_w, dst_b, n_b);
}

// db[n] += sum_m dY[m][n]   (bias gradients of the linear layers); 64 row groups x fixed order
__global__ void colsum_partial_kernel(const float* dY, int M, int N, int ld, float* part) {
    const int n = blockIdx.x * 64 + (threadIdx.x & 63), rg = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int groups = gridDim.y * 4;
    float s = 0.f;
    if (n < N) {
        int m = rg;
        for (; m + 7 * groups < M; m += 8 * groups) {        // 8 loads in flight; the adds keep row order
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = dY[(long long)(m + q * groups) * ld + n];
#pragma unroll
            for (int q = 0; q < 8; ++q) s += v[q];
        }
        for (; m < M; m += groups) s += dY[(long long)m * ld + n];
        part[(long long)rg * N + n] = s;
    }
}
void launch_colsum_acc(const float* dY, int M, int N, int ld, float* db, float* col_ws, hipStream_t st) {
    if (M <= 0) return;
    // the partial sums are gy*4 rows of N floats: 64 x N past the workspace's end from N = 4097 on
    if (N > COLSUM_MAX_N) { mi_launch_fail("column sum: N must be at most 4096 (the 64 x 4096 partial-sum workspace)"); return; }
    const int gy = (M >= 4096 && N <= 1024) ? 64 : 16;         // workspace: 64 x COLSUM_MAX_N floats (engine.hip)
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((N + 63) / 64, gy), dim3(256), 0, st, dY, M, N, ld, col_ws);
    launch_reduce_slabs(col_ws, gy * 4, N, db, N, nullptr, 0, st);
}
