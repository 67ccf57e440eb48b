// The optimizer tail of a minibatch: gradient norm and Adam over the flat parameter / gradient / moment buffers.  gfx950 only.
#include "common.h"
#include "device_util.h"
#include <math.h>

// ------------------------------------------------------------------------------------------ clip + Adam
// torch.nn.utils.clip_grad_norm_(params, c) + optim.Adam(eps=1e-5).step() + zero_grad() (agents/ppo.py:174-176)
// over the flat parameter / gradient / moment buffers.
// 128 fixed chunks -> partials -> fixed-order final sum (deterministic, and 100x the bandwidth of one workgroup)
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* g, long long n, double* part) {
    __shared__ double sb[4];
    const long long chunk = (n + gridDim.x - 1) / gridDim.x, beg = (long long)blockIdx.x * chunk;
    const long long end = beg + chunk < n ? beg + chunk : n;
    double s = 0.0;
    long long k = beg + threadIdx.x;
    for (; k + 3 * 256 < end; k += 4 * 256) {                  // 4 loads in flight, adds in index order
        const double x0 = (double)g[k], x1 = (double)g[k + 256], x2 = (double)g[k + 512], x3 = (double)g[k + 768];
        s += x0 * x0; s += x1 * x1; s += x2 * x2; s += x3 * x3;
    }
    for (; k < end; k += 256) { const double x = (double)g[k]; s += x * x; }
    const double t = block_sum256(s, sb);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// npart > 0: `sumsq` holds the npart fixed-chunk partial sums of launch_sumsq_partials and every wave adds them up itself, in one fixed
// order in fp64 (lane k takes k, k + 64, ...; shuffle tree) -- no launch between the partial sums and the step, same bits in every wave
__global__ void adam_kernel(float* p, float* g, float* m, float* v, long long n, const double* sumsq, int npart, float max_norm, float lr_unused,
                            float beta1, float beta2, float eps, float step_size, float bc2_sqrt, float* gnorm_out) {
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double total;
    if (npart > 0) {
        double t = 0.0;
        for (int q = threadIdx.x & 63; q < npart; q += 64) t += sumsq[q];
        t = wave_sum(t);
        total = __shfl(t, 0, 64);
    } else total = sumsq[0];
    const float norm = (float)sqrt(total);
    float coef = max_norm / (norm + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;
    if (k == 0 && gnorm_out) gnorm_out[0] = norm;
    if (k >= n) return;
    const float gk = g[k] * coef;
    float mk = m[k], vk = v[k];
    mk = mk + (gk - mk) * (1.f - beta1);                 // exp_avg.lerp_(grad, 1 - beta1)
    vk = vk * beta2 + ((1.f - beta2) * gk) * gk;         // exp_avg_sq.mul_(b2).addcmul_(g, g, value=1-b2)
    const float denom = sqrtf(vk) / bc2_sqrt + eps;
    p[k] = p[k] + (-step_size) * (mk / denom);           // param.addcdiv_(exp_avg, denom, value=-step_size)
    m[k] = mk; v[k] = vk;
    g[k] = 0.f;                                          // optimizer.zero_grad()
}
void launch_adam(float* p, float* g, float* m, float* v, long long n, const double* sumsq, int npart, float max_norm, float lr,
                 float beta1, float beta2, float eps, float step_size, float bc2_sqrt, float* gnorm_out, hipStream_t st) {
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, g, m, v, n, sumsq, npart, max_norm, lr,
                       beta1, beta2, eps, step_size, bc2_sqrt, gnorm_out);
}
void launch_sumsq_partials(const float* g, long long n, double* part /* 128 doubles */, hipStream_t st) {
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(128), dim3(256), 0, st, g, n, part);
}
