// Storage.compute_estimates (common/storage.py:56-79): the GAE scan and the advantage normalisation (statistics, cross-rank merge,
// apply).  gfx950 only.
#include "common.h"
#include "device_util.h"
#include <math.h>

// ------------------------------------------------------------------------------------------ GAE scan
// Storage.compute_estimates (common/storage.py:56-77).  One thread per env (coalesced over E),
// serial over T; fp contraction off so every operation rounds exactly like the reference's
// separate fp32 tensor ops (bit-exact advantages/returns).
__global__ void gae_kernel(const float* rew, const float* done, const float* value, float* adv, float* ret, int T, int E,
                           float gamma, float gl, int use_gae) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    float A = 0.f;
    for (int i = T - 1; i >= 0; --i) {
        const long long o = (long long)i * E + e;
        float a_i = 0.f;
        if (use_gae) {
            const float nd = 1.f - done[o];
            const float delta = (rew[o] + (gamma * value[o + E]) * nd) - value[o];
            A = ((gl * A) * nd) + delta;
            a_i = A;
        }
        adv[o] = a_i;
        ret[o] = a_i + value[o];           // use_gae=False: return = adv(=0) + V (the reference's overwrite, storage.py:77)
    }
}
void launch_gae(const float* rew, const float* done, const float* value, float* adv, float* ret, int T, int E,
                float gamma, float lmbda, int use_gae, hipStream_t st) {
    const float gl = (float)((double)gamma * (double)lmbda);
    hipLaunchKernelGGL(gae_kernel, dim3((E + 63) / 64), dim3(64), 0, st, rew, done, value, adv, ret, T, E, gamma, gl, use_gae);
}

// advantage normalisation (common/storage.py:78-79): (A - mean) / (std_unbiased + 1e-8).
// stats3 = {count, mean, M2} in fp64 so that ranks can merge them (Chan) before apply.
__global__ __launch_bounds__(1024) void advnorm_stats_kernel(const float* adv, int n, double* stats3) {
    __shared__ double sb[16];
    __shared__ double s_mean;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double s = 0.0;
    for (int k = tid; k < n; k += 1024) s += (double)adv[k];
    s = wave_sum(s);
    if (lane == 0) sb[w] = s;
    __syncthreads();
    if (tid == 0) { double t = 0.0; for (int k = 0; k < 16; ++k) t += sb[k]; s_mean = n > 0 ? t / n : 0.0; }
    __syncthreads();
    const double mean = s_mean;
    double m2 = 0.0;
    for (int k = tid; k < n; k += 1024) { const double d = (double)adv[k] - mean; m2 += d * d; }
    m2 = wave_sum(m2);
    __syncthreads();
    if (lane == 0) sb[w] = m2;
    __syncthreads();
    if (tid == 0) { double t = 0.0; for (int k = 0; k < 16; ++k) t += sb[k]; stats3[0] = (double)n; stats3[1] = mean; stats3[2] = t; }
}
__global__ void advnorm_apply_kernel(float* adv, int n, const double* stats3) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float mean = (float)stats3[1];
    const float sd = (float)sqrt(stats3[2] / (stats3[0] - 1.0));
    adv[k] = (adv[k] - mean) / (sd + 1e-8f);
}
// Merge of R ranks' {count, mean, M2} triples (fp64) into stats3 -- the device side of mi355/dist.py::merge_adv_stats, same operations
// in the same order (no contraction), so the two agree bit for bit.  Two passes around a pivot, the first non-empty rank's mean:
//   mean = pivot + shift, shift = sum_r c_r (mu_r - pivot) / n;   M2 = sum_r s_r + c_r ((mu_r - pivot) - shift)^2
// The differences of nearby means are exact, and an error of the merged mean reaches M2 only in second order (sum_r c_r (mu_r - mean)
// = 0), where the pairwise recurrence mean += d c / tot rounds a running mean of full magnitude at every rank and carries that into
// every later d: 2.3e-14 of an M2 of 0.1 for eight ranks at mean 1000, sd 0.01, against 3e-15 here (tests/test_gpu_optim_ops.py).
__global__ void advnorm_merge_kernel(const double* all, int R, double* stats3) {
#pragma clang fp contract(off)
    if (threadIdx.x || blockIdx.x) return;
    double n = 0.0, pivot = 0.0, acc = 0.0;
    bool have = false;
    for (int r = 0; r < R; ++r) {
        const double c = all[3 * r], mu = all[3 * r + 1];
        if (c == 0.0) continue;
        if (!have) { pivot = mu; have = true; }
        n = n + c;
        acc = acc + c * (mu - pivot);
    }
    const double shift = have ? acc / n : 0.0;
    double m2 = 0.0;
    for (int r = 0; r < R; ++r) {
        const double c = all[3 * r], mu = all[3 * r + 1], s = all[3 * r + 2];
        if (c == 0.0) continue;
        const double d = (mu - pivot) - shift;
        m2 = (m2 + s) + (c * d) * d;
    }
    stats3[0] = n; stats3[1] = pivot + shift; stats3[2] = m2;
}
void launch_advnorm_merge(const double* all, int R, double* stats3, hipStream_t st) {
    hipLaunchKernelGGL(advnorm_merge_kernel, dim3(1), dim3(64), 0, st, all, R, stats3);
}
void launch_advnorm_stats(const float* adv, int n, double* stats3, hipStream_t st) {
    hipLaunchKernelGGL(advnorm_stats_kernel, dim3(1), dim3(1024), 0, st, adv, n, stats3);
}
void launch_advnorm_apply(float* adv, int n, const double* stats3, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(advnorm_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, st, adv, n, stats3);
}
