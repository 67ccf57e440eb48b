// The distillation loss (distill.py:164-204 of the reference: MSELoss(student(obs).logits, Y_gold), Y_gold = teacher(obs).logits): the
// per-sample terms with the analytic gradient towards the student's raw logits and the finaliser of the mean.  gfx950 only; fp32
// per-sample arithmetic in either precision mode, fp64 block sums in a fixed order (no atomics: a record does not depend on launch
// timing).  The labels themselves need no kernel of their own: they are the rows launch_logp_all (heads.hip, mi_forward's path) writes.
#include "common.h"
#include "device_util.h"
#include "policy_math.h"
#include <math.h>

constexpr int DST_BLK = 64;          // samples per workgroup: one wave, as the PPO loss (loss.hip LOSS_BLK)
int distill_blocks(int n) { return (n + DST_BLK - 1) / DST_BLK; }

// One thread per sample.  lp = the twice-normalised log-probabilities of the row's logits (Categorical(logits=log_softmax(z)).logits,
// common/policy.py:77-87), d_k = lp_k - y_k with y = target row idx[s] (null idx: row s), the row's sum_k d_k^2 -> fp64 block partial.
// dY (null: forward only) = d (scale * sum d^2) / d z through BOTH normalisations: g = 2 scale d arrives at the second log-softmax, whose
// Jacobian is I - 1 p^T with p = softmax(lp) (log_softmax_twice_t's p), then the first, I - 1 q1^T with q1 = softmax(z).  The value
// column takes no part in the loss: exactly 0.
__global__ __launch_bounds__(DST_BLK) void distill_loss_kernel(DistillArgs a) {
    const int s = blockIdx.x * DST_BLK + threadIdx.x;
    float sq = 0.f;
    if (s < a.n) {
        const float* h = a.hout + (long long)s * (a.A + 1);
        float z[MAXA], lp[MAXA], p[MAXA], q1[MAXA], g[MAXA], lse_unused = 0.f;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) z[k] = (k < a.A) ? h[k] : 0.f;
        log_softmax_twice_t<true>(z, a.A, lp, p, lse_unused, q1);
        const float* y = a.target + (long long)(a.idx ? a.idx[s] : s) * a.A;
        float G = 0.f;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) if (k < a.A) {
            const float d = lp[k] - y[k];
            sq += d * d;
            g[k] = 2.f * a.scale * d;
            G += g[k];
        }
        if (a.dY) {
            float G2 = 0.f;
#pragma unroll
            for (int k = 0; k < MAXA; ++k) if (k < a.A) { g[k] -= p[k] * G; G2 += g[k]; }
            float* d = a.dY + (long long)s * (a.A + 1);
#pragma unroll
            for (int k = 0; k < MAXA; ++k) if (k < a.A) d[k] = g[k] - q1[k] * G2;
            d[a.A] = 0.f;
        }
    }
    const double r = wave_sum((double)sq);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = r;
}

// One workgroup: the block partials summed in a fixed order in fp64 (thread t takes blocks t, t + 256, ...; then block_sum256).
// rec8 (may be null): the loss-log record {loss, 0, 0, 0, loss, 0, 0, 0}, loss = sum * inv_count.  acc (may be null): the running fp64 sum
// of a forward-only evaluation over several chunks, acc[0] = (acc_reset ? 0 : acc[0]) + sum -- chunks add in stream order.
__global__ __launch_bounds__(256) void distill_finalize_kernel(const double* partial, int nblk, double inv_count, float* rec8, double* acc, int acc_reset) {
    __shared__ double sb[4];
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += partial[b];
    const double tot = block_sum256(s, sb);
    if (threadIdx.x != 0) return;
    if (rec8) {
        const float loss = (float)(tot * inv_count);
        rec8[0] = loss; rec8[1] = 0.f; rec8[2] = 0.f; rec8[3] = 0.f; rec8[4] = loss; rec8[5] = 0.f; rec8[6] = 0.f; rec8[7] = 0.f;
    }
    if (acc) acc[0] = (acc_reset ? 0.0 : acc[0]) + tot;
}

void launch_distill_loss(const DistillArgs& a, double inv_count, float* rec8, double* acc, int acc_reset, hipStream_t st) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(distill_loss_kernel, dim3(distill_blocks(a.n)), dim3(DST_BLK), 0, st, a);
    hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)a.partial, distill_blocks(a.n), inv_count, rec8, acc, acc_reset);
}
