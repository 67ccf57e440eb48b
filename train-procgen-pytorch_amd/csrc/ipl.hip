// The IPL loss (agents/IPL.py:109-225 with cross_batch_entropy, common/misc_util.py:42-51): the next-value overwrite, the per-sample terms
// with the analytic gradient towards BOTH network passes (obs[t] through dY, obs[t + 1] through g_next), the finaliser of the eight
// summary terms, the next-side seed and the greedy action.  gfx950 only; fp32 per-sample arithmetic in either precision mode, fp64 block
// sums in a fixed order (no atomics: a record does not depend on launch timing).
#include "common.h"
#include "device_util.h"
#include "policy_math.h"
#include <math.h>

constexpr int IPL_BLK = 64;          // samples per workgroup: one wave, as the PPO loss (loss.hip LOSS_BLK)
int ipl_blocks(int n) { return (n + IPL_BLK - 1) / IPL_BLK; }
int ipl_partial_cols(int A) { return IPL_SUMS + A; }

// nv[i] = done ? rew : V(nobs[i])  (IPL.py:129-131: the in-place overwrite cuts the gradient on those rows).  v_src[i * v_stride + v_off]
// is the value column of the nobs pass (the engine: hout, A + 1, A; the op hook: a plain vector)
__global__ __launch_bounds__(IPL_BLK) void ipl_next_value_kernel(IplArgs a, const float* v_src, int v_stride, int v_off) {
    const int s = blockIdx.x * IPL_BLK + threadIdx.x;
    if (s >= a.n) return;
    const int gi = a.idx ? a.idx[s] : s;
    a.nv[s] = (a.done[gi] != 0.f) ? a.rew[gi] : v_src[(long long)s * v_stride + v_off];
}

// One thread per sample.  pred = modifier * logp + v - gamma * nv; loss = mean((pred - rew)^2) - [reward_incentive] mean(pred)
// - [adv_incentive] mean(max_k logp_k) + entropy_coef * mean(H).  Block partial row (fp64): 0 sum (pred - rew)^2, 1 sum pred, 2 sum rew,
// 3 sum pred^2, 4 sum rew^2, 5 sum pred rew, 6 sum H, 7 sum max_k logp_k, 8.. sum p_k.
__global__ __launch_bounds__(IPL_BLK) void ipl_loss_kernel(IplArgs a) {
    const int s = blockIdx.x * IPL_BLK + threadIdx.x;
    const bool live = s < a.n;
    float sums[IPL_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float p[MAXA];
#pragma unroll
    for (int k = 0; k < MAXA; ++k) p[k] = 0.f;
    if (live) {
        const float* h = a.hout + (long long)s * (a.A + 1);
        float z[MAXA], lp[MAXA], lse_unused = 0.f;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) z[k] = (k < a.A) ? h[k] : 0.f;
        log_softmax_twice_t<false>(z, a.A, lp, p, lse_unused, nullptr);
        const int gi = a.idx ? a.idx[s] : s;
        const int act = a.act[gi];
        const float rew = a.rew[gi];
        const bool done = a.done[gi] != 0.f;
        const float v = h[a.A], nv = a.nv[s];
        float H = 0.f, lpa = 0.f, mx = lp[0];
        int kmax = 0;                                   // torch.max / argmax: the lowest index among equal maxima
#pragma unroll
        for (int k = 0; k < MAXA; ++k) if (k < a.A) {
            H -= p[k] * lp[k];
            lpa = (k == act) ? lp[k] : lpa;
            if (lp[k] > mx) { mx = lp[k]; kmax = k; }
        }
        const float ea = expf(lpa);
        const float modifier = a.entropy_modified ? a.alpha * (1.f - ea) : a.alpha;
        // d (modifier * logp) / d logp: alpha, or alpha * (1 - e^logp (1 + logp))
        const float dmod = a.entropy_modified ? a.alpha * (1.f - ea * (1.f + lpa)) : a.alpha;
        const float pred = modifier * lpa + v - a.gamma * nv;
        const float e = pred - rew;
        a.pred[s] = pred;
        a.rew_out[s] = rew;
        // d loss / d pred (the 1 / n_global of the means included)
        const float gp = a.inv_n_global * (2.f * e - (a.reward_incentive ? 1.f : 0.f));
        const float z0 = a.zero_obs_seed ? 0.f : 1.f;  // test switch: only the next-observation path carries gradient
        const float g_lp = gp * dmod;
        const float cH = a.entropy_coef * a.inv_n_global, cM = a.adv_incentive ? a.inv_n_global : 0.f;
        float* d = a.dY + (long long)s * (a.A + 1);
#pragma unroll
        for (int k = 0; k < MAXA; ++k) if (k < a.A) {
            float gk = g_lp * ((k == act ? 1.f : 0.f) - p[k]);
            gk -= cM * ((k == kmax ? 1.f : 0.f) - p[k]);
            gk += cH * (-p[k] * (lp[k] + H));
            d[k] = z0 * gk;
        }
        d[a.A] = z0 * gp;
        a.g_next[s] = done ? 0.f : -a.gamma * gp;
        sums[0] = e * e; sums[1] = pred; sums[2] = rew; sums[3] = pred * pred; sums[4] = rew * rew; sums[5] = pred * rew; sums[6] = H; sums[7] = mx;
    }
    double* row = a.partial + (long long)blockIdx.x * (IPL_SUMS + a.A);
    const int lane = threadIdx.x;
#pragma unroll
    for (int j = 0; j < IPL_SUMS; ++j) {
        // products formed in fp64 where fp32 would round before the sum: the correlation cancels sums of squares
        double x = (double)sums[j];
        if (live && j == 3) x = (double)sums[1] * (double)sums[1];
        if (live && j == 4) x = (double)sums[2] * (double)sums[2];
        if (live && j == 5) x = (double)sums[1] * (double)sums[2];
        const double r = wave_sum(x);
        if (lane == 0) row[j] = r;
    }
#pragma unroll
    for (int k = 0; k < MAXA; ++k) if (k < a.A) { const double r = wave_sum((double)p[k]); if (lane == 0) row[IPL_SUMS + k] = r; }
}

// One workgroup: column c of the partial rows summed by four row groups in a fixed order, then (thread 0) the record in the summary's
// order {entropy, mutual_info, total, rew_corr, gamma, alpha loss (nan: no learned temperature), alpha, mean pred}.
__global__ __launch_bounds__(256) void ipl_finalize_kernel(IplArgs a, int nblk, float* rec) {
    __shared__ double sp[4][IPL_SUMS + MAXA];
    __shared__ double tot[IPL_SUMS + MAXA];
    const int cols = IPL_SUMS + a.A;
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    if (c < cols) {
        double s = 0.0;
        for (int b = g; b < nblk; b += 4) s += a.partial[(long long)b * cols + c];
        sp[g][c] = s;
    }
    __syncthreads();
    if (g == 0 && c < cols) tot[c] = ((sp[0][c] + sp[1][c]) + sp[2][c]) + sp[3][c];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double ig = (double)a.inv_n_global, n = (double)a.n;
    const double mse = tot[0] * ig, mpred = tot[1] * ig, ent = tot[6] * ig, mmax = tot[7] * ig;
    double marg = 0.0;
    for (int k = 0; k < a.A; ++k) { const float q = (float)(tot[IPL_SUMS + k] * ig); marg -= (double)(q * logf(q)); }      // (no epsilon: misc_util.py:46-48)
    double total = mse;
    if (a.reward_incentive) total -= mpred;
    if (a.adv_incentive) total -= mmax;
    total += (double)a.entropy_coef * ent;
    // Pearson's r from the fp64 sums (torch.corrcoef; the n - 1 factors cancel)
    const double cxy = n * tot[5] - tot[1] * tot[2], cxx = n * tot[3] - tot[1] * tot[1], cyy = n * tot[4] - tot[2] * tot[2];
    double corr = cxy / sqrt(cxx * cyy);
    corr = corr > 1.0 ? 1.0 : (corr < -1.0 ? -1.0 : corr);                       // (corrcoef clips to [-1, 1]; NaN stays NaN)
    rec[0] = (float)ent; rec[1] = (float)(marg - ent); rec[2] = (float)total; rec[3] = (float)corr;
    rec[4] = a.gamma; rec[5] = __uint_as_float(0x7fc00000u); rec[6] = a.alpha; rec[7] = (float)mpred;
}

// seed of the second backward pass: zeros in the A logit columns, g_next in the value column
__global__ __launch_bounds__(256) void ipl_next_seed_kernel(const float* g_next, float* dY, int n, int A) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * (A + 1)) return;
    const int s = (int)(i / (A + 1)), k = (int)(i - (long long)s * (A + 1));
    dY[i] = (k == A) ? g_next[s] : 0.f;
}

// idx2[i] = idx[i] + shift: ring row of obs[t + 1] of the sample at ring row idx[i] (shift = E)
__global__ __launch_bounds__(256) void ipl_shift_idx_kernel(const int32_t* idx, int32_t* idx2, int n, int shift) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx2[i] = idx[i] + shift;
}

// IPL.predict(greedy=True) (IPL.py:86-90): probs.argmax(-1) = the first maximum of the normalised log-probabilities; its log-prob and
// the value go out with it
__global__ __launch_bounds__(64) void ipl_greedy_kernel(const float* hout, int n, int A, int32_t* act, float* logp, float* value) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    const float* h = hout + (long long)s * (A + 1);
    float z[MAXA], lp[MAXA], p[MAXA], lse_unused = 0.f;
#pragma unroll
    for (int k = 0; k < MAXA; ++k) z[k] = (k < A) ? h[k] : 0.f;
    log_softmax_twice_t<false>(z, A, lp, p, lse_unused, nullptr);
    float mx = lp[0];              // (on the log-probabilities, as the loss's max term: exp is monotone, so this is probs' first maximum
    int kmax = 0;                  // unless two distinct log-probs round to one probability)
#pragma unroll
    for (int k = 1; k < MAXA; ++k) if (k < A && lp[k] > mx) { mx = lp[k]; kmax = k; }
    act[s] = kmax; logp[s] = mx; value[s] = h[A];
}

void launch_ipl_next_value(const IplArgs& a, const float* v_src, int v_stride, int v_off, hipStream_t st) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(ipl_next_value_kernel, dim3(ipl_blocks(a.n)), dim3(IPL_BLK), 0, st, a, v_src, v_stride, v_off);
}
void launch_ipl_loss(const IplArgs& a, float* rec8, hipStream_t st) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(ipl_loss_kernel, dim3(ipl_blocks(a.n)), dim3(IPL_BLK), 0, st, a);
    hipLaunchKernelGGL(ipl_finalize_kernel, dim3(1), dim3(256), 0, st, a, ipl_blocks(a.n), rec8);
}
void launch_ipl_next_seed(const float* g_next, float* dY, int n, int A, hipStream_t st) {
    if (n <= 0) return;
    const long long tot = (long long)n * (A + 1);
    hipLaunchKernelGGL(ipl_next_seed_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, g_next, dY, n, A);
}
void launch_ipl_shift_idx(const int32_t* idx, int32_t* idx2, int n, int shift, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ipl_shift_idx_kernel, dim3((n + 255) / 256), dim3(256), 0, st, idx, idx2, n, shift);
}
void launch_ipl_greedy(const float* hout, int n, int A, int32_t* act, float* logp, float* value, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ipl_greedy_kernel, dim3((n + 63) / 64), dim3(64), 0, st, hout, n, A, act, logp, value);
}
