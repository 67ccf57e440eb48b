// The PPO loss per sample and the finalisation of a segment's statistics (agents/ppo.py:131-169 with cross_batch_entropy,
// common/misc_util.py:42-51): the device functions shared by the loss kernels (loss.hip) and the fused MLP minibatch pass
// (mlp_fused.hip).  Device code only: include it from .hip files; LossArgs is in common.h.
#pragma once
#include "common.h"
#include "policy_math.h"
#include <math.h>

// agents/ppo.py:131-169 + cross_batch_entropy (common/misc_util.py:42-51), forward statistics and
// the analytic gradient wrt (logits, value).  One thread per sample; A <= 16.
struct SampleTerms {
    float lp[MAXA], p[MAXA];
    float q1[MAXA];           // value_from_logits only: softmax of the raw logits (the FIRST normalisation) = d logsumexp / d logit
    float H, ratio, adv, surr1, surr2, v, oldv, ret, vclip, vs1, vs2;
    int act;
};
template <bool LSE>
__device__ __forceinline__ void sample_terms(const LossArgs& a, int s, SampleTerms& t) {
    const float* h = a.hout + (long long)s * (a.A + 1);
    float z[MAXA];
#pragma unroll
    for (int k = 0; k < MAXA; ++k) z[k] = (k < a.A) ? h[k] : 0.f;
    float lse = 0.f;
    log_softmax_twice_t<LSE>(z, a.A, t.lp, t.p, lse, t.q1);
    const int gi = a.idx[s];
    t.act = a.act[gi];
    t.adv = a.adv[gi]; t.ret = a.ret[gi]; t.oldv = a.old_value[gi];
    t.v = LSE ? lse : h[a.A];       // LSE: column A (fc_value's output) is not part of the model's value
    float H = 0.f, lp_act = 0.f;
#pragma unroll
    for (int k = 0; k < MAXA; ++k) if (k < a.A) { H -= t.p[k] * t.lp[k]; lp_act = (k == t.act) ? t.lp[k] : lp_act; }
    t.H = H;
    t.ratio = expf(lp_act - a.old_logp[gi]);
    t.surr1 = t.ratio * t.adv;
    t.surr2 = fminf(fmaxf(t.ratio, 1.f - a.hp.eps_clip), 1.f + a.hp.eps_clip) * t.adv;
    t.vclip = t.oldv + fminf(fmaxf(t.v - t.oldv, -a.hp.eps_clip), a.hp.eps_clip);
    t.vs1 = (t.v - t.ret) * (t.v - t.ret);
    t.vs2 = (t.vclip - t.ret) * (t.vclip - t.ret);
}

// LSE: the value-loss gradient enters the logits through d v / d logit_k = q1[k]; the value column of dY is zero, which makes fc_value's
// weight and bias gradient exact zeros in the heads' backward.
template <bool LSE>
__device__ __forceinline__ void loss_bwd_sample(const LossArgs& a, int s, const SampleTerms& t) {
    const float ib = a.inv_n_global;
    const float dvl = t.v - t.oldv;
    const float inr = (dvl >= -a.hp.eps_clip && dvl <= a.hp.eps_clip) ? 1.f : 0.f;
    float gv;
    if (t.vs1 > t.vs2) gv = 2.f * (t.v - t.ret);
    else if (t.vs2 > t.vs1) gv = 2.f * (t.vclip - t.ret) * inr;
    else gv = (t.v - t.ret) + (t.vclip - t.ret) * inr;
    const float gvc = a.hp.value_coef * 0.5f * ib * gv;
    // d pi_loss / d logp_act  (torch.min routes to surr1 on <=; a tie is the unclipped regime where both
    // branches carry adv/2 each; clamp passes gradient inside [1-eps, 1+eps])
    const float g_lp = -ib * ((t.surr1 <= t.surr2) ? t.adv : 0.f) * t.ratio;
    const float cH = (-a.hp.entropy_coef * a.hp.entropy_mult + a.hp.x_entropy_coef) * ib;
    float plq = 0.f;
    float lq[MAXA];
    const bool xe = a.hp.x_entropy_coef != 0.f;
    if (xe) {
#pragma unroll
        for (int k = 0; k < MAXA; ++k) if (k < a.A) { lq[k] = logf(a.stats[8 + k]); plq += t.p[k] * lq[k]; }
    }
    float* d = a.dY + (long long)s * (a.A + 1);
#pragma unroll
    for (int k = 0; k < MAXA; ++k) if (k < a.A) {
        float gk = g_lp * ((k == t.act ? 1.f : 0.f) - t.p[k]);
        gk += cH * (-t.p[k] * (t.lp[k] + t.H));
        if (xe) gk += a.hp.x_entropy_coef * ib * t.p[k] * (lq[k] - plq);
        if (LSE) gk += gvc * t.q1[k];
        d[k] = gk;
    }
    d[a.A] = LSE ? 0.f : gvc;
}

// phase 1: block partials -> this rank's contribution to the GLOBAL-minibatch means (x inv_n_global)
// phase 2: (after the optional cross-rank sum of stats[0..2], stats[8..8+A)) derived terms + log record
__device__ __forceinline__ void loss_finalize_body(const LossArgs& a, int nblk, int phase, const float* fs_ptr, float* log_slot) {
    const int k = threadIdx.x;
    if (phase & 1) {
        // column c of the partial rows, summed by blockDim.x / 32 row groups (rows g, g + G, ...) and then over the groups in order
        // (one thread per column walking all rows serially took 29 us for the 128 rows of an 8192-sample minibatch)
        __shared__ float sp[8][32];
        const int c = k & 31, g = k >> 5, G = blockDim.x >> 5;
        const bool col = c < 3 || (c >= 8 && c < 8 + a.A);
        float s = 0.f;
        if (col && g < 8) for (int b = g; b < nblk; b += G) s += a.partial[(long long)b * (8 + a.A) + c];
        if (g < 8) sp[g][c] = s;
        __syncthreads();
        if (g == 0 && col) {
            float t = sp[0][c];
            for (int j = 1; j < (G < 8 ? G : 8); ++j) t += sp[j][c];
            t *= a.inv_n_global;
            if (c == 0) t = -t;            // pi_loss = -mean(min(surr1,surr2))
            if (c == 1) t = 0.5f * t;      // value_loss = 0.5*mean(max(..))
            a.stats[c] = t;
        }
        __syncthreads();
    }
    if ((phase & 2) && k == 0) {
        float marg = 0.f;
        for (int j = 0; j < a.A; ++j) { const float qj = a.stats[8 + j]; marg -= qj * logf(qj); }
        const float ent = a.stats[2], xent = marg - ent;
        const float fs = fs_ptr ? fs_ptr[0] : 0.f;
        const float total = a.stats[0] + a.hp.value_coef * a.stats[1] - a.hp.entropy_coef * ent * a.hp.entropy_mult
                            - a.hp.x_entropy_coef * xent + a.hp.fs_coef * fs;
        a.stats[3] = xent; a.stats[4] = total; a.stats[5] = fs; a.stats[6] = marg;
        if (log_slot) {
            log_slot[0] = a.stats[0]; log_slot[1] = a.stats[1]; log_slot[2] = ent; log_slot[3] = xent;
            log_slot[4] = total; log_slot[5] = fs; log_slot[6] = marg; log_slot[7] = 0.f;
        }
    }
}
