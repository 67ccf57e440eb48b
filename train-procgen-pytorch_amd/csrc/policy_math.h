// The policy's per-sample arithmetic shared by the heads, the sampler, the loss and the saliency seeds: the twice-normalised
// log-softmax of CategoricalPolicy (common/policy.py:77-87) and the Philox4x32-10 uniform the rollout samples with.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#define MAXA 16
// (All loops over the actions run to the compile-time MAXA under `k < A`: with a run-time bound the per-thread arrays are indexed
// dynamically and live in scratch memory -- 180 B per thread, the loss kernel then took 35 us for 8192 samples.)
// LSE (mi_config.value_from_logits; common/policy.py:77-78, v = logits.logsumexp(-1)): also hands out lse = mx + log sum exp(z - mx) of
// the first pass and q1 = exp(z - lse), its softmax.  Off: lse / q1 are not touched and the code is the two-output form.
template <bool LSE>
__device__ __forceinline__ void log_softmax_twice_t(const float* z, int A, float* lp, float* p, float& lse_out, float* q1) {
    float mx = z[0];
#pragma unroll
    for (int a = 1; a < MAXA; ++a) if (a < A) mx = fmaxf(mx, z[a]);
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < MAXA; ++a) if (a < A) s += expf(z[a] - mx);
    const float lse = mx + logf(s);
    float s2 = 0.f;
#pragma unroll
    for (int a = 0; a < MAXA; ++a) if (a < A) { lp[a] = z[a] - lse; const float e1 = expf(lp[a]); s2 += e1; if (LSE) q1[a] = e1; }
    if (LSE) lse_out = lse;
    const float lse2 = logf(s2);                 // Categorical(logits=log_probs) normalises again (policy.py:86-87)
    float s3 = 0.f;
#pragma unroll
    for (int a = 0; a < MAXA; ++a) if (a < A) { lp[a] -= lse2; p[a] = expf(lp[a]); s3 += p[a]; }
#pragma unroll
    for (int a = 0; a < MAXA; ++a) if (a < A) p[a] /= s3;       // Categorical.probs = softmax(logits)
}

__device__ __forceinline__ void philox_round(uint32_t* c, uint32_t* k) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k[0], n2 = hi0 ^ c[3] ^ k[1];
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
}
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds on a 128-bit counter under a
// 64-bit key, the key bumped by the Weyl constants between rounds (the bump after the last round is unused).  Known-answer vectors
// of the Random123 distribution are checked through mi_debug_philox (tests/test_gpu_engine.py) and in oracle/philox.py.
__device__ __forceinline__ void philox4x32_10(uint32_t* c, uint32_t* k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) philox_round(c, k);
}
__device__ __forceinline__ float philox_uniform(unsigned long long seed, unsigned long long ctr) {
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    philox4x32_10(c, k);
    return (float)(c[0] >> 8) * (1.0f / 16777216.0f);     // [0,1), 24 bits
}
// 53-bit uniform in [0, 1) from two Philox words (the episode starts of the device-resident envs): every operation is exact in fp64
__device__ __forceinline__ double philox_u53(uint32_t w0, uint32_t w1) {
    return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) * (1.0 / 9007199254740992.0);
}
