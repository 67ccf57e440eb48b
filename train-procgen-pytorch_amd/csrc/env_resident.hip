// The device-env rollout as ONE resident kernel (mi_env_rollout_resident in include/mi355ppo.h; opt-in beside mi_env_rollout's chain of
// T + 1 policy steps and T env steps).  An env's next observation depends on its own action only, so the E envs are independent
// chains: a workgroup takes RES_R = 16 envs (one MFMA M tile) through all T + 1 policy steps and T env steps and never talks to another
// workgroup -- no grid barrier, no spin wait, no atomics; every loop is bounded by T, the layer count, the layer sizes and
// MC_MAX_ATTEMPTS.  gfx950 only.
//
// Per step: float(state) -> observation ring slot t and LDS; the MLP and the heads in fp32 on v_mfma_f32_16x16x4_f32 with the
// activations ping-ponging between two LDS buffers and the weights streamed from global memory (read-only for the whole launch, shared by
// all workgroups: they live in L2); the sampler's row arithmetic (policy_math.h) and the env step (env_physics.h, fp64, contraction
// off) by the 16 threads that own an env.  Bias and ReLU as forward_mlp / linear_fwd place them: ReLU after every layer but the last
// embedder layer, none in front of the heads.  The policy numbers differ from the chain's by the fp32 summation order of the dot
// products only; the env arithmetic is the chain's own functions.
#include "engine_ctx.h"
#include "policy_math.h"
#include "env_physics.h"
#include "device_util.h"
#include "res_layer.h"      // RES_THREADS, RES_LD, RES_ZLD and res_layer, the layer of a 16-row tile

template <typename Env, bool LSE>
__global__ __launch_bounds__(RES_THREADS) void env_rollout_resident_kernel(typename Env::Args p, ResidentNet net, ResidentRings ring, double* state,
                                                                           int32_t* n_steps, long long* episode, unsigned long long env_seed,
                                                                           unsigned long long seed, int E, int T) {
    constexpr int W = Env::W, A = Env::A;
    __shared__ __attribute__((aligned(16))) float s_x[2][RES_R * RES_LD];
    __shared__ float s_z[RES_R * RES_ZLD];
    __shared__ int s_in[RES_MAX_LAYERS], s_out[RES_MAX_LAYERS], s_vec[RES_MAX_LAYERS];
    __shared__ long long s_w[RES_MAX_LAYERS], s_b[RES_MAX_LAYERS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) {
#pragma unroll
        for (int l = 0; l < RES_MAX_LAYERS; ++l) {
            s_in[l] = net.in[l]; s_out[l] = net.out[l]; s_vec[l] = net.vec[l]; s_w[l] = net.w_off[l]; s_b[l] = net.b_off[l];
        }
    }
    // the thread's env (threads 0 .. 15 own one each; rows >= E of the tail tile compute on zeros and store nothing)
    const int e = blockIdx.x * RES_R + tid;
    const bool owner = tid < RES_R, live = owner && e < E;
    double s[W];
    int ns = 0;
    long long ep = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) s[j] = live ? state[(size_t)e * W + j] : 0.0;
    if (live) { ns = n_steps[e]; ep = episode[e]; }
    const int L = net.n_layers;
    for (int t = 0; t <= T; ++t) {
        const size_t row = (size_t)t * (size_t)E + (size_t)e;
        if (owner) {
            float* x = s_x[0] + tid * RES_LD;
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = (j < W) ? (float)s[j < W ? j : 0] : 0.f;      // K tail zero-padded in LDS
            if (live) {
#pragma unroll
                for (int j = 0; j < W; ++j) ring.obs[row * W + j] = (float)s[j];
            }
        }
        __syncthreads();
        for (int l = 0; l < L; ++l) {
            res_layer(net.params + s_w[l], net.params + s_b[l], s_in[l], s_out[l], s_vec[l] != 0, l + 1 < L, s_x[l & 1], s_x[(l + 1) & 1], RES_LD,
                      wave, lane);
            __syncthreads();
        }
        res_layer(net.params + net.wh_off, net.params + net.bh_off, net.H, A + 1, net.heads_vec != 0, false, s_x[L & 1], s_z, RES_ZLD, wave, lane);
        __syncthreads();
        if (live) {
            // the row arithmetic of sample_kernel (heads.hip): twice-normalised log-softmax, inverse CDF on the Philox uniform of t * E + e
            float z[MAXA], lp[MAXA], pr[MAXA], q1[MAXA];
#pragma unroll
            for (int k = 0; k < MAXA; ++k) z[k] = (k < A) ? s_z[tid * RES_ZLD + (k < A ? k : 0)] : 0.f;
            float lse = 0.f;
            log_softmax_twice_t<LSE>(z, A, lp, pr, lse, q1);
            ring.value[row] = LSE ? lse : s_z[tid * RES_ZLD + A];
            if (t < T) {
                const float uu = philox_uniform(seed, (unsigned long long)t * (unsigned long long)E + (unsigned long long)e);
                float cdf = 0.f;
                int a_sel = 0;
#pragma unroll
                for (int k = 0; k < MAXA; ++k) if (k < A) { cdf += expf(lp[k]); if (cdf <= uu) a_sel = k + 1; }
                if (a_sel > A - 1) a_sel = A - 1;
                float lp_sel = lp[0];
#pragma unroll
                for (int k = 1; k < MAXA; ++k) if (k < A) lp_sel = (k == a_sel) ? lp[k] : lp_sel;
                ring.act[row] = a_sel;
                ring.logp[row] = lp_sel;
                // env_step_kernel's body on the registers
                double reward;
                bool ended = Env::advance(p, s, a_sel, &reward);
                ns += 1;
                ended |= ns >= p.max_steps;
                if (ended) {
                    ep += 1;
                    Env::fresh(p, env_seed, e, ep, s);
                    ns = 0;
                }
                ring.rew[row] = (float)reward;
                ring.done[row] = ended ? 1.0f : 0.0f;
            }
        }
        // (the next step's first LDS write, the observation into s_x[0], comes from the threads that have just read s_z; every other
        // wave touches LDS again only behind the next barrier)
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < W; ++j) state[(size_t)e * W + j] = s[j];
        n_steps[e] = ns;
        episode[e] = ep;
    }
}

template <typename Env>
void env_rollout_resident(const DeviceEnv& d, const ResidentNet& net, const ResidentRings& ring, int E, int T, unsigned long long seed,
                          hipStream_t st) {
    const dim3 grid((unsigned)((E + RES_R - 1) / RES_R)), block(RES_THREADS);
    if (net.lse)
        hipLaunchKernelGGL((env_rollout_resident_kernel<Env, true>), grid, block, 0, st, Env::args(d), net, ring, d.state, d.nsteps, d.episode,
                           d.seed, seed, E, T);
    else
        hipLaunchKernelGGL((env_rollout_resident_kernel<Env, false>), grid, block, 0, st, Env::args(d), net, ring, d.state, d.nsteps, d.episode,
                           d.seed, seed, E, T);
}
template void env_rollout_resident<CartPole>(const DeviceEnv&, const ResidentNet&, const ResidentRings&, int, int, unsigned long long, hipStream_t);
template void env_rollout_resident<CartPoleSwing>(const DeviceEnv&, const ResidentNet&, const ResidentRings&, int, int, unsigned long long, hipStream_t);
template void env_rollout_resident<MountainCar>(const DeviceEnv&, const ResidentNet&, const ResidentRings&, int, int, unsigned long long, hipStream_t);
