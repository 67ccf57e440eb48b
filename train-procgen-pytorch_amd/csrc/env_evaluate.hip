// The evaluation of a policy on a device-resident env as ONE kernel (mi_env_evaluate in include/mi355ppo.h): every env runs exactly K whole
// episodes and the per-episode accounting stays on the device.  The skeleton is the resident rollout's (env_resident.hip): a workgroup takes
// RES_R = 16 envs (one MFMA M tile) and never talks to another workgroup -- no grid barrier, no spin wait, no atomics; the step loop is
// bounded by K * max_steps (an episode ends after max_steps steps at the latest) and a workgroup leaves it once its envs are done.
// gfx950 only.
//
// Per step: float(state) -> LDS; the MLP and the heads in fp32 on v_mfma_f32_16x16x4_f32 through res_layer (res_layer.h), activations
// ping-ponging between two LDS buffers, weights streamed from global memory; the sampler's row arithmetic (policy_math.h) or, in greedy
// mode, the first maximum of the same log-probabilities; the env step (env_physics.h: Env::advance / Env::fresh unchanged, fp64, contraction
// off) by the 16 threads that own an env.
//
// What differs from the rollout kernel: nothing of the context's training state is read or written -- not the env's state / n_steps /
// episode, not a ring.  Episode i (0 .. K - 1) of env e starts at Env::fresh(p, env_seed, e, F + i) or at the caller's row starts[e][i];
// step index t counts an env's steps since the launch began, which IS the loop index because every unfinished env steps every iteration,
// and the sampler's uniform is philox_uniform(seed, t * E + e) as in the rollout.  The owning thread writes one record per (e, i) with
// plain stores.  An env that has finished feeds zeros through the tile and stores nothing more; rows >= E of the tail tile do so from
// the start.
#include "engine_ctx.h"
#include "policy_math.h"
#include "env_physics.h"
#include "device_util.h"
#include "res_layer.h"      // RES_THREADS, RES_LD, RES_ZLD and res_layer, the layer of a 16-row tile

// the fp64 return of an episode: rewards added in step order, each addition rounded on its own (never fused with the reward's last multiply)
__device__ __forceinline__ double eval_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

// The greedy action of a row: the FIRST maximum of the normalised log-probabilities lp[0 .. A) -> its index.  ipl_greedy_kernel's rule
// (ipl.hip; IPL.predict(greedy=True) = probs.argmax(-1)), restated here: that kernel and policy_math.h stay as they are, text and assembly.
__device__ __forceinline__ int first_argmax(const float* lp, int A) {
    float mx = lp[0];
    int kmax = 0;
#pragma unroll
    for (int k = 1; k < MAXA; ++k) if (k < A && lp[k] > mx) { mx = lp[k]; kmax = k; }
    return kmax;
}

template <typename Env, bool LSE, bool GREEDY>
__global__ __launch_bounds__(RES_THREADS) void env_evaluate_kernel(typename Env::Args p, ResidentNet net, EvalRecords rec, unsigned long long env_seed,
                                                                   long long first_episode, unsigned long long seed, int E, int K) {
    constexpr int W = Env::W, A = Env::A;
    __shared__ __attribute__((aligned(16))) float s_x[2][RES_R * RES_LD];
    __shared__ float s_z[RES_R * RES_ZLD];
    __shared__ int s_in[RES_MAX_LAYERS], s_out[RES_MAX_LAYERS], s_vec[RES_MAX_LAYERS];
    __shared__ long long s_w[RES_MAX_LAYERS], s_b[RES_MAX_LAYERS];
    __shared__ int s_running;      // the workgroup's exit decision of a step: written by wave 0, read by everybody behind a barrier
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
    double s[W], ret = 0.0;
    int ns = 0, i = 0;      // steps of the running episode, episodes finished
    // the start of episode i: the planted row or the reset stream's episode F + i; it goes into the record at once
    auto begin_episode = [&]() {
        const size_t r = (size_t)e * (size_t)K + (size_t)i;
        if (rec.starts) {
#pragma unroll
            for (int j = 0; j < W; ++j) s[j] = rec.starts[r * W + j];
        } else {
            Env::fresh(p, env_seed, e, first_episode + (long long)i, s);
        }
#pragma unroll
        for (int j = 0; j < W; ++j) rec.start[r * W + j] = s[j];
    };
#pragma unroll
    for (int j = 0; j < W; ++j) s[j] = 0.0;
    if (live) begin_episode();
    const int L = net.n_layers;
    const int n_iter = K * p.max_steps;      // (the entry refuses a product above 2^20)
    for (int t = 0; t < n_iter; ++t) {
        bool running = live && i < K;
        if (owner) {
            float* x = s_x[0] + tid * RES_LD;
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = (j < W && running) ? (float)s[j < W ? j : 0] : 0.f;      // K tail zero-padded in LDS; a finished env: zeros
        }
        __syncthreads();
        for (int l = 0; l < L; ++l) {
            res_layer(net.params + s_w[l], net.params + s_b[l], s_in[l], s_out[l], s_vec[l] != 0, l + 1 < L, s_x[l & 1], s_x[(l + 1) & 1], RES_LD,
                      wave, lane);
            __syncthreads();
        }
        res_layer(net.params + net.wh_off, net.params + net.bh_off, net.H, A + 1, net.heads_vec != 0, false, s_x[L & 1], s_z, RES_ZLD, wave, lane);
        __syncthreads();
        if (running) {
            const size_t r = (size_t)e * (size_t)K + (size_t)i;
            float z[MAXA], lp[MAXA], pr[MAXA], q1[MAXA];
#pragma unroll
            for (int k = 0; k < MAXA; ++k) z[k] = (k < A) ? s_z[tid * RES_ZLD + (k < A ? k : 0)] : 0.f;
            float lse = 0.f;
            log_softmax_twice_t<LSE>(z, A, lp, pr, lse, q1);
            if (ns == 0) rec.value0[r] = LSE ? lse : s_z[tid * RES_ZLD + A];      // the value head at the episode's first observation
            int a_sel = 0;
            if (GREEDY) {
                a_sel = first_argmax(lp, A);
            } else {
                // the rollout's rule: inverse CDF on the Philox uniform of t * E + e
                const float uu = philox_uniform(seed, (unsigned long long)t * (unsigned long long)E + (unsigned long long)e);
                float cdf = 0.f;
#pragma unroll
                for (int k = 0; k < MAXA; ++k) if (k < A) { cdf += expf(lp[k]); if (cdf <= uu) a_sel = k + 1; }
                if (a_sel > A - 1) a_sel = A - 1;
            }
            // env_step_kernel's body on the registers, with the episode's accounting instead of the rings
            double reward;
            const bool terminated = Env::advance(p, s, a_sel, &reward);
            ns += 1;
            ret = eval_add(ret, reward);
            if (terminated || ns >= p.max_steps) {
                rec.ret[r] = ret;
                rec.length[r] = ns;
                rec.terminated[r] = terminated ? 1 : 0;      // (advance's own flag: a truncation has 0)
                i += 1;
                ns = 0;
                ret = 0.0;
                if (i < K) begin_episode();
            }
            running = i < K;
        }
        // The exit is workgroup-uniform: wave 0 (it holds every owner) publishes whether any of its envs still runs, everybody reads the
        // word behind the barrier, and its next write lies behind the barriers of the next step.  (The next step's first LDS write, the
        // observation into s_x[0], comes from the threads that have just read s_z; every other wave touches those buffers again only
        // behind the next barrier.)
        if (wave == 0) {
            const bool any = __ballot(running) != 0ull;
            if (lane == 0) s_running = any ? 1 : 0;
        }
        __syncthreads();
        if (!s_running) break;
    }
}

template <typename Env>
void env_evaluate(const DeviceEnv& d, const ResidentNet& net, const EvalRecords& rec, int E, int K, long long first_episode,
                  unsigned long long seed, bool greedy, hipStream_t st) {
    const dim3 grid((unsigned)((E + RES_R - 1) / RES_R)), block(RES_THREADS);
#define EVAL_LAUNCH(LSE, GREEDY)                                                                                                     \
    hipLaunchKernelGGL((env_evaluate_kernel<Env, LSE, GREEDY>), grid, block, 0, st, Env::args(d), net, rec, d.seed, first_episode, seed, E, K)
    if (net.lse) { if (greedy) EVAL_LAUNCH(true, true); else EVAL_LAUNCH(true, false); }
    else { if (greedy) EVAL_LAUNCH(false, true); else EVAL_LAUNCH(false, false); }
#undef EVAL_LAUNCH
}
template void env_evaluate<CartPole>(const DeviceEnv&, const ResidentNet&, const EvalRecords&, int, int, long long, unsigned long long, bool, hipStream_t);
template void env_evaluate<CartPoleSwing>(const DeviceEnv&, const ResidentNet&, const EvalRecords&, int, int, long long, unsigned long long, bool, hipStream_t);
template void env_evaluate<MountainCar>(const DeviceEnv&, const ResidentNet&, const EvalRecords&, int, int, long long, unsigned long long, bool, hipStream_t);
