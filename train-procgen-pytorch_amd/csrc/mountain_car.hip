// The device-resident mountain car (mi_env_mountain_car_create / mi_env_rollout): MountainCarVec (common/env/vec_envs.py; the reference's
// discrete_env/mountain_car_pre_vec.py:194-209 on pre_vec_env.py:78-118) with state, dynamics, termination, episode resets, reward and
// done in HBM.  One thread per env, fp64, no LDS, no atomics; a dozen floating-point operations and one cos (dense rewards: one sin) per
// env and step -- as for the cart-pole the point is that a rollout needs no host round trip.  gfx950 only.
#include "common.h"
#include "policy_math.h"

#define MC_MAX_ATTEMPTS 32

// The start of episode `episode` of env e: low + (high - low) * u per column (start_space, mountain_car_pre_vec.py:158-161), drawn again
// while goal_position > right_boundary (StartSpace.sample's condition, helper_pre_vec.py:28-38).  The stream is the device env's own:
// Philox4x32-10 keyed by the env's seed, counter {e, episode lo, episode hi, 3 * attempt + b}, b = 0..2 = two uniforms each (columns 2b
// and 2b + 1 from words {0, 1} and {2, 3}; 10 words needed, 12 drawn).  The loop is BOUNDED: after MC_MAX_ATTEMPTS rejected attempts the
// last draw is kept with goal_position = right_boundary.  The host refuses range sets that accept a draw with probability below 1/2,
// so that happens with probability at most 2^-32 per reset.  The velocity column has low == high == 0: 0 + 0 * u = 0 exactly.
__device__ __forceinline__ void mountain_car_fresh(const MountainCarArgs& p, unsigned long long seed, int e, long long episode, double* s) {
#pragma clang fp contract(off)
    bool ok = false;
    for (int attempt = 0; attempt < MC_MAX_ATTEMPTS && !ok; ++attempt) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            uint32_t c[4] = {(uint32_t)e, (uint32_t)(unsigned long long)episode, (uint32_t)((unsigned long long)episode >> 32), (uint32_t)(3 * attempt + b)};
            uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
            philox4x32_10(c, k);
            s[2 * b] = p.low[2 * b] + (p.high[2 * b] - p.low[2 * b]) * philox_u53(c[0], c[1]);
            if (2 * b + 1 < 5) s[2 * b + 1] = p.low[2 * b + 1] + (p.high[2 * b + 1] - p.low[2 * b + 1]) * philox_u53(c[2], c[3]);
        }
        ok = !(s[4] > s[3]);
    }
    if (!ok) s[4] = s[3];
}
__device__ __forceinline__ void mountain_car_store(const double* s, double* state_row, float* obs_row) {
#pragma unroll
    for (int j = 0; j < 5; ++j) { state_row[j] = s[j]; obs_row[j] = (float)s[j]; }
}

// MountainCarVec.step in its operation order (fp contraction off: every operation rounds as numpy's separate array operations do; the
// clips are numpy's minimum(maximum(x, lo), hi), the wall test an exact ==).  act: E actions in {0, 1, 2} (ring slot t); obs_next: E x 5
// (ring slot t + 1); rew / done: E each (ring slot t).  As on the host the reward is that of the post-step, pre-reset position, done is
// this step's termination flag and the stored observation is the post-reset state.
__global__ __launch_bounds__(64) void mountain_car_step_kernel(MountainCarArgs p, double* state, int32_t* n_steps, long long* episode,
                                                               const int32_t* act, unsigned long long seed, float* obs_next, float* rew,
                                                               float* done, int E) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    double s[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = state[(size_t)e * 5 + j];
    double pos = s[0], vel = s[1];
    const double gravity = s[2], right = s[3], goal = s[4];
    vel = vel + ((double)(act[e] - 1) * p.force + cos(3.0 * pos) * (-gravity));
    vel = vel < -p.max_speed ? -p.max_speed : vel;
    vel = vel > p.max_speed ? p.max_speed : vel;
    pos = pos + vel;
    pos = pos < p.left_boundary ? p.left_boundary : pos;
    pos = pos > right ? right : pos;
    if (pos == p.left_boundary && vel < 0.0) vel = 0.0;
    bool ended = (pos >= goal) & (vel >= p.goal_velocity);
    const double reward = p.sparse_rewards ? -1.0 : sin(3.0 * pos) * 0.45 + 0.55 - 1.0;
    s[0] = pos; s[1] = vel;
    int ns = n_steps[e] + 1;
    ended |= ns >= p.max_steps;
    if (ended) {
        const long long ep = episode[e] + 1;
        mountain_car_fresh(p, seed, e, ep, s);
        episode[e] = ep;
        ns = 0;
    }
    n_steps[e] = ns;
    mountain_car_store(s, state + (size_t)e * 5, obs_next + (size_t)e * 5);
    rew[e] = (float)reward;
    done[e] = ended ? 1.0f : 0.0f;
}

// every env starts a fresh episode (mi_env_reset): episode += 1, n_steps = 0, the state of that episode
__global__ __launch_bounds__(64) void mountain_car_reset_kernel(MountainCarArgs p, double* state, int32_t* n_steps, long long* episode,
                                                                unsigned long long seed, float* obs, int E) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    double s[5];
    const long long ep = episode[e] + 1;
    mountain_car_fresh(p, seed, e, ep, s);
    episode[e] = ep;
    n_steps[e] = 0;
    mountain_car_store(s, state + (size_t)e * 5, obs + (size_t)e * 5);
}

// float(state) into a ring slot: observation 0 of a rollout
__global__ __launch_bounds__(256) void mountain_car_emit_obs_kernel(const double* state, float* obs, int n /* E * 5 */) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) obs[k] = (float)state[k];
}

void launch_mountain_car_step(const MountainCarArgs& p, double* state, int32_t* n_steps, long long* episode, const int32_t* act,
                              unsigned long long seed, float* obs_next, float* rew, float* done, int E, hipStream_t st) {
    if (E <= 0) return;
    hipLaunchKernelGGL(mountain_car_step_kernel, dim3((E + 63) / 64), dim3(64), 0, st, p, state, n_steps, episode, act, seed, obs_next, rew, done, E);
}
void launch_mountain_car_reset(const MountainCarArgs& p, double* state, int32_t* n_steps, long long* episode, unsigned long long seed,
                               float* obs, int E, hipStream_t st) {
    if (E <= 0) return;
    hipLaunchKernelGGL(mountain_car_reset_kernel, dim3((E + 63) / 64), dim3(64), 0, st, p, state, n_steps, episode, seed, obs, E);
}
void launch_mountain_car_emit_obs(const double* state, float* obs, int E, hipStream_t st) {
    if (E <= 0) return;
    hipLaunchKernelGGL(mountain_car_emit_obs_kernel, dim3((E * 5 + 255) / 256), dim3(256), 0, st, state, obs, E * 5);
}
