// The device-resident cart-pole (mi_env_cartpole_create / mi_env_rollout): CartPoleVec (common/env/vec_envs.py; the reference's
// discrete_env/cartpole_pre_vec.py:214-262 on pre_vec_env.py:86-118) with state, physics, termination, episode resets, reward and
// done in HBM.  One thread per env, fp64, no LDS, no atomics; about thirty floating-point operations per env and step -- the point is
// not the arithmetic but that a rollout needs no host round trip.  gfx950 only.
#include "common.h"
#include "policy_math.h"

// The start of episode `episode` of env e: low + (high - low) * u per column (start_space, cartpole_pre_vec.py:163-171).  The stream is
// the device env's own: Philox4x32-10 keyed by the env's seed, counter {e, episode lo, episode hi, block}, block 0..4 = two uniforms each
// (18 words needed, 20 drawn).  CartPoleVec draws a whole (E, 9) numpy block whenever any env ends; that is not reproduced.
__device__ __forceinline__ void cartpole_fresh(const CartPoleArgs& p, unsigned long long seed, int e, long long episode, double* s) {
#pragma clang fp contract(off)
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        uint32_t c[4] = {(uint32_t)e, (uint32_t)(unsigned long long)episode, (uint32_t)((unsigned long long)episode >> 32), (uint32_t)b};
        uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
        philox4x32_10(c, k);
        s[2 * b] = p.low[2 * b] + (p.high[2 * b] - p.low[2 * b]) * philox_u53(c[0], c[1]);
        if (2 * b + 1 < 9) s[2 * b + 1] = p.low[2 * b + 1] + (p.high[2 * b + 1] - p.low[2 * b + 1]) * philox_u53(c[2], c[3]);
    }
}
__device__ __forceinline__ void cartpole_store(const double* s, double* state_row, float* obs_row) {
#pragma unroll
    for (int j = 0; j < 9; ++j) { state_row[j] = s[j]; obs_row[j] = (float)s[j]; }
}

// CartPoleVec.step in its operation order (fp contraction off: every operation rounds as numpy's separate array operations do).
// act: E actions (ring slot t); obs_next: E x 9 (ring slot t + 1); rew / done: E each (ring slot t).  As on the host, done is this
// step's termination flag and the stored observation is the post-reset state.
__global__ __launch_bounds__(64) void cartpole_step_kernel(CartPoleArgs p, double* state, int32_t* n_steps, long long* episode,
                                                           const int32_t* act, unsigned long long seed, float* obs_next, float* rew,
                                                           float* done, int E) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    double s[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) s[j] = state[(size_t)e * 9 + j];
    const double x = s[0], xd = s[1], th = s[2], thd = s[3], g = s[4], length = s[5], m_cart = s[6], m_pole = s[7], f_mag = s[8];
    const double tau = 0.02;
    const double force = (act[e] == 0 ? -1.0 : 1.0) * f_mag;
    const double ct = cos(th), st = sin(th);
    const double pml = m_pole * length, total = m_pole + m_cart;
    const double temp = (force + (pml * (thd * thd)) * st) / total;
    const double thacc = (g * st - ct * temp) / (length * (4.0 / 3.0 - (m_pole * (ct * ct)) / total));
    const double xacc = temp - ((pml * thacc) * ct) / total;
    s[0] = x + tau * xd; s[1] = xd + tau * xacc; s[2] = th + tau * thd; s[3] = thd + tau * thacc;
    bool ended = (s[0] < -p.x_threshold) | (s[0] > p.x_threshold) | (s[2] < -p.theta_threshold) | (s[2] > p.theta_threshold);
    int ns = n_steps[e] + 1;
    ended |= ns >= p.max_steps;
    if (ended) {
        const long long ep = episode[e] + 1;
        cartpole_fresh(p, seed, e, ep, s);
        episode[e] = ep;
        ns = 0;
    }
    n_steps[e] = ns;
    cartpole_store(s, state + (size_t)e * 9, obs_next + (size_t)e * 9);
    rew[e] = 1.0f;
    done[e] = ended ? 1.0f : 0.0f;
}

// every env starts a fresh episode (mi_env_reset): episode += 1, n_steps = 0, the state of that episode
__global__ __launch_bounds__(64) void cartpole_reset_kernel(CartPoleArgs p, double* state, int32_t* n_steps, long long* episode,
                                                            unsigned long long seed, float* obs, int E) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    double s[9];
    const long long ep = episode[e] + 1;
    cartpole_fresh(p, seed, e, ep, s);
    episode[e] = ep;
    n_steps[e] = 0;
    cartpole_store(s, state + (size_t)e * 9, obs + (size_t)e * 9);
}

// float(state) into a ring slot: observation 0 of a rollout
__global__ __launch_bounds__(256) void cartpole_emit_obs_kernel(const double* state, float* obs, int n /* E * 9 */) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) obs[k] = (float)state[k];
}

void launch_cartpole_step(const CartPoleArgs& p, double* state, int32_t* n_steps, long long* episode, const int32_t* act,
                          unsigned long long seed, float* obs_next, float* rew, float* done, int E, hipStream_t st) {
    if (E <= 0) return;
    hipLaunchKernelGGL(cartpole_step_kernel, dim3((E + 63) / 64), dim3(64), 0, st, p, state, n_steps, episode, act, seed, obs_next, rew, done, E);
}
void launch_cartpole_reset(const CartPoleArgs& p, double* state, int32_t* n_steps, long long* episode, unsigned long long seed, float* obs,
                           int E, hipStream_t st) {
    if (E <= 0) return;
    hipLaunchKernelGGL(cartpole_reset_kernel, dim3((E + 63) / 64), dim3(64), 0, st, p, state, n_steps, episode, seed, obs, E);
}
void launch_cartpole_emit_obs(const double* state, float* obs, int E, hipStream_t st) {
    if (E <= 0) return;
    hipLaunchKernelGGL(cartpole_emit_obs_kernel, dim3((E * 9 + 255) / 256), dim3(256), 0, st, state, obs, E * 9);
}
