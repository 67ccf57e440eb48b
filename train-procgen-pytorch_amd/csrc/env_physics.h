// The physics of the device-resident envs, shared by their translation units (env_device.hip: the step / reset kernels and the mi_env_*
// entries; env_resident.hip: the one-launch rollout; env_evaluate.hip: the one-launch evaluation).  An env is a physics struct (CartPole, CartPoleSwing, MountainCar): `Args` (its kernel arguments),
// `W` (state columns = observation width), `A` (actions), `args(DeviceEnv)` (its member of the context's union) and two device functions
//     fresh(p, seed, e, episode, s)         the start of episode `episode` of env e into s[W]
//     advance(p, s, act, &reward) -> ended  one step on s[W] in the host env's operation order; reward of this step
// fp contraction is off in every function that does env arithmetic (the pragma is lexically scoped): each operation rounds as numpy's
// separate array operations do.  Device code only.
#pragma once
#include "engine_ctx.h"
#include "policy_math.h"

// low + (high - low) * u per column (start_space of the reference's pre-vectorised envs).  The stream is the device env's own:
// Philox4x32-10 keyed by the env's seed, counter {e, episode lo, episode hi, block0 + b}, b = 0 .. (W + 1) / 2 - 1 = two 53-bit
// uniforms each (columns 2b and 2b + 1 from words {0, 1} and {2, 3}; an odd W leaves the last two words unused).  The host envs draw
// whole numpy blocks whenever any env ends; that is not reproduced.
template <int W, typename Args>
__device__ __forceinline__ void env_draw(const Args& p, unsigned long long seed, int e, long long episode, int block0, double* s) {
#pragma clang fp contract(off)
#pragma unroll
    for (int b = 0; b < (W + 1) / 2; ++b) {
        uint32_t c[4] = {(uint32_t)e, (uint32_t)(unsigned long long)episode, (uint32_t)((unsigned long long)episode >> 32), (uint32_t)(block0 + b)};
        uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
        philox4x32_10(c, k);
        s[2 * b] = p.low[2 * b] + (p.high[2 * b] - p.low[2 * b]) * philox_u53(c[0], c[1]);
        if (2 * b + 1 < W) s[2 * b + 1] = p.low[2 * b + 1] + (p.high[2 * b + 1] - p.low[2 * b + 1]) * philox_u53(c[2], c[3]);
    }
}

// The Euler step of Florian's cart-pole equations with the per-env parameters (tau = 0.02), in CartPoleVec.step's operation order: what
// the cart-pole and the swing-up share.  Advances the four dynamic columns of s[9] in place.
__device__ __forceinline__ void cartpole_euler(double* s, int act) {
#pragma clang fp contract(off)
    const double x = s[0], xd = s[1], th = s[2], thd = s[3], g = s[4], length = s[5], m_cart = s[6], m_pole = s[7], f_mag = s[8];
    const double tau = 0.02;
    const double force = (act == 0 ? -1.0 : 1.0) * f_mag;
    const double ct = cos(th), st = sin(th);
    const double pml = m_pole * length, total = m_pole + m_cart;
    const double temp = (force + (pml * (thd * thd)) * st) / total;
    const double thacc = (g * st - ct * temp) / (length * (4.0 / 3.0 - (m_pole * (ct * ct)) / total));
    const double xacc = temp - ((pml * thacc) * ct) / total;
    s[0] = x + tau * xd; s[1] = xd + tau * xacc; s[2] = th + tau * thd; s[3] = thd + tau * thacc;
}

// CartPoleVec (the reference's discrete_env/cartpole_pre_vec.py:214-262 on pre_vec_env.py:86-118): blocks 0..4 of an episode's
// counters (18 words needed, 20 drawn); reward 1 every step.
struct CartPole {
    using Args = CartPoleArgs;
    static constexpr int W = 9, A = 2;
    static const Args& args(const DeviceEnv& d) { return d.args.cp; }
    static __device__ __forceinline__ void fresh(const Args& p, unsigned long long seed, int e, long long episode, double* s) {
        env_draw<W>(p, seed, e, episode, 0, s);
    }
    static __device__ __forceinline__ bool advance(const Args& p, double* s, int act, double* reward) {
#pragma clang fp contract(off)
        cartpole_euler(s, act);
        *reward = 1.0;
        return (s[0] < -p.x_threshold) | (s[0] > p.x_threshold) | (s[2] < -p.theta_threshold) | (s[2] > p.theta_threshold);
    }
};

// CartPoleSwingVec (discrete_env/cartpole_swing_pre_vec.py:195-239): the cart-pole's dynamics and start stream (the pole hangs down:
// theta starts around pi, which is a matter of `low` / `high` alone), termination beyond +-x_threshold only -- no angle threshold --
// and the reward of the post-step, pre-reset state: max(cos(theta), 0) * cos((x / x_threshold) * (pi / 2)).  The clamp is numpy's
// `rt[rt < 0] = 0` (a NaN stays); a row that ends with the clamp on has cos(..) < 0 and yields -0.0, as on the host.
struct CartPoleSwing {
    using Args = CartPoleSwingArgs;
    static constexpr int W = 9, A = 2;
    static const Args& args(const DeviceEnv& d) { return d.args.cs; }
    static __device__ __forceinline__ void fresh(const Args& p, unsigned long long seed, int e, long long episode, double* s) {
        env_draw<W>(p, seed, e, episode, 0, s);
    }
    static __device__ __forceinline__ bool advance(const Args& p, double* s, int act, double* reward) {
#pragma clang fp contract(off)
        cartpole_euler(s, act);
        double rt = cos(s[2]);
        rt = rt < 0.0 ? 0.0 : rt;
        const double rx = cos((s[0] / p.x_threshold) * (3.141592653589793 / 2.0));
        *reward = rt * rx;
        return (s[0] < -p.x_threshold) | (s[0] > p.x_threshold);
    }
};

// MountainCarVec (discrete_env/mountain_car_pre_vec.py:194-209 on pre_vec_env.py:78-118).  The start is drawn again while
// goal_position > right_boundary (StartSpace.sample's condition, helper_pre_vec.py:28-38): attempt a uses blocks 3a .. 3a + 2 (10 words
// needed, 12 drawn).  The loop is BOUNDED: after MC_MAX_ATTEMPTS rejected attempts the last draw is kept with goal_position =
// right_boundary.  The host refuses range sets that accept a draw with probability below 1/2, so that happens with probability at most
// 2^-32 per reset.  The velocity column has low == high == 0: 0 + 0 * u = 0 exactly.  The clips of the step are numpy's
// minimum(maximum(x, lo), hi), the wall test an exact ==; the reward is that of the post-step, pre-reset position.
#define MC_MAX_ATTEMPTS 32
struct MountainCar {
    using Args = MountainCarArgs;
    static constexpr int W = 5, A = 3;
    static const Args& args(const DeviceEnv& d) { return d.args.mc; }
    static __device__ __forceinline__ void fresh(const Args& p, unsigned long long seed, int e, long long episode, double* s) {
        bool ok = false;
        for (int attempt = 0; attempt < MC_MAX_ATTEMPTS && !ok; ++attempt) {
            env_draw<W>(p, seed, e, episode, 3 * attempt, s);
            ok = !(s[4] > s[3]);
        }
        if (!ok) s[4] = s[3];
    }
    static __device__ __forceinline__ bool advance(const Args& p, double* s, int act, double* reward) {
#pragma clang fp contract(off)
        double pos = s[0], vel = s[1];
        const double gravity = s[2], right = s[3], goal = s[4];
        vel = vel + ((double)(act - 1) * p.force + cos(3.0 * pos) * (-gravity));
        vel = vel < -p.max_speed ? -p.max_speed : vel;
        vel = vel > p.max_speed ? p.max_speed : vel;
        pos = pos + vel;
        pos = pos < p.left_boundary ? p.left_boundary : pos;
        pos = pos > right ? right : pos;
        if (pos == p.left_boundary && vel < 0.0) vel = 0.0;
        const bool ended = (pos >= goal) & (vel >= p.goal_velocity);
        *reward = p.sparse_rewards ? -1.0 : sin(3.0 * pos) * 0.45 + 0.55 - 1.0;
        s[0] = pos; s[1] = vel;
        return ended;
    }
};

// the one-launch rollout of an env (env_resident.hip instantiates it for every struct; env_device.hip puts it into the env's table row)
template <typename Env>
MI_INTERNAL void env_rollout_resident(const DeviceEnv& d, const ResidentNet& net, const ResidentRings& ring, int E, int T, unsigned long long seed,
                                      hipStream_t st);
// the one-launch evaluation of an env, K whole episodes each (env_evaluate.hip instantiates it likewise)
template <typename Env>
MI_INTERNAL void env_evaluate(const DeviceEnv& d, const ResidentNet& net, const EvalRecords& rec, int E, int K, long long first_episode,
                              unsigned long long seed, bool greedy, hipStream_t st);
