// The device-resident envs (mi_env_* in include/mi355ppo.h): the numpy vector envs of common/env/vec_envs.py with state, physics,
// termination, episode resets, reward and done in HBM.  One thread per env, fp64, no LDS, no atomics; a few dozen floating-point
// operations per env and step -- the point is not the arithmetic but that a rollout needs no host round trip.  gfx950 only.
//
// An env is a physics struct (CartPole, CartPoleSwing, MountainCar): `Args` (its kernel arguments), `W` (state columns = observation width), `A`
// (actions), `args(DeviceEnv)` (its member of the context's union) and two device functions
//     fresh(p, seed, e, episode, s)         the start of episode `episode` of env e into s[W]
//     advance(p, s, act, &reward) -> ended  one step on s[W] in the host env's operation order; reward of this step
// The kernels, the launchers, the create checks and every other mi_env_* entry are shared: they reach an env through its table row
// (EnvOps, below) alone.  fp contraction is off in every function that does env arithmetic (the pragma is lexically scoped): each operation
// rounds as numpy's separate array operations do.
#include "engine_ctx.h"
#include "policy_math.h"
#include "env_physics.h"

template <int W>
__device__ __forceinline__ void env_store(const double* s, double* state_row, float* obs_row) {
#pragma unroll
    for (int j = 0; j < W; ++j) { state_row[j] = s[j]; obs_row[j] = (float)s[j]; }
}

// One step of every env.  act: E actions (ring slot t); obs_next: E x W (ring slot t + 1); rew / done: E each (ring slot t).  As on the
// host, done is this step's termination flag (truncation at max_steps included) and the stored observation is the post-reset state.
template <typename Env>
__global__ __launch_bounds__(64) void env_step_kernel(typename Env::Args p, double* state, int32_t* n_steps, long long* episode,
                                                      const int32_t* act, unsigned long long seed, float* obs_next, float* rew,
                                                      float* done, int E) {
    constexpr int W = Env::W;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    double s[W], reward;
#pragma unroll
    for (int j = 0; j < W; ++j) s[j] = state[(size_t)e * W + j];
    bool ended = Env::advance(p, s, act[e], &reward);
    int ns = n_steps[e] + 1;
    ended |= ns >= p.max_steps;
    if (ended) {
        const long long ep = episode[e] + 1;
        Env::fresh(p, seed, e, ep, s);
        episode[e] = ep;
        ns = 0;
    }
    n_steps[e] = ns;
    env_store<W>(s, state + (size_t)e * W, obs_next + (size_t)e * W);
    rew[e] = (float)reward;
    done[e] = ended ? 1.0f : 0.0f;
}

// every env starts a fresh episode (mi_env_reset): episode += 1, n_steps = 0, the state of that episode
template <typename Env>
__global__ __launch_bounds__(64) void env_reset_kernel(typename Env::Args p, double* state, int32_t* n_steps, long long* episode,
                                                       unsigned long long seed, float* obs, int E) {
    constexpr int W = Env::W;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    double s[W];
    const long long ep = episode[e] + 1;
    Env::fresh(p, seed, e, ep, s);
    episode[e] = ep;
    n_steps[e] = 0;
    env_store<W>(s, state + (size_t)e * W, obs + (size_t)e * W);
}

// float(state) into a ring slot: observation 0 of a rollout
__global__ __launch_bounds__(256) void env_emit_obs_kernel(const double* state, float* obs, int n /* E * W */) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) obs[k] = (float)state[k];
}

template <typename Env>
static void env_step(const DeviceEnv& d, int E, const int32_t* act, float* obs_next, float* rew, float* done, hipStream_t st) {
    hipLaunchKernelGGL(env_step_kernel<Env>, dim3((E + 63) / 64), dim3(64), 0, st, Env::args(d), d.state, d.nsteps, d.episode, act, d.seed,
                       obs_next, rew, done, E);
}
template <typename Env>
static void env_reset(const DeviceEnv& d, int E, float* obs, hipStream_t st) {
    hipLaunchKernelGGL(env_reset_kernel<Env>, dim3((E + 63) / 64), dim3(64), 0, st, Env::args(d), d.state, d.nsteps, d.episode, d.seed, obs, E);
}

// ------------------------------------------------------------------------------------------ the env table and the mi_env_* entry points
// The serial rollout of the cart-pole / mountain-car sets is T + 1 round trips: policy step -> actions to the host -> the numpy env's
// step -> the next observations up.  With the env on the device a rollout is ONE call that enqueues T + 1 policy steps and T env steps
// on the main stream and returns; the only host wait is the caller's read of the reward / done rings afterwards.  A context holds at
// most one env: the create call points c->env.ops at its row, and every other mi_env_* entry goes through that row.
template <typename Env>
static int env_max_steps(const DeviceEnv& d) { return Env::args(d).max_steps; }
template <typename Env>
static constexpr EnvOps env_row(const char* entry, const char* columns, const char* actions, const char* action_range) {
    return {entry, columns, actions, action_range, Env::W, Env::A, env_step<Env>, env_reset<Env>, env_rollout_resident<Env>, env_evaluate<Env>, env_max_steps<Env>};
}
static const EnvOps CARTPOLE_ENV = env_row<CartPole>("mi_env_cartpole_create", "the cart-pole's nine state columns", "push left / push right",
                                                     "mi_env_step: every action must be 0 or 1");
static const EnvOps CARTPOLE_SWING_ENV = env_row<CartPoleSwing>("mi_env_cartpole_swing_create", "the swing-up cart-pole's nine state columns",
                                                                "push left / push right", "mi_env_step: every action must be 0 or 1");
static const EnvOps MOUNTAIN_CAR_ENV = env_row<MountainCar>("mi_env_mountain_car_create", "the mountain car's five state columns",
                                                            "push left / none / push right", "mi_env_step: every action must be 0, 1 or 2");

// what every create call checks, in this order (the context's shape before its occupancy), worded from the env's row
static int env_check(mi_ctx* c, const EnvOps& o, int max_steps, const double* low, const double* high) {
    const std::string f = std::string(o.entry) + ": ", w = std::to_string(o.width), a = std::to_string(o.n_actions);
    ARG(c->cfg.arch == MI_ARCH_MLP, f + "arch must be MI_ARCH_MLP");
    ARG(c->cfg.obs_dim == o.width, f + "obs_dim must be " + w + " (" + o.columns + ")");
    ARG(c->cfg.n_actions == o.n_actions, f + "n_actions must be " + a + " (" + o.actions + ")");
    ARG(c->E >= 2, f + "n_envs must be at least 2");
    ARG(!c->gru_on, f + "a recurrent context (mi_set_gru) is not supported");
    ARG(!c->env.ops, f + "this context already has an env");
    ARG(max_steps >= 1, f + "max_steps must be at least 1");
    for (int j = 0; j < o.width; ++j) ARG(low[j] <= high[j], f + "low must not exceed high");      // (also refuses NaN)
    return 0;
}
// the env's buffers (the same seven allocations whatever the env) and the fields every mi_env_* entry reads
static int env_attach(mi_ctx* c, const EnvOps* ops, uint64_t seed) {
    const size_t E = c->E, W = ops->width;
    DeviceEnv& d = c->env;
    DevPool& m = c->pool; DevPool::Group all(m);
    HIPC(m.dev(&d.state, E * W)); HIPC(m.dev(&d.nsteps, E)); HIPC(m.dev(&d.episode, E));
    HIPC(m.dev(&d.s_act, E)); HIPC(m.dev(&d.s_obs, E * W)); HIPC(m.dev(&d.s_rew, E)); HIPC(m.dev(&d.s_done, E));
    all.keep = true;
    d.seed = seed;
    d.ops = ops;
    return 0;
}
int mi_env_cartpole_create(mi_ctx* c, const mi_cartpole_params* p, uint64_t seed) {
    ARG(c && p, "null"); JOIN(c);
    const EnvOps& o = CARTPOLE_ENV;
    if (int r = env_check(c, o, p->max_steps, p->low, p->high)) return r;
    CartPoleArgs& a = c->env.args.cp;
    for (int j = 0; j < 9; ++j) { a.low[j] = p->low[j]; a.high[j] = p->high[j]; }
    a.x_threshold = p->x_threshold; a.theta_threshold = p->theta_threshold; a.max_steps = p->max_steps;
    return env_attach(c, &o, seed);
}
int mi_env_cartpole_swing_create(mi_ctx* c, const mi_cartpole_swing_params* p, uint64_t seed) {
    ARG(c && p, "null"); JOIN(c);
    const EnvOps& o = CARTPOLE_SWING_ENV;
    if (int r = env_check(c, o, p->max_steps, p->low, p->high)) return r;
    ARG(p->x_threshold > 0, "mi_env_cartpole_swing_create: x_threshold must be positive (the reward divides by it)");      // (also refuses NaN)
    CartPoleSwingArgs& a = c->env.args.cs;
    for (int j = 0; j < 9; ++j) { a.low[j] = p->low[j]; a.high[j] = p->high[j]; }
    a.x_threshold = p->x_threshold; a.max_steps = p->max_steps;
    return env_attach(c, &o, seed);
}
int mi_env_mountain_car_create(mi_ctx* c, const mi_mountain_car_params* p, uint64_t seed) {
    ARG(c && p, "null"); JOIN(c);
    const EnvOps& o = MOUNTAIN_CAR_ENV;
    if (int r = env_check(c, o, p->max_steps, p->low, p->high)) return r;
    ARG(p->max_speed >= 0, "mi_env_mountain_car_create: max_speed must not be negative");
    // (the start loop is bounded on the device whatever the ranges; the host's acceptance rule makes its fallback a 2^-32 event)
    MountainCarArgs& a = c->env.args.mc;
    for (int j = 0; j < 5; ++j) { a.low[j] = p->low[j]; a.high[j] = p->high[j]; }
    a.left_boundary = p->left_boundary; a.max_speed = p->max_speed; a.force = p->force;
    a.goal_velocity = p->goal_velocity; a.max_steps = p->max_steps; a.sparse_rewards = p->sparse_rewards != 0;
    return env_attach(c, &o, seed);
}
#define ENV(c) ARG((c)->env.ops, "no env on this context (mi_env_cartpole_create / mi_env_cartpole_swing_create / mi_env_mountain_car_create)")
int mi_env_reset(mi_ctx* c) {
    ARG(c, "null"); JOIN(c); ENV(c);
    c->env.ops->reset(c->env, c->E, c->obsf, c->stream);
    HIPC(hipGetLastError());
    return 0;
}
int mi_env_step(mi_ctx* c, const int64_t* act, float* obs_out, float* rew_out, float* done_out) {
    ARG(c && act, "null"); JOIN(c); ENV(c);
    const DeviceEnv& d = c->env;
    const size_t E = c->E, W = d.ops->width;
    for (size_t e = 0; e < E; ++e) ARG(act[e] >= 0 && act[e] < d.ops->n_actions, d.ops->action_range);
    HIPC(hipStreamSynchronize(c->stream));      // (h_i may still be the source / destination of an earlier call's copy)
    for (size_t e = 0; e < E; ++e) c->h_i[e] = (int32_t)act[e];
    HIPC(hipMemcpyAsync(d.s_act, c->h_i, E * 4, hipMemcpyHostToDevice, c->stream));
    d.ops->step(d, c->E, d.s_act, d.s_obs, d.s_rew, d.s_done, c->stream);
    HIPC(hipGetLastError());
    if (obs_out) HIPC(hipMemcpyAsync(obs_out, d.s_obs, E * W * 4, hipMemcpyDeviceToHost, c->stream));
    if (rew_out) HIPC(hipMemcpyAsync(rew_out, d.s_rew, E * 4, hipMemcpyDeviceToHost, c->stream));
    if (done_out) HIPC(hipMemcpyAsync(done_out, d.s_done, E * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_env_rollout(mi_ctx* c, uint64_t seed) {
    ARG(c, "null"); JOIN(c); ENV(c);
    ARG(!c->gru_on, "mi_env_rollout: a recurrent context (mi_set_gru) is not supported");
    const DeviceEnv& d = c->env;
    const size_t E = c->E, W = d.ops->width;
    hipLaunchKernelGGL(env_emit_obs_kernel, dim3((unsigned)((E * W + 255) / 256)), dim3(256), 0, c->stream, d.state, c->obsf, (int)(E * W));
    for (int t = 0; t < c->T; ++t) {
        if (int r = issue_policy_step(c, t, seed, nullptr)) return r;
        d.ops->step(d, c->E, c->act + t * E, c->obsf + (t + 1) * E * W, c->rew + t * E, c->done + t * E, c->stream);
    }
    return issue_policy_step(c, c->T, seed, nullptr);
}
// The same rollout as ONE launch (env_resident.hip): every refusal comes before the launch, so a refused call leaves every ring as it was.
int mi_env_rollout_resident(mi_ctx* c, uint64_t seed) {
    ARG(c, "null"); JOIN(c); ENV(c);
    const std::string f = "mi_env_rollout_resident: ";
    ARG(!c->gru_on, f + "a recurrent context (mi_set_gru) is not supported");
    { const std::string why = resident_shape_refusal(c); ARG(why.empty(), f + why); }
    const DeviceEnv& d = c->env;
    ARG(c->cfg.obs_dim == d.ops->width && c->cfg.obs_dim <= 16, f + "obs_dim must be the env's state width");
    const ResidentNet net = resident_net(c);
    const ResidentRings ring = {c->obsf, c->act, c->logp, c->value, c->rew, c->done};
    c->prof.phase = 0;
    d.ops->rollout(d, net, ring, c->E, c->T, seed, c->stream);
    HIPC(hipGetLastError());
    return 0;
}
// K whole episodes of every env in ONE launch (env_evaluate.hip).  Every refusal comes before any launch or allocation; the env's state /
// n_steps / episode and the rings are neither read nor written, so a training run may call this between two iterations.
#define EVAL_MAX_STEPS (1ll << 20)      // episodes * max_steps of one launch: tens of seconds at the resident rollout's 27 us per step
int mi_env_evaluate(mi_ctx* c, int32_t episodes, uint64_t seed, int32_t greedy, int64_t first_episode, const double* starts, double* ret,
                    int32_t* length, int32_t* terminated, float* value0, double* start_out) {
    ARG(c, "null"); JOIN(c); ENV(c);
    const std::string f = "mi_env_evaluate: ";
    ARG(!c->gru_on, f + "a recurrent context (mi_set_gru) is not supported");
    { const std::string why = resident_shape_refusal(c); ARG(why.empty(), f + why); }
    const DeviceEnv& d = c->env;
    ARG(c->cfg.obs_dim == d.ops->width && c->cfg.obs_dim <= 16, f + "obs_dim must be the env's state width");
    ARG(episodes >= 1, f + "episodes must be at least 1");
    ARG((long long)episodes * (long long)d.ops->max_steps(d) <= EVAL_MAX_STEPS,
        f + "episodes * max_steps must be at most 2^20 = 1048576 (evaluate further episodes with another call and another first_episode)");
    ARG(first_episode >= 1, f + "first_episode must be at least 1");
    const size_t E = c->E, W = d.ops->width, K = (size_t)episodes, n = E * K;
    if (starts) for (size_t k = 0; k < n * W; ++k) ARG(!isnan(starts[k]), f + "starts must not hold a NaN");
    // the device buffers of the planted starts and the records: one group of the context's pool, given back when the call returns (the
    // pool frees a group only as a whole and newest first, so nothing is kept between calls; behind the synchronise below, and hipFree
    // waits for the device on the paths that leave early)
    double *ev_starts = nullptr, *ev_ret = nullptr, *ev_start = nullptr; int32_t *ev_len = nullptr, *ev_term = nullptr; float* ev_v0 = nullptr;
    DevPool& m = c->pool; DevPool::Group all(m);
    HIPC(m.dev(&ev_starts, starts ? n * W : 1)); HIPC(m.dev(&ev_ret, n)); HIPC(m.dev(&ev_len, n)); HIPC(m.dev(&ev_term, n));
    HIPC(m.dev(&ev_v0, n)); HIPC(m.dev(&ev_start, n * W));
    if (starts) HIPC(hipMemcpyAsync(ev_starts, starts, n * W * 8, hipMemcpyHostToDevice, c->stream));
    const ResidentNet net = resident_net(c);
    const EvalRecords rec = {starts ? ev_starts : nullptr, ev_ret, ev_len, ev_term, ev_v0, ev_start};
    d.ops->evaluate(d, net, rec, c->E, episodes, (long long)first_episode, seed, greedy != 0, c->stream);
    HIPC(hipGetLastError());
    if (ret) HIPC(hipMemcpyAsync(ret, ev_ret, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (length) HIPC(hipMemcpyAsync(length, ev_len, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (terminated) HIPC(hipMemcpyAsync(terminated, ev_term, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (value0) HIPC(hipMemcpyAsync(value0, ev_v0, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (start_out) HIPC(hipMemcpyAsync(start_out, ev_start, n * W * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_env_get_state(mi_ctx* c, double* state, int32_t* n_steps, int64_t* episode) {
    ARG(c, "null"); JOIN(c); ENV(c);
    const DeviceEnv& d = c->env;
    const size_t E = c->E, W = d.ops->width;
    if (state) HIPC(hipMemcpyAsync(state, d.state, E * W * 8, hipMemcpyDeviceToHost, c->stream));
    if (n_steps) HIPC(hipMemcpyAsync(n_steps, d.nsteps, E * 4, hipMemcpyDeviceToHost, c->stream));
    if (episode) HIPC(hipMemcpyAsync(episode, d.episode, E * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return 0;
}
int mi_env_set_state(mi_ctx* c, const double* state, const int32_t* n_steps, const int64_t* episode) {
    ARG(c, "null"); JOIN(c); ENV(c);
    const DeviceEnv& d = c->env;
    const size_t E = c->E, W = d.ops->width;
    if (n_steps) for (size_t e = 0; e < E; ++e) ARG(n_steps[e] >= 0, "mi_env_set_state: n_steps must not be negative");
    if (state) HIPC(hipMemcpyAsync(d.state, state, E * W * 8, hipMemcpyHostToDevice, c->stream));
    if (n_steps) HIPC(hipMemcpyAsync(d.nsteps, n_steps, E * 4, hipMemcpyHostToDevice, c->stream));
    if (episode) HIPC(hipMemcpyAsync(d.episode, episode, E * 8, hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));      // caller buffers may be pageable temporaries
    return 0;
}
