/* libmi355ppo -- C ABI of the MI355X-native PPO hot path.
 *
 * The reference (tbuckworth/train-procgen-pytorch) has no FFI for this path: its boundary is the
 * duck-typed Python API of agents/ppo.py (PPO), common/storage.py (Storage) and common/policy.py
 * (CategoricalPolicy) -- SURVEY.md section 8(b).  This header is the C boundary a binding for that API
 * sits on (ours: train-procgen-pytorch_amd/mi355/engine.py via ctypes).  Each entry
 * point names the reference interface it replaces.
 *
 * Conventions: every function returns 0 on success and a negative code on error (mi_last_error()
 * gives the text).  The caller owns all host buffers; the context owns all device memory.  One
 * context per GPU per process.  All work is issued on the context's HIP stream; functions that
 * return data to host buffers synchronise that stream before returning, the others are asynchronous
 * (use mi_sync).  No torch types appear here.
 */
#ifndef MI355PPO_H
#define MI355PPO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_ctx mi_ctx;

enum { MI_ARCH_IMPALA = 0, MI_ARCH_MLP = 1 };

typedef struct mi_config {
    int32_t arch;          /* MI_ARCH_IMPALA: common/model.py:167-209 ; MI_ARCH_MLP: common/model.py:954-980 */
    int32_t n_steps;       /* T  (Storage num_steps, common/storage.py:9) */
    int32_t n_envs;        /* E  local envs on this rank (Storage num_envs) */
    int32_t n_actions;     /* A  (CategoricalPolicy action_size, common/policy.py:22) ; 1 <= A <= 16 */
    int32_t obs_dim;       /* MLP only: observation vector length (IMPALA is fixed 64x64x3 uint8 NHWC) */
    int32_t mlp_depth;     /* MLP only: MLPModel depth (>= 2) */
    int32_t mlp_width;     /* MLP only: MLPModel mid_weight */
    int32_t out_dim;       /* embedder.output_dim.  IMPALA: a multiple of 64 in [64, 512] (0 = 256, the reference's default);
                              MLP: latent_size */
    int32_t max_batch;     /* largest number of samples one mi_minibatch / mi_forward call may carry */
    int32_t device;        /* HIP device ordinal */
    int32_t precision;     /* IMPALA activations / activation gradients in HBM: 0 = fp32 (parity mode), 1 = bf16 storage +
                              bf16 matrix cores with fp32 accumulation for the 16/32-channel convs (BASELINE config 3);
                              parameters, gradients of parameters, Adam, losses and GAE are fp32 in both modes */
    int32_t value_from_logits; /* 0: value = fc_value(hidden) (common/policy.py:79-80); 1: CategoricalPolicy(logsumexp_logits_is_v=True),
                              value = logsumexp of the raw fc_policy logits (policy.py:77-78).  fc_value keeps its place in the flat vectors,
                              receives an exactly zero gradient and never changes; the value-loss gradient flows into the logits.
                              Any other value is refused.  (The first slot of what was reserved[5]: 0 is the earlier behaviour.) */
    int32_t reserved[4];
    void*   stream;        /* hipStream_t to issue on, or NULL for a stream owned by the context */
} mi_config;

/* PPO.__init__ hyper-parameters used inside the minibatch step (agents/ppo.py:10-70) */
typedef struct mi_hparams {
    float eps_clip, value_coef, entropy_coef, x_entropy_coef, entropy_multiplier, fs_coef;
} mi_hparams;

const char* mi_last_error(void);
int mi_create(const mi_config* cfg, mi_ctx** out);
int mi_destroy(mi_ctx* ctx);
int mi_sync(mi_ctx* ctx);
/* pinned (page-locked) host memory for the rollout staging buffers: mi_put_obs / mi_put_step from such a
 * buffer is a true asynchronous DMA (the reference copies pageable numpy arrays, agents/ppo.py:74-76) */
void* mi_host_alloc(size_t bytes);
void  mi_host_free(void* p);
/* page-lock caller-owned memory in place -- the buffer an env hands its frames out in (Procgen's rgb buffer keeps its address from
 * step to step) -- so that mi_rollout_submit / mi_put_obs DMA straight out of it: no staging copy on the host (the reference copies
 * every observation twice on the host before its H2D, common/storage.py:39-44 and agents/ppo.py:74).  Negative where the runtime
 * refuses the range; the caller then stages through mi_host_alloc memory as before. */
int   mi_host_register(void* p, size_t bytes);
int   mi_host_unregister(void* p);

/* ---- parameters / optimiser state: flat fp32 vectors in the REFERENCE's policy.parameters() order and
 *      tensor layouts (policy.state_dict(), train.py:257-263 / agents/ppo.py:271-276).  The library
 *      converts to / from its device layouts (NHWC filter banks, NHWC-flatten fc columns). */
int64_t mi_param_count(mi_ctx* ctx);
int mi_set_params(mi_ctx* ctx, const float* flat, int64_t n);
int mi_get_params(mi_ctx* ctx, float* flat, int64_t n);
/* dst's parameters := src's, device to device in stream order (same architecture, sizes and device): how the validation rollouts'
 * inference-only twin context follows the trained policy (agents/ppo.py:241-252 use one policy object for both env sets) */
int mi_copy_params(mi_ctx* dst, mi_ctx* src);
int mi_get_grads(mi_ctx* ctx, float* flat, int64_t n);                     /* accumulated, un-clipped */
int mi_set_adam_state(mi_ctx* ctx, const float* exp_avg, const float* exp_avg_sq, int64_t n);
int mi_get_adam_state(mi_ctx* ctx, float* exp_avg, float* exp_avg_sq, int64_t n);

/* ---- rollout storage (Storage.store / store_last, common/storage.py:39-54).  t in [0, T]. */
int mi_put_obs(mi_ctx* ctx, int32_t t, const void* obs, size_t bytes);     /* E frames uint8 NHWC, or E x obs_dim fp32 */
int mi_get_obs(mi_ctx* ctx, int32_t t, void* obs, size_t bytes);           /* Storage.obs_batch[t] read-back */
int mi_put_step(mi_ctx* ctx, int32_t t, const float* rew, const float* done);            /* rew/done (E,) */
/* teacher forcing / compat path: overwrite what the policy step stored.  Any pointer may be NULL. */
int mi_put_policy_outputs(mi_ctx* ctx, int32_t t, const int32_t* act, const float* logp, const float* value);
enum { MI_F_REW = 0, MI_F_DONE, MI_F_VALUE, MI_F_LOGP, MI_F_ADV, MI_F_RET, MI_F_ACT };
int mi_read_field(mi_ctx* ctx, int32_t field, float* out, int64_t n);      /* (T,E) fp32; VALUE is (T+1,E); ACT as float */
int mi_write_field(mi_ctx* ctx, int32_t field, const float* in, int64_t n);

/* ---- PPO.predict on the stored observation of step t (agents/ppo.py:72-81): forward, sample, log_prob.
 *      t < T: writes act/logp/value[t]; t == T: writes value[T] only (store_last).  u: optional E uniforms
 *      in [0,1) for the inverse-CDF sampler (NULL -> Philox4x32-10 keyed by seed and t*E+e).
 *      Host outputs may be NULL (then the call does not synchronise). */
int mi_policy_step(mi_ctx* ctx, int32_t t, uint64_t seed, const float* u,
                   int64_t* act_out, float* logp_out, float* value_out);

/* ---- one call per rollout step for the agent's own loop (agents/ppo.py:228-231 fused): stores the PREVIOUS step's
 *      reward / done (t >= 1; what Storage.store(t-1) receives after env.step), runs the policy step on slot t
 *      (forward, GRU if set -- its done mask is done_prev --, fused heads + sample) and returns act / logp / value
 *      through ONE packed read-back.  rew_prev / done_prev may be NULL (t == 0). */
int mi_rollout_step(mi_ctx* ctx, int32_t t, const float* rew_prev, const float* done_prev, uint64_t seed, const float* u,
                    int64_t* act_out, float* logp_out, float* value_out);

/* ---- the device-resident cart-pole (opt-in; the host env is common/env/vec_envs.py CartPoleVec = the reference's
 *      discrete_env/cartpole_pre_vec.py:20-262 on pre_vec_env.py:21-125): state, physics, termination, episode resets, reward and done
 *      live in HBM, and mi_env_rollout enqueues a whole rollout with no host synchronisation.  On an MLP context with obs_dim == 9 and
 *      n_actions == 2 only; anything else is refused with a message that names the field, and so are a context with a GRU set and a
 *      second create on the same context.  The env's buffers belong to the context: mi_destroy frees them.
 *      State: double [E][9] in CartPoleVec's column order {x, x_dot, theta, theta_dot, gravity, pole_length, cart_mass, pole_mass,
 *      force_mag}, int32 n_steps [E] (steps of the running episode), int64 episode [E] (0 after create; every start of an episode adds 1).
 *      A step is CartPoleVec.step in fp64 in the same operation order; an env ends beyond +-x_threshold / +-theta_threshold or when
 *      n_steps reaches max_steps, and then starts episode + 1 at once: done is the step's termination flag, the observation the
 *      post-reset state, the reward 1.  The thresholds arrive as doubles (the caller computes degrees * 2 pi / 360 as CartPoleVec does).
 *      A fresh state is low + (high - low) * u per column, u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53 from two words of Philox4x32-10
 *      keyed by `seed` with the counter {env index, episode low word, episode high word, block}, block 0..4 giving columns 2 block and
 *      2 block + 1 from words {0, 1} and {2, 3}.  This stream is the device env's own: CartPoleVec draws an (E, 9) numpy block whenever
 *      any env ends, which is not reproduced.
 *      mi_env_reset: every env starts a fresh episode; float(state) goes into observation slot 0.  Asynchronous.
 *      mi_env_step: one env step on the caller's actions (0 / 1; the mountain car below: 0 / 1 / 2), results on the host (any output may be NULL), one synchronisation; it
 *      goes through a staging slot and changes no ring (VecEnv.step, and the teacher-forcing hook of the tests).
 *      mi_env_rollout: float(state) -> observation slot 0; for t in [0, T): the policy step on slot t exactly as
 *      mi_policy_step(t, seed, NULL, NULL, NULL, NULL) enqueues it (same kernels, same Philox counters t * E + e), then the env step on
 *      act[t] -> obs[t + 1], rew[t], done[t]; then the policy step on slot T (value[T] only).  All on the context's stream; returns
 *      without synchronising (the rings are read with mi_read_field / mi_get_obs as after any rollout).
 *      mi_env_get_state / mi_env_set_state: test and checkpoint hooks; any pointer may be NULL (that part is skipped). */
typedef struct mi_cartpole_params {
    double low[9], high[9];          /* start ranges per state column */
    double x_threshold, theta_threshold;
    int32_t max_steps;
} mi_cartpole_params;
int mi_env_cartpole_create(mi_ctx* ctx, const mi_cartpole_params* params, uint64_t seed);
/* ---- the device-resident swing-up cart-pole (the host env is common/env/vec_envs.py CartPoleSwingVec = the reference's
 *      discrete_env/cartpole_swing_pre_vec.py:19-239 on pre_vec_env.py:21-125).  The cart-pole's context shape (MLP, obs_dim == 9,
 *      n_actions == 2), state layout, dynamics (the same device function), refusals and start stream (blocks 0..4); the pole hangs down
 *      at the start, which is the caller's `low` / `high` alone (theta in pi -+ 0.05).  What differs in a step: an env ends beyond
 *      +-x_threshold or when n_steps reaches max_steps -- there is NO angle threshold -- and the reward is that of the post-step,
 *      pre-reset state, float(rt * rx) with rt = cos(theta), set to 0 where rt < 0, and rx = cos((x / x_threshold) * (pi / 2)); a row
 *      that has just ended beyond x_threshold with rt == 0 yields -0.0, as CartPoleSwingVec does.  x_threshold divides, so a value that
 *      is not positive (or NaN) is refused by name. */
typedef struct mi_cartpole_swing_params {
    double low[9], high[9];          /* start ranges per state column */
    double x_threshold;
    int32_t max_steps;
} mi_cartpole_swing_params;
int mi_env_cartpole_swing_create(mi_ctx* ctx, const mi_cartpole_swing_params* params, uint64_t seed);
/* ---- the device-resident mountain car (the host env is common/env/vec_envs.py MountainCarVec = the reference's
 *      discrete_env/mountain_car_pre_vec.py:15-219 on pre_vec_env.py:21-125 and helper_pre_vec.py:4-38).  A context holds ONE env: the
 *      create call fixes its kind, and mi_env_reset / _step / _rollout / _get_state / _set_state below dispatch on it; W, the state
 *      width, is 9 for the cart-pole and 5 here, the legal actions 0 / 1 there and 0 / 1 / 2 here.  On an MLP context with obs_dim == 5
 *      and n_actions == 3 only; the refusals are the cart-pole's, by field name.
 *      State: double [E][5] = {position, velocity, gravity, right_boundary, goal_position}; n_steps and episode as for the cart-pole.
 *      A step is MountainCarVec.step in fp64 in the same operation order (contraction off): v += (a - 1) * force + cos(3 p) * (-gravity),
 *      clipped to +-max_speed; p += v, clipped to [left_boundary, right_boundary]; v = 0 where p == left_boundary and v < 0; the env
 *      ends where p >= goal_position and v >= goal_velocity, or when n_steps reaches max_steps, and then starts episode + 1 at once.
 *      The reward is float(-1) with sparse_rewards, else float(sin(3 p) * 0.45 + 0.55 - 1) of the post-step, pre-reset position; done is
 *      the step's flag, the observation float(the post-reset state).
 *      A fresh state is low + (high - low) * u per column with the cart-pole's u, from Philox4x32-10 keyed by `seed` with the counter
 *      {env index, episode low word, episode high word, 3 * attempt + b}, b = 0..2 giving columns 2 b and 2 b + 1 from words {0, 1} and
 *      {2, 3}.  Attempts 0, 1, ... are drawn until !(goal_position > right_boundary) (StartSpace.sample's condition).  The loop is
 *      bounded: after 32 rejected attempts the last draw is kept with goal_position = right_boundary.  The caller (MountainCarVec /
 *      DeviceMountainCar) refuses range sets that accept a draw with probability below 1/2, so the fallback is taken with probability at
 *      most 2^-32 per reset.  The velocity column has low == high == 0 and comes out exactly 0.  As for the cart-pole the stream is the
 *      device env's own: MountainCarVec's numpy block draws are not reproduced. */
typedef struct mi_mountain_car_params {
    double low[5], high[5];          /* start ranges per state column */
    double left_boundary, max_speed, force, goal_velocity;
    int32_t max_steps, sparse_rewards;
} mi_mountain_car_params;
int mi_env_mountain_car_create(mi_ctx* ctx, const mi_mountain_car_params* params, uint64_t seed);
int mi_env_reset(mi_ctx* ctx);
int mi_env_step(mi_ctx* ctx, const int64_t* act, float* obs_out /* E x W */, float* rew_out, float* done_out);
int mi_env_rollout(mi_ctx* ctx, uint64_t seed);
/* mi_env_rollout as ONE launch (opt-in): a workgroup carries 16 envs through all T + 1 policy steps and T env steps -- the MLP and the heads
 * in fp32 on the matrix cores with the activations in LDS, the sampler and the env step on the threads that own an env.  It leaves what
 * mi_env_rollout(ctx, seed) leaves -- observation slots 0..T, act / logp / rew / done [T], value [T + 1], the env's state / n_steps / episode --
 * from the same sampling counters t * E + e and the same reset stream; the env arithmetic is the same code, the policy numbers differ by
 * fp32 summation order only.  Asynchronous on the context's stream.  Refused by name, before anything is written: no env on the context,
 * a context with a GRU set, mlp_depth above 16, mlp_width or out_dim not a multiple of 16 or above 512, more than 15 actions. */
int mi_env_rollout_resident(mi_ctx* ctx, uint64_t seed);
/* The evaluation of the context's policy on its env as ONE launch: every env runs exactly `episodes` (K) whole episodes on the resident
 * rollout's skeleton (16 envs per workgroup, the MLP on the matrix cores, the env step in fp64) and the per-episode records stay on the
 * device until the call copies them out.  Episode i (0 .. K - 1) of env e starts at the reset stream's episode first_episode + i of env e
 * (the create call's seed) or, with `starts` [E][K][W], at row starts[e][i]; it ends as in mi_env_step: the env's own termination or
 * n_steps == max_steps.  Step index t counts an env's steps since the launch began.  greedy == 0: the rollout's sampler, the uniform of
 * (seed, t * E + e) and the inverse CDF on the twice-normalised log-probabilities; greedy != 0: the first maximum of those
 * log-probabilities (mi_predict_greedy's rule; `seed` is unused).  value_from_logits contexts are allowed in both modes.
 * Records, [E][K] each (any output may be NULL): ret = the fp64 sum of the env's fp64 rewards in step order; length; terminated = the
 * env's own flag at the last step (0 for a truncation); value0 = the value head at the episode's first observation; start_out [E][K][W] =
 * the state the episode began in (the parameter columns it was drawn with).
 * A pure function of the parameters, the env's arguments and seed, first_episode, episodes, seed, greedy and starts: the env's state /
 * n_steps / episode and every ring are neither read nor written, so a training run may call it between two iterations.  Synchronises.
 * Refused by name, before any launch or allocation: no env on the context, a context with a GRU set, the shapes mi_env_rollout_resident
 * refuses, episodes < 1, episodes * max_steps > 2^20 (call again with another first_episode), first_episode < 1, a NaN in starts. */
int mi_env_evaluate(mi_ctx* ctx, int32_t episodes, uint64_t seed, int32_t greedy, int64_t first_episode, const double* starts /* may be NULL */,
                    double* ret, int32_t* length, int32_t* terminated, float* value0, double* start_out);
int mi_env_get_state(mi_ctx* ctx, double* state /* E x W */, int32_t* n_steps, int64_t* episode);
int mi_env_set_state(mi_ctx* ctx, const double* state, const int32_t* n_steps, const int64_t* episode);

/* ---- pipelined rollout: the same step as mi_rollout_step, per ENV GROUP and split into submit / wait, so that the frame upload and
 *      forward pass of one group run beside the host's env.step of another (agents/ppo.py:225-231 is strictly serial; an env's next
 *      observation depends on its own action only, so G contiguous groups of E/G envs form G independent chains).
 *      mi_rollout_groups(G) (1 <= G <= 4, E % G == 0) gives each group a stream (a lane, below). mi_rollout_submit(t, g, frames, ...) enqueues on
 *      group g's stream: the H2D copy of the group's E/G observations (frames: pinned host memory from mi_host_alloc, valid until the
 *      matching wait; NULL = ring slot t already holds them) into ring slot t, the forward + sample on them, and the store of the
 *      previous step's reward / done of the group (rew_prev / done_prev: E/G floats each, may be NULL at t == 0); it returns at once.
 *      mi_rollout_wait(g, ...) blocks until that step's results (E/G entries each) are on the host.  One step per group in flight.
 *      Sampling uses the Philox counters t*E + e of mi_rollout_step: grouped and ungrouped rollouts draw the same actions.
 *      Any other entry point first orders the context's main stream behind all group streams.
 *      The groups' uploads take turns on the PCIe link (each reserves bytes / rate from the end of the previous reservation; environment
 *      variable MI355_COPY_GBPS, default 40, 0 = off): issued together they share the link, finish together and keep the chains in
 *      lock-step.  Uploads of at most 512 KB from device-visible pinned memory are pulled by a kernel instead of the copy engine. */
int mi_rollout_groups(mi_ctx* ctx, int32_t n_groups);
int mi_rollout_submit(mi_ctx* ctx, int32_t t, int32_t group, const void* frames, size_t bytes, const float* rew_prev,
                      const float* done_prev, uint64_t seed, const float* u);
int mi_rollout_wait(mi_ctx* ctx, int32_t group, int64_t* act_out, float* logp_out, float* value_out);
/* The group streams are LANES: at most four streams per process and device, created at the greatest stream priority on first use,
 * lent to the contexts and destroyed when the last context that holds one is destroyed.  A context with G groups holds G different
 * lanes for its lifetime; two live contexts hold disjoint lanes as long as their groups number four or fewer in all, beyond that lanes are shared
 * (still correct: every group orders itself by its own events).  mi_rollout_lane_info reports what the groups of this context run
 * on: *n = groups with a lane, prio[g] = the stream priority, stream_id[g] = an id of the stream that is equal for two groups (of any
 * contexts) exactly when they share a lane. */
int mi_rollout_lane_info(mi_ctx* ctx, int32_t* n, int32_t* prio /* [4] */, uint64_t* stream_id /* [4] */);

/* ---- PPO.predict(obs, hidden, done) on caller data (agents/ppo.py:72-81) when the caller has not said which
 *      storage slot the observation belongs to: obs (E frames / rows) is staged on the device, forward + sample
 *      run on it, and mi_commit_staged(t) later moves the staged observation and policy outputs into ring slot t
 *      (what Storage.store / store_last do with the same arrays, common/storage.py:39-54) without a second PCIe trip. */
int mi_predict_staged(mi_ctx* ctx, const void* obs, size_t bytes, uint64_t seed, uint64_t counter, const float* u,
                      int64_t* act_out, float* logp_out, float* value_out);
/* PPO.predict_w_value_saliency (agents/ppo.py:83-94): mi_predict_staged + d value / d observation (value.backward()): grad_out is
 * [E][64][64][3] floats (NHWC, with respect to the k/255 float frames) for IMPALA, [E][obs_dim] for the MLP.  With a GRU set (mi_set_gru)
 * the step is the recurrent one -- it consumes the hidden state / done flags of mi_rec_state and advances the state like a policy step --
 * and the gradient runs back through the GRU cell's input path (common/model.py:219-225 under autograd).  Discards (zeroes) the
 * parameter-gradient buffer, so not inside an accumulating update.  With mi_config.value_from_logits the value differentiated is the
 * logsumexp of the logits: the backward pass is seeded with softmax(logits) in the logit columns (recurrent: softmax(logits) W_pi per row
 * into the GRU cell) instead of a 1 in the value column. */
int mi_value_saliency(mi_ctx* ctx, const void* obs, size_t bytes, uint64_t seed, uint64_t counter, const float* u,
                      int64_t* act_out, float* logp_out, float* value_out, float* grad_out);
int mi_commit_staged(mi_ctx* ctx, int32_t t);

/* ---- recurrent policies (CategoricalPolicy(recurrent=True), common/policy.py:48-50,66-67; GRU.forward prediction
 *      branch, common/model.py:219-225): h' = GRU(feat, h * (1 - done)), heads on h'.  As in the reference's
 *      algo: ppo the GRU runs in predict only and is never trained: its weights are set once,
 *      in nn.GRU's layout (weight_ih_l0 (3H,H), weight_hh_l0 (3H,H), bias_ih_l0 (3H), bias_hh_l0 (3H); gates r,z,n).
 *      mi_rec_state sets the hidden state (NULL keeps the device copy) and the done flags (NULL = zeros) that the
 *      NEXT mi_policy_step / mi_predict_staged consumes; mi_get_hidden reads the state after it. */
int mi_set_gru(mi_ctx* ctx, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh);
int mi_rec_state(mi_ctx* ctx, const float* hidden /* E x H or NULL */, const float* done /* E or NULL */);
int mi_get_hidden(mi_ctx* ctx, float* hidden /* E x H */);
/* ---- recurrent policies on the pipelined rollout (mi_rollout_groups / submit / wait; the reference's serial loop is agents/ppo.py:225-236
 *      with hidden_state / done carried from step to step, common/model.py:212-225 for the cell).  With a GRU set every group step runs
 *      the cell on its own rows as ONE fused launch: h' = GRU(x, h (1 - done)), where h is the step's input state and done is the group's
 *      done of step t-1 (handed over with the submit), at t == 0 that of mi_rec_begin.  The heads sample on h'.  A row's numbers do
 *      not depend on the number of groups (no split-K: G = 2 and G = 4 give bit-identical rollouts); against the serial mi_rollout_step
 *      they differ by the GEMMs' summation order only.
 *      mi_rec_begin(hidden, done) starts such a rollout: hidden (E x H; NULL = the device's current state) and done (E; NULL = zeros)
 *      are the carried-in state and flags of its step 0, uploaded in stream order on the main stream with no host wait (the groups' first
 *      submits order themselves behind it).  Required before the groups' step 0 of every recurrent rollout.  The first call allocates the
 *      context's hidden ring: (T + 1) x E x H floats, slot t = the input state of step t before masking (what Storage.store records as
 *      hidden_state, common/storage.py:39-54).  mi_get_hidden_ring(t0, t1, out) copies slots [t0, t1) into out ((t1 - t0) x E x H);
 *      mi_get_hidden reads h' of the last step (the bootstrap step's state that the serial loop carries into the next iteration). */
int mi_rec_begin(mi_ctx* ctx, const float* hidden /* E x H or NULL */, const float* done /* E or NULL */);
int mi_get_hidden_ring(mi_ctx* ctx, int32_t t0, int32_t t1, float* out /* (t1 - t0) x E x H */);
/* policy(obs, hx, masks) for a recurrent policy on E observations: consumes / advances the state like a policy step */
int mi_forward_rec(mi_ctx* ctx, const void* obs, float* logp_all, float* value, float* hidden_out);

/* ---- stateless forward on caller data (policy(obs, hx, masks) / hidden_to_output, common/policy.py:61-87).
 *      obs: n frames uint8 NHWC or n x obs_dim fp32.  logp_all: n x A normalised log-probs
 *      (Categorical.logits); value: n; feat: n x out_dim.  Outputs may be NULL. */
int mi_forward(mi_ctx* ctx, const void* obs, int32_t n, float* logp_all, float* value, float* feat);

/* ---- Storage.compute_estimates (common/storage.py:56-79) on the device-resident rollout */
int mi_compute_estimates(mi_ctx* ctx, float gamma, float lmbda, int32_t use_gae, int32_t normalize_adv);
/* multi-rank advantage normalisation: stats = {count, mean, M2} (fp64) of the local un-normalised advantages */
int mi_adv_stats(mi_ctx* ctx, double stats3[3]);
int mi_adv_apply(mi_ctx* ctx, const double stats3[3]);

/* ---- one minibatch of PPO.optimize (agents/ppo.py:119-170): gather by flat index i = t*E + e (local),
 *      forward, loss, backward; gradients ACCUMULATE into the flat gradient buffer (the reference's
 *      unscaled accumulation).  n_global = size of the global minibatch the means are taken over
 *      (= n_idx on one GPU).  Appends one 8-float record to the device loss log:
 *      {pi_loss, value_loss, entropy, x_ent, total, feature_sparsity, marginal_entropy, 0}. */
int mi_minibatch(mi_ctx* ctx, const int64_t* idx, int32_t n_idx, int32_t n_global, const mi_hparams* hp);
/* gradient accumulation (agents/ppo.py:155-177: the gradients of batch_size / mini_batch_size minibatches are SUMMED before one
 * optimizer step) in one pass: idx holds the gathered samples of n_seg minibatches back to back (seg_n[k] entries each, sum =
 * n_idx <= max_batch), every one a global minibatch of n_global samples.  Same gradients up to fp32 summation order, one log
 * record per segment; needs x_entropy_coef == 0 and fs_coef == 0 (no batch-level loss term) and multirank mode 0 or 2.  On R ranks
 * a rank's share of a global minibatch is ~1/R of it: this keeps its launches at single-GPU size. */
int mi_minibatch_multi(mi_ctx* ctx, const int64_t* idx, int32_t n_idx, const int32_t* seg_n, int32_t n_seg, int32_t n_global,
                       const mi_hparams* hp);
/* (new, opt-in: train.py --fused_update, PPO(fused_update=True), Engine.minibatch_fused) mi_minibatch_multi's pass for an MLP context in
 * TWO kernel launches behind the index pull instead of the chain's twenty-odd (csrc/mlp_fused.hip): launch 1 takes a tile of 16
 * gathered samples per workgroup through the gather, the MLP and the heads on the fp32 matrix cores with the activations in LDS, the
 * per-sample loss and dY, and the data gradients back through the layers, and leaves every layer's input and output gradient for all
 * rows in global memory; launch 2 sums every layer's weight and bias gradient tile by tile over all rows in row order into the flat
 * gradient buffer (+=, as the chain) and derives each segment's statistics row and log record.  No float atomics, no grid barrier: two
 * calls on the same inputs give the same bits.  The contract is mi_minibatch_multi's (n_seg == 1 is mi_minibatch): same index staging,
 * same log_count / statistics ring / loss log bookkeeping; mi_optimizer_step, mi_get_grads and mi_loss_log_read work after it as after
 * the chain; gradients and records equal the chain's up to fp32 summation order.
 * Refused, each message starting with "mi_minibatch_fused: ", before any launch and before the loss log, the index ring or the
 * gradient buffer change: arch other than MI_ARCH_MLP; a recurrent context (mi_set_gru); multirank mode other than 0; an armed or
 * in-flight gradient exchange or an initialised communicator; x_entropy_coef != 0 or fs_coef != 0 (the batch-level terms need the
 * two-phase loss, which stays on the chain); mlp_depth outside 2 .. 16, mlp_width or out_dim not a multiple of 16 or above 512,
 * n_actions above 15, obs_dim above 16; n_idx < 1 or > max_batch, n_global < 1, n_seg outside 1 .. 16 (the chain's limit), a segment of no
 * samples, segments that do not add up to n_idx, an index outside [0, T * E); a pending multirank minibatch; a full loss log. */
int mi_minibatch_fused(mi_ctx* ctx, const int64_t* idx, int32_t n_idx, const int32_t* seg_n, int32_t n_seg, int32_t n_global,
                       const mi_hparams* hp);
/* clip_grad_norm_ + Adam.step + zero_grad (agents/ppo.py:174-176); adam_step = 1-based step count */
int mi_optimizer_step(mi_ctx* ctx, float lr, float max_grad_norm, int32_t adam_step, float* grad_norm_out);
int mi_loss_log_read(mi_ctx* ctx, float* out, int32_t max_records, int32_t* n_records, int32_t reset);

/* ---- training the recurrence (algo: ppo-pure, agents/ppo_pure.py:98-176: optimize() calls policy(obs, hidden_state, mask), which for a
 *      recurrent policy is the training branch of GRU.forward, common/model.py:226-277 -- the hidden state is recomputed over the whole
 *      trajectory of the minibatch's envs and the gradient flows back through time).  Single GPU; the GRU arithmetic is fp32 in both
 *      precision modes.  Off (the default, algo: ppo, agents/ppo.py:125-128) the GRU stays frozen and nothing here changes a number.
 *      mi_gru_train(1) (after mi_set_gru; width a multiple of 64 in [64, 512]) allocates the GRU's gradient and Adam moments -- one
 *      vector {weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0} of 2 * 3H^2 + 2 * 3H floats, beside the flat vectors (mi_param_count
 *      does not change).  From then on mi_optimizer_step clips by the global norm over the flat AND the GRU gradients (one coefficient,
 *      clip_grad_norm_(policy.parameters()), ppo_pure.py:160), reports that norm, steps Adam on both and zeroes both; mi_copy_params from
 *      such a context also copies the GRU weights (the destination needs mi_set_gru).
 *      mi_minibatch_rec: one recurrent minibatch (ppo_pure.py:121-156 with Storage.fetch_train_generator(recurrent=True),
 *      common/storage.py:93-110) = the n_env envs of env_idx x all T steps, rows time-major; h0 = hidden_states_batch[0, envs] (n_env x H);
 *      the mask of step t is 1 - done[t, e], the done stored WITH step t (ppo_pure.py:124), where the rollout masks with the done of step
 *      t - 1.  n_env * T <= max_batch; n_global as in mi_minibatch; fs_coef must be 0 (ppo-pure has no such term); multirank modes 1 / 2
 *      and the in-library gradient exchange are refused, and so is a context created with value_from_logits.  Gradients accumulate until mi_optimizer_step; one loss-log record per call.
 *      mi_get_gru / mi_get_gru_grads read the weights / accumulated gradients in nn.GRU's layout; the Adam moments travel as the one
 *      vector above (n = 2 * 3H^2 + 2 * 3H). */
int mi_gru_train(mi_ctx* ctx, int32_t enabled);
int mi_minibatch_rec(mi_ctx* ctx, const int64_t* env_idx, int32_t n_env, const float* h0 /* n_env x H */, int32_t n_global, const mi_hparams* hp);
int mi_get_gru(mi_ctx* ctx, float* w_ih, float* w_hh, float* b_ih, float* b_hh);
int mi_get_gru_grads(mi_ctx* ctx, float* w_ih, float* w_hh, float* b_ih, float* b_hh);
int mi_get_gru_adam_state(mi_ctx* ctx, float* exp_avg, float* exp_avg_sq, int64_t n);
int mi_set_gru_adam_state(mi_ctx* ctx, const float* exp_avg, const float* exp_avg_sq, int64_t n);

/* ---- the sparse-autoencoder agent (algo: sae; reference agents/sae.py, models common/model.py:1623-1667) on an existing IMPALA context:
 *      stage 1 trains a sparse autoencoder on the 2048 block-3 features (ImpalaModel.forward_to_pool, common/model.py:186-196) of the
 *      FROZEN policy, stage 2 a linear probe (fc_policy, fc_value) that acts from its codes.  Non-recurrent, single GPU, serial rollout
 *      steps: a context with a GRU set, more than one rank or env groups is refused.  The policy's forward pass runs in the context's
 *      precision; all SAE / probe arithmetic is fp32.  Nothing here changes a number of the PPO entry points.
 *      mi_sae_create(sae_dim, rho) (SAE.__init__, agents/sae.py:60-65; sae_dim a multiple of 64 in [64, 4096]) allocates, only now: the
 *      SAE {encoder.0.weight [S][2048], .bias [S], decoder.0.weight [2048][S], .bias [2048]} and the probe {fc_policy.weight [A][S], .bias [A],
 *      fc_value.weight [1][S], .bias [1]} with gradients and Adam moments, a feature ring [T+1][E][2048] (539 MB at T = E = 256) and a logit
 *      ring [T][E][A]; the value / action / reward / done rings are the context's own (mi_read_field, mi_put_step, mi_put_policy_outputs).
 *      `which` selects the model: 0 = SAE, 1 = probe.  Flat vectors are in model.parameters() order and the reference's layouts: the
 *      encoder's 2048 input columns and the decoder's 2048 rows are channel-major ch*64 + p (Flatten() on NCHW); the library permutes to
 *      its pixel-major feature order as it does for embedder.fc.weight.  mi_sae_get_hidden / mi_sae_put_ring use the same order. */
int mi_sae_create(mi_ctx* ctx, int32_t sae_dim, float rho);
/* releases what mi_sae_create allocated, so that the context can get another SAE.  Optional: the state belongs to the context and
 * mi_destroy releases a live one.  Returns 0 also when there is nothing to release. */
int mi_sae_destroy(mi_ctx* ctx);
int64_t mi_sae_param_count(mi_ctx* ctx, int32_t which);
int mi_sae_set_params(mi_ctx* ctx, int32_t which, const float* flat, int64_t n);
int mi_sae_get_params(mi_ctx* ctx, int32_t which, float* flat, int64_t n);
int mi_sae_get_grads(mi_ctx* ctx, int32_t which, float* flat, int64_t n);                  /* accumulated, un-clipped */
int mi_sae_set_adam_state(mi_ctx* ctx, int32_t which, const float* exp_avg, const float* exp_avg_sq, int64_t n);
int mi_sae_get_adam_state(mi_ctx* ctx, int32_t which, float* exp_avg, float* exp_avg_sq, int64_t n);
/* SAEStorage.store / store_last of caller data (common/storage.py:533-548): hidden (E x 2048; t in [0, T]) and the policy's logits
 * (E x A; t < T) into ring step t.  Either pointer may be NULL.  mi_sae_get_hidden / mi_sae_get_logits read a ring step back;
 * t == -1: the hidden / logits of the last mi_sae_step that did not store (for the bootstrap step T the logits are read the same way). */
int mi_sae_put_ring(mi_ctx* ctx, int32_t t, const float* hidden, const float* logits);
int mi_sae_get_hidden(mi_ctx* ctx, int32_t t, float* out /* E x 2048 */);
int mi_sae_get_logits(mi_ctx* ctx, int32_t t, float* out /* E x A */);
/* SAE.get_hidden_and_acts (agents/sae.py:73-86) on E frames: one forward of the frozen policy; hidden = ReLU(block-3 output), the
 * normalised log-probabilities p.logits and the value; one action per env from Philox4x32-10 keyed by (seed, counter + e), the counter
 * being the context's own (0 at mi_sae_create, + E per call) -- from the policy's distribution (act_from_probe == 0) or from
 * Categorical(logits = probe(encode(hidden))) (agents/sae.py:81-84).  u: optional E uniforms instead of the generator.  store != 0:
 * hidden, the POLICY's logits (never the probe's), value and action go into ring step t (SAEStorage.store); t == T stores hidden and
 * value only (store_last); the frames go into the context's observation ring (mi_get_obs).  store == 0 changes no ring (validation rollouts: the reference reads storage_valid through fetch_log_data
 * only).  act_out / value_out (E each) may be NULL. */
int mi_sae_step(mi_ctx* ctx, int32_t t, const void* obs, size_t bytes, int32_t act_from_probe, int32_t store, uint64_t seed, const float* u,
                int64_t* act_out, float* value_out);
/* one minibatch of SAE.optimize_sae (agents/sae.py:151-156) on ring rows idx (flat t*E + e, n <= max_batch): pre = x W_e^T + b_e,
 * enc = relu(pre), rec = enc W_d^T + b_d, recon = mean((rec - x)^2), rho_hat_j = mean_b enc_bj, KL = sum_j rho log((rho + eps) /
 * (rho_hat_j + eps)) + (1 - rho) log((1 - rho + eps) / (1 - rho_hat_j + eps)), eps = 1e-10 (common/model.py:1645-1653; rho_hat_j >= 1
 * gives NaN as there), loss = recon + sparse_coef KL.  Gradients accumulate un-scaled.  log_out (may be NULL): {recon, KL, loss}. */
int mi_sae_minibatch(mi_ctx* ctx, const int64_t* idx, int32_t n, float sparse_coef, float* log_out);
/* one minibatch of SAE.optimize_linear_model (agents/sae.py:193-201): the encoder runs forward only; logit_loss = KLDivLoss(batchmean)(
 * log_softmax(enc W_p^T + b_p), softmax(stored logits)); value_loss = ((value_hat - value_batch)**2).mean() AS WRITTEN there --
 * (n,1) - (n,) broadcasts, so it is the mean over all n^2 pairs (i, j) of (v_hat_i - v_j)^2; loss = logit_loss + value_loss.
 * log_out (may be NULL): {value_loss, logit_loss, loss}. */
int mi_sae_probe_minibatch(mi_ctx* ctx, const int64_t* idx, int32_t n, float* log_out);
/* clip_grad_norm_ + Adam(eps=1e-5).step + zero_grad on one model (agents/sae.py:159-162, :204-207); adam_step = 1-based step count */
int mi_sae_optimizer_step(mi_ctx* ctx, int32_t which, float lr, float max_grad_norm, int32_t adam_step, float* grad_norm_out);
/* test hook: the forward pass of mi_sae_minibatch on ring rows idx -> enc (n x S) and rec (n x 2048, the reference's column order) */
int mi_sae_debug_forward(mi_ctx* ctx, const int64_t* idx, int32_t n, float* enc_out, float* rec_out);

/* ---- the IPL agent (algo: IPL; reference agents/IPL.py:109-225 with IPLStorage, common/storage.py:279-361) on a plain context: the same
 *      rings, network passes, clip, Adam and parameter vectors as PPO -- mi_optimizer_step, mi_get/set_params, mi_get/set_adam_state and
 *      mi_get_grads are reused unchanged.  The loss arithmetic is fp32 in both precision modes.
 *      mi_ipl_minibatch: one minibatch of IPL.optimize on ring rows idx (flat t*E + e, t < T); nobs is ring row idx + E (slot T is what
 *      store_last / the bootstrap step wrote).  v = V(obs), nv = V(nobs) with nv[done] = rew[done] (no gradient through those rows),
 *      modifier = alpha or, with MI_IPL_ENTROPY_MODIFIED, alpha (1 - exp(logp)); pred = modifier logp + v - gamma nv;
 *      loss = mean((pred - rew)^2) - [MI_IPL_REWARD_INCENTIVE] mean(pred) - [MI_IPL_ADV_INCENTIVE] mean(max_k logp_k) + entropy_coef mean(H).
 *      Three forward and two backward passes: the gradient reaches the network through obs AND nobs and ACCUMULATES into the flat
 *      gradient buffer like mi_minibatch's.  n <= max_batch; the means are taken over n_global.  Appends one 8-float record to the loss
 *      log (mi_loss_log_read), in the order of IPL's summary: {entropy, mutual_info, total, rew_corr, gamma, alpha loss (NaN: the
 *      temperature is not learned), alpha, mean pred}.  Refused by name: multirank mode != 0 or an armed gradient exchange, a context with
 *      a GRU set, one created with value_from_logits, n > max_batch.
 *      mi_ipl_read_pred: pred and the gathered reward of the last mi_ipl_minibatch (IPL.last_predicted_reward / last_reward), n = its size.
 *      mi_predict_greedy: IPL.predict(obs, greedy=True) (IPL.py:82-94) on E caller observations, staged like mi_predict_staged (so that
 *      mi_commit_staged can store them): act = the first arg-max of the normalised log-probabilities, its log-prob, the value. */
enum { MI_IPL_ENTROPY_MODIFIED = 1, MI_IPL_REWARD_INCENTIVE = 2, MI_IPL_ADV_INCENTIVE = 4,
       MI_IPL_DEBUG_ZERO_OBS_SEED = 256 /* test switch: the obs-side seed dY is zeroed, only the nobs path carries gradient */ };
typedef struct mi_ipl_hparams {
    float gamma, alpha, entropy_coef;
    int32_t flags;         /* MI_IPL_* */
} mi_ipl_hparams;
int mi_ipl_minibatch(mi_ctx* ctx, const int64_t* idx, int32_t n, int32_t n_global, const mi_ipl_hparams* hp);
int mi_ipl_read_pred(mi_ctx* ctx, float* pred_out, float* rew_out, int32_t n);
int mi_predict_greedy(mi_ctx* ctx, const void* obs, size_t bytes, int64_t* act_out, float* logp_out, float* value_out);
/* op-level test hook: only the IPL kernels (next value, loss + finaliser, next-side seed) on caller arrays -- hout [n][A+1] of the obs
 * pass, nv_raw [n] = V(nobs) before the done overwrite, act / rew / done [n].  Out (any may be NULL): rec8 the record, dY [n][A+1] the
 * obs-side seed, gnext [n] = d loss / d nv (exactly 0 on done rows), pred [n].  n in [1, 65536], A in [1, 16], means over n. */
int mi_op_ipl_loss(mi_ctx* ctx, int32_t n, int32_t A, const float* hout, const float* nv_raw, const int32_t* act, const float* rew,
                   const float* done, const mi_ipl_hparams* hp, float* rec8_out, float* dY_out, float* gnext_out, float* pred_out);
/* op-level test hook: the greedy action of n head rows hout [n][A+1] -> act [n] (lowest index among equal maxima) */
int mi_op_ipl_greedy(mi_ctx* ctx, int32_t n, int32_t A, const float* hout, int32_t* act_out);

/* ---- policy distillation (the reference's distill.py:128-234: a student is fitted with MSELoss + Adam to the normalised logits a trained
 *      teacher gives on the observations the STUDENT visited) on plain contexts: the same rings, network passes and parameter vectors as
 *      PPO; mi_get/set_params, mi_get/set_adam_state, mi_get_grads and mi_loss_log_read are reused unchanged.  The loss arithmetic is fp32
 *      in both precision modes.  Non-recurrent, one rank; the value head takes no part (its gradient is exactly 0).
 *      mi_distill_label(data, teacher): the teacher's forward pass -- its own network program and precision -- over all T * E observation
 *      rows of data's ring, read in place in chunks of the teacher's max_batch; the normalised log-probabilities (the rows mi_forward
 *      hands out, bit for bit) go to data's target ring [T * E][A], allocated by the first call.  data == teacher is allowed (the
 *      validation set labels itself).  The teacher's stream waits for data's ring and data's stream for the labels; asynchronous.
 *      mi_distill_minibatch(student, idx, n, n_global): one minibatch on ring rows idx (flat t*E + e) of the student's own ring and target
 *      ring: forward, lp = the twice-normalised log-probabilities, loss = sum (lp - y)^2 / (n_global * A), backward through both
 *      normalisations.  Gradients ACCUMULATE into the flat gradient buffer like mi_minibatch's; one record {loss, 0, 0, 0, loss, 0, 0, 0}
 *      is appended to the loss log.
 *      mi_distill_loss(student, data, loss_out): forward only -- the student on all of data's rows in chunks of the student's max_batch
 *      against data's targets, one fp64 sum in a fixed order -> the mean over T * E * A elements.  Changes neither the gradient buffer nor
 *      the loss log.  Synchronises.
 *      Refused, each message starting with the entry's name, before any launch and before the loss log, the index ring or the gradient
 *      buffer change: a context with a GRU set on either side; value_from_logits on the student; multirank mode != 0 or an armed gradient
 *      exchange; two contexts of different observation kind, obs_dim, n_actions or device; n > max_batch; mi_distill_minibatch /
 *      mi_distill_loss before any label call has filled the target ring they read. */
int mi_distill_label(mi_ctx* data, mi_ctx* teacher);
int mi_distill_minibatch(mi_ctx* student, const int64_t* idx, int32_t n, int32_t n_global);
int mi_distill_loss(mi_ctx* student, mi_ctx* data, float* loss_out);
/* read-back of data's target ring, [T * E][A] floats (n = their number), for tests and for callers that keep the labels; synchronises */
int mi_distill_targets(mi_ctx* data, float* out, int64_t n);
/* mi_optimizer_step with the caller's Adam eps (the distiller: torch's default 1e-8).  max_grad_norm = +inf switches the clip off: the
 * kernel's coefficient min(max_grad_norm / (norm + 1e-6), 1) is then exactly 1. */
int mi_optimizer_step_eps(mi_ctx* ctx, float lr, float max_grad_norm, float eps, int32_t adam_step, float* grad_norm_out);
/* op-level test hook: only the distillation loss kernels on caller arrays -- hout [n][A+1], target [n][A].  Out (either may be NULL): rec8
 * the record, dY [n][A+1] the backward seed (value column exactly 0).  n in [1, 65536], A in [1, 16], the mean over n_global * A. */
int mi_op_distill_loss(mi_ctx* ctx, int32_t n, int32_t A, const float* hout, const float* target, int32_t n_global, float* rec8_out, float* dY_out);

/* ---- data-parallel collectives inside the boundary: RCCL over xGMI, one communicator per context (SURVEY 8(b) mi_allreduce_grads,
 *      8(e) C1-C3).  Rank 0 obtains a 128-byte id (mi_comm_unique_id) and hands it to every rank by any host channel
 *      (mi355/dist.py uses torch.distributed.broadcast_object_list); every rank then calls mi_comm_init(id, rank, world).
 *      C1: the flat gradient is summed over the ranks once per optimizer step.  mi_allreduce_arm() before the LAST accumulated
 *      mi_minibatch* of a step makes that backward pass hand its gradient regions to a side stream as they become final (embedder.fc +
 *      heads -- 84 % of the bytes -- right after the first launches of the backward pass, the conv layers after the slab reduction), so
 *      the exchange overlaps the backward pass; mi_allreduce_grads() sends whatever an armed pass has not sent (the whole buffer
 *      when nothing was armed).  mi_optimizer_step waits for the exchange on the device (no host sync).
 *      C2: mi_adv_normalize_global = advantage statistics {count, mean, M2} all-gathered in fp64, merged and applied on the device.
 *      C3 / logging: mi_allreduce_buffer sums the first n floats of MI_PTR_LOSS_STATS / MI_PTR_STATS_RING on the context's stream. */
enum { MI_PTR_GRADS = 0, MI_PTR_LOSS_STATS = 1, MI_PTR_PARAMS = 2, MI_PTR_STATS_RING = 3, MI_PTR_FS_KEYS = 4 };
int mi_comm_unique_id(void* out128, size_t bytes);
int mi_comm_init(mi_ctx* ctx, const void* id128, size_t bytes, int32_t rank, int32_t world);
int mi_comm_destroy(mi_ctx* ctx);
int mi_allreduce_arm(mi_ctx* ctx);
int mi_allreduce_grads(mi_ctx* ctx);
int mi_allreduce_buffer(mi_ctx* ctx, int32_t which, int64_t n_floats);
int mi_adv_normalize_global(mi_ctx* ctx);

/* ---- raw device pointers for collectives issued by the host side (the gloo path of the CPU tests; RCCL runs inside the library, above) */
int mi_device_ptr(mi_ctx* ctx, int32_t which, void** ptr, int64_t* n_floats);
/* two-phase loss finalisation for multi-rank runs (phase 2 after the cross-rank sum of the stats) */
int mi_set_multirank(mi_ctx* ctx, int32_t enabled);   /* 0 single rank; 1 stats all-reduced per minibatch (mi_minibatch_finish); 2 deferred */
int mi_minibatch_finish(mi_ctx* ctx);      /* multirank mode 1: phase 2 + backward after the stats all-reduce */
/* fs_coef != 0 on more than one rank (IMPALA, multirank mode 1; SURVEY 8(e) C3 -- reference agents/ppo.py:148-169, common/model.py:207 on the
 * GLOBAL minibatch): before mi_minibatch, hand over the global minibatch position of every local row (ascending); mi_minibatch then
 * leaves this rank's per-column candidates (value bits << 32 | 0xffffffff - position, 2048 int64) in MI_PTR_FS_KEYS; max-all-reduce them
 * (mi_allreduce_buffer(MI_PTR_FS_KEYS, 2048), or torch.distributed on the aliased buffer) before mi_minibatch_finish, which adds the
 * gradient on the rank that owns each column's winning row and logs the global metric. */
int mi_minibatch_positions(mi_ctx* ctx, const int32_t* global_positions, int32_t n);
/* multirank mode 2 (x_entropy_coef == 0 and fs_coef == 0: the backward pass needs no cross-rank statistic): mi_minibatch runs to
 * completion, this rank's partial loss sums of minibatch k go to ring slot k (MI_PTR_STATS_RING, 32 floats each); once per
 * optimize() the caller sums the first 32 * n_minibatches floats over the ranks and calls mi_loss_log_finalize. */
int mi_loss_log_finalize(mi_ctx* ctx);

/* ---- live kernel timing for bench.py's roofline leg: HIP events recorded on the context's stream around every
 *      conv / pool / GEMM launch.  Classes are reported separately for the rollout phase (phase 0, n = E) and the
 *      update phase (phase 1, n = minibatch).  mi_profile_read fills up to max_rows rows of
 *      {class id, phase, launches, total ms, total samples, total algorithmic bytes, total algorithmic flops}
 *      (layer-boundary model of SURVEY.md 8(d)); names via mi_profile_class_name. */
int mi_profile_enable(mi_ctx* ctx, int32_t enabled);   /* low byte: 0 off, 1 update phase only, 2 rollout + update; bits 8.. = P (0 -> 1):
                                                         * bracket every P-th minibatch of the update phase (sampling keeps the
                                                         * event records' own cost, ~7 us of stream time per launch, out of the run) */
int mi_profile_read(mi_ctx* ctx, double* rows7, int32_t max_rows, int32_t* n_rows, int32_t reset);
const char* mi_profile_class_name(int32_t class_id);

/* ---- op-level entry points for parity tests (host buffers in, host buffers out; NHWC fp32) */
int mi_op_conv3x3(mi_ctx* ctx, int32_t mode /*0 fwd,1 dgrad,2 wgrad; a block's first conv, bf16: 3 conv+pool fwd, 4 / 5 wgrad / dgrad from the pooled gradient,
                  6 / 7 block2.conv's fused dgrad+wgrad launch returning dW / dx*/, int32_t cin, int32_t cout, int32_t hw, int32_t n,
                  const void* in, int32_t in_is_u8, int32_t relu_in, const float* w_ref /*[cout][cin][3][3]*/,
                  const float* bias, const float* res, const float* mask, const float* dout,
                  float* out /*fwd/dgrad: activations; wgrad: [cout][cin][3][3]*/, float* dbias_out);
/* bf16 precision only: the fused residual-block kernels.  mode 0 forward (x, w1, b1, w2, b2 -> out_a = conv1 output,
 * out_y = block output); mode 1 data gradients (x = dy, a_fwd, x_fwd, w1, w2 -> out_a = d conv1-output, out_y = d block-input);
 * mode 3: res1 + res2 forward in one launch with the same (w1, b1, w2, b2) for both blocks (out_a = second conv1 output);
 * mode 2 (16 channels @32x32, 32 channels @16x16) the whole backward in one launch: out_y = d block-input, out_a[0 .. 2*(9*ch*ch+ch)) = {dW1, db1, dW2, db2};
 * mode 4: res1 + res2 forward in one launch with four distinct convs, as the training forward runs them: w1 = [res1.conv1; res1.conv2],
 * b1 = [res1.conv1.bias; res1.conv2.bias], w2 / b2 the same for res2; out_a = [A1; A2] (each block's conv1 output), out_y = [P1; P2]
 * (each block's output), 2 x n x hw x hw x ch floats each.
 * Every mode poisons its outputs before the launch (a skipped element reads back as NaN) and fails with -4 when a kernel writes
 * past the end of an output tensor or into a weight-gradient slab row past its grid.  mi_op_conv3x3 and mi_op_maxpool do the same.
 * Replaces ResidualBlock.forward and its autograd (common/model.py:141-146). */
int mi_op_resblock(mi_ctx* ctx, int32_t mode, int32_t ch, int32_t hw, int32_t n, const float* x, const float* w1, const float* b1,
                   const float* w2, const float* b2, const float* a_fwd, const float* x_fwd, float* out_a, float* out_y);
int mi_op_maxpool(mi_ctx* ctx, int32_t mode /*0 fwd,1 bwd*/, int32_t n, int32_t hw, int32_t c,
                  const float* in, const float* dout, float* out);
int mi_op_gemm(mi_ctx* ctx, int32_t M, int32_t N, int32_t K, const float* A, int64_t sam, int64_t sak,
               const float* B, int64_t sbk, int64_t sbn, float* C);
/* bf16 embedder.fc kernels (2048 -> D, D a multiple of 64 in [64, 512]) on caller data through the production launchers; independent of
 * the context's sizes and precision.  x [n][2048] is rounded to bf16 on the host, W is fc.weight [D][2048] as the kernels index it.
 * mode 0: (x, W, b) -> out = y [n][D] = relu(relu(x) W^T + b), the update-sized forward; mode 1: the same through the rollout-sized forward;
 * mode 2: (dy [n][D], W, x = the ReLU mask source, required) -> out = dx [n][2048] = (dy W) * (x > 0), bf16 widened to fp32;
 * mode 3: (dy, x) with out = gW [D][2048] and out_b = gb [D] holding the initial gradients -> gW += dy^T relu(x), gb += colsum(dy).
 * Refused (-1): D outside the eight widths, n outside [1, 65536] (the upper limit only keeps the hook's allocations sane), mode 2 without x.
 * W goes through launch_fc_pack; production fills the same two images in repack_all_kernel, which only the end-to-end tests compare.
 * Outputs are poisoned and followed by canary bands as in mi_op_resblock. */
int mi_op_fc_bf16(mi_ctx* ctx, int32_t mode, int32_t n, int32_t D, const float* x, const float* W, const float* b, const float* dy,
                  float* out, float* out_b);
/* op-level: the generic GEMM of the linear layers (csrc/gemm.hip, direct and split-K with its reduce) on caller data through the production
 * launchers; independent of the context's sizes and precision.  d0, d1, d2 = (n, in, out) for forms 0 .. 2, (M, N, K) for form 3.
 * form 0: linear_fwd.   A = X [n][in], B = W [out][in], bias [out] or NULL -> C = Y [n][out] = relu?(relu?(X) W^T + b).  Flags RELU_X, RELU_OUT, X_BF16.
 * form 1: linear_dgrad. A = dY [n][out], B = W [out][in], mask [n][in] or NULL -> C = dX [n][in] = (dY W) * (mask > 0).  Flag X_BF16.
 * form 2: linear_wgrad. A = dY [n][out], B = X [n][in]; C = gW [out][in] and gb [out] (out <= 4096) in / out: += dY^T relu?(X), += colsum(dY).
 *         Flags RELU_X, X_BF16.
 * form 3: launch_gemm itself.  strides5 = {sam, sak, sbk, sbn, ldc}: A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn]; C and mask are
 *         [M][ldc] (ldc >= N), bias [N] or NULL.  Flags RELU_OUT, ACCUMULATE (C in / out), USE_WS (without it the workspace is NULL and K is
 *         never split, as the SAE's calls).  ws_floats < 0: the context's workspace size; otherwise an override no larger than it.
 * X_BF16: the activation-typed operands (X; for form 1 the mask and dX) are bf16 on the device: they go up rounded on the host and dX
 * comes back widened.  strides5 is NULL and ws_floats negative outside form 3.
 * plan2 = {split, k_chunk}: the number of K slabs the call ran (1 = one launch without the reduce) and K per slab.
 * Outputs are poisoned and followed by canary bands as in mi_op_resblock, in / out targets start from the caller's values, and the slabs of
 * a split call are poisoned too; with ldc > N, columns N .. ldc - 1 of C come back as the poison (all-ones words) or the call fails with -4.
 * Refused (-1): a size below 1 or above 65536, a tensor above 2^26 elements (the limits only keep the hook's allocations sane), ws_floats
 * above the context's, a flag or operand the form does not have. */
enum { MI_LIN_RELU_X = 1, MI_LIN_RELU_OUT = 2, MI_LIN_X_BF16 = 4, MI_LIN_ACCUMULATE = 8, MI_LIN_USE_WS = 16 };
int mi_op_linear(mi_ctx* ctx, int32_t form, int32_t d0, int32_t d1, int32_t d2, const int64_t* strides5, int32_t flags, int64_t ws_floats,
                 const float* A, const float* B, const float* bias, const float* mask, float* C, float* gb, int32_t* plan2);
/* op-level: the fixed-order sums behind every weight and bias gradient (csrc/reduce.hip) on caller data through the production launchers,
 * any context.  The targets are in / out (the kernels accumulate) and sit in poisoned, canary-banded buffers as in mi_op_resblock.
 * mode 0: launch_reduce_slabs.  src [a = nslab][b = slab_len] (src_len = a * b); dst_w [n_w] += the sums of elements [0, n_w), dst_b [n_b] +=
 *         those of [n_w, n_w + n_b); elements past n_w + n_b are dropped.  dst_b is NULL exactly when n_b = 0 (the column sum's use).
 * mode 1: launch_reduce_all_slabs, n_desc (<= 64) layers in one launch.  desc: n_desc x {src_off, w_off, b_off, nslab, slab_len, n_w} (int64;
 *         offsets, slab_len and n_w multiples of 4); src = the slab workspace (src_len floats), dst_w = one flat gradient vector of n_w floats:
 *         layer k adds its first n_w[k] sums at w_off[k] and the other slab_len[k] - n_w[k] at b_off[k].  a, b, ld, dst_b, n_b unused.
 * mode 2: launch_colsum_acc.  src = dY [a = M][ld], dst_w = db [n_w = b = N] += the column sums of the first N columns; the workspace is
 *         exactly the engine's 64 x 4096 floats.  N > 4096 is refused by the launcher (-4) before anything is launched. */
int mi_op_reduce(mi_ctx* ctx, int32_t mode, const float* src, int64_t src_len, int32_t a, int32_t b, int32_t ld, const int64_t* desc,
                 int32_t n_desc, float* dst_w, int64_t n_w, float* dst_b, int32_t n_b);
/* op-level: the optimizer tail on caller vectors -- partial sums of squares, then clip + Adam + zero_grad, with the host scalars from the
 * code mi_optimizer_step and mi_sae_optimizer_step use.  p, g, m, v [n] in / out; *gnorm_out = the unclipped gradient norm.
 * variant 0: one vector, 128 partial sums (mi_optimizer_step).  variant 1: a second vector p2, g2, m2, v2 [n2 >= 4] under the same norm (256
 * partial sums), stepped in four pieces [off5[k], off5[k + 1]) with 0 = off5[0] < .. < off5[4] = n2 (mi_optimizer_step after mi_gru_train).
 * variant 2: the SAE agent's kernel with torch's own constants (mi_sae_optimizer_step).  The second vector is NULL / 0 outside variant 1. */
int mi_op_adam(mi_ctx* ctx, int32_t variant, int64_t n, float* p, float* g, float* m, float* v, int64_t n2, float* p2, float* g2, float* m2,
               float* v2, const int64_t* off5, float lr, float max_norm, int32_t step, float* gnorm_out);
/* op-level: the cross-rank merge of R (<= 4096) advantage statistics {count, mean, M2} (fp64) -> stats3_out, as mi_adv_normalize_global runs it */
int mi_op_adv_merge(mi_ctx* ctx, const double* all, int32_t R, double* stats3_out);
/* op-level: the policy / value heads at update size (csrc/heads.hip) on caller data through the production launchers, any context.
 * mode 0: heads_fwd_kernel.  out = hout [n][O] = feat [n][256] Wh^T + bh; H must be 256.  dY, gW, gb unused.
 * mode 1: heads_bwd_kernel + its slab sum, H in [1, 256].  out = dfeat [n][H] = (dY [n][O] Wh) * (feat > 0 if relu_mask); gW [O][H] and gb [O]
 *         hold the initial gradients and receive += dY^T feat, += colsum(dY).  The workspace is the 512 * (O*H + O) floats the launcher asks
 *         for, poisoned.  bh unused.
 * Refused (-1) before any launch: O outside [1, 16], mode 0 with H != 256, mode 1 with H > 256, n outside [1, 65536].
 * Outputs are poisoned and followed by canary bands as in mi_op_resblock. */
int mi_op_heads(mi_ctx* ctx, int32_t mode, int32_t n, int32_t H, int32_t O, const float* feat, const float* Wh, const float* bh, const float* dY,
                int32_t relu_mask, float* out, float* gW, float* gb);
/* op-level: the rollout's sampling kernels on caller data, any context.  (a) heads_sample_kernel on feat [n][H], Wh [A + 1][H], bh [A + 1]
 * (H in [1, 4096]: every staging branch) with hout requested and no staging / flag / ticket pointers; (b) sample_kernel and (c)
 * logp_all_kernel on the hout that (a) wrote.  u [n] = the uniforms, or NULL: Philox(seed, counter + row).
 * Out: act2 [2][n] and logp2 [2][n] of (a), (b); value3 [3][n] of (a), (b), (c); pack [n][3] and hout [n][A + 1] of (a); table [n][A] of (c). */
int mi_op_sample(mi_ctx* ctx, int32_t n, int32_t H, int32_t A, const float* feat, const float* Wh, const float* bh, const float* u, uint64_t seed,
                 uint64_t counter, int32_t value_from_logits, int32_t* act2, float* logp2, float* value3, float* pack, float* hout, float* table);
/* op-level: the PPO loss kernels alone (csrc/loss.hip) on caller arrays, any context.  hout [n][A + 1]; idx [n] into act, old_logp, old_value,
 * ret, adv [n_rows]; means and gradients scale with 1 / n_global; hp->fs_coef must be 0.
 * mode 0: loss_fwd_kernel, loss_finalize_kernel (phase 3), loss_bwd_kernel: the two-phase path, the only one where x_entropy_coef != 0 is legal.
 * mode 1: loss_fwd_seg_kernel with the gradient in the same pass + loss_finalize_seg_kernel (phase 3) over n_seg <= 16 segments of seg_n[k] >= 0
 *         consecutive samples (sum n), as mi_minibatch_multi; x_entropy_coef != 0 is refused.  An empty segment's record is not meaningful.
 * Out: dY [n][A + 1]; partial [blocks][8 + A], blocks = sum ceil(segment / 64) (columns 0..2 and 8..8+A written, the others poison);
 * stats [segments][32] (0 pi_loss 1 value_loss 2 entropy 3 x_ent 4 total 5 fs 6 marg, 8.. q[A]; the others poison); log [segments][8]. */
int mi_op_ppo_loss(mi_ctx* ctx, int32_t mode, int32_t n, int32_t A, const float* hout, const int32_t* idx, int32_t n_rows, const int32_t* act,
                   const float* old_logp, const float* old_value, const float* ret, const float* adv, const mi_hparams* hp,
                   int32_t value_from_logits, int32_t n_global, const int32_t* seg_n, int32_t n_seg, float* dY_out, float* partial_out,
                   float* stats_out, float* log_out);
int mi_selftest_mfma(mi_ctx* ctx, float* max_err);
/* what the last mi_minibatch left in the activation buffers (first n samples), fp32 NHWC: which = 8 * block + k, k = 0 pooled map,
 * 1 res1.conv1 out, 2 res1 out, 3 res2.conv1 out, 4 block out, 5 max-pool arg-max (window position ky*3+kx); which = 100: features
 * (after mi_minibatch_rec: the embedder output x; 101 = h_t, 102 = dX of that pass).
 * Lets a parity test run the oracle's backward pass on the ENGINE's forward tensors (teacher forcing, tests/test_gpu_bf16.py). */
int mi_debug_read(mi_ctx* ctx, int32_t which, int32_t n, float* out);
/* The production sampler's generator (dist.sample() of agents/ppo.py:77 is torch's; here Philox4x32-10 keyed by (seed, t*E + e)):
 * n x {c0,c1,c2,c3,k0,k1} in; out4 = n x 4 output words of the ten-round bijection (checked against the Random123 known-answer
 * vectors), u_out = n uniforms exactly as the sample kernels draw them for seed = k0 | k1 << 32, counter = c0 | c1 << 32. */
int mi_debug_philox(mi_ctx* ctx, const uint32_t* ctr_key6, int32_t n, uint32_t* out4, float* u_out);
/* test hook: the pipelined rollout's fused GRU step on caller data -- n rows, width H (a multiple of 64 in [64, 512], independent of the
 * context's), x / h: n x H, done: n, weights in nn.GRU's layout (common/model.py:212-225); h_out = h' = GRU(x, h (1 - done)), h_copy (may
 * be NULL) = the kernel's second copy of h' (the hidden ring's next slot in the rollout) */
int mi_debug_gru_step(mi_ctx* ctx, int32_t n, int32_t H, const float* x, const float* h, const float* done, const float* w_ih,
                      const float* w_hh, const float* b_ih, const float* b_hh, float* h_out, float* h_copy);
/* test hook: the GRU over a trajectory (the sequential kernels of mi_minibatch_rec and the GEMMs around them; GRU.forward's training branch,
 * common/model.py:226-277, and its autograd) on caller data -- n envs x T steps, rows time-major (row t * n + i), width H (a multiple of 64 in
 * [64, 512], independent of the context's); x: T*n x H, h0: n x H, mask: T*n (multiplies the state that enters step t), weights in nn.GRU's
 * layout.  out_h = h_t of all rows.  dOut (T*n x H = dL/dh_t, or NULL: forward only) -> dX (T*n x H), dW_ih, dW_hh (3H x H), db_ih, db_hh (3H). */
int mi_debug_gru_seq(mi_ctx* ctx, int32_t T, int32_t n, int32_t H, const float* x, const float* h0, const float* mask, const float* w_ih,
                     const float* w_hh, const float* b_ih, const float* b_hh, const float* dOut, float* out_h, float* dX, float* dW_ih,
                     float* dW_hh, float* db_ih, float* db_hh);
/* measurement hook: wall-clock microseconds per policy step of slot t (the step's launches + a stream wait, `iters` times), issued
 * eagerly (mode 0) or as one replay of a hipGraph captured from the same launches (mode 1) */
int mi_debug_step_latency(mi_ctx* ctx, int32_t t, int32_t iters, int32_t mode, float* us_out);
/* measurement hook: do the lanes run side by side?  Launches on the stream of every group in `mask` (bit g = group g of this context)
 * one 64-thread workgroup that executes s_sleep 127 `iters` times (capped at 4096; a fixed trip count, nothing to wait on), waits for
 * all of them and returns the host wall time from first launch to last completion in microseconds. */
int mi_debug_lane_probe(mi_ctx* ctx, int32_t mask, int32_t iters, float* usec);
/* bit 0 set: rollout-sized bf16 inference passes use the separate block-2 / block-3 kernels instead of the fused launch
 * (rollout_bf16.hip) -- the A side of the bit-equality test of the two paths;
 * bit 2 set: a group's frames always go up by DMA copy, never pulled by a kernel (A/B timing);
 * bit 4 set: a minibatch pass keeps the logged statistics and embedder.fc's weight gradient on the main stream instead of
 * forking them onto the side stream -- the A side of the bit-equality test of the two orders */
int mi_debug_flags(mi_ctx* ctx, int32_t flags);
/* out = {device allocations, pinned host allocations, events} that the contexts of this process (and the agents' state on them) hold
 * right now.  Destroying a context takes each count back to what it was before mi_create. */
int mi_debug_live_resources(int64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
