"""Thin ctypes layer over the C ABI in include/mi355ppo.h.

There is deliberately NO fallback: if libmi355ppo.so is missing or no MI355X is visible, creating an
Engine raises.  (The CPU restatement under oracle/ is test infrastructure and is never imported here.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ARCH_IMPALA, ARCH_MLP = 0, 1
F_REW, F_DONE, F_VALUE, F_LOGP, F_ADV, F_RET, F_ACT = range(7)
PTR_GRADS, PTR_LOSS_STATS, PTR_PARAMS, PTR_STATS_RING, PTR_FS_KEYS = 0, 1, 2, 3, 4
LOSS_FIELDS = ("pi_loss", "value_loss", "entropy", "x_ent", "total", "fs", "marg", "_pad")


class EngineError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("arch", C.c_int32), ("n_steps", C.c_int32), ("n_envs", C.c_int32), ("n_actions", C.c_int32),
                ("obs_dim", C.c_int32), ("mlp_depth", C.c_int32), ("mlp_width", C.c_int32), ("out_dim", C.c_int32),
                ("max_batch", C.c_int32), ("device", C.c_int32), ("precision", C.c_int32), ("value_from_logits", C.c_int32),
                ("reserved", C.c_int32 * 4),
                ("stream", C.c_void_p)]


class _HParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("eps_clip", "value_coef", "entropy_coef", "x_entropy_coef",
                                         "entropy_multiplier", "fs_coef")]


class _CartPoleParams(C.Structure):
    _fields_ = [("low", C.c_double * 9), ("high", C.c_double * 9), ("x_threshold", C.c_double), ("theta_threshold", C.c_double),
                ("max_steps", C.c_int32)]


class _CartPoleSwingParams(C.Structure):
    _fields_ = [("low", C.c_double * 9), ("high", C.c_double * 9), ("x_threshold", C.c_double), ("max_steps", C.c_int32)]


class _MountainCarParams(C.Structure):
    _fields_ = [("low", C.c_double * 5), ("high", C.c_double * 5), ("left_boundary", C.c_double), ("max_speed", C.c_double),
                ("force", C.c_double), ("goal_velocity", C.c_double), ("max_steps", C.c_int32), ("sparse_rewards", C.c_int32)]


class _IplHParams(C.Structure):
    _fields_ = [("gamma", C.c_float), ("alpha", C.c_float), ("entropy_coef", C.c_float), ("flags", C.c_int32)]


IPL_ENTROPY_MODIFIED, IPL_REWARD_INCENTIVE, IPL_ADV_INCENTIVE, IPL_DEBUG_ZERO_OBS_SEED = 1, 2, 4, 256
IPL_FIELDS = ("entropy", "mutual_info", "total", "rew_corr", "gamma", "alpha_loss", "alpha", "pred_reward")


def lib_path():
    return os.path.join(_HERE, "libmi355ppo.so")


EXPORTS = ("mi_last_error mi_create mi_destroy mi_sync mi_host_alloc mi_host_free mi_host_register mi_host_unregister mi_param_count mi_set_params "
           "mi_get_params mi_copy_params mi_get_grads mi_set_adam_state mi_get_adam_state mi_put_obs mi_get_obs mi_put_step "
           "mi_put_policy_outputs mi_read_field mi_write_field mi_policy_step mi_rollout_step mi_rollout_groups mi_rollout_lane_info mi_rollout_submit mi_rollout_wait mi_predict_staged mi_value_saliency mi_commit_staged mi_set_gru mi_rec_state mi_get_hidden mi_rec_begin mi_get_hidden_ring mi_forward_rec mi_forward mi_compute_estimates "
           "mi_adv_stats mi_adv_apply mi_minibatch mi_minibatch_multi mi_minibatch_fused mi_optimizer_step mi_loss_log_read mi_device_ptr "
           "mi_set_multirank mi_minibatch_finish mi_loss_log_finalize mi_profile_enable mi_profile_read mi_profile_class_name mi_op_conv3x3 mi_op_resblock mi_op_maxpool mi_op_gemm mi_op_fc_bf16 mi_op_linear mi_op_reduce mi_op_adam mi_op_adv_merge mi_op_heads mi_op_sample mi_op_ppo_loss mi_selftest_mfma mi_debug_read mi_debug_flags mi_comm_unique_id mi_comm_init mi_comm_destroy mi_allreduce_arm mi_allreduce_grads mi_allreduce_buffer mi_adv_normalize_global mi_minibatch_positions mi_debug_philox mi_debug_gru_step mi_debug_step_latency mi_debug_lane_probe mi_debug_live_resources "
           "mi_gru_train mi_minibatch_rec mi_get_gru mi_get_gru_grads mi_get_gru_adam_state mi_set_gru_adam_state mi_debug_gru_seq "
           "mi_sae_create mi_sae_destroy mi_sae_param_count mi_sae_set_params mi_sae_get_params mi_sae_get_grads mi_sae_set_adam_state mi_sae_get_adam_state mi_sae_put_ring "
           "mi_sae_get_hidden mi_sae_get_logits mi_sae_step mi_sae_minibatch mi_sae_probe_minibatch mi_sae_optimizer_step mi_sae_debug_forward "
           "mi_ipl_minibatch mi_ipl_read_pred mi_predict_greedy mi_op_ipl_loss mi_op_ipl_greedy "
           "mi_distill_label mi_distill_minibatch mi_distill_loss mi_optimizer_step_eps mi_op_distill_loss mi_distill_targets "
           "mi_env_cartpole_create mi_env_cartpole_swing_create mi_env_mountain_car_create mi_env_reset mi_env_step mi_env_rollout mi_env_rollout_resident mi_env_evaluate mi_env_get_state mi_env_set_state").split()


def load_library():
    """dlopen the in-tree library (built by `make -C csrc` / __graft_entry__.build())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise EngineError(f"{path} not found: build it with `make -C train-procgen-pytorch_amd/csrc` "
                          "(python __graft_entry__.py build).  There is no CPU fallback.")
    lib = C.CDLL(path)
    lib.mi_last_error.restype = C.c_char_p
    lib.mi_param_count.restype = C.c_int64
    lib.mi_sae_param_count.restype = C.c_int64
    lib.mi_host_alloc.restype = C.c_void_p
    lib.mi_host_alloc.argtypes = [C.c_size_t]
    lib.mi_host_free.argtypes = [C.c_void_p]
    lib.mi_host_free.restype = None
    lib.mi_profile_class_name.restype = C.c_char_p
    lib.mi_host_register.argtypes = [C.c_void_p, C.c_size_t]
    lib.mi_host_unregister.argtypes = [C.c_void_p]
    # the per-env-step entry point is called T+1 times per iteration: declared argtypes let plain ints / addresses through
    # without building ctypes wrapper objects on every call
    lib.mi_rollout_step.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mi_rollout_submit.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.mi_rollout_wait.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    _LIB = lib
    return lib


def live_resources():
    """(device allocations, pinned host allocations, events) that the contexts of this process hold right now: each is back at its
    earlier value once a context is closed (mi_debug_live_resources)."""
    out = (C.c_int64 * 3)()
    if load_library().mi_debug_live_resources(out) != 0:
        raise EngineError("mi_debug_live_resources failed")
    return tuple(int(v) for v in out)


def _fp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class Engine:
    """One device context (one GPU).  Methods mirror the C entry points one to one."""

    def __init__(self, arch, n_steps, n_envs, n_actions, max_batch, obs_dim=0, mlp_depth=0, mlp_width=0, out_dim=256,
                 device=0, stream=None, precision="fp32", value_from_logits=False):
        self.lib = load_library()
        self.arch = ARCH_IMPALA if arch in ("impala", ARCH_IMPALA) else ARCH_MLP
        cfg = _Config(arch=self.arch, n_steps=n_steps, n_envs=n_envs, n_actions=n_actions, obs_dim=obs_dim,
                      mlp_depth=mlp_depth, mlp_width=mlp_width, out_dim=out_dim, max_batch=max_batch, device=device,
                      precision={"fp32": 0, "bf16": 1}[precision], value_from_logits=int(bool(value_from_logits)), stream=stream)
        self.precision = precision
        self.value_from_logits = bool(value_from_logits)      # CategoricalPolicy(logsumexp_logits_is_v=True): value = logsumexp(logits)
        self.T, self.E, self.A, self.max_batch = n_steps, n_envs, n_actions, max(max_batch, n_envs)
        self.H = (out_dim or 256) if self.arch == ARCH_IMPALA else out_dim
        self.obs_dim = obs_dim
        self._ctx = C.c_void_p()
        self._chk(self.lib.mi_create(C.byref(cfg), C.byref(self._ctx)))
        self.n_params = int(self.lib.mi_param_count(self._ctx))
        self._pinned = []
        self._registered = {}          # address -> (nbytes, array kept alive): caller buffers page-locked in place (mi_host_register)
        self._register_refused = 0

    # ------------------------------------------------------------------ plumbing
    def _chk(self, rc):
        if rc != 0:
            raise EngineError(f"libmi355ppo error {rc}: {self.lib.mi_last_error().decode()}")

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            for p in self._pinned:
                self.lib.mi_host_free(C.c_void_p(p))
            self._pinned = []
            for p in list(getattr(self, "_registered", {})):
                self.lib.mi_host_unregister(p)
            self._registered = {}
            if getattr(self, "sae_dim", None) is not None:          # (optional: the context owns the SAE agent's state and mi_destroy releases it)
                self.lib.mi_sae_destroy(self._ctx)
                self.sae_dim = None
            self.lib.mi_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self.lib.mi_sync(self._ctx))

    def pinned(self, shape, dtype):
        """numpy array over page-locked host memory owned by this engine."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.mi_host_alloc(n)
        if not p:
            raise EngineError("mi_host_alloc failed")
        self._pinned.append(p)
        self._pinned_n = getattr(self, "_pinned_n", {})
        self._pinned_n[p] = n
        buf = (C.c_char * n).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    MAX_REGISTERED = 64

    def dma_ready(self, arr):
        """True if `arr` (C-contiguous numpy) can be handed to rollout_submit / put_obs as it is: memory from Engine.pinned, or
        caller memory page-locked in place now (mi_host_register, once per buffer: an env that hands its frames out in the same few
        buffers step after step -- Procgen's rgb buffer, a pool -- is uploaded from where it lies, with no staging copy).  False when
        the runtime refuses the range or the env keeps producing new buffers (more than MAX_REGISTERED distinct ones): stage it."""
        addr = arr.__array_interface__['data'][0]
        hit = self._registered.get(addr)
        if hit is not None:
            return hit[0] >= arr.nbytes
        if getattr(self, "_pinned_n", {}).get(addr, -1) >= arr.nbytes:
            return True
        if len(self._registered) >= self.MAX_REGISTERED or self._register_refused >= 8 or not arr.flags.c_contiguous:
            return False
        base = arr
        while isinstance(getattr(base, "base", None), np.ndarray):
            base = base.base
        if self.lib.mi_host_register(addr, arr.nbytes) != 0:
            self._register_refused += 1
            return False
        self._registered[addr] = (arr.nbytes, base)
        return True

    # ------------------------------------------------------------------ parameters
    def set_params(self, flat):
        flat = _f32(flat)
        self._chk(self.lib.mi_set_params(self._ctx, _fp(flat), C.c_int64(flat.size)))

    def get_params(self):
        out = np.empty(self.n_params, np.float32)
        self._chk(self.lib.mi_get_params(self._ctx, _fp(out), C.c_int64(out.size)))
        return out

    def copy_params_from(self, src):
        """This context's parameters := src's (another Engine on the same GPU), device to device, ordered on both streams."""
        self._chk(self.lib.mi_copy_params(self._ctx, src._ctx))

    def get_grads(self):
        out = np.empty(self.n_params, np.float32)
        self._chk(self.lib.mi_get_grads(self._ctx, _fp(out), C.c_int64(out.size)))
        return out

    def set_adam_state(self, m, v):
        m, v = _f32(m), _f32(v)
        self._chk(self.lib.mi_set_adam_state(self._ctx, _fp(m), _fp(v), C.c_int64(m.size)))

    def get_adam_state(self):
        m, v = np.empty(self.n_params, np.float32), np.empty(self.n_params, np.float32)
        self._chk(self.lib.mi_get_adam_state(self._ctx, _fp(m), _fp(v), C.c_int64(m.size)))
        return m, v

    # ------------------------------------------------------------------ rollout storage
    def put_obs(self, t, obs):
        want = np.uint8 if self.arch == ARCH_IMPALA else np.float32
        obs = np.ascontiguousarray(obs, dtype=want)
        self._chk(self.lib.mi_put_obs(self._ctx, C.c_int32(t), _fp(obs), C.c_size_t(obs.nbytes)))
        return obs      # caller keeps it alive until the next sync

    def get_obs(self, t):
        if self.arch == ARCH_IMPALA:
            out = np.empty((self.E, 64, 64, 3), np.uint8)
        else:
            out = np.empty((self.E, self.obs_dim), np.float32)
        self._chk(self.lib.mi_get_obs(self._ctx, C.c_int32(t), _fp(out), C.c_size_t(out.nbytes)))
        return out

    def put_step(self, t, rew, done):
        rew, done = _f32(rew), _f32(done)
        self._chk(self.lib.mi_put_step(self._ctx, C.c_int32(t), _fp(rew), _fp(done)))
        return rew, done

    def put_policy_outputs(self, t, act=None, logp=None, value=None):
        act = None if act is None else np.ascontiguousarray(act, dtype=np.int32)
        logp = None if logp is None else _f32(logp)
        value = None if value is None else _f32(value)
        self._chk(self.lib.mi_put_policy_outputs(self._ctx, C.c_int32(t), _fp(act), _fp(logp), _fp(value)))

    def read_field(self, field):
        n = (self.T + 1) * self.E if field == F_VALUE else self.T * self.E
        out = np.empty(n, np.float32)
        self._chk(self.lib.mi_read_field(self._ctx, C.c_int32(field), _fp(out), C.c_int64(n)))
        return out.reshape(-1, self.E)

    def write_field(self, field, arr):
        arr = _f32(arr).reshape(-1)
        self._chk(self.lib.mi_write_field(self._ctx, C.c_int32(field), _fp(arr), C.c_int64(arr.size)))

    def read_field_into(self, field, out):
        """read_field into a caller array (C-contiguous float32 of the field's size, e.g. a Storage's pinned mirror): no allocation."""
        if out.dtype != np.float32 or not out.flags.c_contiguous:
            raise EngineError("read_field_into needs a C-contiguous float32 array")
        self._chk(self.lib.mi_read_field(self._ctx, C.c_int32(field), _fp(out), C.c_int64(out.size)))
        return out

    # ------------------------------------------------------------------ device-resident envs (mi_env_*): cart-pole, swing-up cart-pole, mountain car
    _env_width = 0          # columns of the env's state = the observation width: set by the create call from its params struct

    def _env_create(self, create, params, low, high, seed, *scalars):
        """What the create calls share: low / high as the params struct's arrays (their length is the env's width), the 64-bit seed."""
        W = dict(params._fields_)["low"]._length_
        low, high = np.asarray(low, np.float64).reshape(W), np.asarray(high, np.float64).reshape(W)
        p = params((C.c_double * W)(*low), (C.c_double * W)(*high), *scalars)
        self._chk(create(self._ctx, C.byref(p), C.c_uint64(int(seed) & (2 ** 64 - 1))))
        self._env_width = W

    def env_cartpole_create(self, low, high, x_threshold, theta_threshold, max_steps, seed=0):
        self._env_create(self.lib.mi_env_cartpole_create, _CartPoleParams, low, high, seed, float(x_threshold), float(theta_threshold), int(max_steps))

    def env_cartpole_swing_create(self, low, high, x_threshold, max_steps, seed=0):
        self._env_create(self.lib.mi_env_cartpole_swing_create, _CartPoleSwingParams, low, high, seed, float(x_threshold), int(max_steps))

    def env_mountain_car_create(self, low, high, left_boundary, max_speed, force, goal_velocity, max_steps, sparse_rewards=True, seed=0):
        self._env_create(self.lib.mi_env_mountain_car_create, _MountainCarParams, low, high, seed, float(left_boundary), float(max_speed),
                         float(force), float(goal_velocity), int(max_steps), int(bool(sparse_rewards)))

    def env_reset(self):
        """Every env starts a fresh episode; observation slot 0 holds float32(state).  Asynchronous."""
        self._chk(self.lib.mi_env_reset(self._ctx))

    def env_state(self):
        """-> (state (E, W) float64, n_steps (E,) int32, episode (E,) int64) as they are on the device; W = the created env's state width."""
        s, n, ep = np.empty((self.E, self._env_width or 1), np.float64), np.empty(self.E, np.int32), np.empty(self.E, np.int64)
        self._chk(self.lib.mi_env_get_state(self._ctx, _fp(s), _fp(n), _fp(ep)))
        return s, n, ep

    def env_set_state(self, state=None, n_steps=None, episode=None):
        s = None if state is None else np.ascontiguousarray(state, dtype=np.float64)
        n = None if n_steps is None else np.ascontiguousarray(n_steps, dtype=np.int32)
        ep = None if episode is None else np.ascontiguousarray(episode, dtype=np.int64)
        for a, size, name in ((s, (self._env_width or 1) * self.E, "state"), (n, self.E, "n_steps"), (ep, self.E, "episode")):
            if a is not None and a.size != size:
                raise EngineError(f"env_set_state: {name} must have {size} elements")
        self._chk(self.lib.mi_env_set_state(self._ctx, _fp(s), _fp(n), _fp(ep)))

    def env_step(self, act):
        """One env step on caller actions -> (obs (E, W), rew (E,), done (E,)) float32 on the host; the rings are not touched."""
        act = np.ascontiguousarray(act, dtype=np.int64).reshape(-1)
        if act.size != self.E:
            raise EngineError(f"env_step: {act.size} actions for {self.E} envs")
        obs, rew, done = np.empty((self.E, self._env_width or 1), np.float32), np.empty(self.E, np.float32), np.empty(self.E, np.float32)
        self._chk(self.lib.mi_env_step(self._ctx, _fp(act), _fp(obs), _fp(rew), _fp(done)))
        return obs, rew, done

    def env_rollout(self, seed=0, resident=False):
        """The whole rollout -- T + 1 policy steps, T env steps -- enqueued on the engine's stream; returns without waiting.  resident: as ONE
        kernel launch (mi_env_rollout_resident: same rings, state, sampling counters and reset stream; values / log-probabilities differ
        from the chain's by fp32 summation order) instead of the chain of launches."""
        call = self.lib.mi_env_rollout_resident if resident else self.lib.mi_env_rollout
        self._chk(call(self._ctx, C.c_uint64(seed)))

    def env_evaluate(self, episodes, seed=0, greedy=False, first_episode=1 << 40, starts=None):
        """Every env runs exactly `episodes` whole episodes of the engine's policy in ONE kernel launch (mi_env_evaluate) -> dict of numpy
        arrays, (E, K) each: ret float64 (the fp64 sum of the env's rewards), length int32, terminated int32 (the env's own flag: 0 for a
        truncation at max_steps), value0 float32 (the value head at the episode's first observation), and start (E, K, W) float64 (the
        state the episode began in).  Episode i of env e starts at the reset stream's episode first_episode + i -- the default keeps
        evaluation episodes disjoint from any training run's, whose counters start at 1 -- or at starts[e, i] (E, K, W).  greedy: the first
        arg-max of the log-probabilities instead of the sampler's uniform of (seed, t * E + e).  The env's state and the rollout rings are
        neither read nor written.  Synchronises."""
        K, W = int(episodes), self._env_width or 1
        n = max(K, 0)
        if starts is not None:
            starts = np.ascontiguousarray(starts, dtype=np.float64)
            if starts.size != self.E * n * W:
                raise EngineError(f"env_evaluate: starts must have {self.E} x {n} x {W} elements")
        out = dict(ret=np.zeros((self.E, n), np.float64), length=np.zeros((self.E, n), np.int32), terminated=np.zeros((self.E, n), np.int32),
                   value0=np.zeros((self.E, n), np.float32), start=np.zeros((self.E, n, W), np.float64))
        self._chk(self.lib.mi_env_evaluate(self._ctx, C.c_int32(K), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_int32(int(bool(greedy))),
                                           C.c_int64(int(first_episode)), _fp(starts), _fp(out["ret"]), _fp(out["length"]), _fp(out["terminated"]),
                                           _fp(out["value0"]), _fp(out["start"])))
        return out

    # ------------------------------------------------------------------ policy
    def policy_step(self, t, seed=0, u=None, want_outputs=True):
        u = None if u is None else _f32(u)
        if not want_outputs:
            self._chk(self.lib.mi_policy_step(self._ctx, C.c_int32(t), C.c_uint64(seed), _fp(u), None, None, None))
            return None
        act = np.empty(self.E, np.int64)
        logp = np.empty(self.E, np.float32)
        val = np.empty(self.E, np.float32)
        self._chk(self.lib.mi_policy_step(self._ctx, C.c_int32(t), C.c_uint64(seed), _fp(u), _fp(act), _fp(logp), _fp(val)))
        return act, logp, val

    def rollout_step(self, t, rew_prev=None, done_prev=None, seed=0, u=None):
        """store(t-1)'s reward/done + policy step on slot t in one call (one packed upload, one packed read-back).
        (Called 257 times per iteration between GPU steps: one result buffer, raw pointers instead of .ctypes -- 2 us per call.)"""
        u = None if u is None else _f32(u)
        if rew_prev is not None and (not isinstance(rew_prev, np.ndarray) or rew_prev.dtype != np.float32 or not rew_prev.flags.c_contiguous):
            rew_prev = _f32(rew_prev)
        if done_prev is not None and (not isinstance(done_prev, np.ndarray) or done_prev.dtype != np.float32 or not done_prev.flags.c_contiguous):
            done_prev = _f32(done_prev)
        E = self.E
        out = np.empty(4 * E, np.float32)                       # [act as int64 | logp | value]
        p = out.__array_interface__['data'][0]
        rc = self.lib.mi_rollout_step(self._ctx, t, None if rew_prev is None else rew_prev.__array_interface__['data'][0],
                                      None if done_prev is None else done_prev.__array_interface__['data'][0], seed,
                                      None if u is None else u.__array_interface__['data'][0], p, p + 8 * E, p + 12 * E)
        if rc:
            self._chk(rc)
        return out[:2 * E].view(np.int64), out[2 * E:3 * E], out[3 * E:]

    # pipelined rollout: env groups, submit / wait (see include/mi355ppo.h)
    def rollout_groups(self, n_groups):
        self._chk(self.lib.mi_rollout_groups(self._ctx, C.c_int32(n_groups)))
        self.n_groups = n_groups

    def lane_info(self):
        """[(stream priority, stream id)] of this engine's env groups; two groups share a lane exactly when their ids are equal"""
        n, prio, sid = C.c_int32(0), (C.c_int32 * 4)(), (C.c_uint64 * 4)()
        self._chk(self.lib.mi_rollout_lane_info(self._ctx, C.byref(n), prio, sid))
        return [(int(prio[g]), int(sid[g])) for g in range(n.value)]

    def rollout_submit(self, t, group, frames=None, rew_prev=None, done_prev=None, seed=0, u=None):
        """frames: this group's observations in PINNED memory (Engine.pinned), kept unchanged until rollout_wait(group); None = slot t holds them."""
        addr = lambda a: None if a is None else a.__array_interface__['data'][0]
        if rew_prev is not None and (rew_prev.dtype != np.float32 or not rew_prev.flags.c_contiguous):
            rew_prev = _f32(rew_prev)
        if done_prev is not None and (done_prev.dtype != np.float32 or not done_prev.flags.c_contiguous):
            done_prev = _f32(done_prev)
        u = None if u is None else _f32(u)
        if frames is not None and not frames.flags.c_contiguous:
            raise EngineError("rollout_submit needs a contiguous (pinned) frame buffer")
        rc = self.lib.mi_rollout_submit(self._ctx, t, group, addr(frames), 0 if frames is None else frames.nbytes, addr(rew_prev), addr(done_prev), seed, addr(u))
        if rc:
            self._chk(rc)
        self._keep_alive = (frames, rew_prev, done_prev, u)

    def rollout_wait(self, group):
        n = self.E // getattr(self, "n_groups", 1)
        out = np.empty(4 * n, np.float32)                       # [act as int64 | logp | value]
        p = out.__array_interface__['data'][0]
        rc = self.lib.mi_rollout_wait(self._ctx, group, p, p + 8 * n, p + 12 * n)
        if rc:
            self._chk(rc)
        return out[:2 * n].view(np.int64), out[2 * n:3 * n], out[3 * n:]

    def rollout_wait_into(self, group, act_addr, logp_addr, val_addr):
        """rollout_wait writing into caller arrays (raw addresses of this group's int64 / float32 / float32 slices): the collector's
        per-group-step call, no allocation."""
        rc = self.lib.mi_rollout_wait(self._ctx, group, act_addr, logp_addr, val_addr)
        if rc:
            self._chk(rc)

    def predict_staged(self, obs, seed=0, counter=0, u=None):
        want = np.uint8 if self.arch == ARCH_IMPALA else np.float32
        obs = np.ascontiguousarray(obs, dtype=want)
        u = None if u is None else _f32(u)
        act, logp, val = np.empty(self.E, np.int64), np.empty(self.E, np.float32), np.empty(self.E, np.float32)
        self._chk(self.lib.mi_predict_staged(self._ctx, _fp(obs), C.c_size_t(obs.nbytes), C.c_uint64(seed),
                                             C.c_uint64(counter), _fp(u), _fp(act), _fp(logp), _fp(val)))
        return act, logp, val

    def value_saliency(self, obs, seed=0, counter=0, u=None):
        """predict_staged + d value / d observation: (act, logp, value, grad) with grad (E,64,64,3) NHWC for IMPALA / (E,obs_dim) for the MLP."""
        want = np.uint8 if self.arch == ARCH_IMPALA else np.float32
        obs = np.ascontiguousarray(obs, dtype=want)
        u = None if u is None else _f32(u)
        act, logp, val = np.empty(self.E, np.int64), np.empty(self.E, np.float32), np.empty(self.E, np.float32)
        grad = np.empty((self.E, 64, 64, 3) if self.arch == ARCH_IMPALA else (self.E, self.obs_dim), np.float32)
        self._chk(self.lib.mi_value_saliency(self._ctx, _fp(obs), C.c_size_t(obs.nbytes), C.c_uint64(seed), C.c_uint64(counter), _fp(u),
                                             _fp(act), _fp(logp), _fp(val), _fp(grad)))
        return act, logp, val, grad

    def commit_staged(self, t):
        self._chk(self.lib.mi_commit_staged(self._ctx, C.c_int32(t)))

    def set_gru(self, w_ih, w_hh, b_ih, b_hh):
        a = [_f32(x) for x in (w_ih, w_hh, b_ih, b_hh)]
        self._chk(self.lib.mi_set_gru(self._ctx, *[_fp(x) for x in a]))

    # ------------------------------------------------------------------ GRU training (algo: ppo-pure)
    GRU_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

    def gru_shapes(self):
        H = self.H
        return ((3 * H, H), (3 * H, H), (3 * H,), (3 * H,))

    def gru_count(self):
        return 2 * 3 * self.H * self.H + 2 * 3 * self.H

    def gru_train(self, enabled=True):
        """The GRU becomes a trained parameter set: gradient + Adam moments beside the flat vectors, one global clip norm (mi_gru_train)."""
        self._chk(self.lib.mi_gru_train(self._ctx, C.c_int32(int(enabled))))
        self.gru_trained = bool(enabled)

    def _gru4(self, fn):
        out = [np.empty(sh, np.float32) for sh in self.gru_shapes()]
        self._chk(fn(self._ctx, *[_fp(x) for x in out]))
        return tuple(out)

    def get_gru(self):
        """(w_ih, w_hh, b_ih, b_hh) as they are on the device, nn.GRU's layout."""
        return self._gru4(self.lib.mi_get_gru)

    def get_gru_grads(self):
        return self._gru4(self.lib.mi_get_gru_grads)

    def get_gru_adam_state(self):
        """(exp_avg, exp_avg_sq), each one vector {w_ih, w_hh, b_ih, b_hh}."""
        n = self.gru_count()
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        self._chk(self.lib.mi_get_gru_adam_state(self._ctx, _fp(m), _fp(v), C.c_int64(n)))
        return m, v

    def set_gru_adam_state(self, m, v):
        m, v = _f32(m).reshape(-1), _f32(v).reshape(-1)
        self._chk(self.lib.mi_set_gru_adam_state(self._ctx, _fp(m), _fp(v), C.c_int64(m.size)))

    def minibatch_rec(self, envs, h0, n_global, hp):
        """One recurrent minibatch: the envs of `envs` x all T steps, from the initial hidden states h0 (len(envs), H) (mi_minibatch_rec)."""
        envs = np.ascontiguousarray(envs, dtype=np.int64).reshape(-1)
        h0 = _f32(h0)
        if h0.size != envs.size * self.H:
            raise EngineError(f"minibatch_rec: h0 must be (n_env, H) = ({envs.size}, {self.H})")
        self._chk(self.lib.mi_minibatch_rec(self._ctx, _fp(envs), C.c_int32(envs.size), _fp(h0), C.c_int32(n_global), C.byref(hp)))

    def debug_gru_seq(self, x, h0, mask, w_ih, w_hh, b_ih, b_hh, d_out=None):
        """The GRU over a trajectory on caller data (mi_debug_gru_seq): x (T, n, H), h0 (n, H), mask (T, n), nn.GRU-layout weights -> h (T, n, H);
        with d_out (T, n, H) = dL/dh also (h, dX, dW_ih, dW_hh, db_ih, db_hh)."""
        x = _f32(x)
        T, n, H = x.shape
        a = [_f32(v) for v in (h0, mask, w_ih, w_hh, b_ih, b_hh)]
        d_out = None if d_out is None else _f32(d_out)
        out = np.empty((T, n, H), np.float32)
        g = [None] * 5 if d_out is None else [np.empty(sh, np.float32) for sh in ((T, n, H), (3 * H, H), (3 * H, H), (3 * H,), (3 * H,))]
        self._chk(self.lib.mi_debug_gru_seq(self._ctx, C.c_int32(T), C.c_int32(n), C.c_int32(H), _fp(x), *[_fp(v) for v in a], _fp(d_out),
                                            _fp(out), *[_fp(v) for v in g]))
        return out if d_out is None else (out, *g)

    def rec_state(self, hidden=None, done=None):
        hidden = None if hidden is None else _f32(hidden)
        done = None if done is None else _f32(done)
        self._chk(self.lib.mi_rec_state(self._ctx, _fp(hidden), _fp(done)))

    def get_hidden(self):
        out = np.empty((self.E, self.H), np.float32)
        self._chk(self.lib.mi_get_hidden(self._ctx, _fp(out)))
        return out

    def rec_begin(self, hidden=None, done=None):
        """Carried-in hidden state (E, H) / done flags (E,) of a pipelined recurrent rollout's step 0 (mi_rec_begin: stream-ordered, no host
        wait; None = the device's current state / zeros).  Call before the groups' first rollout_submit of every rollout."""
        hidden = None if hidden is None else _f32(hidden).reshape(self.E, self.H)
        done = None if done is None else _f32(done).reshape(self.E)
        self._chk(self.lib.mi_rec_begin(self._ctx, _fp(hidden), _fp(done)))

    def get_hidden_ring(self, t0, t1, out=None):
        """Slots [t0, t1) of the hidden ring, (t1 - t0, E, H) float32: slot t = the input hidden state of step t of the last pipelined
        recurrent rollout.  out: a C-contiguous float32 array of that shape to fill (page-locked: Engine.dma_ready)."""
        if out is None:
            out = np.empty((t1 - t0, self.E, self.H), np.float32)
        elif out.dtype != np.float32 or not out.flags.c_contiguous or out.size != (t1 - t0) * self.E * self.H:
            raise EngineError("get_hidden_ring needs a C-contiguous float32 array of (t1 - t0) * E * H elements")
        self._chk(self.lib.mi_get_hidden_ring(self._ctx, C.c_int32(t0), C.c_int32(t1), _fp(out)))
        return out

    def forward_rec(self, obs):
        want = np.uint8 if self.arch == ARCH_IMPALA else np.float32
        obs = np.ascontiguousarray(obs, dtype=want)
        lp, val, hid = np.empty((self.E, self.A), np.float32), np.empty(self.E, np.float32), np.empty((self.E, self.H), np.float32)
        self._chk(self.lib.mi_forward_rec(self._ctx, _fp(obs), _fp(lp), _fp(val), _fp(hid)))
        return lp, val, hid

    def forward(self, obs, want_feat=False):
        want = np.uint8 if self.arch == ARCH_IMPALA else np.float32
        obs = np.ascontiguousarray(obs, dtype=want)
        n = obs.shape[0]
        lp = np.empty((n, self.A), np.float32)
        val = np.empty(n, np.float32)
        feat = np.empty((n, self.H), np.float32) if want_feat else None
        self._chk(self.lib.mi_forward(self._ctx, _fp(obs), C.c_int32(n), _fp(lp), _fp(val), _fp(feat)))
        return (lp, val, feat) if want_feat else (lp, val)

    # ------------------------------------------------------------------ estimates
    def compute_estimates(self, gamma, lmbda, use_gae=True, normalize_adv=True):
        self._chk(self.lib.mi_compute_estimates(self._ctx, C.c_float(gamma), C.c_float(lmbda), C.c_int32(int(use_gae)),
                                                C.c_int32(int(normalize_adv))))

    def adv_stats(self):
        s = (C.c_double * 3)()
        self._chk(self.lib.mi_adv_stats(self._ctx, s))
        return np.array(list(s), dtype=np.float64)

    def adv_apply(self, stats3):
        s = (C.c_double * 3)(*[float(x) for x in stats3])
        self._chk(self.lib.mi_adv_apply(self._ctx, s))

    # ------------------------------------------------------------------ optimisation
    @staticmethod
    def hparams(eps_clip=0.2, value_coef=0.5, entropy_coef=0.01, x_entropy_coef=0.0, entropy_multiplier=1.0, fs_coef=0.0):
        return _HParams(eps_clip, value_coef, entropy_coef, x_entropy_coef, entropy_multiplier, fs_coef)

    def minibatch(self, idx, n_global, hp):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        self._chk(self.lib.mi_minibatch(self._ctx, _fp(idx), C.c_int32(idx.size), C.c_int32(n_global), C.byref(hp)))

    def minibatch_multi(self, idx, seg_n, n_global, hp):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        seg = np.ascontiguousarray(seg_n, dtype=np.int32)
        self._chk(self.lib.mi_minibatch_multi(self._ctx, _fp(idx), C.c_int32(idx.size), seg.ctypes.data_as(C.c_void_p), C.c_int32(seg.size),
                                              C.c_int32(n_global), C.byref(hp)))

    def minibatch_fused(self, idx, seg_n, n_global, hp):
        """minibatch_multi's pass of an MLP engine in two kernel launches (mi_minibatch_fused, csrc/mlp_fused.hip): same bookkeeping, gradients and
        records equal up to fp32 summation order.  One segment (seg_n = [len(idx)]) is minibatch()."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        seg = np.ascontiguousarray(seg_n, dtype=np.int32)
        self._chk(self.lib.mi_minibatch_fused(self._ctx, _fp(idx), C.c_int32(idx.size), seg.ctypes.data_as(C.c_void_p), C.c_int32(seg.size),
                                              C.c_int32(n_global), C.byref(hp)))

    def minibatch_finish(self):
        self._chk(self.lib.mi_minibatch_finish(self._ctx))

    def loss_log_finalize(self):
        self._chk(self.lib.mi_loss_log_finalize(self._ctx))

    def set_multirank(self, enabled):
        self._chk(self.lib.mi_set_multirank(self._ctx, C.c_int32(int(enabled))))

    def optimizer_step(self, lr, max_grad_norm, adam_step, want_norm=False):
        g = C.c_float(0)
        self._chk(self.lib.mi_optimizer_step(self._ctx, C.c_float(lr), C.c_float(max_grad_norm), C.c_int32(adam_step),
                                             C.byref(g) if want_norm else None))
        return g.value if want_norm else None

    def loss_log(self, reset=True, max_records=4096):
        out = np.empty((max_records, 8), np.float32)
        n = C.c_int32(0)
        self._chk(self.lib.mi_loss_log_read(self._ctx, _fp(out), C.c_int32(max_records), C.byref(n), C.c_int32(int(reset))))
        return out[:n.value].copy()

    # ------------------------------------------------------------------ IPL agent (algo: IPL)
    @staticmethod
    def ipl_hparams(gamma=0.99, alpha=1.0, entropy_coef=0.0, entropy_modified=False, reward_incentive=False, adv_incentive=False,
                    debug_zero_obs_seed=False):
        flags = (IPL_ENTROPY_MODIFIED * bool(entropy_modified) | IPL_REWARD_INCENTIVE * bool(reward_incentive) |
                 IPL_ADV_INCENTIVE * bool(adv_incentive) | IPL_DEBUG_ZERO_OBS_SEED * bool(debug_zero_obs_seed))
        return _IplHParams(gamma, alpha, entropy_coef, int(flags))

    def ipl_minibatch(self, idx, n_global, hp):
        """One minibatch of IPL.optimize on ring rows idx (mi_ipl_minibatch): gradients accumulate, one record (IPL_FIELDS) in the loss log."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        self._chk(self.lib.mi_ipl_minibatch(self._ctx, _fp(idx), C.c_int32(idx.size), C.c_int32(n_global), C.byref(hp)))

    def ipl_read_pred(self, n):
        """(pred, rew) of the last ipl_minibatch (n = its size): IPL.last_predicted_reward / last_reward."""
        pred, rew = np.empty(n, np.float32), np.empty(n, np.float32)
        self._chk(self.lib.mi_ipl_read_pred(self._ctx, _fp(pred), _fp(rew), C.c_int32(n)))
        return pred, rew

    def predict_greedy(self, obs):
        """IPL.predict(obs, greedy=True) on E observations, staged like predict_staged -> (act, logp, value)."""
        want = np.uint8 if self.arch == ARCH_IMPALA else np.float32
        obs = np.ascontiguousarray(obs, dtype=want)
        act, logp, val = np.empty(self.E, np.int64), np.empty(self.E, np.float32), np.empty(self.E, np.float32)
        self._chk(self.lib.mi_predict_greedy(self._ctx, _fp(obs), C.c_size_t(obs.nbytes), _fp(act), _fp(logp), _fp(val)))
        return act, logp, val

    def op_ipl_loss(self, hout, nv_raw, act, rew, done, hp):
        """The IPL kernels alone on caller arrays (mi_op_ipl_loss): hout (n, A + 1), nv_raw / act / rew / done (n,) ->
        (record (8,), dY (n, A + 1), g_next (n,), pred (n,))."""
        hout = _f32(hout)
        n, A = hout.shape[0], hout.shape[1] - 1
        nv_raw, rew, done = (_f32(a).reshape(n) for a in (nv_raw, rew, done))
        act = np.ascontiguousarray(act, dtype=np.int32).reshape(n)
        rec, dY, gn, pred = np.empty(8, np.float32), np.empty((n, A + 1), np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
        self._chk(self.lib.mi_op_ipl_loss(self._ctx, C.c_int32(n), C.c_int32(A), _fp(hout), _fp(nv_raw), _fp(act), _fp(rew), _fp(done),
                                          C.byref(hp), _fp(rec), _fp(dY), _fp(gn), _fp(pred)))
        return rec, dY, gn, pred

    def op_ipl_greedy(self, hout):
        """First arg-max of the normalised log-probabilities of head rows hout (n, A + 1) (mi_op_ipl_greedy)."""
        hout = _f32(hout)
        act = np.empty(hout.shape[0], np.int32)
        self._chk(self.lib.mi_op_ipl_greedy(self._ctx, C.c_int32(hout.shape[0]), C.c_int32(hout.shape[1] - 1), _fp(hout), _fp(act)))
        return act

    # ------------------------------------------------------------------ policy distillation (distill.py)
    def distill_label(self, teacher):
        """The teacher engine's normalised log-probabilities of all T * E observation rows of THIS engine's ring -> this engine's target
        ring (mi_distill_label); `teacher` may be this engine itself.  Asynchronous, ordered on both streams."""
        self._chk(self.lib.mi_distill_label(self._ctx, teacher._ctx))

    def distill_targets(self):
        """This engine's target ring (T * E, A) as the last distill_label left it (mi_distill_targets)."""
        out = np.empty((self.T * self.E, self.A), np.float32)
        self._chk(self.lib.mi_distill_targets(self._ctx, _fp(out), C.c_int64(out.size)))
        return out

    def distill_minibatch(self, idx, n_global):
        """One minibatch of the distiller's fit on ring rows idx (mi_distill_minibatch): MSE of the twice-normalised log-probabilities against
        the target ring; gradients accumulate, one record {loss, 0, 0, 0, loss, 0, 0, 0} in the loss log."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        self._chk(self.lib.mi_distill_minibatch(self._ctx, _fp(idx), C.c_int32(idx.size), C.c_int32(n_global)))

    def distill_loss(self, data):
        """Forward only: this engine's policy on all rows of `data`'s ring against data's target ring -> the mean squared error
        (mi_distill_loss).  Changes neither the gradients nor the loss log."""
        out = C.c_float(0)
        self._chk(self.lib.mi_distill_loss(self._ctx, data._ctx, C.byref(out)))
        return out.value

    def optimizer_step_eps(self, lr, max_grad_norm, eps, adam_step, want_norm=False):
        """optimizer_step with the caller's Adam eps (mi_optimizer_step_eps); max_grad_norm = inf: no clipping."""
        g = C.c_float(0)
        self._chk(self.lib.mi_optimizer_step_eps(self._ctx, C.c_float(lr), C.c_float(max_grad_norm), C.c_float(eps), C.c_int32(adam_step),
                                                 C.byref(g) if want_norm else None))
        return g.value if want_norm else None

    def op_distill_loss(self, hout, target, n_global=None):
        """The distillation loss kernels alone on caller arrays (mi_op_distill_loss): hout (n, A + 1), target (n, A) ->
        (record (8,), dY (n, A + 1)); the mean runs over n_global * A elements (default: n)."""
        hout = _f32(hout)
        n, A = hout.shape[0], hout.shape[1] - 1
        target = _f32(target).reshape(n, A)
        rec, dY = np.empty(8, np.float32), np.empty((n, A + 1), np.float32)
        self._chk(self.lib.mi_op_distill_loss(self._ctx, C.c_int32(n), C.c_int32(A), _fp(hout), _fp(target),
                                              C.c_int32(n if n_global is None else n_global), _fp(rec), _fp(dY)))
        return rec, dY

    # ------------------------------------------------------------------ sparse-autoencoder agent (algo: sae)
    SAE, PROBE = 0, 1                     # `which` of the mi_sae_* entry points
    SAE_INPUT_DIM = 2048                   # ImpalaModel.encoded_dim
    SAE_DIMS = tuple(range(64, 4097, 64))

    def sae_create(self, sae_dim, rho):
        """Allocates the SAE, the probe, their optimiser state and the feature / logit rings on this context (mi_sae_create)."""
        if self.arch != ARCH_IMPALA:
            raise NotImplementedError("architecture mlpmodel: the SAE agent needs ImpalaModel (encoded_dim / forward_to_pool exist only there)")
        if int(sae_dim) not in self.SAE_DIMS:
            raise NotImplementedError(f"sae_dim={sae_dim}: supported are the multiples of 64 in [64, 4096]")
        self._chk(self.lib.mi_sae_create(self._ctx, C.c_int32(int(sae_dim)), C.c_float(rho)))
        self.sae_dim = int(sae_dim)

    def sae_param_count(self, which):
        return int(self.lib.mi_sae_param_count(self._ctx, C.c_int32(which)))

    def sae_set_params(self, which, flat):
        flat = _f32(flat).reshape(-1)
        self._chk(self.lib.mi_sae_set_params(self._ctx, C.c_int32(which), _fp(flat), C.c_int64(flat.size)))

    def sae_get_params(self, which):
        out = np.empty(self.sae_param_count(which), np.float32)
        self._chk(self.lib.mi_sae_get_params(self._ctx, C.c_int32(which), _fp(out), C.c_int64(out.size)))
        return out

    def sae_get_grads(self, which):
        out = np.empty(self.sae_param_count(which), np.float32)
        self._chk(self.lib.mi_sae_get_grads(self._ctx, C.c_int32(which), _fp(out), C.c_int64(out.size)))
        return out

    def sae_set_adam_state(self, which, m, v):
        m, v = _f32(m).reshape(-1), _f32(v).reshape(-1)
        self._chk(self.lib.mi_sae_set_adam_state(self._ctx, C.c_int32(which), _fp(m), _fp(v), C.c_int64(m.size)))

    def sae_get_adam_state(self, which):
        n = self.sae_param_count(which)
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        self._chk(self.lib.mi_sae_get_adam_state(self._ctx, C.c_int32(which), _fp(m), _fp(v), C.c_int64(n)))
        return m, v

    def sae_put_ring(self, t, hidden=None, logits=None):
        """hidden (E, 2048) in the reference's column order / the policy's logits (E, A) into ring step t (SAEStorage.store / store_last)."""
        hidden = None if hidden is None else _f32(hidden).reshape(self.E, self.SAE_INPUT_DIM)
        logits = None if logits is None else _f32(logits).reshape(self.E, self.A)
        self._chk(self.lib.mi_sae_put_ring(self._ctx, C.c_int32(t), _fp(hidden), _fp(logits)))

    def sae_get_hidden(self, t):
        out = np.empty((self.E, self.SAE_INPUT_DIM), np.float32)
        self._chk(self.lib.mi_sae_get_hidden(self._ctx, C.c_int32(t), _fp(out)))
        return out

    def sae_get_logits(self, t):
        out = np.empty((self.E, self.A), np.float32)
        self._chk(self.lib.mi_sae_get_logits(self._ctx, C.c_int32(t), _fp(out)))
        return out

    def sae_step(self, t, obs, act_from_probe=False, store=True, seed=0, u=None):
        """SAE.get_hidden_and_acts on E uint8 NHWC frames (mi_sae_step) -> (act (E,) int64, value (E,))."""
        obs = np.ascontiguousarray(obs, dtype=np.uint8)
        u = None if u is None else _f32(u)
        act, val = np.empty(self.E, np.int64), np.empty(self.E, np.float32)
        self._chk(self.lib.mi_sae_step(self._ctx, C.c_int32(t), _fp(obs), C.c_size_t(obs.nbytes), C.c_int32(int(bool(act_from_probe))),
                                       C.c_int32(int(bool(store))), C.c_uint64(seed), _fp(u), _fp(act), _fp(val)))
        return act, val

    def sae_minibatch(self, idx, sparse_coef):
        """One minibatch of optimize_sae on ring rows idx -> (recon, KL, loss)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        log = np.empty(3, np.float32)
        self._chk(self.lib.mi_sae_minibatch(self._ctx, _fp(idx), C.c_int32(idx.size), C.c_float(sparse_coef), _fp(log)))
        return log

    def sae_probe_minibatch(self, idx):
        """One minibatch of optimize_linear_model on ring rows idx -> (value_loss, logit_loss, loss)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        log = np.empty(3, np.float32)
        self._chk(self.lib.mi_sae_probe_minibatch(self._ctx, _fp(idx), C.c_int32(idx.size), _fp(log)))
        return log

    def sae_optimizer_step(self, which, lr, max_grad_norm, adam_step, want_norm=False):
        g = C.c_float(0)
        self._chk(self.lib.mi_sae_optimizer_step(self._ctx, C.c_int32(which), C.c_float(lr), C.c_float(max_grad_norm), C.c_int32(adam_step),
                                                 C.byref(g) if want_norm else None))
        return g.value if want_norm else None

    def sae_debug_forward(self, idx):
        """(enc (n, S), rec (n, 2048)) of ring rows idx: the forward pass of sae_minibatch (test hook)."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        enc, rec = np.empty((idx.size, self.sae_dim), np.float32), np.empty((idx.size, self.SAE_INPUT_DIM), np.float32)
        self._chk(self.lib.mi_sae_debug_forward(self._ctx, _fp(idx), C.c_int32(idx.size), _fp(enc), _fp(rec)))
        return enc, rec

    # ------------------------------------------------------------------ RCCL collectives (inside the library)
    def comm_unique_id(self):
        buf = (C.c_char * 128)()
        self._chk(self.lib.mi_comm_unique_id(buf, C.c_size_t(128)))
        return bytes(buf)

    def comm_init(self, id_bytes, rank, world):
        buf = (C.c_char * 128).from_buffer_copy(id_bytes)
        self._chk(self.lib.mi_comm_init(self._ctx, buf, C.c_size_t(128), C.c_int32(rank), C.c_int32(world)))
        self.comm_world = world

    def allreduce_arm(self):
        self._chk(self.lib.mi_allreduce_arm(self._ctx))

    def allreduce_grads(self):
        self._chk(self.lib.mi_allreduce_grads(self._ctx))

    def allreduce_buffer(self, which, n):
        self._chk(self.lib.mi_allreduce_buffer(self._ctx, C.c_int32(which), C.c_int64(n)))

    def adv_normalize_global(self):
        self._chk(self.lib.mi_adv_normalize_global(self._ctx))

    def device_ptr(self, which):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.lib.mi_device_ptr(self._ctx, C.c_int32(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    # ------------------------------------------------------------------ live kernel timing
    def profile_enable(self, mode=1):
        """0 off, 1 update-phase kernels only, 2 rollout + update."""
        self._chk(self.lib.mi_profile_enable(self._ctx, C.c_int32(int(mode))))

    def profile_read(self, reset=True):
        rows = np.zeros((64, 7), np.float64)
        n = C.c_int32(0)
        self._chk(self.lib.mi_profile_read(self._ctx, _fp(rows), C.c_int32(64), C.byref(n), C.c_int32(int(reset))))
        out = []
        for r in rows[:n.value]:
            out.append(dict(kernel=self.lib.mi_profile_class_name(C.c_int32(int(r[0]))).decode(), phase="rollout" if r[1] == 0 else "update",
                            launches=int(r[2]), ms=float(r[3]), samples=int(r[4]), bytes=float(r[5]), flops=float(r[6])))
        return out

    # ------------------------------------------------------------------ op-level (tests)
    def op_conv3x3(self, mode, cin, cout, hw, w_ref, inp=None, relu_in=False, bias=None, res=None, mask=None, dout=None):
        is_u8 = inp is not None and inp.dtype == np.uint8
        n = (inp if inp is not None else dout).shape[0]
        # modes: 0 forward, 1 dgrad, 2 wgrad; a block's first conv in bf16 precision also 3 = conv+maxpool forward,
        # 4 / 5 = weight / data gradient from the POOLED gradient (dout) and the forward's arg-max (inp is needed for it);
        # 6 / 7 = the fused data + weight gradient launch of block2.conv, returning (dW, db) / dx
        inp = None if inp is None else np.ascontiguousarray(inp)
        w_ref = _f32(w_ref)
        bias, res, mask, dout = (None if a is None else _f32(a) for a in (bias, res, mask, dout))
        if mode in (2, 4, 6):
            out, db = np.empty((cout, cin, 3, 3), np.float32), np.empty(cout, np.float32)
        elif mode == 3:
            out, db = np.empty((n, hw // 2, hw // 2, cout), np.float32), None
        elif mode in (5, 7):
            out, db = np.empty((n, hw, hw, cin), np.float32), None
        else:
            out, db = np.empty((n, hw, hw, cin if mode == 1 else cout), np.float32), None
        self._chk(self.lib.mi_op_conv3x3(self._ctx, C.c_int32(mode), C.c_int32(cin), C.c_int32(cout), C.c_int32(hw),
                                         C.c_int32(n), _fp(inp), C.c_int32(int(is_u8)), C.c_int32(int(relu_in)), _fp(w_ref),
                                         _fp(bias), _fp(res), _fp(mask), _fp(dout), _fp(out), _fp(db)))
        return (out, db) if mode in (2, 4, 6) else out

    def op_resblock(self, mode, x, w1, w2, b1=None, b2=None, a_fwd=None, x_fwd=None):
        """bf16 precision: fused residual block.  mode 0 -> (conv1 output, block output); mode 1 (x = dy) -> (d conv1-output, d block-input);
        mode 2 (16 channels @32x32, x = dy) -> (flat {dW1, db1, dW2, db2} in the head of the first array, d block-input);
        mode 3: res1 + res2 in one launch, both blocks with (w1, b1, w2, b2) -> (res2's conv1 output, block output);
        mode 4: res1 + res2 in one launch with distinct weights: w1 / b1 = res1's (conv1, conv2) stacked ([2, ch, ch, 3, 3] / [2, ch]),
        w2 / b2 = res2's -> ([A1, A2], [P1, P2]), each [2, n, hw, hw, ch] (res conv1 outputs, res block outputs)."""
        x = _f32(x)
        n, hw, _, ch = x.shape
        w1, w2 = _f32(w1), _f32(w2)
        b1, b2, a_fwd, x_fwd = (None if a is None else _f32(a) for a in (b1, b2, a_fwd, x_fwd))
        if mode == 4:
            assert w1.size == w2.size == 2 * 9 * ch * ch and b1.size == b2.size == 2 * ch, "mode 4 takes each block's two convs stacked"
            oa, oy = np.empty((2,) + x.shape, np.float32), np.empty((2,) + x.shape, np.float32)
        else:
            oa, oy = np.empty(max(x.size, 2 * (9 * ch * ch + ch)), np.float32), np.empty_like(x)      # mode 2 packs the weight gradients into oa
        self._chk(self.lib.mi_op_resblock(self._ctx, C.c_int32(mode), C.c_int32(ch), C.c_int32(hw), C.c_int32(n), _fp(x), _fp(w1), _fp(b1),
                                          _fp(w2), _fp(b2), _fp(a_fwd), _fp(x_fwd), _fp(oa), _fp(oy)))
        if mode == 4:
            return oa, oy
        return (oa if mode == 2 else oa[:x.size].reshape(x.shape)), oy

    def op_maxpool(self, mode, x, dout=None):
        x = _f32(x)
        n, hw, _, c = x.shape
        dout = None if dout is None else _f32(dout)
        out = np.empty((n, hw // 2, hw // 2, c) if mode == 0 else x.shape, np.float32)
        self._chk(self.lib.mi_op_maxpool(self._ctx, C.c_int32(mode), C.c_int32(n), C.c_int32(hw), C.c_int32(c), _fp(x),
                                         _fp(dout), _fp(out)))
        return out

    def op_gemm(self, A, B, transpose_a=False, transpose_b=False):
        """C = op(A) @ op(B) with the operands left in place (strided access inside the kernel)."""
        A, B = _f32(A), _f32(B)
        M, K = (A.shape[1], A.shape[0]) if transpose_a else A.shape
        N = B.shape[0] if transpose_b else B.shape[1]
        sam, sak = (1, A.shape[1]) if transpose_a else (A.shape[1], 1)
        sbk, sbn = (1, B.shape[1]) if transpose_b else (B.shape[1], 1)
        out = np.empty((M, N), np.float32)
        self._chk(self.lib.mi_op_gemm(self._ctx, C.c_int32(M), C.c_int32(N), C.c_int32(K), _fp(A), C.c_int64(sam),
                                      C.c_int64(sak), _fp(B), C.c_int64(sbk), C.c_int64(sbn), _fp(out)))
        return out

    def op_fc_bf16(self, mode, D, x=None, W=None, b=None, dy=None, gW0=None, gb0=None):
        """The bf16 embedder.fc kernels (2048 -> D) on caller data through the production launchers (mi_op_fc_bf16), any context.
        mode 0 / 1 (x, W, b) -> y (n, D) by the update-sized / rollout-sized forward; mode 2 (dy, W, x = mask source) -> dx (n, 2048);
        mode 3 (dy, x, gW0, gb0) -> (gW0 + dy^T relu(x), gb0 + colsum(dy))."""
        x, W, b, dy = (None if a is None else _f32(a) for a in (x, W, b, dy))
        n = (dy if mode >= 2 and dy is not None else x).shape[0]
        out_b = None
        if mode <= 1:
            out = np.empty((n, D), np.float32)
        elif mode == 2:
            out = np.empty((n, 2048), np.float32)
        else:
            out, out_b = np.array(gW0, dtype=np.float32, order="C"), np.array(gb0, dtype=np.float32, order="C")
        self._chk(self.lib.mi_op_fc_bf16(self._ctx, C.c_int32(mode), C.c_int32(n), C.c_int32(D), _fp(x), _fp(W), _fp(b), _fp(dy), _fp(out),
                                         _fp(out_b)))
        return (out, out_b) if mode == 3 else out

    def op_linear(self, form, A, B, bias=None, mask=None, C0=None, gb0=None, relu_x=False, relu_out=False, x_bf16=False, dims=None,
                  strides=None, use_ws=True, ws_floats=-1):
        """The generic GEMM (csrc/gemm.hip) on caller data through the production launchers (mi_op_linear), any context
        -> (out, (split, k_chunk)), the plan the call ran.
        form 0: A = X (n, in), B = W (out, in), bias -> Y (n, out); form 1: A = dY (n, out), B = W, mask (n, in) -> dX (n, in);
        form 2: A = dY, B = X (n, in), C0 = gW0 (out, in), gb0 -> out = (gW0 + dY^T relu?(X), gb0 + colsum(dY)).  x_bf16: the activation-typed
        operands are bf16 on the device.
        form 3: launch_gemm itself; A and B are flat buffers, dims = (M, N, K), strides = (sam, sak, sbk, sbn, ldc), mask and C0 (M, ldc);
        C0 is given exactly when the call accumulates.  -> C (M, ldc) whole: the columns from N on hold the poison (all-ones words)."""
        A, B = _f32(A), _f32(B)
        bias, mask = (None if a is None else _f32(a) for a in (bias, mask))
        flags = (1 if relu_x else 0) | (2 if relu_out else 0) | (4 if x_bf16 else 0)
        out_b, st = None, None
        if form == 3:
            M, N, K = dims
            st = np.asarray(strides, np.int64)
            assert st.shape == (5,)
            flags |= (8 if C0 is not None else 0) | (16 if use_ws else 0)
            out = np.empty((max(M, 1), int(st[4])), np.float32) if C0 is None else np.array(C0, dtype=np.float32, order="C")
            assert out.shape == (max(M, 1), int(st[4]))
            d = (M, N, K)
        else:
            n = A.shape[0]
            if form == 0:
                d = (n, A.shape[1], B.shape[0])
                out = np.empty((n, d[2]), np.float32)
            elif form == 1:
                d = (n, B.shape[1], B.shape[0])
                out = np.empty((n, d[1]), np.float32)
            else:
                d = (n, B.shape[1], A.shape[1])
                out, out_b = np.array(C0, dtype=np.float32, order="C"), np.array(gb0, dtype=np.float32, order="C")
        plan = np.zeros(2, np.int32)
        self._chk(self.lib.mi_op_linear(self._ctx, C.c_int32(form), C.c_int32(d[0]), C.c_int32(d[1]), C.c_int32(d[2]), _fp(st), C.c_int32(flags),
                                        C.c_int64(ws_floats), _fp(A), _fp(B), _fp(bias), _fp(mask), _fp(out), _fp(out_b), _fp(plan)))
        plan = (int(plan[0]), int(plan[1]))
        return ((out, out_b) if form == 2 else out), plan

    def _op_reduce(self, mode, src, a, b, ld, desc, dst_w, dst_b):
        src, w = _f32(src).reshape(-1), np.array(dst_w, dtype=np.float32, order="C").reshape(-1)
        bb = None if dst_b is None else np.array(dst_b, dtype=np.float32, order="C").reshape(-1)
        desc = None if desc is None else np.ascontiguousarray(desc, dtype=np.int64).reshape(-1, 6)
        self._chk(self.lib.mi_op_reduce(self._ctx, C.c_int32(mode), _fp(src), C.c_int64(src.size), C.c_int32(a), C.c_int32(b), C.c_int32(ld),
                                        _fp(desc), C.c_int32(0 if desc is None else desc.shape[0]), _fp(w), C.c_int64(w.size), _fp(bb),
                                        C.c_int32(0 if bb is None else bb.size)))
        return w, bb

    def op_reduce_slabs(self, partial, dst_w, dst_b=None):
        """launch_reduce_slabs on partial (nslab, slab_len) (mi_op_reduce mode 0) -> (dst_w + the sums of the first len(dst_w) elements,
        dst_b + those of the next len(dst_b), or None); elements past both are dropped."""
        partial = _f32(partial)
        return self._op_reduce(0, partial, partial.shape[0], partial.shape[1], 0, None, dst_w, dst_b)

    def op_reduce_all_slabs(self, ws, desc, grads):
        """launch_reduce_all_slabs (mi_op_reduce mode 1): desc rows {src_off, w_off, b_off, nslab, slab_len, n_w}, ws the flat slab
        workspace, grads the flat gradient vector -> grads + every layer's sums."""
        return self._op_reduce(1, ws, 0, 0, 0, desc, grads, None)[0]

    def op_colsum(self, dY, N, db):
        """launch_colsum_acc on dY (M, ld) (mi_op_reduce mode 2) -> db + the column sums of the first N columns."""
        dY = _f32(dY)
        return self._op_reduce(2, dY, dY.shape[0], N, dY.shape[1], None, db, None)[0]

    def op_adam(self, variant, p, g, m, v, lr, max_norm, step, second=None, offsets=None):
        """The optimizer tail on caller vectors (mi_op_adam) -> (p', g', m', v', norm); variant 0 the PPO path, 2 the SAE agent's kernel,
        1 with second = (p2, g2, m2, v2) under the same norm, stepped in the four pieces offsets[k]:offsets[k + 1] ->
        (p', g', m', v', norm, (p2', g2', m2', v2'))."""
        a = [np.array(x, dtype=np.float32, order="C").reshape(-1) for x in (p, g, m, v)]
        s = [None] * 4 if second is None else [np.array(x, dtype=np.float32, order="C").reshape(-1) for x in second]
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        if any(x.size != a[0].size for x in a) or (second is not None and (any(x.size != s[0].size for x in s) or off is None or off.size != 5)):
            raise EngineError("op_adam: p, g, m, v must have one length; the second vector needs five offsets")
        gn = C.c_float(0)
        self._chk(self.lib.mi_op_adam(self._ctx, C.c_int32(variant), C.c_int64(a[0].size), *[_fp(x) for x in a],
                                      C.c_int64(0 if second is None else s[0].size), *[_fp(x) for x in s], _fp(off), C.c_float(lr),
                                      C.c_float(max_norm), C.c_int32(step), C.byref(gn)))
        norm = np.float32(gn.value)
        return (*a, norm) if second is None else (*a, norm, tuple(s))

    def op_adv_merge(self, stats_list):
        """launch_advnorm_merge on R triples {count, mean, M2} (mi_op_adv_merge) -> the merged triple (float64)."""
        a = np.ascontiguousarray(stats_list, dtype=np.float64).reshape(-1, 3)
        out = np.empty(3, np.float64)
        self._chk(self.lib.mi_op_adv_merge(self._ctx, _fp(a), C.c_int32(a.shape[0]), _fp(out)))
        return out

    def op_heads_fwd(self, feat, Wh, bh):
        """launch_heads_fwd on feat (n, 256), Wh (O, 256), bh (O,) (mi_op_heads mode 0) -> hout (n, O)."""
        feat, Wh, bh = _f32(feat), _f32(Wh), _f32(bh)
        n, H, O = feat.shape[0], feat.shape[1], Wh.shape[0]
        out = np.empty((n, O), np.float32)
        self._chk(self.lib.mi_op_heads(self._ctx, C.c_int32(0), C.c_int32(n), C.c_int32(H), C.c_int32(O), _fp(feat), _fp(Wh), _fp(bh), None,
                                       C.c_int32(0), _fp(out), None, None))
        return out

    def op_heads_bwd(self, dY, feat, Wh, relu_mask, gW0, gb0):
        """launch_heads_bwd and its slab sum on dY (n, O), feat (n, H), Wh (O, H) (mi_op_heads mode 1) ->
        (dfeat (n, H), gW0 + dY^T feat, gb0 + colsum(dY))."""
        dY, feat, Wh = _f32(dY), _f32(feat), _f32(Wh)
        n, H, O = feat.shape[0], feat.shape[1], Wh.shape[0]
        gW, gb = np.array(gW0, dtype=np.float32, order="C").reshape(O, H), np.array(gb0, dtype=np.float32, order="C").reshape(O)
        if dY.shape != (n, O) or Wh.shape != (O, H):
            raise EngineError("op_heads_bwd: dY (n, O), feat (n, H), Wh (O, H)")
        out = np.empty((n, H), np.float32)
        self._chk(self.lib.mi_op_heads(self._ctx, C.c_int32(1), C.c_int32(n), C.c_int32(H), C.c_int32(O), _fp(feat), _fp(Wh), None, _fp(dY),
                                       C.c_int32(int(bool(relu_mask))), _fp(out), _fp(gW), _fp(gb)))
        return out, gW, gb

    def op_sample(self, feat, Wh, bh, u=None, seed=0, counter=0, value_from_logits=False):
        """The three sampling kernels on caller data (mi_op_sample): heads_sample_kernel on feat (n, H), Wh (A + 1, H), bh (A + 1,), then
        sample_kernel and logp_all_kernel on the hout it wrote -> dict(fused=(act, logp, value), sample=(act, logp, value), pack (n, 3),
        hout (n, A + 1), table (n, A), table_value (n,)).  u (n,) or None: Philox(seed, counter + row)."""
        feat, Wh, bh = _f32(feat), _f32(Wh), _f32(bh).reshape(-1)
        n, H, A = feat.shape[0], feat.shape[1], Wh.shape[0] - 1
        if Wh.shape != (A + 1, H) or bh.size != A + 1:
            raise EngineError("op_sample: feat (n, H), Wh (A + 1, H), bh (A + 1,)")
        u = None if u is None else _f32(u).reshape(n)
        act, logp, val = np.empty((2, n), np.int32), np.empty((2, n), np.float32), np.empty((3, n), np.float32)
        pack, hout, table = np.empty((n, 3), np.float32), np.empty((n, A + 1), np.float32), np.empty((n, A), np.float32)
        self._chk(self.lib.mi_op_sample(self._ctx, C.c_int32(n), C.c_int32(H), C.c_int32(A), _fp(feat), _fp(Wh), _fp(bh), _fp(u), C.c_uint64(seed),
                                        C.c_uint64(counter), C.c_int32(int(bool(value_from_logits))), _fp(act), _fp(logp), _fp(val), _fp(pack),
                                        _fp(hout), _fp(table)))
        return dict(fused=(act[0], logp[0], val[0]), sample=(act[1], logp[1], val[1]), pack=pack, hout=hout, table=table, table_value=val[2])

    def op_ppo_loss(self, mode, hout, idx, act, old_logp, old_value, ret, adv, hp, value_from_logits=False, n_global=None, seg_n=None):
        """The PPO loss kernels on caller arrays (mi_op_ppo_loss): mode 0 the two-phase path (loss_fwd, finalize, loss_bwd), mode 1 the
        one-pass segmented path over seg_n.  hout (n, A + 1); idx (n,) into act / old_logp / old_value / ret / adv ->
        (dY (n, A + 1), partial (blocks, 8 + A), stats (segments, 32), log (segments, 8))."""
        hout = _f32(hout)
        n, A = hout.shape[0], hout.shape[1] - 1
        idx, act = np.ascontiguousarray(idx, dtype=np.int32).reshape(n), np.ascontiguousarray(act, dtype=np.int32).reshape(-1)
        arrs = [_f32(a).reshape(-1) for a in (old_logp, old_value, ret, adv)]
        if any(a.size != act.size for a in arrs):
            raise EngineError("op_ppo_loss: act, old_logp, old_value, ret, adv must have one length")
        seg = np.ascontiguousarray([n] if (mode == 0 or seg_n is None) else seg_n, dtype=np.int32)
        nblk = int(sum(-(-int(k) // 64) for k in seg))
        dY, partial = np.empty((n, A + 1), np.float32), np.empty((nblk, 8 + A), np.float32)
        stats, log = np.empty((seg.size, 32), np.float32), np.empty((seg.size, 8), np.float32)
        self._chk(self.lib.mi_op_ppo_loss(self._ctx, C.c_int32(mode), C.c_int32(n), C.c_int32(A), _fp(hout), _fp(idx), C.c_int32(act.size), _fp(act),
                                          *[_fp(a) for a in arrs], C.byref(hp), C.c_int32(int(bool(value_from_logits))),
                                          C.c_int32(n if n_global is None else n_global), _fp(seg), C.c_int32(seg.size), _fp(dY), _fp(partial),
                                          _fp(stats), _fp(log)))
        return dY, partial, stats, log

    def debug_read(self, which, n):
        """Activation tensor `which` (see include/mi355ppo.h mi_debug_read) of the last minibatch pass, first n samples, fp32 NHWC."""
        if which in (100, 101, 102):        # features; after minibatch_rec: 100 the embedder output x, 101 h_t, 102 dX
            out = np.empty((n, self.H), np.float32)
        else:
            b = which >> 3
            hw, ch = (32, 16, 8)[b], (16, 32, 32)[b]
            out = np.empty((n, hw, hw, ch), np.float32)
        self._chk(self.lib.mi_debug_read(self._ctx, C.c_int32(which), C.c_int32(n), _fp(out)))
        return out

    def minibatch_positions(self, gpos):
        """Global minibatch positions of the next minibatch()'s rows (fs_coef != 0 on several ranks, include/mi355ppo.h)."""
        g = np.ascontiguousarray(gpos, dtype=np.int32)
        self._chk(self.lib.mi_minibatch_positions(self._ctx, g.ctypes.data_as(C.c_void_p), C.c_int32(g.size)))

    def debug_philox(self, ctr_key6):
        """(n,6) uint32 {c0..c3,k0,k1} -> ((n,4) uint32 Philox4x32-10 output words, (n,) the sampler's uniforms for seed k0|k1<<32, counter c0|c1<<32)."""
        a = np.ascontiguousarray(ctr_key6, dtype=np.uint32).reshape(-1, 6)
        out, u = np.empty((a.shape[0], 4), np.uint32), np.empty(a.shape[0], np.float32)
        self._chk(self.lib.mi_debug_philox(self._ctx, _fp(a), C.c_int32(a.shape[0]), _fp(out), _fp(u)))
        return out, u

    def debug_gru_step(self, x, h, done, w_ih, w_hh, b_ih, b_hh, with_copy=False):
        """The pipelined rollout's fused GRU step on caller data (mi_debug_gru_step): x, h (n, H), done (n,), nn.GRU-layout weights ->
        h' (n, H), or (h', the kernel's second copy of h') with with_copy."""
        x, h = _f32(x), _f32(h)
        n, H = x.shape
        a = [_f32(v) for v in (done, w_ih, w_hh, b_ih, b_hh)]
        out = np.empty((n, H), np.float32)
        cp = np.empty((n, H), np.float32) if with_copy else None
        self._chk(self.lib.mi_debug_gru_step(self._ctx, C.c_int32(n), C.c_int32(H), _fp(x), _fp(h), *[_fp(v) for v in a], _fp(out), _fp(cp)))
        return (out, cp) if with_copy else out

    def debug_step_latency(self, t, iters=200, graph=False):
        """microseconds per policy step of slot t (launches + stream wait), eager or as a replayed hipGraph of the same launches"""
        us = C.c_float(0)
        self._chk(self.lib.mi_debug_step_latency(self._ctx, C.c_int32(t), C.c_int32(iters), C.c_int32(int(graph)), C.byref(us)))
        return us.value

    def debug_lane_probe(self, mask, iters):
        """microseconds from first launch to last completion of one fixed-length sleeping workgroup on each group stream in `mask`"""
        us = C.c_float(0)
        self._chk(self.lib.mi_debug_lane_probe(self._ctx, C.c_int32(mask), C.c_int32(iters), C.byref(us)))
        return us.value

    def debug_flags(self, flags):
        self._chk(self.lib.mi_debug_flags(self._ctx, C.c_int32(flags)))

    def selftest_mfma(self):
        e = C.c_float(0)
        self._chk(self.lib.mi_selftest_mfma(self._ctx, C.byref(e)))
        return e.value
