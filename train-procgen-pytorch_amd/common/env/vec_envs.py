"""Host-side vectorised environments that speak the baselines VecEnv protocol the agent drives
(reset() -> obs ; step(act) -> (obs, rew, done, info) ; close()), reference:
common/env/procgen_wrappers.py:45-124.  Rollout collection stays on the host (north_star).

* CartPoleVec   -- the reference's 9-observation pre-vectorised cart-pole (discrete_env/cartpole_pre_vec.py) restated in numpy,
                   the plumbing config C1 (MLPModel(9, ...)).
* DeviceCartPole -- the same env resident on the device (opt-in, train.py --device_env).
* CartPoleSwingVec -- the reference's pre-vectorised swing-up cart-pole (discrete_env/cartpole_swing_pre_vec.py) restated in numpy and
                   pinned to the reference's own class by a trajectory fixture: the cart-pole's 9 observations, 2 actions and dynamics,
                   the pole starts hanging down, reward for holding it up near the centre (`--env_name cartpole_swing`, create_vector_env).
* DeviceCartPoleSwing -- the same env resident on the device (opt-in, train.py --device_env).
* MountainCarVec -- the reference's 5-observation pre-vectorised mountain car (discrete_env/mountain_car_pre_vec.py) restated in numpy
                   and pinned to the reference's own class by a trajectory fixture (MLPModel(5, ...), 3 actions).
* DeviceMountainCar -- the same env resident on the device (opt-in, train.py --device_env).
* SyntheticFrames -- random uint8 64x64x3 frames, N(0,1) rewards, Bernoulli(0.01) dones: the synthetic
                   learner-side workload of SURVEY 8(d) / bench.py.
* create_procgen_env -- the real engine if the `procgen` package is importable (it is not in the build image).
"""
from fnmatch import fnmatchcase
from typing import Callable, NamedTuple

import numpy as np


class _Space:
    def __init__(self, shape=None, n=None):
        self.shape, self.n = shape, n


class StepInfo:
    """One vector-env step's `info`, kept column-wise.

    The reference's protocol hands the agent a list of E dicts per step and walks them entry by entry afterwards
    (`Storage.fetch_log_data`, common/storage.py:130-162: T*E dict look-ups per iteration; `VecNormalize.step_wait`,
    procgen_wrappers.py:336-337: E dict writes per step).  A StepInfo answers to the same uses -- len(), info[i] -> dict,
    iteration, `'key' in info[0]` -- but holds what the wrappers add (`env_reward`, ...) as ONE array per key and leaves the
    env's own per-env dicts (`rows`, e.g. Procgen's prev_level_seed / level_complete) untouched; `column(key)` is what the logging
    path reads.  `StepInfo.join(parts)` shows the infos of several env groups as one step's info without copying."""
    __slots__ = ("n", "columns", "rows", "parts")

    def __init__(self, n, columns=None, rows=None, parts=None):
        self.n, self.columns, self.rows, self.parts = n, columns or {}, rows, parts

    @staticmethod
    def join(parts):
        parts = [p if isinstance(p, StepInfo) else StepInfo(len(p), rows=p) for p in parts]
        return parts[0] if len(parts) == 1 else StepInfo(sum(p.n for p in parts), parts=parts)

    def __len__(self):
        return self.n

    def has(self, key):
        if self.parts is not None:
            return bool(self.parts) and self.parts[0].has(key)
        return key in self.columns or bool(self.rows) and key in self.rows[0]

    def column(self, key):
        if self.parts is not None:
            return np.concatenate([p.column(key) for p in self.parts])
        if key in self.columns:
            return np.asarray(self.columns[key])
        return np.array([r[key] for r in self.rows])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.n))]
        if i < 0:
            i += self.n
        if self.parts is not None:
            for p in self.parts:
                if i < p.n:
                    return p[i]
                i -= p.n
            raise IndexError(i)
        d = dict(self.rows[i]) if self.rows else {}
        for k, v in self.columns.items():
            d[k] = v[i]
        return d

    def __iter__(self):
        return (self[i] for i in range(self.n))


def _cartpole_setup(self, n_envs, degrees, h_range, min_gravity, max_gravity, min_pole_length, max_pole_length, min_cart_mass, max_cart_mass,
                    min_pole_mass, max_pole_mass, min_force_mag, max_force_mag, max_steps, seed):
    """The constructor part that CartPoleVec and DeviceCartPole share: the thresholds (cartpole_pre_vec.py:131-132) and the start ranges
    per state column (:163-171)."""
    if n_envs < 2:
        raise Exception("n_envs must be greater than or equal to 2")
    self.n_envs = self.num_envs = n_envs
    self.max_steps, self.seed = max_steps, int(seed)
    self.theta_threshold, self.x_threshold = degrees * 2 * np.pi / 360, h_range
    self.low = np.array([-0.05] * 4 + [min_gravity, min_pole_length, min_cart_mass, min_pole_mass, min_force_mag])
    self.high = np.array([0.05] * 4 + [max_gravity, max_pole_length, max_cart_mass, max_pole_mass, max_force_mag])
    self.observation_space = _Space(shape=(9,))
    self.action_space = _Space(n=2)


class CartPoleVec:
    """The reference's pre-vectorised cart-pole (discrete_env/cartpole_pre_vec.py:20-205 on discrete_env/pre_vec_env.py:21-125),
    restated in numpy: BASELINE config 1's env.  Observation = the 9-column state (cartpole_pre_vec.py:136-149, 197-208)

        [x, x_dot, theta, theta_dot, gravity, pole_length, cart_mass, pole_mass, force_mag]

    -- the four dynamic variables plus the five physics parameters an episode was drawn with, which is why the reference builds
    MLPModel(9, ...) for `--env_name cartpole`.  Every episode start draws all nine uniformly from [low, high] (start_space,
    :163-171: the dynamic variables from +-0.05, the parameters from their min/max range); Florian's equations with the per-env
    parameters, Euler steps of tau = 0.02 (:214-245); termination beyond +-h_range or +-degrees (:254-262), truncation at max_steps
    (pre_vec_env.py:86-87); reward 1 every step; info[i] = {'env_reward': 1.0} (:112-113).  Kept from the reference: when ANY env ends,
    a whole (n_envs, 9) block is drawn and only the ended rows take their values (pre_vec_env.py:111-118), and `done` is the
    `terminated` array AFTER the reset.  The generator is numpy's default_rng(seed) -- what gymnasium's seeding.np_random(seed)
    constructs (PCG64 over SeedSequence(seed)).  The STEP is pinned to the reference's class: tests/golden/g18_cartpole_swing.npz case c/
    holds one teacher-forced step of CartPoleVecEnv and tests/test_cartpole_swing_host.py reproduces it bit for bit on the rows that go
    on, with done equal.  Trajectories from a seed are NOT the reference's: its constructor ends in reset(seed=seed) and so draws one
    block that this constructor does not draw; tests/test_env_pipeline.py checks the dynamics against a scalar
    restatement of the same equations."""
    tau = 0.02

    def __init__(self, n_envs, degrees=12, h_range=2.4, min_gravity=9.8, max_gravity=10.4, min_pole_length=0.5, max_pole_length=1.0,
                 min_cart_mass=1.0, max_cart_mass=1.5, min_pole_mass=0.1, max_pole_mass=0.2, min_force_mag=10., max_force_mag=10.,
                 max_steps=500, seed=0, **_ignored):
        _cartpole_setup(self, n_envs, degrees, h_range, min_gravity, max_gravity, min_pole_length, max_pole_length, min_cart_mass, max_cart_mass,
                        min_pole_mass, max_pole_mass, min_force_mag, max_force_mag, max_steps, seed)
        self.rng = np.random.default_rng(seed)
        self.reward = np.ones(n_envs)
        self.info = StepInfo(n_envs, {"env_reward": self.reward})
        self.state = np.zeros((n_envs, 9))
        self.terminated = np.full(n_envs, True)
        self.n_steps = np.zeros(n_envs)

    def _set(self):
        fresh = self.rng.uniform(low=self.low, high=self.high, size=(self.n_envs, 9))
        self.state[self.terminated] = fresh[self.terminated]
        self.n_steps[self.terminated] = 0
        return self.state

    def reset(self):
        self.terminated = np.full(self.n_envs, True)
        self.n_steps = np.zeros(self.n_envs)
        return self._set()

    def step(self, act):
        act = np.asarray(act)
        assert act.size == self.n_envs and np.all(act < 2)
        x, xd, th, thd, g, length, m_cart, m_pole, f_mag = self.state.T
        force = np.where(act.reshape(-1) == 0, -1.0, 1.0) * f_mag
        ct, st = np.cos(th), np.sin(th)
        pml, total = m_pole * length, m_pole + m_cart
        temp = (force + pml * thd ** 2 * st) / total
        thacc = (g * st - ct * temp) / (length * (4.0 / 3.0 - m_pole * ct ** 2 / total))
        xacc = temp - pml * thacc * ct / total
        self.state = np.vstack((x + self.tau * xd, xd + self.tau * xacc, th + self.tau * thd, thd + self.tau * thacc,
                                g, length, m_cart, m_pole, f_mag)).T
        nx, nth = self.state[:, 0], self.state[:, 2]
        self.terminated = (nx < -self.x_threshold) | (nx > self.x_threshold) | (nth < -self.theta_threshold) | (nth > self.theta_threshold)
        self.n_steps += 1
        self.terminated[self.n_steps >= self.max_steps] = True
        if np.any(self.terminated):
            self._set()
        return self.state, self.reward, self.terminated, self.info

    def close(self):
        pass


def _create_pre_vec(ranges, host_cls, device_cls, hyperparameters, is_valid, seed, n_envs, device):
    """create_pre_vec / assign_env_vars (pre_vec_env.py:207-223, helper_pre_vec.py:52-66) behind create_cartpole and create_mountain_car:
    `ranges` holds [training value, validation value] of every constructor argument; a hyper-parameter `<name>` (training) or `<name>_v`
    (validation) overrides an entry, and max_steps may come from the hyper-parameters too.  device: build device_cls, not host_cls."""
    suffix, i = ("_v", -1) if is_valid else ("", 0)
    kw = {k: hyperparameters.get(k + suffix, v[i]) for k, v in ranges.items()}
    if "max_steps" in hyperparameters:
        kw["max_steps"] = hyperparameters["max_steps"]
    cls = device_cls if device else host_cls
    return cls(n_envs if n_envs is not None else hyperparameters.get("n_envs", 32), seed=seed, **kw)


# create_cartpole (discrete_env/cartpole_pre_vec.py:397-412): [training value, validation value] of every constructor argument
CARTPOLE_PARAM_RANGE = {"degrees": [12], "h_range": [2.4], "min_gravity": [9.8, 10.4], "max_gravity": [10.4, 24.8],
                        "min_pole_length": [0.5, 1.0], "max_pole_length": [1.0, 2.0], "min_cart_mass": [1.0, 2.], "max_cart_mass": [1.5, 3.],
                        "min_pole_mass": [0.1, .2], "max_pole_mass": [0.2, .4], "min_force_mag": [10.], "max_force_mag": [10.]}


class _DeviceEnv:
    """What the device-resident envs share: the env lives in an engine context.  `attach_engine(engine)` (the agent does it) creates it
    there through the subclass's `_create`; reset() / step(act) then go through mi_env_reset / mi_env_step, one synchronisation each."""
    on_device = True
    engine = None

    def attach_engine(self, engine):
        """Create the env in `engine`'s context (an MLP engine with this env's observation width, action count and n_envs environments)."""
        if self.engine is engine:
            return
        if engine.E != self.n_envs:
            raise ValueError(f"engine has {engine.E} envs, the env {self.n_envs}")
        self._create(engine)
        self.engine = engine

    def _eng(self):
        if self.engine is None:
            raise RuntimeError(f"{type(self).__name__} is not attached to an engine yet: construct the agent with it (or call attach_engine) first")
        return self.engine

    def reset(self):
        eng = self._eng()
        eng.env_reset()
        return eng.get_obs(0)

    def step(self, act):
        obs, rew, done = self._eng().env_step(act)
        return obs, rew, done, StepInfo(self.n_envs, {"env_reward": rew})

    def close(self):
        pass


class DeviceCartPole(_DeviceEnv):
    """CartPoleVec with the env on the device (train.py --device_env; csrc/env_device.hip `CartPole`, mi_env_* in include/mi355ppo.h): state,
    physics, termination, episode resets, reward and done live in HBM next to the policy, so that the agent collects a whole rollout
    with ONE call and no host round trip per step (agents/ppo.py `_collect_device`).  Same constructor arguments, spaces, ranges,
    thresholds (the same fp64 bits) and step arithmetic (fp64, the same operation order) as CartPoleVec.

    What differs is the random stream of the episode starts.  CartPoleVec draws a whole (n_envs, 9) block from numpy's PCG64 whenever ANY
    env ends and keeps the ended rows; that is NOT reproduced.  Here the start of episode k of env e is low + (high - low) * u per column
    with u a 53-bit uniform from Philox4x32-10 keyed by `seed`, counter {e, k low word, k high word, block}: a function of (seed, env,
    episode) alone, whatever the other envs do.  Trajectories of the two classes therefore agree step for step until the first reset and
    in distribution afterwards.

    The env lives in an engine context: `attach_engine(engine)` (the agent does it) creates it there; reset() / step(act) then go through
    mi_env_reset / mi_env_step, one synchronisation each, so the VecEnv protocol and the public predict / store loop still work.
    Limits: the 9-observation MLP cart-pole, non-recurrent policies, one GPU."""

    def __init__(self, n_envs, degrees=12, h_range=2.4, min_gravity=9.8, max_gravity=10.4, min_pole_length=0.5, max_pole_length=1.0,
                 min_cart_mass=1.0, max_cart_mass=1.5, min_pole_mass=0.1, max_pole_mass=0.2, min_force_mag=10., max_force_mag=10.,
                 max_steps=500, seed=0, **_ignored):
        _cartpole_setup(self, n_envs, degrees, h_range, min_gravity, max_gravity, min_pole_length, max_pole_length, min_cart_mass, max_cart_mass,
                        min_pole_mass, max_pole_mass, min_force_mag, max_force_mag, max_steps, seed)

    def _create(self, engine):
        engine.env_cartpole_create(self.low, self.high, self.x_threshold, self.theta_threshold, self.max_steps, self.seed)


def create_cartpole(hyperparameters, is_valid=False, seed=0, n_envs=None, device=False):
    """create_cartpole / create_pre_vec / assign_env_vars (cartpole_pre_vec.py:397-412, pre_vec_env.py:207-223, helper_pre_vec.py:52-66):
    the validation env draws its physics from the SECOND value of every range (heavier, longer, stronger gravity); a hyper-parameter
    `<name>` (training) or `<name>_v` (validation) overrides a range entry (config.yml `cartpole`: degrees_v 9, h_range_v 1.8);
    max_steps may come from the hyper-parameters too.  device=True: the same arguments build the device-resident DeviceCartPole."""
    return _create_pre_vec(CARTPOLE_PARAM_RANGE, CartPoleVec, DeviceCartPole, hyperparameters, is_valid, seed, n_envs, device)


def _cartpole_swing_setup(self, n_envs, h_range, min_gravity, max_gravity, min_pole_length, max_pole_length, min_cart_mass, max_cart_mass,
                          min_pole_mass, max_pole_mass, min_force_mag, max_force_mag, max_steps, seed):
    """The constructor part that CartPoleSwingVec and DeviceCartPoleSwing share: the one threshold (cartpole_swing_pre_vec.py:124) and
    the start ranges per state column (:155-163: the pole hangs down, theta in pi -+ 0.05)."""
    if n_envs < 2:
        raise Exception("n_envs must be greater than or equal to 2")
    self.n_envs = self.num_envs = n_envs
    self.max_steps, self.seed = max_steps, int(seed)
    self.x_threshold = h_range
    self.low = np.array([-0.05, -0.05, np.pi - 0.05, -0.05, min_gravity, min_pole_length, min_cart_mass, min_pole_mass, min_force_mag],
                        dtype=np.float64)
    self.high = np.array([0.05, 0.05, np.pi + 0.05, 0.05, max_gravity, max_pole_length, max_cart_mass, max_pole_mass, max_force_mag],
                         dtype=np.float64)
    self.observation_space = _Space(shape=(9,))
    self.action_space = _Space(n=2)


class CartPoleSwingVec:
    """The reference's pre-vectorised swing-up cart-pole (discrete_env/cartpole_swing_pre_vec.py:19-239 on discrete_env/pre_vec_env.py:21-125),
    restated in numpy float64: the env of `--env_name cartpole_swing`, which the reference's sweep runs with the `mlpmodel` set.
    Observation = the cart-pole's 9-column state

        [x, x_dot, theta, theta_dot, gravity, pole_length, cart_mass, pole_mass, force_mag]

    and its 2 actions and Euler step (tau = 0.02, CartPoleVec.step's operation order), but another task: every episode starts with the
    pole hanging DOWN (theta drawn from pi -+ 0.05, the other dynamic variables from +-0.05, the parameters from their ranges); an
    episode terminates only beyond +-h_range -- there is no angle threshold -- and is truncated at max_steps (default 1000).  Reward, of
    the post-step, pre-reset state (:230-238): rt = cos(theta), set to 0 where rt < 0 (the pole below the horizontal), rx = cos((x /
    x_threshold) * (pi / 2)) (1 in the centre, 0 at the edge), reward = rt * rx.  A row that has just ended beyond the edge with rt = 0
    has rx < 0 and yields -0.0: kept.  info = {'env_reward': reward}.  When ANY env ends a whole (n_envs, 9) block is drawn and only the
    ended rows take their values, and `done` is the `terminated` array AFTER the reset.

    The generator is numpy's default_rng(seed) -- what gymnasium's seeding.np_random(seed) constructs -- and is consumed exactly as the
    reference consumes it, including the block its constructor draws through reset(seed=seed) before the caller's own reset().  Parity
    is PINNED: tests/golden/g18_cartpole_swing.npz holds trajectories of the reference's own class
    (tests/golden/make_golden_cartpole_swing.py) and tests/test_cartpole_swing_host.py reproduces them bit for bit."""
    tau = 0.02

    def __init__(self, n_envs, h_range=2.4, min_gravity=9.8, max_gravity=10.4, min_pole_length=0.5, max_pole_length=1.0, min_cart_mass=1.0,
                 max_cart_mass=1.5, min_pole_mass=0.1, max_pole_mass=0.2, min_force_mag=10., max_force_mag=10., max_steps=1000, seed=0,
                 **_ignored):
        _cartpole_swing_setup(self, n_envs, h_range, min_gravity, max_gravity, min_pole_length, max_pole_length, min_cart_mass, max_cart_mass,
                              min_pole_mass, max_pole_mass, min_force_mag, max_force_mag, max_steps, seed)
        self.rng = np.random.default_rng(seed)
        self.reward = np.zeros(n_envs)
        self.info = StepInfo(n_envs, {"env_reward": self.reward})
        self.state = np.zeros((n_envs, 9))
        self.reset()                                     # the reference's constructor ends in reset(seed=seed): one block is consumed here

    def _set(self):
        fresh = self.rng.uniform(low=self.low, high=self.high, size=(self.n_envs, 9))
        self.state[self.terminated] = fresh[self.terminated]
        self.n_steps[self.terminated] = 0
        return self.state

    def reset(self):
        self.terminated = np.full(self.n_envs, True)
        self.n_steps = np.zeros(self.n_envs)
        return self._set()

    def step(self, act):
        act = np.asarray(act)
        assert act.size == self.n_envs and np.all(act < 2)
        x, xd, th, thd, g, length, m_cart, m_pole, f_mag = self.state.T
        force = np.where(act.reshape(-1) == 0, -1.0, 1.0) * f_mag
        ct, st = np.cos(th), np.sin(th)
        pml, total = m_pole * length, m_pole + m_cart
        temp = (force + pml * thd ** 2 * st) / total
        thacc = (g * st - ct * temp) / (length * (4.0 / 3.0 - m_pole * ct ** 2 / total))
        xacc = temp - pml * thacc * ct / total
        nx, nth = x + self.tau * xd, th + self.tau * thd
        self.state = np.vstack((nx, xd + self.tau * xacc, nth, thd + self.tau * thacc, g, length, m_cart, m_pole, f_mag)).T
        self.terminated = (nx < -self.x_threshold) | (nx > self.x_threshold)
        rt = np.cos(nth)
        rt[rt < 0] = 0
        self.reward = rt * np.cos((nx / self.x_threshold) * (np.pi / 2.0))
        self.info = StepInfo(self.n_envs, {"env_reward": self.reward})
        self.n_steps += 1
        self.terminated[self.n_steps >= self.max_steps] = True
        if np.any(self.terminated):
            self._set()
        return self.state, self.reward, self.terminated, self.info

    def close(self):
        pass


class DeviceCartPoleSwing(_DeviceEnv):
    """CartPoleSwingVec with the env on the device (train.py --device_env; csrc/env_physics.h `CartPoleSwing`, mi_env_* in include/mi355ppo.h):
    same constructor arguments, spaces, start ranges and threshold (the same fp64 bits) and the same step arithmetic in fp64 in the same
    operation order -- the dynamics are the device function DeviceCartPole runs.  As for DeviceCartPole the stream of the episode starts
    is the device env's own: the start of episode k of env e comes from Philox4x32-10 keyed by `seed`, counter {e, k low word, k high word,
    block}; CartPoleSwingVec's numpy block draws are NOT reproduced, so the two classes agree step for step until the first reset and in
    distribution afterwards.  The reward reaches the host as float32.
    Limits: the 9-observation MLP policy, non-recurrent, one GPU."""

    def __init__(self, n_envs, h_range=2.4, min_gravity=9.8, max_gravity=10.4, min_pole_length=0.5, max_pole_length=1.0, min_cart_mass=1.0,
                 max_cart_mass=1.5, min_pole_mass=0.1, max_pole_mass=0.2, min_force_mag=10., max_force_mag=10., max_steps=1000, seed=0,
                 **_ignored):
        _cartpole_swing_setup(self, n_envs, h_range, min_gravity, max_gravity, min_pole_length, max_pole_length, min_cart_mass, max_cart_mass,
                              min_pole_mass, max_pole_mass, min_force_mag, max_force_mag, max_steps, seed)

    def _create(self, engine):
        engine.env_cartpole_swing_create(self.low, self.high, self.x_threshold, self.max_steps, self.seed)


# create_cartpole_swing (discrete_env/cartpole_swing_pre_vec.py:313-327): create_cartpole's ranges without `degrees`
CARTPOLE_SWING_PARAM_RANGE = {k: v for k, v in CARTPOLE_PARAM_RANGE.items() if k != "degrees"}


def create_cartpole_swing(hyperparameters, is_valid=False, seed=0, n_envs=None, device=False):
    """create_cartpole_swing / create_pre_vec / assign_env_vars: as create_cartpole -- the validation env takes the SECOND value of every
    range, a hyper-parameter `<name>` (training) or `<name>_v` (validation) overrides a range entry, max_steps may come from the
    hyper-parameters too (else the class's 1000).  device=True: the same arguments build the device-resident DeviceCartPoleSwing."""
    return _create_pre_vec(CARTPOLE_SWING_PARAM_RANGE, CartPoleSwingVec, DeviceCartPoleSwing, hyperparameters, is_valid, seed, n_envs, device)


def mountain_car_acceptance(min_goal_position, max_goal_position, min_right_boundary, max_right_boundary):
    """P(goal_position <= right_boundary) for independent uniforms goal_position ~ U[min_goal, max_goal], right_boundary ~ U[min_right,
    max_right]: the probability that the start space accepts a draw.  With F the distribution function of goal_position and H its
    antiderivative (0 below min_goal, a parabola up to max_goal, a line of slope 1 beyond), it is the mean of F over the boundary's
    range, (H(max_right) - H(min_right)) / (max_right - min_right); a range of width 0 is a point."""
    a, b, c, d = float(min_goal_position), float(max_goal_position), float(min_right_boundary), float(max_right_boundary)
    if b == a:
        F, H = (lambda r: 1.0 if r >= a else 0.0), (lambda r: max(r - a, 0.0))
    else:
        F = lambda r: min(max((r - a) / (b - a), 0.0), 1.0)
        H = lambda r: 0.0 if r <= a else (r - a) ** 2 / (2 * (b - a)) if r <= b else (b - a) / 2 + (r - b)
    return F(c) if d == c else (H(d) - H(c)) / (d - c)


def _mountain_car_setup(self, n_envs, goal_velocity, left_boundary, min_start_position, max_start_position, max_speed, min_goal_position,
                        max_goal_position, min_gravity, max_gravity, min_right_boundary, max_right_boundary, force, max_steps, sparse_rewards, seed):
    """The constructor part that MountainCarVec and DeviceMountainCar share: the reference's three range assertions
    (mountain_car_pre_vec.py:141-146), the start ranges per state column (:158-159) and the scalars of the step."""
    assert min_start_position >= left_boundary, f"min_start_position ({min_start_position}) must be >= left_boundary ({left_boundary})"
    assert max_start_position <= min_right_boundary, f"max_start_position ({max_start_position}) must be <= min_right_boundary ({min_right_boundary})"
    assert max_goal_position <= max_right_boundary, f"max_goal_position ({max_goal_position}) must be <= max_right_boundary ({max_right_boundary})"
    if n_envs < 2:
        raise Exception("n_envs must be greater than or equal to 2")
    accept = mountain_car_acceptance(min_goal_position, max_goal_position, min_right_boundary, max_right_boundary)
    if not accept >= 0.5:
        raise ValueError(f"mountain_car: the start space accepts a draw (goal_position <= right_boundary) with probability {accept:.4g} < 1/2 "
                         f"for min_goal_position {min_goal_position}, max_goal_position {max_goal_position}, min_right_boundary "
                         f"{min_right_boundary}, max_right_boundary {max_right_boundary}: the rejection sampling would run long or for ever")
    self.n_envs = self.num_envs = n_envs
    self.max_steps, self.sparse_rewards, self.seed = max_steps, bool(sparse_rewards), int(seed)
    self.goal_velocity, self.left_boundary, self.max_speed, self.force = goal_velocity, left_boundary, max_speed, force
    self.low = np.array([min_start_position, 0, min_gravity, min_right_boundary, min_goal_position], dtype=np.float64)
    self.high = np.array([max_start_position, 0, max_gravity, max_right_boundary, max_goal_position], dtype=np.float64)
    self.observation_space = _Space(shape=(5,))
    self.action_space = _Space(n=3)


class MountainCarVec:
    """The reference's pre-vectorised mountain car (discrete_env/mountain_car_pre_vec.py:15-219 on discrete_env/pre_vec_env.py:21-125 and
    helper_pre_vec.py:4-38), restated in numpy float64: the env of the `mountain_car` hyper-parameter set.  Observation = the 5-column state

        [position, velocity, gravity, right_boundary, goal_position]

    -- the two dynamic variables plus the three parameters an episode was drawn with; 3 actions (push left / none / push right).  A step
    (:194-209): v += (a - 1) * force + cos(3 p) * (-gravity), clipped to +-max_speed; p += v, clipped to [left_boundary, right_boundary];
    v = 0 where the car sits on the left wall with v < 0; terminated where p >= goal_position and v >= goal_velocity; truncation at
    max_steps (pre_vec_env.py:84-86).  Reward -1 with sparse_rewards, else the height sin(3 p) * 0.45 + 0.55 - 1 of the post-step,
    pre-reset position; info = {'env_reward': reward}.  When ANY env ends a whole block is drawn and only the ended rows take their
    values, and `done` is the `terminated` array AFTER the reset.

    Episode starts are StartSpace.sample with its condition (helper_pre_vec.py:28-38): (10 n, 5) uniforms, rows with goal_position >
    right_boundary dropped, further (10 n, 5) blocks while fewer than n rows remain, the first n kept.  The generator is numpy's
    default_rng(seed) -- what gymnasium's seeding.np_random(seed) constructs -- and is consumed exactly as the reference consumes it,
    including the draw its constructor makes through reset(seed=seed) before the caller's own reset().  Parity is PINNED:
    tests/golden/g17_mountain_car.npz holds trajectories of the reference's own class (tests/golden/make_golden_mountain_car.py) and
    tests/test_mountain_car_host.py reproduces them bit for bit.

    One addition: a range set whose draws are accepted with probability below 1/2 (`mountain_car_acceptance`) is refused at
    construction; the reference would loop long or for ever on it."""

    def __init__(self, n_envs=2, goal_velocity=0, left_boundary=-1.2, min_start_position=-0.6, max_start_position=-0.4, max_speed=0.07,
                 min_goal_position=0.5, max_goal_position=3, min_gravity=0.001, max_gravity=0.0025, min_right_boundary=0.6,
                 max_right_boundary=5, force=0.001, max_steps=500, sparse_rewards=True, seed=0, **_ignored):
        _mountain_car_setup(self, n_envs, goal_velocity, left_boundary, min_start_position, max_start_position, max_speed, min_goal_position,
                            max_goal_position, min_gravity, max_gravity, min_right_boundary, max_right_boundary, force, max_steps,
                            sparse_rewards, seed)
        self.rng = np.random.default_rng(seed)
        self.reward = np.full(n_envs, -1.0)
        self.info = StepInfo(n_envs, {"env_reward": self.reward})
        self.state = np.zeros((n_envs, 5))
        self.reset()                                     # the reference's constructor ends in reset(seed=seed): one sample is consumed here

    def _sample(self):
        n = self.n_envs
        x = self.rng.uniform(low=self.low, high=self.high, size=(n * 10, 5))
        x = x[(x[:, 4] > x[:, 3]) == False]              # noqa: E712 (the reference's expression: a NaN row would be kept)
        while len(x) < n:
            z = self.rng.uniform(low=self.low, high=self.high, size=(n * 10, 5))
            x = np.vstack((x, z[(z[:, 4] > z[:, 3]) == False]))      # noqa: E712
        return x[:n]

    def _set(self):
        fresh = self._sample()
        self.state[self.terminated] = fresh[self.terminated]
        self.n_steps[self.terminated] = 0
        return self.state

    def reset(self):
        self.terminated = np.full(self.n_envs, True)
        self.n_steps = np.zeros(self.n_envs)
        return self._set()

    def step(self, act):
        act = np.asarray(act)
        assert act.size == self.n_envs and np.all(act < 3)
        p, v, g, rb, gp = self.state.T
        v = v + ((act.reshape(-1) - 1) * self.force + np.cos(3 * p) * (-g))
        v = np.clip(v, -self.max_speed, self.max_speed)
        p = np.clip(p + v, self.left_boundary, rb)
        v[(p == self.left_boundary) & (v < 0)] = 0
        self.terminated = (p >= gp) & (v >= self.goal_velocity)
        self.state = np.vstack((p, v, g, rb, gp)).T
        if not self.sparse_rewards:
            self.reward = np.sin(3 * p) * 0.45 + 0.55 - 1
            self.info = StepInfo(self.n_envs, {"env_reward": self.reward})
        self.n_steps += 1
        self.terminated[self.n_steps >= self.max_steps] = True
        if np.any(self.terminated):
            self._set()
        return self.state, self.reward, self.terminated, self.info

    def close(self):
        pass


class DeviceMountainCar(_DeviceEnv):
    """MountainCarVec with the env on the device (train.py --device_env; csrc/env_device.hip `MountainCar`, mi_env_* in include/mi355ppo.h): same
    constructor arguments, assertions, spaces, start ranges and scalars (the same fp64 bits) and the same step arithmetic in fp64 in
    the same operation order.  As for DeviceCartPole the stream of the episode starts is the device env's own: the start of episode k of
    env e comes from Philox4x32-10 keyed by `seed`, counter {e, k low word, k high word, 3 * attempt + block}; attempts 0, 1, ... are
    drawn until goal_position <= right_boundary, and after 32 rejected attempts the last draw is kept with goal_position =
    right_boundary (probability at most 2^-32 per reset under the acceptance rule of the constructor).  MountainCarVec's numpy block
    draws are NOT reproduced: the two classes agree step for step until the first reset and in distribution afterwards.
    Limits: the 5-observation MLP mountain car, non-recurrent policies, one GPU."""

    def __init__(self, n_envs=2, goal_velocity=0, left_boundary=-1.2, min_start_position=-0.6, max_start_position=-0.4, max_speed=0.07,
                 min_goal_position=0.5, max_goal_position=3, min_gravity=0.001, max_gravity=0.0025, min_right_boundary=0.6,
                 max_right_boundary=5, force=0.001, max_steps=500, sparse_rewards=True, seed=0, **_ignored):
        _mountain_car_setup(self, n_envs, goal_velocity, left_boundary, min_start_position, max_start_position, max_speed, min_goal_position,
                            max_goal_position, min_gravity, max_gravity, min_right_boundary, max_right_boundary, force, max_steps,
                            sparse_rewards, seed)

    def _create(self, engine):
        engine.env_mountain_car_create(self.low, self.high, self.left_boundary, self.max_speed, self.force, self.goal_velocity, self.max_steps,
                                       self.sparse_rewards, self.seed)


# create_mountain_car (discrete_env/mountain_car_pre_vec.py:312-328): [training value, validation value] of every constructor argument
MOUNTAIN_CAR_PARAM_RANGE = {"goal_velocity": [0], "left_boundary": [-1.2], "min_right_boundary": [0.6, 1.], "max_right_boundary": [1., 5.],
                            "max_speed": [0.07], "min_goal_position": [0, 0.6], "max_goal_position": [0.6, 3], "force": [0.001],
                            "min_gravity": [0.001, 0.0015], "max_gravity": [0.0015, 0.0025], "sparse_rewards": [True]}


def create_mountain_car(hyperparameters, is_valid=False, seed=0, n_envs=None, device=False):
    """create_mountain_car / create_pre_vec / assign_env_vars: as create_cartpole -- the validation env takes the SECOND value of every
    range (goal and right wall further out, stronger gravity; about 21 % of its start draws are rejected), a hyper-parameter `<name>`
    (training) or `<name>_v` (validation) overrides a range entry, sparse_rewards among them; max_steps may come from the
    hyper-parameters too.  device=True: the same arguments build the device-resident DeviceMountainCar."""
    return _create_pre_vec(MOUNTAIN_CAR_PARAM_RANGE, MountainCarVec, DeviceMountainCar, hyperparameters, is_valid, seed, n_envs, device)


class VectorEnv(NamedTuple):
    """One pre-vectorised env of train.py: `label` is how refusals name it, `create` its create_* function, the two classes its host
    and device-resident forms."""
    label: str
    create: Callable
    host_cls: type
    device_cls: type


# env-name pattern (fnmatch: `cartpole*` = every name that starts with cartpole) -> the env.  train.py's env construction, its exclusion
# of these envs from the env groups and its --device_env check all read this table, so a further env is one entry here.
VECTOR_ENVS = {"cartpole*": VectorEnv("the cart-pole (cartpole*)", create_cartpole, CartPoleVec, DeviceCartPole),
               "mountain_car": VectorEnv("mountain_car", create_mountain_car, MountainCarVec, DeviceMountainCar)}


def vector_env(env_name):
    """The VECTOR_ENVS entry of an env name, or None (synthetic frames, Procgen)."""
    return next((v for pattern, v in VECTOR_ENVS.items() if fnmatchcase(env_name, pattern)), None)


def create_vector_env(env_name, hyperparameters, is_valid=False, seed=0, n_envs=None, device=False):
    """Build the pre-vectorised env of an env name that `vector_env` knows: the swing-up cart-pole for the exact name `cartpole_swing`
    (the reference's env_constructor maps that name to create_cartpole_swing; the `cartpole*` row would build the balance task under
    it), else the `create` of the name's VECTOR_ENVS row."""
    create = create_cartpole_swing if env_name == "cartpole_swing" else vector_env(env_name).create
    return create(hyperparameters, is_valid, seed=seed, n_envs=n_envs, device=device)


def device_env_labels():
    """`the cart-pole (cartpole*) and mountain_car`: the envs that have a device-resident form, for messages."""
    labels = [v.label for v in VECTOR_ENVS.values()]
    return ", ".join(labels[:-1]) + " and " + labels[-1]


class SyntheticFrames:
    def __init__(self, n_envs, n_actions=15, seed=0, pool=8):
        self.n_envs = n_envs
        self.rng = np.random.default_rng(seed)
        self.observation_space = _Space(shape=(3, 64, 64))
        self.action_space = _Space(n=n_actions)
        self._pool = [self.rng.integers(0, 256, size=(n_envs, 64, 64, 3), dtype=np.uint8) for _ in range(pool)]
        self._k = 0
        self._level = np.arange(n_envs) % 500

    def _obs(self):
        self._k = (self._k + 1) % len(self._pool)
        return self._pool[self._k]                       # uint8 NHWC: what Procgen's 'rgb' delivers

    def reset(self):
        return self._obs()

    def step(self, act):
        rew = self.rng.standard_normal(self.n_envs).astype(np.float32)
        done = self.rng.random(self.n_envs) < 0.01
        return self._obs(), rew, done, StepInfo(self.n_envs, {"env_reward": rew, "prev_level_seed": self._level})

    def close(self):
        pass


class SyntheticTape(SyntheticFrames):
    """SyntheticFrames with every random draw made up front (a tape of `length` steps, replayed in a loop): step() is a few
    microseconds of host work whatever n_envs is.  bench.py's stand-in for the Procgen engine -- the metric excludes env.step's own
    cost, and a group's env.step sits INSIDE the rollout's dependency chain, so the stand-in must not be what the chain waits for.
    Frames are handed out from a small pool of ordinary (pageable) numpy arrays, as an engine would from its own buffers."""

    def __init__(self, n_envs, n_actions=15, seed=0, pool=4, length=256):
        super().__init__(n_envs, n_actions, seed, pool)
        self._rew = self.rng.standard_normal((length, n_envs)).astype(np.float32)
        self._done = self.rng.random((length, n_envs)) < 0.01
        self._info = [StepInfo(n_envs, {"env_reward": self._rew[i], "prev_level_seed": self._level}) for i in range(length)]
        self._i = -1

    def step(self, act):
        self._i = i = (self._i + 1) % len(self._info)
        return self._obs(), self._rew[i], self._done[i], self._info[i]


class EnvGroups:
    """G independent vector envs shown as ONE VecEnv of sum(n_envs) environments (reset / step concatenate in group order), plus
    `.env_groups` for the agent's pipelined collector (agents/ppo.py `_collect_pipelined`): an env's next observation depends only
    on its own action, so the agent steps group g on the host while the device works on the other groups' frames."""

    def __init__(self, envs):
        self.env_groups = list(envs)
        e0 = self.env_groups[0]
        self.n_envs = self.num_envs = sum(getattr(e, "n_envs", getattr(e, "num_envs", 0)) for e in self.env_groups)
        self.observation_space, self.action_space = e0.observation_space, e0.action_space
        for k in ("combos", "unique_actions"):
            if hasattr(e0, k):
                setattr(self, k, getattr(e0, k))

    def reset(self):
        return np.concatenate([e.reset() for e in self.env_groups])

    def step(self, act):
        act = np.asarray(act)
        outs, o = [], 0
        for e in self.env_groups:
            n = getattr(e, "n_envs", getattr(e, "num_envs", 0))
            outs.append(e.step(act[o:o + n])); o += n
        return (np.concatenate([x[0] for x in outs]), np.concatenate([x[1] for x in outs]), np.concatenate([x[2] for x in outs]),
                StepInfo.join([x[3] for x in outs]))

    def reward_state(self):
        rs = getattr(self.env_groups[0], "reward_state", None)
        return rs() if callable(rs) else None

    def close(self):
        for e in self.env_groups:
            e.close()


def create_procgen_env(**kwargs):
    """The Procgen engine behind the one-object wrapper chain of common/env/procgen_pipeline.py (uint8 NHWC frames out)."""
    from common.env.procgen_pipeline import create_procgen_env as make
    return make(**kwargs)
