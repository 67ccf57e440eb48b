"""Shared inputs of the swing-up cart-pole tests (tests/test_cartpole_swing_host.py, tests/test_gpu_cartpole_swing_env.py): the fixture G18
(trajectories of the reference's own classes, tests/golden/make_golden_cartpole_swing.py), CartPoleSwingVec's own step arithmetic driven
by the numpy restatement of the device env's reset stream (the float64 replay; the stream is the cart-pole's, cartpole_inputs.fresh_state,
with the swing-up's ranges), and the planted rollout case.  The float64 reference of the dynamics and the reward is CartPoleSwingVec.step
itself (common/env/vec_envs.py), never a copy of it."""
import json
import os

import numpy as np

import cartpole_inputs as CI
from common.env.vec_envs import CartPoleSwingVec

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_cartpole_swing.npz")
ONE_STEP_E = 70
ONE_STEP_ENDED = {51, 53, 60, 61}      # x just beyond +h_range and -h_range, two truncations
CLAMP_ROWS = {54: False, 55: True, 56: False, 57: True}      # theta lands 1e-6 short of / beyond +pi/2, -pi/2: the reward clamp off / on
ENV_MARGIN = 1e-9                      # resident_inputs.ENV_MARGIN: the distance a compared post-step x keeps from +-h_range
SMALL = dict(max_steps=5)              # truncations after 5 steps (nobody drifts from +-0.05 to +-2.4 in 5)
H_RANGE = 2.4
_cache = {}


def golden():
    """The fixture as a dict (loaded once; the arrays are shared between tests and must not be written to)."""
    if "z" not in _cache:
        with np.load(GOLD, allow_pickle=False) as z:
            _cache["z"] = {k: z[k] for k in z.files}
        for v in _cache["z"].values():
            v.setflags(write=False)
    return _cache["z"]


def one_step_case():
    """-> dict(state (70, 9), n_steps, episode, act, kw, seed, out_state, rew, done): case (b) of the fixture.  The episode numbers are the
    tests' own (the reference has none); one lies beyond 2^32, on an ended row."""
    z = golden()
    episode = np.random.default_rng(70).integers(1, 1000, ONE_STEP_E).astype(np.int64)
    episode[51] = 2 ** 33 + 5
    return dict(state=z["b/state"], n_steps=z["b/n_steps"], act=z["b/act"], episode=episode, kw=json.loads(bytes(z["b/kw"]).decode()),
                seed=int(z["seeds"][1]), out_state=z["b/out_state"], rew=z["b/rew"], done=z["b/done"])


class ReplayCartPoleSwing(CartPoleSwingVec):
    """CartPoleSwingVec.step as it is, with the episode starts of the device env: `_set` gives the ended rows episode + 1 from the Philox
    restatement instead of numpy's block draw.  `post` is the state right after the last Euler step, before any reset."""

    def __init__(self, n_envs, seed=0, **kw):
        self.philox_seed = seed
        self.episode = np.zeros(n_envs, np.int64)
        self.post = None
        super().__init__(n_envs, seed=seed, **kw)      # (its constructor resets once: every env is in episode 1 afterwards)

    def _set(self):
        self.post = self.state.copy()
        idx = np.nonzero(self.terminated)[0]
        self.episode[idx] += 1
        self.state[idx] = CI.fresh_state(self.low, self.high, self.philox_seed, idx, self.episode[idx])
        self.n_steps[idx] = 0
        return self.state

    def step(self, act):
        self.post = None
        out = super().step(act)
        if self.post is None:
            self.post = self.state.copy()
        return out

    def load(self, state, n_steps, episode):
        self.state = np.array(state, np.float64)
        self.n_steps = np.array(n_steps, np.float64)
        self.episode = np.array(episode, np.int64)
        self.terminated = np.full(self.n_envs, False)

    def margin(self):
        """smallest distance of the last step's post-step x from +-x_threshold (the only threshold this env has)"""
        return np.abs(np.abs(self.post[:, 0]) - self.x_threshold).min()


def replay(env, state, n_steps, episode, actions):
    """Run `env` (a ReplayCartPoleSwing) from (state, n_steps, episode) on actions (T, E) -> obs (T + 1, E, 9) float64 (obs[0] = state,
    obs[t + 1] = the post-reset state of step t), rew (T, E) float64, done (T, E) bool, beyond (T, E) bool (the post-step x lies beyond
    +-x_threshold: a termination; done without it is a truncation), the smallest threshold margin of all steps."""
    env.load(state, n_steps, episode)
    obs, rew, done, beyond, margin = [env.state.copy()], [], [], [], np.inf
    for a in actions:
        s, r, d, _ = env.step(a)
        obs.append(s.copy()); rew.append(np.array(r, np.float64)); done.append(d.copy())
        beyond.append(np.abs(env.post[:, 0]) > env.x_threshold)
        margin = min(margin, env.margin())
    return np.stack(obs), np.stack(rew), np.stack(done), np.stack(beyond), margin


def plant(state):
    """The three planted rows of the rollout tests, written into a copy of `state` (E >= 3, h_range = 2.4).  Env 0: x = h_range - 0.005 with
    x_dot = 0.5, so x + tau * x_dot = h_range + 0.005 after step 1 whatever the action.  Env 1: upright at rest (theta = 0.01): rewards
    above 0.9, truncated.  Env 2: theta = 0.3 at rest, beyond the balance task's 12 degrees: it must go on until it is truncated."""
    s = np.array(state, np.float64)
    s[0, :4] = (H_RANGE - 0.005, 0.5, np.pi, 0.0)
    s[1, :4] = (0.0, 0.0, 0.01, 0.0)
    s[2, :4] = (0.0, 0.0, 0.3, 0.0)
    return s


# the resident-beside-the-chain case: E = 70 (four 16-env tiles and a 6-row tail), the network and parameters of resident_inputs' "cartpole"
# case (kind "cartpole": the same network shapes), the swing-up's env.  The sampler seed is the first from 77 on for which no uniform lies
# within resident_inputs.U_CLEAR of a float64 CDF edge (checked in tests/test_cartpole_swing_host.py), so that two fp32 evaluations of the
# policy that differ in summation order pick the same actions.
RESIDENT_CASE = dict(kind="cartpole", kw={}, E=70, T=8, depth=4, width=64, out=64, lse=0, env_seed=21, seed=78)


def resident_start(c=RESIDENT_CASE):
    """(state, n_steps, episode): every env at the start of episode 1 (what mi_env_reset leaves after the create call), the three rows planted"""
    E = c["E"]
    rp = ReplayCartPoleSwing(E, seed=c["env_seed"], **SMALL)
    return plant(rp.state), np.zeros(E, np.int32), np.ones(E, np.int64)


def oracle_rollout(c=RESIDENT_CASE):
    """The float64 rollout of the case (resident_inputs.rollout's loop with this env): -> dict(act (T, E), rew, done, beyond, udist (T + 1, E),
    margin).  Computed once and shared: read only."""
    if "oracle" not in _cache:
        import resident_inputs as RI
        from oracle import philox
        E, T = c["E"], c["T"]
        flat = RI.params_of(c)
        env = ReplayCartPoleSwing(E, seed=c["env_seed"], **SMALL)
        env.load(*resident_start(c))
        out = {k: [] for k in ("act", "rew", "done", "beyond", "udist")}
        margin = np.inf
        for t in range(T + 1):
            u = philox.uniform(c["seed"], t * E + np.arange(E))
            _, _, act, _, udist = RI.policy_rows(c, flat, env.state.astype(np.float32), u)
            out["udist"].append(udist)
            if t == T:
                break
            _, r, d, _ = env.step(np.asarray(act, np.int64))
            out["act"].append(act); out["rew"].append(np.array(r, np.float64)); out["done"].append(np.array(d, bool))
            out["beyond"].append(np.abs(env.post[:, 0]) > env.x_threshold)
            margin = min(margin, env.margin())
        out = {k: np.stack(v) for k, v in out.items()}
        for v in out.values():
            v.setflags(write=False)
        out["margin"] = margin
        _cache["oracle"] = out
    return _cache["oracle"]


def within_f32_ulp(got, want64, ulps=1):
    """got (float32) lies within `ulps` float32 ulp of float32(want64), and is 0 wherever want64 is 0 (by value: -0.0 counts as 0)"""
    w32 = np.asarray(want64, np.float64).astype(np.float32)
    ok = np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= ulps * np.spacing(np.abs(w32)).astype(np.float64)
    return ok & ((np.asarray(want64) != 0) | (got == 0))
