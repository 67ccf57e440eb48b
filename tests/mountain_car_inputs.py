"""Shared inputs of the mountain-car tests (tests/test_mountain_car_host.py, tests/test_gpu_mountain_car_env.py): the fixture G17
(trajectories of the reference's own class, tests/golden/make_golden_mountain_car.py), a numpy restatement of the device env's reset
stream with its attempt counter and bounded fallback, and MountainCarVec's own step arithmetic driven by that stream (the float64
replay).  The float64 reference of the dynamics is MountainCarVec.step itself (common/env/vec_envs.py), never a copy of it."""
import json
import os

import numpy as np

from common.env.vec_envs import MountainCarVec
from oracle.philox import philox4x32_10

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_mountain_car.npz")
MAX_ATTEMPTS = 32
VALID = dict(min_right_boundary=1., max_right_boundary=5., min_goal_position=0.6, max_goal_position=3, min_gravity=0.0015, max_gravity=0.0025)
ONE_STEP_E = 70
ONE_STEP_ENDED = {51, 53, 56, 60, 61}      # just beyond the goal, beyond it fast enough, clipped onto a goal at the right wall, two truncations
_cache = {}


def golden():
    """The fixture as a dict (loaded once; the arrays are shared between tests and must not be written to)."""
    if "z" not in _cache:
        with np.load(GOLD, allow_pickle=False) as z:
            _cache["z"] = {k: z[k] for k in z.files}
        for v in _cache["z"].values():
            v.setflags(write=False)
    return _cache["z"]


def one_step_case(sparse=True):
    """-> dict(state (70, 5), n_steps, episode, act, kw, seed, out_state, rew, done): case (b) of the fixture, or (c) with sparse=False.
    The episode numbers are the tests' own (the reference has none); one lies beyond 2^32, on an ended row."""
    z, p = golden(), "b/" if sparse else "c/"
    kw = json.loads(bytes(z["b/kw"]).decode())
    if not sparse:
        kw["sparse_rewards"] = False
    episode = np.random.default_rng(70).integers(1, 1000, ONE_STEP_E).astype(np.int64)
    episode[51] = 2 ** 33 + 5
    return dict(state=z["b/state"], n_steps=z["b/n_steps"], act=z["b/act"], episode=episode, kw=kw, seed=int(z["seeds"][1]),
                out_state=z[p + "out_state"], rew=z[p + "rew"], done=z[p + "done"])


def philox_u53(seed, env, episode, attempt):
    """The five 53-bit uniforms of attempt `attempt` at the start of episode `episode` of env `env` (csrc/env_device.hip):
    Philox4x32-10 keyed by the 64-bit seed, counter {env, episode low word, episode high word, 3 * attempt + b}, b = 0..2; output words
    {0, 1} and {2, 3} of block b give the uniforms of columns 2b and 2b + 1 as ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53 (10 words used, 12
    drawn).  env, episode, attempt: ints or int arrays of one shape -> (n, 5) float64 in [0, 1)."""
    env, episode, attempt = np.broadcast_arrays(np.asarray(env, np.int64).reshape(-1), np.asarray(episode, np.int64).reshape(-1),
                                                np.asarray(attempt, np.int64).reshape(-1))
    n = env.size
    ctr = np.zeros((n, 3, 4), np.uint32)
    ep = episode.astype(np.uint64)
    ctr[:, :, 0] = env.astype(np.uint64).astype(np.uint32)[:, None]
    ctr[:, :, 1] = (ep & np.uint64(0xffffffff)).astype(np.uint32)[:, None]
    ctr[:, :, 2] = (ep >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[:, :, 3] = (3 * attempt[:, None] + np.arange(3)[None, :]).astype(np.uint32)
    key = np.empty((n * 3, 2), np.uint32)
    key[:, 0] = np.uint32(int(seed) & 0xffffffff)
    key[:, 1] = np.uint32((int(seed) >> 32) & 0xffffffff)
    w = philox4x32_10(ctr.reshape(-1, 4), key).reshape(n, 6, 2)
    u = ((w[:, :, 0] >> np.uint32(5)).astype(np.float64) * 67108864.0 + (w[:, :, 1] >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53
    return u[:, :5]


def fresh_state(low, high, seed, env, episode, max_attempts=MAX_ATTEMPTS):
    """-> (state (n, 5), attempts (n,)): low + (high - low) * u per column, attempts 0, 1, ... drawn until !(goal_position >
    right_boundary); attempts = the number drawn.  After max_attempts rejected attempts the last draw is kept with goal_position =
    right_boundary (attempts = max_attempts then, as for a row accepted at the last attempt)."""
    env, episode = np.broadcast_arrays(np.asarray(env, np.int64).reshape(-1), np.asarray(episode, np.int64).reshape(-1))
    state, attempts = np.zeros((env.size, 5)), np.zeros(env.size, np.int64)
    todo = np.arange(env.size)
    for a in range(max_attempts):
        state[todo] = low[None, :] + (high - low)[None, :] * philox_u53(seed, env[todo], episode[todo], a)
        attempts[todo] = a + 1
        todo = todo[state[todo, 4] > state[todo, 3]]
        if not todo.size:
            break
    state[todo, 4] = state[todo, 3]
    return state, attempts


def within_ulp(a, b, ulps):
    return np.abs(a - b) <= ulps * np.spacing(np.abs(b))


class ReplayMountainCar(MountainCarVec):
    """MountainCarVec.step as it is, with the episode starts of the device env: `_set` gives the ended rows episode + 1 from the Philox
    restatement instead of numpy's block draw.  `post` is the state right after the dynamics of the last step, before any reset, and
    `post_reward` that step's reward."""

    def __init__(self, n_envs, seed=0, **kw):
        self.philox_seed = seed
        self.episode = np.zeros(n_envs, np.int64)
        self.post = None
        super().__init__(n_envs, seed=seed, **kw)      # (its constructor resets once: every env is in episode 1 afterwards)

    def _set(self):
        self.post = self.state.copy()
        idx = np.nonzero(self.terminated)[0]
        self.episode[idx] += 1
        self.state[idx] = fresh_state(self.low, self.high, self.philox_seed, idx, self.episode[idx])[0]
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

    def margin_ok(self, eps=1e-9):
        """Per row of the last step: may its done flag be compared with another implementation's?  The post-step position is at least
        eps away from goal_position or is a clipped constant (right_boundary, left_boundary), and the post-step velocity is at least
        eps away from goal_velocity or is a clipped or zeroed constant (+-max_speed, 0 on the left wall)."""
        p, v, rb, gp = self.post[:, 0], self.post[:, 1], self.post[:, 3], self.post[:, 4]
        pos = (np.abs(p - gp) >= eps) | (p == rb) | (p == self.left_boundary)
        vel = (np.abs(v - self.goal_velocity) >= eps) | (np.abs(v) == self.max_speed) | ((v == 0) & (p == self.left_boundary))
        return pos & vel


def replay(env, state, n_steps, episode, actions):
    """Run `env` (a ReplayMountainCar) from (state, n_steps, episode) on actions (T, E) -> obs (T + 1, E, 5) float64 (obs[0] = state,
    obs[t + 1] = the post-reset state of step t), rew (T, E) float64, done (T, E) bool, reached (T, E) bool (the post-step state meets
    the goal: a termination; done without it is a truncation), margin_ok (T, E) bool."""
    env.load(state, n_steps, episode)
    obs, rew, done, reached, ok = [env.state.copy()], [], [], [], []
    for a in actions:
        s, r, d, _ = env.step(a)
        obs.append(s.copy()); rew.append(np.array(r, np.float64)); done.append(d.copy())
        reached.append((env.post[:, 0] >= env.post[:, 4]) & (env.post[:, 1] >= env.goal_velocity))
        ok.append(env.margin_ok())
    return np.stack(obs), np.stack(rew), np.stack(done), np.stack(reached), np.stack(ok)
