"""Shared inputs of the device cart-pole tests (tests/test_cartpole_device_host.py, tests/test_gpu_cartpole_env.py): a numpy restatement of
the device env's reset stream, CartPoleVec's own step arithmetic driven by that stream (the float64 replay), and the teacher-forced
one-step case.  The float64 reference of the dynamics is CartPoleVec.step itself (common/env/vec_envs.py), never a copy of it."""
import numpy as np

from common.env.vec_envs import CartPoleVec
from oracle.philox import philox4x32_10


def philox_u53(seed, env, episode):
    """The nine 53-bit uniforms of the start of episode `episode` of env `env` (csrc/env_device.hip): Philox4x32-10 keyed by the 64-bit
    seed, counter {env, episode low word, episode high word, block}, block 0..4; output words {0, 1} and {2, 3} of block b give the
    uniforms of columns 2b and 2b + 1 as ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53 (18 words used, 20 drawn).  env, episode: ints or int
    arrays of one shape -> (n, 9) float64 in [0, 1)."""
    env, episode = np.broadcast_arrays(np.asarray(env, np.int64).reshape(-1), np.asarray(episode, np.int64).reshape(-1))
    n = env.size
    ctr = np.zeros((n, 5, 4), np.uint32)
    ep = episode.astype(np.uint64)
    ctr[:, :, 0] = env.astype(np.uint64).astype(np.uint32)[:, None]
    ctr[:, :, 1] = (ep & np.uint64(0xffffffff)).astype(np.uint32)[:, None]
    ctr[:, :, 2] = (ep >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[:, :, 3] = np.arange(5, dtype=np.uint32)[None, :]
    key = np.empty((n * 5, 2), np.uint32)
    key[:, 0] = np.uint32(int(seed) & 0xffffffff)
    key[:, 1] = np.uint32((int(seed) >> 32) & 0xffffffff)
    w = philox4x32_10(ctr.reshape(-1, 4), key).reshape(n, 10, 2)
    u = ((w[:, :, 0] >> np.uint32(5)).astype(np.float64) * 67108864.0 + (w[:, :, 1] >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53
    return u[:, :9]


def fresh_state(low, high, seed, env, episode):
    """low + (high - low) * u per column: the state an episode starts in."""
    return low[None, :] + (high - low)[None, :] * philox_u53(seed, env, episode)


def within_ulp(a, b, ulps):
    return np.abs(a - b) <= ulps * np.spacing(np.abs(b))


class ReplayCartPole(CartPoleVec):
    """CartPoleVec.step as it is, with the episode starts of the device env: `_set` gives the ended rows episode + 1 from the Philox
    restatement instead of numpy's block draw.  `post` is the state right after the last Euler step, before any reset."""

    def __init__(self, n_envs, seed=0, **kw):
        super().__init__(n_envs, seed=seed, **kw)
        self.philox_seed = seed
        self.episode = np.zeros(n_envs, np.int64)
        self.post = None

    def _set(self):
        self.post = self.state.copy()
        idx = np.nonzero(self.terminated)[0]
        self.episode[idx] += 1
        self.state[idx] = fresh_state(self.low, self.high, self.philox_seed, idx, self.episode[idx])
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
        """smallest distance of the last step's post-step x / theta from a threshold"""
        return min(np.abs(np.abs(self.post[:, 0]) - self.x_threshold).min(), np.abs(np.abs(self.post[:, 2]) - self.theta_threshold).min())


def replay(env, state, n_steps, episode, actions):
    """Run `env` (a ReplayCartPole) from (state, n_steps, episode) on actions (T, E) -> obs (T + 1, E, 9) float64 (obs[0] = state, obs[t + 1]
    = the post-reset state of step t), done (T, E) bool, beyond (T, E) bool (the post-step x or theta lies beyond a threshold: a
    termination; done without it is a truncation), the smallest threshold margin of all steps."""
    env.load(state, n_steps, episode)
    obs, done, beyond, margin = [env.state.copy()], [], [], np.inf
    for a in actions:
        s, _, d, _ = env.step(a)
        obs.append(s.copy()); done.append(d.copy())
        beyond.append((np.abs(env.post[:, 0]) > env.x_threshold) | (np.abs(env.post[:, 2]) > env.theta_threshold))
        margin = min(margin, env.margin())
    return np.stack(obs), np.stack(done), np.stack(beyond), margin


# ---- the teacher-forced one-step case: E = 70 = a full wave plus a 6-row tail
ONE_STEP_E, ONE_STEP_MAX_STEPS, ONE_STEP_SEED = 70, 37, 0x1234567890abcdef
THRESHOLD_ROWS = slice(50, 58)        # {+x, -x, +theta, -theta} x {just inside, just outside}
TRUNCATION_ROWS = slice(58, 62)       # n_steps = max_steps - 1 (58, 59: truncate), max_steps - 2 (60, 61: do not)


def one_step_case():
    """-> dict(state (70, 9), n_steps, episode, act, env kwargs).  Rows 0-49 and 62-69: random interior states, both actions; rows
    50-57: the post-step x (theta) lands 1e-6 inside / outside +-x_threshold (+-theta_threshold) -- the Euler step x + tau * x_dot with
    x_dot = 0.5 (theta_dot = 0.25) is exact to ~1e-17, far inside the 1e-9 the test asks for; rows 58-61: the step counter one and two
    short of max_steps.  Episode numbers include one beyond 2^32 (the counter's high word)."""
    rng = np.random.default_rng(70)
    E = ONE_STEP_E
    ref = CartPoleVec(E, max_steps=ONE_STEP_MAX_STEPS)
    state = rng.uniform(ref.low, ref.high, size=(E, 9))
    state[:, :4] = rng.uniform(-0.15, 0.15, size=(E, 4)) * np.array([4.0, 4.0, 1.0, 4.0])      # interior: |x| <= 0.6, |theta| <= 0.15
    act = rng.integers(0, 2, E)
    act[:2] = (0, 1)
    tau, d = CartPoleVec.tau, 1e-6
    for k, (col, thr, rate) in enumerate(((0, ref.x_threshold, 0.5), (0, -ref.x_threshold, -0.5),
                                          (2, ref.theta_threshold, 0.25), (2, -ref.theta_threshold, -0.25))):
        for j, inside in enumerate((True, False)):
            r = THRESHOLD_ROWS.start + 2 * k + j
            state[r, :4] = 0.01
            state[r, col + 1] = rate
            target = thr - np.sign(thr) * d if inside else thr + np.sign(thr) * d
            state[r, col] = target - tau * rate
    n_steps = rng.integers(0, ONE_STEP_MAX_STEPS - 2, E).astype(np.int32)
    n_steps[58:60] = ONE_STEP_MAX_STEPS - 1
    n_steps[60:62] = ONE_STEP_MAX_STEPS - 2
    episode = rng.integers(1, 1000, E).astype(np.int64)
    episode[51] = 2 ** 33 + 5              # an ended row (x just outside): the next episode's counter has a high word
    return dict(state=state, n_steps=n_steps, episode=episode, act=act, kw=dict(max_steps=ONE_STEP_MAX_STEPS))
