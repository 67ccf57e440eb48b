"""The float64 CPU oracle of a whole device-env rollout (mi_env_rollout / mi_env_rollout_resident) and the cases of the resident-rollout
tests (tests/test_resident_rollout_host.py on the CPU, tests/test_gpu_resident_rollout.py on the GPU).  Nothing here touches a GPU.

A rollout is, for t = 0 .. T: observation = float32(state); the MLP and the heads on it in float64 from the flat parameter vector (offsets
from mi355/layout.py); the sampler's uniform of (seed, t * E + e) (oracle/philox.py) and the inverse CDF of oracle.ppo_oracle.sample_actions
on the twice-normalised log-probabilities (policy_inputs.policy_terms); for t < T the env step, which is CartPoleVec.step /
MountainCarVec.step themselves driven by the numpy restatement of the device env's Philox reset stream (cartpole_inputs.ReplayCartPole,
mountain_car_inputs.ReplayMountainCar).  `forced` replaces the oracle's own observations and actions by a device ring's: the stepwise
rule of the GPU test when a device action differs from the oracle's.

Every case is checked on the CPU first (test_resident_rollout_host.py): every replay margin holds, no sampler uniform lies within 1e-4
(ten of the suite's 1e-5 sampler margins) of a float64 CDF edge, and its two rollouts hold a termination, a truncation, a reset and every
action value -- so the oracle alone leaves no row out.  The seeds below were chosen for that, on the CPU, by running this file."""
import numpy as np
import torch
import torch.nn.functional as F

import cartpole_inputs as CI
import mountain_car_inputs as MI
import policy_inputs as PI
from mi355 import layout
from oracle import philox
from oracle import ppo_oracle as O

ENV_MARGIN = 1e-9               # the existing rollout tests' distance of a post-step state from a threshold
U_CLEAR = 10 * PI.U_MARGIN      # what the host test asks of every uniform
POOL_N = PI.POOL_N              # rows torch's float32 error is measured on when a case has fewer than 256
WIDTH = {"cartpole": 9, "mountain_car": 5}
ACTIONS = {"cartpole": 2, "mountain_car": 3}
ENV_KW = {"cartpole": dict(max_steps=5, h_range=0.06), "mountain_car": dict(max_steps=5, **MI.VALID)}

# name -> kind, env kwargs beyond ENV_KW, E, T, depth, width, out, value_from_logits, env seed, sampler seed (of rollout 1; rollout 2: + 1);
# scale: the parameters are scale * default_rng(11).standard_normal (0.2 unless given: at width 256 that saturates the policy, one action only)
CASES = {
    "cartpole": dict(kind="cartpole", kw={}, E=70, T=8, depth=4, width=64, out=64, lse=0, env_seed=21, seed=77),
    "mountain_car_sparse": dict(kind="mountain_car", kw={}, E=70, T=8, depth=4, width=64, out=64, lse=0, env_seed=21, seed=77),
    "mountain_car_dense": dict(kind="mountain_car", kw=dict(sparse_rewards=False), E=70, T=8, depth=4, width=64, out=64, lse=0, env_seed=21, seed=77),
    "wide": dict(kind="cartpole", kw={}, E=18, T=3, depth=4, width=256, out=64, lse=0, env_seed=21, seed=77, scale=0.06),
    "shallow": dict(kind="cartpole", kw={}, E=16, T=3, depth=2, width=64, out=64, lse=0, env_seed=21, seed=77),
    "lse": dict(kind="cartpole", kw={}, E=18, T=3, depth=4, width=64, out=64, lse=1, env_seed=21, seed=77),
}
TEST1 = ("cartpole", "mountain_car_sparse", "mountain_car_dense")
TEST2 = ("wide", "shallow", "lse")
_cache = {}


def env_kwargs(c):
    return dict(ENV_KW[c["kind"]], **c["kw"])


def make_replay(c):
    cls = CI.ReplayCartPole if c["kind"] == "cartpole" else MI.ReplayMountainCar
    return cls(c["E"], seed=c["env_seed"], **env_kwargs(c))


def shapes_of(c):
    return layout.mlp_param_shapes(ACTIONS[c["kind"]], WIDTH[c["kind"]], c["depth"], c["width"], c["out"])


def params_of(c, seed=11):
    """scale * default_rng(11).standard_normal, float32, in the reference's parameters() order (what Engine.set_params takes)"""
    n = sum(int(np.prod(s)) for s in shapes_of(c).values())
    return (c.get("scale", 0.2) * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def fresh(c, env, episode):
    """the state episode `episode` of env `env` starts in (the device env's reset stream restated)"""
    rp = make_replay(c)
    if c["kind"] == "cartpole":
        return CI.fresh_state(rp.low, rp.high, c["env_seed"], env, episode)
    return MI.fresh_state(rp.low, rp.high, c["env_seed"], env, episode)[0]


def initial_state(c):
    """What mi_env_reset leaves right after the create call (every env at the start of episode 1) with the states of the two existing
    rollout tests planted: env 0 ends at its first step whatever the action, env 1 cannot end before it is truncated."""
    E = c["E"]
    s = fresh(c, np.arange(E), np.ones(E, np.int64))
    if c["kind"] == "cartpole":
        s[0, :4] = (0.055, 0.5, 0.0, 0.0)
        s[1, :4] = 0.0
    else:
        s[0, :2] = (s[0, 4] - 1e-3, 0.07)
        s[1, :2] = (-0.5, 0.0)
    return s, np.zeros(E, np.int32), np.ones(E, np.int64)


def head_rows(c, flat, obs, dtype=torch.float64):
    """hout (n, A + 1) = [fc_policy; fc_value] on the MLP's output, in dtype: ReLU after every embedder layer but the last, none in
    front of the heads (MLPModel, common/model.py:954-980; CategoricalPolicy)."""
    p = {k: torch.as_tensor(v).to(dtype) for k, v in layout.unflatten(shapes_of(c), flat).items()}
    x = torch.as_tensor(np.array(obs, np.float32)).to(dtype)
    names = ["embedder.model.0"] + [f"embedder.model.2.{2 * k}" for k in range(c["depth"] - 2)] + ["embedder.model.3"]
    for i, nm in enumerate(names):
        x = F.linear(x, p[nm + ".weight"], p[nm + ".bias"])
        if i + 1 < len(names):
            x = torch.relu(x)
    return torch.cat([F.linear(x, p["fc_policy.weight"], p["fc_policy.bias"]), F.linear(x, p["fc_value.weight"], p["fc_value.bias"])], dim=1)


def policy_rows(c, flat, obs, u, dtype=torch.float64):
    """-> lp (n, A), value (n), act (n), logp (n), udist (n): distance of u to the nearest CDF edge that separates two actions"""
    lp, value = PI.policy_terms(head_rows(c, flat, obs, dtype), bool(c["lse"]))
    uu = torch.as_tensor(np.array(u)).to(dtype)
    act, logp = O.sample_actions(lp, uu)
    cdf = torch.cumsum(torch.exp(lp), dim=1)[:, :-1]
    udist = (cdf - uu.reshape(-1, 1)).abs().min(dim=1).values
    return lp.numpy(), value.numpy(), act.numpy(), logp.numpy(), udist.numpy().astype(np.float64)


def _env_margin(c, env):
    """per row of the last step: may its done flag be compared with another implementation's?"""
    if c["kind"] == "mountain_car":
        return env.margin_ok(ENV_MARGIN)
    return (np.abs(np.abs(env.post[:, 0]) - env.x_threshold) >= ENV_MARGIN) & (np.abs(np.abs(env.post[:, 2]) - env.theta_threshold) >= ENV_MARGIN)


def _ended_by_state(c, env):
    if c["kind"] == "mountain_car":
        return (env.post[:, 0] >= env.post[:, 4]) & (env.post[:, 1] >= env.goal_velocity)
    return (np.abs(env.post[:, 0]) > env.x_threshold) | (np.abs(env.post[:, 2]) > env.theta_threshold)


def rollout(c, flat, state, n_steps, episode, seed, forced=None):
    """One rollout from (state, n_steps, episode) -> dict: obs (T + 1, E, W) float32, act (T, E), logp (T, E) and value (T + 1, E) float64, rew
    (T, E) float64, done (T, E) bool, terminated (T, E) bool (ended by the state; done without it is a truncation), margin_ok (T, E),
    udist (T + 1, E), state / n_steps / episode afterwards.  forced = (obs ring (T + 1, E, W), actions (T, E)): the policy rows are computed
    on the ring's own observations and the env is stepped on the given actions."""
    E, T = c["E"], c["T"]
    env = make_replay(c)
    env.load(state, n_steps, episode)
    out = {k: [] for k in ("obs", "act", "logp", "value", "rew", "done", "terminated", "margin_ok", "udist")}
    for t in range(T + 1):
        obs = env.state.astype(np.float32)
        out["obs"].append(obs)
        u = philox.uniform(seed, t * E + np.arange(E))
        _, value, act, logp, udist = policy_rows(c, flat, obs if forced is None else forced[0][t], u)
        out["value"].append(value); out["udist"].append(udist)
        if t == T:
            break
        out["act"].append(act); out["logp"].append(logp)
        _, r, d, _ = env.step(np.asarray(act if forced is None else forced[1][t], np.int64))
        out["rew"].append(np.array(r, np.float64)); out["done"].append(np.array(d, bool))
        out["terminated"].append(_ended_by_state(c, env)); out["margin_ok"].append(_env_margin(c, env))
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(state=env.state.copy(), n_steps=env.n_steps.astype(np.int32), episode=env.episode.copy())
    return out


def oracle(name):
    """The case's parameters, initial state and two consecutive oracle rollouts (seeds s, s + 1), computed once and shared: read only."""
    if name not in _cache:
        c = CASES[name]
        flat = params_of(c)
        s0 = initial_state(c)
        r1 = rollout(c, flat, *s0, c["seed"])
        r2 = rollout(c, flat, r1["state"], r1["n_steps"], r1["episode"], c["seed"] + 1)
        for r in (r1, r2):
            for v in r.values():
                v.setflags(write=False)
        flat.setflags(write=False)
        _cache[name] = dict(c=c, flat=flat, s0=s0, rollouts=(r1, r2))
    return _cache[name]


def torch_errors(c, flat, obs, seed=0):
    """Relative L2 error of torch's own float32 CPU evaluation of the network, value and selected log-probability, against float64 on the
    observation rows obs (n, W) -> (value error, logp error).  With fewer than 256 rows the error is measured on POOL_N rows of the same
    distribution instead: the starts of episodes 1 .. of the case's env (policy_inputs' rule: a few numbers do not estimate an error)."""
    obs = np.asarray(obs, np.float32).reshape(-1, WIDTH[c["kind"]])
    if obs.shape[0] < 256:
        k = np.arange(POOL_N)
        obs = fresh(c, k % c["E"], 1 + k // c["E"]).astype(np.float32)
    u = philox.uniform(seed, np.arange(obs.shape[0]))
    lp64, v64, act, logp64, _ = policy_rows(c, flat, obs, u)
    lp32, v32, _, _, _ = policy_rows(c, flat, obs, u, torch.float32)
    logp32 = np.take_along_axis(lp32, act.reshape(-1, 1), axis=1).reshape(-1)
    return PI.rel_l2(v32.astype(np.float64), v64), PI.rel_l2(logp32.astype(np.float64), logp64)


def coverage(c, rollouts):
    """what the two rollouts of a case contain -> dict of counts"""
    done = np.concatenate([r["done"] for r in rollouts]); term = np.concatenate([r["terminated"] for r in rollouts])
    act = np.concatenate([r["act"] for r in rollouts])
    return dict(terminations=int((done & term).sum()), truncations=int((done & ~term).sum()), resets=int(done.sum()),
                actions=sorted(int(a) for a in np.unique(act)), margin_ok=bool(all(r["margin_ok"].all() for r in rollouts)),
                min_udist=float(min(r["udist"].min() for r in rollouts)))


if __name__ == "__main__":      # how the seeds above were chosen: the first sampler seed from 77 on for which a case passes the host checks
    for name, c in CASES.items():
        for seed in range(77, 140):
            c["seed"] = seed
            _cache.pop(name, None)
            cov = coverage(c, oracle(name)["rollouts"])
            if (cov["margin_ok"] and cov["min_udist"] >= U_CLEAR and cov["terminations"] and cov["truncations"]
                    and cov["actions"] == list(range(ACTIONS[c["kind"]]))):
                break
        print(name, "seed", seed, cov)
