"""The float64 CPU oracle of a device-env evaluation (mi_env_evaluate, Engine.env_evaluate) and the cases of the evaluation tests
(tests/test_evaluate_host.py on the CPU, tests/test_gpu_evaluate.py on the GPU).  Nothing here touches a GPU.

An evaluation of K episodes per env is built out of what the rollout tests already have: resident_inputs.policy_rows / head_rows (the MLP
and the heads in float64 from the flat parameter vector), the replay envs (cartpole_inputs.ReplayCartPole,
cartpole_swing_inputs.ReplayCartPoleSwing, mountain_car_inputs.ReplayMountainCar: the host envs' own step arithmetic on the device env's
reset stream) and oracle/philox.py.  From the start of episode F of every env -- or the planted row starts[e, 0] -- it runs K * max_steps
oracle steps with the uniforms of (seed, t * E + e), t the step index since the beginning; each env is cut after its K-th done, returns are
float64 sums in step order, and a planted start replaces the reset stream's state whenever an env begins its next episode.  In greedy
mode the action is the first arg-max of the float64 log-probabilities.

Every case is checked on the CPU first (test_evaluate_host.py), over its evaluated steps only: every env margin holds, no sampler uniform
lies within U_CLEAR of a float64 CDF edge (sampled) or the two largest log-probabilities differ by at least GREEDY_GAP (greedy), every
action value occurs, there is a termination and a truncation, and in the dense-reward cases at least half of the steps have |reward| >=
0.1.  The seeds below were chosen for that, on the CPU, by running this file."""
import numpy as np

import cartpole_swing_inputs as CSI
import resident_inputs as RI
from oracle import philox

ENV_MARGIN = RI.ENV_MARGIN
U_CLEAR = RI.U_CLEAR
GREEDY_GAP = 1e-3             # a thousand times float32's error on these logits
F_DEFAULT = 1 << 40           # Engine.env_evaluate's default first_episode: the counter's high word is in use
MAX_STEPS = 5
# a mountain car that can reach its goal within five steps: the goal lies among the start positions, the push is twenty times the default,
# and the right wall sometimes lies below the goal (rejected start draws: acceptance 0.94)
MC_KW = dict(force=0.02, min_goal_position=-0.55, max_goal_position=-0.2, min_right_boundary=-0.4, max_right_boundary=0.5,
             min_gravity=0.0015, max_gravity=0.0025, sparse_rewards=False)

# name -> kind (the network's: observation width and action count of resident_inputs), env (the replay class), env kwargs beyond
# resident_inputs.ENV_KW, E, K, greedy, depth, width, out, value_from_logits, env seed, sampler seed, starts (None or the name of a
# function below), param_seed (greedy cases).  All: max_steps = 5, parameters 0.2 * default_rng(param_seed or 11).standard_normal.
CASES = {
    "cartpole_sampled": dict(kind="cartpole", env="cartpole", kw={}, E=18, K=3, greedy=False, depth=4, width=64, out=64, lse=0, env_seed=21, seed=77, starts=None),
    "cartpole_greedy": dict(kind="cartpole", env="cartpole", kw={}, E=18, K=3, greedy=True, depth=4, width=64, out=64, lse=0, env_seed=21, seed=77, param_seed=47, starts=None),
    "exact_tile": dict(kind="cartpole", env="cartpole", kw={}, E=16, K=1, greedy=False, depth=4, width=64, out=64, lse=0, env_seed=21, seed=78, starts=None),
    "mountain_car_dense": dict(kind="mountain_car", env="mountain_car", kw=MC_KW, E=18, K=2, greedy=False, depth=4, width=64, out=64, lse=0, env_seed=21, seed=77, starts=None),
    "swing_planted": dict(kind="cartpole", env="cartpole_swing", kw={}, E=18, K=2, greedy=True, depth=4, width=64, out=64, lse=0, env_seed=21, seed=77, param_seed=18, starts="swing_starts"),
    "lse": dict(kind="cartpole", env="cartpole", kw={}, E=18, K=2, greedy=False, depth=4, width=64, out=64, lse=1, env_seed=21, seed=77, starts=None),
    "shallow": dict(kind="cartpole", env="cartpole", kw={}, E=16, K=2, greedy=True, depth=2, width=64, out=64, lse=0, env_seed=21, seed=77, param_seed=29, starts=None),
    "cartpole_starts": dict(kind="cartpole", env="cartpole", kw={}, E=18, K=3, greedy=False, depth=4, width=64, out=64, lse=0, env_seed=21, seed=77, starts="cartpole_starts"),
}
DENSE = ("mountain_car_dense", "swing_planted")
_cache = {}


def env_kwargs(c):
    if c["env"] == "cartpole_swing":
        return dict(CSI.SMALL, **c["kw"])
    return RI.env_kwargs(c)


def make_replay(c):
    if c["env"] == "cartpole_swing":
        return CSI.ReplayCartPoleSwing(c["E"], seed=c["env_seed"], **env_kwargs(c))
    return RI.make_replay(c)


def fresh(c, env, episode):
    """the state episode `episode` of env `env` starts in (the device env's reset stream restated)"""
    if c["env"] == "cartpole_swing":
        rp = make_replay(c)
        return CSI.CI.fresh_state(rp.low, rp.high, c["env_seed"], env, episode)
    return RI.fresh(c, env, episode)


def stream_starts(c, first_episode=F_DEFAULT):
    """(E, K, W): episode i of env e from the reset stream's episode first_episode + i"""
    E, K = c["E"], c["K"]
    e, i = np.meshgrid(np.arange(E), np.arange(K), indexing="ij")
    return fresh(c, e.reshape(-1), first_episode + i.reshape(-1)).reshape(E, K, -1)


def cartpole_starts(c):
    """The reset stream's starts with the two rows of resident_inputs.initial_state planted in every episode of envs 0 and 1: env 0 ends
    at its first step whatever the action (x + tau * x_dot = 0.065 > h_range = 0.06), env 1 cannot end before it is truncated."""
    s = stream_starts(c)
    s[0, :, :4] = (0.055, 0.5, 0.0, 0.0)
    s[1, :, :4] = 0.0
    return s


def swing_starts(c):
    """Near upright: the reset stream's parameter columns, the cart near the middle, theta within +-0.3 of upright, at rest -- rewards
    near 1.  Env 0's first episode is cartpole_swing_inputs.plant's row that leaves the track at its first step whatever the action."""
    s = stream_starts(c)
    rng = np.random.default_rng(18)
    E, K = c["E"], c["K"]
    s[:, :, 0] = rng.uniform(-0.5, 0.5, (E, K))
    s[:, :, 1] = 0.0
    s[:, :, 2] = rng.uniform(-0.3, 0.3, (E, K))
    s[:, :, 3] = 0.0
    s[0, 0, :4] = (CSI.H_RANGE - 0.005, 0.5, 0.05, 0.0)
    return s


def starts_of(c):
    return None if c["starts"] is None else globals()[c["starts"]](c)


def _margin_ok(c, env):
    if c["env"] == "cartpole_swing":
        return np.abs(np.abs(env.post[:, 0]) - env.x_threshold) >= ENV_MARGIN
    return RI._env_margin(c, env)


def _terminated(c, env):
    if c["env"] == "cartpole_swing":
        return np.abs(env.post[:, 0]) > env.x_threshold
    return RI._ended_by_state(c, env)


def evaluate(c, flat, seed=None, first_episode=F_DEFAULT, starts="case", greedy=None):
    """The float64 evaluation -> dict: the records ret (E, K) float64, length, terminated (int32), value0 (float64), start (E, K, W); and per
    evaluated step (flat arrays, one entry per env that was still running): obs (float32 rows), act, rew, margin_ok, udist (sampled) or
    gap (greedy: the distance of the two largest log-probabilities), steps = the loop iterations used."""
    E, K = c["E"], c["K"]
    seed = c["seed"] if seed is None else seed
    greedy = c["greedy"] if greedy is None else greedy
    planted = starts_of(c) if isinstance(starts, str) else starts
    start = stream_starts(c, first_episode) if planted is None else np.array(planted, np.float64)
    env = make_replay(c)
    max_steps = env.max_steps
    env.load(start[:, 0], np.zeros(E, np.int32), np.full(E, first_episode, np.int64))
    rec = dict(ret=np.zeros((E, K)), length=np.zeros((E, K), np.int32), terminated=np.zeros((E, K), np.int32), value0=np.zeros((E, K)), start=start)
    idx, ns, acc = np.zeros(E, np.int64), np.zeros(E, np.int64), np.zeros(E)
    steps = {k: [] for k in ("obs", "act", "rew", "margin_ok", "udist", "gap")}
    n_iter = 0
    for t in range(K * max_steps):
        run = idx < K
        if not run.any():
            break
        n_iter += 1
        obs = env.state.astype(np.float32)
        u = philox.uniform(seed, t * E + np.arange(E))
        lp, value, act, _, udist = RI.policy_rows(c, flat, obs, u)
        top = np.sort(lp, axis=1)
        if greedy:
            act = np.argmax(lp, axis=1)                      # (numpy's argmax: the first maximum)
        first = run & (ns == 0)
        rec["value0"][first, idx[first]] = value[first]
        _, r, d, _ = env.step(np.asarray(act, np.int64))
        r, d = np.array(r, np.float64) * np.ones(E), np.array(d, bool)
        term, ok = _terminated(c, env), _margin_ok(c, env)
        steps["obs"].append(obs[run]); steps["act"].append(np.asarray(act)[run]); steps["rew"].append(r[run]); steps["margin_ok"].append(ok[run])
        steps["udist"].append(udist[run]); steps["gap"].append((top[:, -1] - top[:, -2])[run])
        acc[run] += r[run]
        ns[run] += 1
        for e in np.nonzero(run & d)[0]:
            rec["ret"][e, idx[e]], rec["length"][e, idx[e]], rec["terminated"][e, idx[e]] = acc[e], ns[e], int(term[e])
            idx[e] += 1
            acc[e], ns[e] = 0.0, 0
            if idx[e] < K and planted is not None:
                env.state[e] = start[e, idx[e]]              # the planted row replaces the reset stream's state
    assert (idx >= K).all()                                  # (an episode has at most max_steps steps)
    out = {k: np.concatenate(v) for k, v in steps.items()}
    out.update(rec, steps=n_iter)
    return out


def params_of(c):
    """resident_inputs' parameters; a greedy case names the generator's seed (param_seed): both actions must be some row's arg-max"""
    return RI.params_of(c, c.get("param_seed", 11))


def oracle(name):
    """The case's parameters, planted starts (or None) and oracle evaluation, computed once and shared: read only."""
    if name not in _cache:
        c = CASES[name]
        flat = params_of(c)
        starts = starts_of(c)
        ev = evaluate(c, flat, starts=starts)
        for v in list(ev.values()) + [flat] + ([] if starts is None else [starts]):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = dict(c=c, flat=flat, starts=starts, ev=ev, max_steps=make_replay(c).max_steps)
    return _cache[name]


def coverage(name, ev):
    """what a case's evaluation contains -> dict"""
    c = CASES[name]
    return dict(terminations=int(ev["terminated"].sum()), truncations=int((ev["terminated"] == 0).sum()),
                actions=sorted(int(a) for a in np.unique(ev["act"])), margin_ok=bool(ev["margin_ok"].all()),
                min_udist=float(ev["udist"].min()), min_gap=float(ev["gap"].min()), dense_share=float((np.abs(ev["rew"]) >= 0.1).mean()),
                steps=int(ev["steps"]), env_steps=int(ev["length"].sum()), greedy=c["greedy"])


def covered(name, cov):
    c = CASES[name]
    clear = cov["min_gap"] >= GREEDY_GAP if c["greedy"] else cov["min_udist"] >= U_CLEAR
    return bool(cov["margin_ok"] and clear and cov["terminations"] and cov["truncations"] and cov["actions"] == list(range(RI.ACTIONS[c["kind"]]))
                and (name not in DENSE or cov["dense_share"] >= 0.5))


if __name__ == "__main__":      # how the seeds above were chosen: the first seed from 77 on for which a case passes the host checks
    for name, c in CASES.items():      # (the sampler seed in sampled mode; a greedy case draws no uniforms: the seed of its parameters moves instead)
        for seed in range(77, 140) if not c["greedy"] else range(11, 74):
            c["param_seed" if c["greedy"] else "seed"] = seed
            _cache.pop(name, None)
            cov = coverage(name, oracle(name)["ev"])
            if covered(name, cov):
                break
        print(name, "param_seed" if c["greedy"] else "seed", seed, cov)
