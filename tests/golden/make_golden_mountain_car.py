#!/usr/bin/env python3
"""Generate G17 (tests/golden/g17_mountain_car.npz): trajectories of the reference's own pre-vectorised mountain car
(discrete_env/mountain_car_pre_vec.py MountainCarVecEnv / create_mountain_car) on the CPU.

    python tests/golden/make_golden_mountain_car.py <path of the reference checkout>

The reference class needs gymnasium and the reference's helper_local (which imports far more); neither is needed for what runs here,
so this file registers stand-in modules with the handful of names the class touches -- gymnasium.Env, spaces.Box / spaces.Discrete,
error.DependencyNotInstalled, utils.seeding.np_random (what gymnasium's does for an int seed: numpy's default_rng(seed)) and
helper_local.DictToArgs -- and then imports the reference's module from the given path.  Data only; no test runs this file.

Keys
  a_train/ a_valid/  (a) create_mountain_car(args(seed = A_SEED), {"n_envs": 6, "max_steps": 5}, is_valid) -> reset() -> 40 steps on the
                     fixed actions `act` (40, 6): obs0 (6, 5), obs (40, 6, 5), rew (40, 6), done (40, 6).  The validation ranges reject
                     about 21 % of the start draws; asserted here: at least one reset of the validation run kept a row that an
                     unconditioned draw would not have put there.
  b/                 (b) one teacher-forced step at E = 70 (a full wave + a 6-row tail), goal_velocity = 0.01, max_steps = 37, validation
                     ranges, seed B_SEED: inputs state (70, 5), n_steps (70,), act (70,), kw (json); outputs out_state, rew, done.
  c/                 (c) the same step with sparse_rewards = False: out_state, rew, done.
Rows of (b): 0-49, 64-69 random interior rows (actions 0, 1, 2 in rows 0-2, random after); 50 / 51 land 1e-6 inside / outside
goal_position; 52 lands beyond the goal with velocity < goal_velocity, 53 the same with velocity above; 54, 55 hit left_boundary with
negative velocity; 56 is clipped at right_boundary == goal_position (ends), 57 is clipped at right_boundary below goal_velocity (goes
on); 58 / 59 are clipped at +max_speed / -max_speed; 60, 61 are one step short of max_steps (truncated), 62, 63 two steps short.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g17_mountain_car.npz")
A_SEED, B_SEED, B_E, B_MAX_STEPS = 17, 1717, 70, 37
VALID = dict(min_right_boundary=1., max_right_boundary=5., min_goal_position=0.6, max_goal_position=3, min_gravity=0.0015, max_gravity=0.0025)
B_KW = dict(goal_velocity=0.01, left_boundary=-1.2, max_speed=0.07, force=0.001, max_steps=B_MAX_STEPS, **VALID)


def install_stand_ins():
    class Env:
        pass

    class Box:
        def __init__(self, low, high, dtype=np.float32):
            self.low, self.high, self.dtype, self.shape = low, high, dtype, np.shape(low)

    class Discrete:
        def __init__(self, n):
            self.n = n

    class DependencyNotInstalled(Exception):
        pass

    class DictToArgs:
        def __init__(self, d):
            self.__dict__.update(d)

    def mod(name, **names):
        m = types.ModuleType(name)
        m.__dict__.update(names)
        sys.modules[name] = m
        return m

    spaces = mod("gymnasium.spaces", Box=Box, Discrete=Discrete)
    error = mod("gymnasium.error", DependencyNotInstalled=DependencyNotInstalled)
    seeding = mod("gymnasium.utils.seeding", np_random=lambda seed: (np.random.default_rng(seed), seed))
    utils = mod("gymnasium.utils", seeding=seeding)
    mod("gymnasium", Env=Env, spaces=spaces, error=error, utils=utils)
    mod("helper_local", DictToArgs=DictToArgs)
    return DictToArgs


def watch_rejections(env, n):
    """Count the resets whose kept rows differ from the first n rows of the unconditioned block (a rejected row came before the n-th
    accepted one).  The start space's condition is called once per block with the whole block."""
    cond, hits = env.start_space.condition, []

    def seen(x):
        r = cond(x)
        keep = np.nonzero(r == False)[0]      # noqa: E712
        hits.append(len(keep) >= n and keep[n - 1] != n - 1)
        return r
    env.start_space.condition = seen
    return hits


def case_a(ref, DictToArgs, is_valid):
    env = ref.create_mountain_car(DictToArgs({"render": False, "seed": A_SEED}), {"n_envs": 6, "max_steps": 5}, is_valid)
    hits = watch_rejections(env, 6)
    act = np.random.default_rng(A_SEED + 1 + is_valid).integers(0, 3, (40, 6))
    obs0 = np.array(env.reset(), np.float64)
    obs, rew, done = [], [], []
    for a in act:
        o, r, d, _ = env.step(a)
        obs.append(np.array(o, np.float64)); rew.append(np.array(r, np.float64)); done.append(np.array(d, bool))
    done = np.stack(done)
    assert done.sum() == 8 * 6                         # every env is truncated after each 5 steps; nobody reaches a goal in 5
    if is_valid:
        assert any(hits), "no reset of the validation run met a rejected row"
    else:
        assert not any(hits)
    return dict(obs0=obs0, act=act.astype(np.int64), obs=np.stack(obs), rew=np.stack(rew), done=done)


def one_step_inputs():
    rng = np.random.default_rng(B_SEED)
    E, kw = B_E, B_KW
    state = np.zeros((E, 5))
    state[:, 0] = rng.uniform(-1.0, 0.4, E)
    state[:, 1] = rng.uniform(-0.05, 0.05, E)
    state[:, 2] = rng.uniform(kw["min_gravity"], kw["max_gravity"], E)
    state[:, 3] = rng.uniform(kw["min_right_boundary"], kw["max_right_boundary"], E)
    state[:, 4] = np.minimum(rng.uniform(kw["min_goal_position"], kw["max_goal_position"], E), state[:, 3])
    act = rng.integers(0, 3, E)
    act[:3] = (0, 1, 2)

    def start_for(target, v, g, a):
        """position p with p + v'(p) = target, v'(p) = v + (a - 1) * force + cos(3 p) * (-g): a contraction with factor 3 g."""
        p = target - v
        for _ in range(60):
            p = target - (v + ((a - 1) * kw["force"] + np.cos(3 * p) * (-g)))
        return p
    g, d = 0.002, 1e-6
    for row, (target, v, a, rb, gp) in {50: (0.9 - d, 0.05, 1, 2.0, 0.9), 51: (0.9 + d, 0.05, 1, 2.0, 0.9),
                                        52: (0.9 + 1e-3, 0.005, 1, 2.0, 0.9), 53: (0.9 + 1e-3, 0.03, 1, 2.0, 0.9)}.items():
        state[row] = (start_for(target, v, g, a), v, g, rb, gp)
        act[row] = a
    state[54] = (-1.19, -0.05, g, 2.0, 0.9); act[54] = 0
    state[55] = (-1.19, -0.05, g, 2.0, 0.9); act[55] = 2
    state[56] = (0.98, 0.06, g, 1.0, 1.0); act[56] = 1
    state[57] = (1.0 - 1e-3, 0.006, g, 1.0, 0.8); act[57] = 1
    state[58] = (-0.9, 0.069, g, 2.0, 0.9); act[58] = 2
    state[59] = (0.1, -0.069, g, 2.0, 0.9); act[59] = 0
    n_steps = rng.integers(0, B_MAX_STEPS - 2, E).astype(np.int32)
    n_steps[60:62] = B_MAX_STEPS - 1
    n_steps[62:64] = B_MAX_STEPS - 2
    return state, n_steps, act.astype(np.int64)


def one_step(ref, state, n_steps, act, **extra):
    env = ref.MountainCarVecEnv(n_envs=B_E, seed=B_SEED, **B_KW, **extra)
    env.state = state.copy()                           # (the reference's step updates the velocity column in place)
    env.n_steps = n_steps.astype(np.float64)
    env.terminated = np.full(B_E, False)
    o, r, d, _ = env.step(act)
    return dict(out_state=np.array(o, np.float64), rew=np.array(r, np.float64), done=np.array(d, bool))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    DictToArgs = install_stand_ins()
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import discrete_env.mountain_car_pre_vec as ref
    out = {}
    for name, is_valid in (("a_train", False), ("a_valid", True)):
        out.update({f"{name}/{k}": v for k, v in case_a(ref, DictToArgs, is_valid).items()})
    state, n_steps, act = one_step_inputs()
    b, c = one_step(ref, state, n_steps, act), one_step(ref, state, n_steps, act, sparse_rewards=False)
    assert set(np.nonzero(b["done"])[0]) == {51, 53, 56, 60, 61} and np.array_equal(b["done"], c["done"])
    assert (b["rew"] == -1).all() and (c["rew"] != -1).all()
    assert b["out_state"][57, 0] == 1.0 and (b["out_state"][54:56, :2] == (-1.2, 0.0)).all()
    assert b["out_state"][58, 1] == 0.07 and b["out_state"][59, 1] == -0.07
    out.update({"b/state": state, "b/n_steps": n_steps, "b/act": act, "b/kw": np.frombuffer(json.dumps(B_KW).encode(), np.uint8)})
    out.update({f"b/{k}": v for k, v in b.items()})
    out.update({f"c/{k}": v for k, v in c.items()})
    out["seeds"] = np.array([A_SEED, B_SEED], np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
