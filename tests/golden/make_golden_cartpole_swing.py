#!/usr/bin/env python3
"""Generate G18 (tests/golden/g18_cartpole_swing.npz): trajectories of the reference's own pre-vectorised swing-up cart-pole
(discrete_env/cartpole_swing_pre_vec.py CartPoleSwingVecEnv / create_cartpole_swing) and one step of its balance class
(discrete_env/cartpole_pre_vec.py CartPoleVecEnv) on the CPU.

    python tests/golden/make_golden_cartpole_swing.py <path of the reference checkout>

The stand-in modules are those of make_golden_mountain_car.py (install_stand_ins, imported); the stand-in Env additionally gets the class
attribute `_np_random = None`, as gymnasium's Env has: the swing-up constructor reads it before PreVecEnv sets it.  Data only; no test
runs this file.

Keys
  a_train/ a_valid/  (a) create_cartpole_swing(args(seed = A_SEED), {"n_envs": 6, "max_steps": 5}, is_valid) -> reset() -> 40 steps on the
                     fixed actions `act` (40, 6): obs0 (6, 9), obs (40, 6, 9), rew (40, 6), done (40, 6).
  b/                 (b) one teacher-forced step at E = 70 (a full wave + a 6-row tail), max_steps = 37, validation ranges, seed B_SEED:
                     inputs state (70, 9), n_steps (70,), act (70,), kw (json); outputs out_state, rew, done.
  c/                 (c) the BALANCE class, one teacher-forced step at E = 70 on the states of tests/cartpole_inputs.one_step_case():
                     out_state, done.
Rows of (b): 0-49, 64-69 random interior rows (|x| <= 2.3, theta uniform in +-12 -- several turns, nothing wraps --, |theta_dot| <= 8,
which keeps the accelerations below 1e2; actions 0, 1 in rows 0, 1, random after); 50 / 51 land 1e-6 inside / outside +h_range, 52 / 53
the same at -h_range (x_dot = +-0.5); 54 / 55 land 1e-6 below / above +pi/2 (the reward clamp off / on), 56 / 57 1e-6 above / below
-pi/2 (off / on), theta_dot = 0.25; 58, 59 hold theta = 0.3, -0.3 at rest (beyond 12 degrees: they go on); 60, 61 are one step short of
max_steps (truncated), 62, 63 two steps short.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT, os.path.join(ROOT, "train-procgen-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from make_golden_mountain_car import install_stand_ins      # noqa: E402

OUT = os.path.join(HERE, "g18_cartpole_swing.npz")
A_SEED, B_SEED, B_E, B_MAX_STEPS = 17, 1818, 70, 37
H_RANGE, TAU = 2.4, 0.02
VALID = dict(min_gravity=10.4, max_gravity=24.8, min_pole_length=1.0, max_pole_length=2.0, min_cart_mass=2., max_cart_mass=3.,
             min_pole_mass=.2, max_pole_mass=.4, min_force_mag=10., max_force_mag=10.)
B_KW = dict(h_range=H_RANGE, max_steps=B_MAX_STEPS, **VALID)
B_ENDED = {51, 53, 60, 61}


def case_a(ref, DictToArgs, is_valid):
    env = ref.create_cartpole_swing(DictToArgs({"render": False, "seed": A_SEED}), {"n_envs": 6, "max_steps": 5}, is_valid)
    act = np.random.default_rng(A_SEED + 1 + is_valid).integers(0, 2, (40, 6))
    obs0 = np.array(env.reset(), np.float64)
    obs, rew, done = [], [], []
    for a in act:
        o, r, d, _ = env.step(a)
        obs.append(np.array(o, np.float64)); rew.append(np.array(r, np.float64)); done.append(np.array(d, bool))
    done = np.stack(done)
    assert done.sum() == 8 * 6                         # every env is truncated after each 5 steps; nobody leaves +-2.4 in 5
    return dict(obs0=obs0, act=act.astype(np.int64), obs=np.stack(obs), rew=np.stack(rew), done=done)


def one_step_inputs():
    rng = np.random.default_rng(B_SEED)
    E, kw = B_E, B_KW
    state = np.zeros((E, 9))
    state[:, 0] = rng.uniform(-2.3, 2.3, E)
    state[:, 1] = rng.uniform(-1.0, 1.0, E)
    state[:, 2] = rng.uniform(-12.0, 12.0, E)
    state[:, 3] = rng.uniform(-8.0, 8.0, E)
    for j, name in enumerate(("gravity", "pole_length", "cart_mass", "pole_mass", "force_mag")):
        state[:, 4 + j] = rng.uniform(kw["min_" + name], kw["max_" + name], E)
    act = rng.integers(0, 2, E)
    act[:2] = (0, 1)
    d = 1e-6
    for k, (col, thr, rate) in enumerate(((0, H_RANGE, 0.5), (0, -H_RANGE, -0.5), (2, np.pi / 2, 0.25), (2, -np.pi / 2, 0.25))):
        for j, inside in enumerate((True, False)):
            r = 50 + 2 * k + j
            state[r, :4] = 0.01
            state[r, col + 1] = rate
            target = thr - np.sign(thr) * d if inside else thr + np.sign(thr) * d
            state[r, col] = target - TAU * rate
    state[58, :4] = (0.0, 0.0, 0.3, 0.0)
    state[59, :4] = (0.0, 0.0, -0.3, 0.0)
    n_steps = rng.integers(0, B_MAX_STEPS - 2, E).astype(np.int32)
    n_steps[60:62] = B_MAX_STEPS - 1
    n_steps[62:64] = B_MAX_STEPS - 2
    return state, n_steps, act.astype(np.int64)


def teacher_forced(env, state, n_steps, act):
    env.state = state.copy()
    env.n_steps = n_steps.astype(np.float64)
    env.terminated = np.full(len(state), False)
    o, r, d, _ = env.step(act)
    return dict(out_state=np.array(o, np.float64), rew=np.array(r, np.float64), done=np.array(d, bool))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import cartpole_inputs as CI                       # (before the reference's path goes first: its `common` package would shadow ours)
    DictToArgs = install_stand_ins()
    sys.modules["gymnasium"].Env._np_random = None
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import discrete_env.cartpole_swing_pre_vec as ref
    import discrete_env.cartpole_pre_vec as ref_balance
    out = {}
    for name, is_valid in (("a_train", False), ("a_valid", True)):
        out.update({f"{name}/{k}": v for k, v in case_a(ref, DictToArgs, is_valid).items()})
    state, n_steps, act = one_step_inputs()
    b = teacher_forced(ref.CartPoleSwingVecEnv(n_envs=B_E, seed=B_SEED, **B_KW), state, n_steps, act)
    assert set(np.nonzero(b["done"])[0]) == B_ENDED and not b["done"][58:60].any()
    assert (b["rew"] > 0).sum() >= 20 and (b["rew"] == 0).sum() >= 20
    assert b["rew"][55] == 0 and 0 < b["rew"][54] < 2e-6 and b["rew"][57] == 0 and 0 < b["rew"][56] < 2e-6
    out.update({"b/state": state, "b/n_steps": n_steps, "b/act": act, "b/kw": np.frombuffer(json.dumps(B_KW).encode(), np.uint8)})
    out.update({f"b/{k}": v for k, v in b.items()})
    c = CI.one_step_case()
    bal = teacher_forced(ref_balance.CartPoleVecEnv(n_envs=CI.ONE_STEP_E, seed=B_SEED, **c["kw"]), c["state"], c["n_steps"], c["act"])
    out.update({"c/out_state": bal["out_state"], "c/done": bal["done"]})
    out["seeds"] = np.array([A_SEED, B_SEED], np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
