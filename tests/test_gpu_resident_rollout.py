"""The one-launch rollout of the device-resident envs (csrc/env_resident.hip, mi_env_rollout_resident, Engine.env_rollout(resident=True),
PPO(resident_rollout=True), train.py --resident_rollout) against the float64 CPU rollout oracle of tests/resident_inputs.py, beside the
chain of launches it replaces (mi_env_rollout), and through the agent and the command line.

The oracle's cases are checked on the CPU in tests/test_resident_rollout_host.py: every replay margin holds and no sampler uniform is within
1e-4 of a float64 CDF edge, so the device's actions are expected to BE the oracle's.  Should one differ all the same, the comparison falls
back to the stepwise rule: the policy rows on the ring's own observations, the env replayed on the ring's own actions, rows whose uniform is
within 1e-5 of a float64 CDF edge left out, at most 1 % of them.

value / logp: relative L2 error against float64 <= 8 x the error of torch's own float32 CPU evaluation of the same network on the same
observations against float64 (policy_inputs.check_measured: the bound comes from torch, never from the kernel).  The measured ratios are
printed and on record in profiles/resident_rollout.md."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import policy_inputs as PI
import resident_inputs as RI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "train-procgen-pytorch_amd")


def _engine(c, T=None, E=None, **kw):
    from mi355.engine import Engine
    E = E or c["E"]
    return Engine("mlp", T or c["T"], E, RI.ACTIONS[c["kind"]], E, obs_dim=RI.WIDTH[c["kind"]], mlp_depth=c["depth"], mlp_width=c["width"],
                  out_dim=c["out"], value_from_logits=bool(c["lse"]), **kw)


def _device_env(c, eng):
    from common.env.vec_envs import DeviceCartPole, DeviceMountainCar
    cls = DeviceCartPole if c["kind"] == "cartpole" else DeviceMountainCar
    env = cls(eng.E, seed=c["env_seed"], **RI.env_kwargs(c))
    env.attach_engine(eng)
    return env


def _read(eng):
    from mi355.engine import F_ACT, F_ADV, F_DONE, F_LOGP, F_RET, F_REW, F_VALUE
    r = dict(rew=eng.read_field(F_REW), done=eng.read_field(F_DONE), logp=eng.read_field(F_LOGP), value=eng.read_field(F_VALUE),
             act=eng.read_field(F_ACT).astype(np.int64), adv=eng.read_field(F_ADV), ret=eng.read_field(F_RET),
             obs=np.stack([eng.get_obs(t) for t in range(eng.T + 1)]))
    r["state"], r["n_steps"], r["episode"] = eng.env_state()
    return r


def _check(name, k, c, flat, got, start, want, seed):
    """one device rollout `got` against the oracle's `want` (or, if an action differs, against the stepwise rule) -> the measured ratios"""
    T, A = c["T"], RI.ACTIONS[c["kind"]]
    what = f"{name} rollout {k + 1}"
    keep_t = np.ones(want["udist"].shape, bool)
    if not np.array_equal(got["act"], want["act"]):
        print(f"{what}: {int((got['act'] != want['act']).sum())} device actions differ from the oracle's: stepwise comparison on the ring's own rows")
        want = RI.rollout(c, flat, *start, seed, forced=(got["obs"], got["act"]))
        edge = want["udist"] < PI.U_MARGIN
        PI.check_cap(edge[:T], what)
        PI.check_actions(got["act"].reshape(-1), want["act"].reshape(-1), edge[:T].reshape(-1), A, what)
        keep_t = ~edge
    else:
        assert want["margin_ok"].all()
    assert want["margin_ok"].all(), f"{what}: a replay margin does not hold on the device's own actions"
    assert np.array_equal(got["done"], want["done"].astype(np.float32)), what
    if c["kind"] == "mountain_car" and not RI.env_kwargs(c).get("sparse_rewards", True):
        r32 = want["rew"].astype(np.float32)
        ulps = np.abs(got["rew"].astype(np.float64) - r32) / np.spacing(np.abs(r32))
        print(f"{what}: dense reward, max float32 ulps from the replay: {ulps.max()}")
        assert RI.MI.within_ulp(got["rew"], r32, 1).all(), what
    else:
        assert np.array_equal(got["rew"], want["rew"].astype(np.float32)), what
    w32 = want["obs"]
    assert (np.abs(got["obs"] - w32) <= 1e-6 * np.abs(w32)).all(), (what, np.abs(got["obs"] - w32).max())
    assert np.array_equal(got["obs"][T], got["state"].astype(np.float32)), what                  # slot T is float32(state)
    # the env's own arithmetic (fp64 sin / cos) differs from numpy's in the last digits at most: the observations' rule on the state
    assert (np.abs(got["state"] - want["state"]) <= 1e-6 * np.abs(want["state"])).all(), what
    assert np.array_equal(got["n_steps"], want["n_steps"]) and np.array_equal(got["episode"], want["episode"]), what
    terr_v, terr_lp = RI.torch_errors(c, flat, want["obs"] if keep_t.all() else got["obs"])
    ev, _ = PI.check_measured(got["value"][keep_t], want["value"][keep_t], terr_v, what=what + " value")
    el, _ = PI.check_measured(got["logp"][keep_t[:T]], want["logp"][keep_t[:T]], terr_lp, what=what + " logp")
    print(f"{what}: value error {ev:.3e} = {ev / terr_v:.2f} x torch float32's {terr_v:.3e}; logp error {el:.3e} = {el / terr_lp:.2f} x torch float32's "
          f"{terr_lp:.3e} (bound: 8 x)")
    return ev / terr_v, el / terr_lp


def _two_rollouts(name):
    o = RI.oracle(name)
    c, flat = o["c"], o["flat"]
    eng = _engine(c)
    eng.set_params(flat)
    _device_env(c, eng).reset()
    eng.env_set_state(*o["s0"])                     # (reset() left episode 1 of every env; the planted rows and exactly the oracle's bits)
    got = []
    for k in range(2):
        eng.env_rollout(c["seed"] + k, resident=True)
        got.append(_read(eng))
    eng.close()
    assert np.array_equal(got[1]["obs"][0], got[0]["obs"][c["T"]])                                # slot 0 of rollout 2 is slot T of rollout 1
    start = o["s0"]
    for k in range(2):
        _check(name, k, c, flat, got[k], start, o["rollouts"][k], c["seed"] + k)
        start = (got[k]["state"], got[k]["n_steps"], got[k]["episode"])
    return got


# ------------------------------------------------------------------------------------------ 1: against the oracle, E = 70, T = 8
@pytest.mark.parametrize("name", RI.TEST1)
def test_two_resident_rollouts_match_the_float64_oracle(name):
    """E = 70 (four full 16-env tiles and a 6-row tail), T = 8, max_steps = 5, MLP 4 x 64 -> 64: terminations, truncations, resets (the mountain
    car's validation ranges: rejected start draws) and every action inside one launch; two launches in a row."""
    got = _two_rollouts(name)
    assert got[0]["done"][0, 0] == 1 and got[0]["done"][4, 1] == 1 and not got[0]["done"][:4, 1].any()      # the planted rows


# ------------------------------------------------------------------------------------------ 2: widths and depths
@pytest.mark.parametrize("name", RI.TEST2)
def test_widths_depths_and_the_logsumexp_value(name):
    """wide: E = 18 (a tile and a 2-row tail), depth 4, width 256, out 64 -- the shipped sets' network: the K = 256 loops and the N = 64 last
    layer; shallow: depth 2, E = 16 (exactly one tile); lse: value_from_logits."""
    _two_rollouts(name)


# ------------------------------------------------------------------------------------------ 3: beside the chain
@pytest.mark.parametrize("name", ("cartpole", "mountain_car_dense", "wide"))
def test_resident_rollout_beside_the_chain(name):
    """From one saved state: mi_env_rollout, then mi_env_rollout_resident.  Same actions, rewards, dones, observations and env state
    (the env arithmetic is the same code); value / logp within twice test 1's bound of each other; adv / ret untouched by either."""
    from mi355.engine import F_ADV, F_RET
    o = RI.oracle(name)
    c, flat = o["c"], o["flat"]
    T, E = c["T"], c["E"]
    eng = _engine(c)
    eng.set_params(flat)
    _device_env(c, eng).reset()
    rng = np.random.default_rng(5)
    adv, ret = rng.standard_normal((T, E)).astype(np.float32), rng.standard_normal((T, E)).astype(np.float32)
    eng.write_field(F_ADV, adv); eng.write_field(F_RET, ret)
    eng.env_set_state(*o["s0"])
    eng.env_rollout(c["seed"])
    chain = _read(eng)
    eng.env_set_state(*o["s0"])
    eng.env_rollout(c["seed"], resident=True)
    res = _read(eng)
    eng.close()
    for k in ("act", "rew", "done", "obs", "state", "n_steps", "episode"):
        assert np.array_equal(chain[k], res[k]), k
    for r in (chain, res):
        assert np.array_equal(r["adv"], adv) and np.array_equal(r["ret"], ret)
    terr_v, terr_lp = RI.torch_errors(c, flat, res["obs"])
    dv, dl = PI.rel_l2(res["value"].astype(np.float64), chain["value"].astype(np.float64)), PI.rel_l2(res["logp"].astype(np.float64), chain["logp"].astype(np.float64))
    print(f"{name}: resident against the chain: value {dv:.3e} = {dv / terr_v:.2f} x torch float32's error, logp {dl:.3e} = {dl / terr_lp:.2f} x (bound: 16 x)")
    assert dv <= 16 * terr_v and dl <= 16 * terr_lp


# ------------------------------------------------------------------------------------------ 4: refusals by name
def test_refusals_by_name_leave_the_rings_alone():
    from mi355.engine import Engine, EngineError, F_ACT, F_DONE, F_LOGP, F_REW, F_VALUE
    from common.env.vec_envs import DeviceCartPole
    T, E = 2, 4
    rng = np.random.default_rng(9)

    def sentinel(eng, W=9):
        s = dict(obs=rng.standard_normal((T + 1, E, W)).astype(np.float32), rew=rng.standard_normal((T, E)).astype(np.float32),
                 done=rng.standard_normal((T, E)).astype(np.float32), logp=rng.standard_normal((T, E)).astype(np.float32),
                 value=rng.standard_normal((T + 1, E)).astype(np.float32), act=rng.integers(0, 2, (T, E)))
        for t in range(T + 1):
            eng.put_obs(t, s["obs"][t])
        for f, k in ((F_REW, "rew"), (F_DONE, "done"), (F_LOGP, "logp"), (F_VALUE, "value")):
            eng.write_field(f, s[k])
        for t in range(T):
            eng.put_policy_outputs(t, act=s["act"][t])
        return s

    def untouched(eng, s):
        for f, k in ((F_REW, "rew"), (F_DONE, "done"), (F_LOGP, "logp"), (F_VALUE, "value")):
            assert np.array_equal(eng.read_field(f), s[k]), k
        assert np.array_equal(eng.read_field(F_ACT).astype(np.int64), s["act"])
        assert np.array_equal(np.stack([eng.get_obs(t) for t in range(T + 1)]), s["obs"])

    mk = lambda **kw: Engine("mlp", T, E, 2, E, obs_dim=9, **dict(dict(mlp_depth=4, mlp_width=64, out_dim=64), **kw))
    # no env on the context
    eng = mk()
    s = sentinel(eng)
    with pytest.raises(EngineError, match="no env"):
        eng.env_rollout(1, resident=True)
    untouched(eng, s)
    # a context that got a GRU after its env
    DeviceCartPole(E, seed=1).attach_engine(eng)
    H = 64
    eng.set_gru(*(0.1 * rng.standard_normal(n).astype(np.float32) for n in (3 * H * H, 3 * H * H, 3 * H, 3 * H)))
    s = sentinel(eng)
    with pytest.raises(EngineError, match="mi_env_rollout_resident: a recurrent context"):
        eng.env_rollout(1, resident=True)
    untouched(eng, s)
    eng.close()
    # shapes outside the list
    for kw, msg in ((dict(mlp_width=72), "mi_env_rollout_resident: mlp_width must be a multiple of 16 and at most 512"),
                    (dict(mlp_width=528), "mi_env_rollout_resident: mlp_width must be a multiple of 16 and at most 512"),
                    (dict(out_dim=40), "mi_env_rollout_resident: out_dim must be a multiple of 16 and at most 512"),
                    (dict(mlp_depth=17), "mi_env_rollout_resident: mlp_depth must be at least 2 and at most 16")):
        eng = mk(**kw)
        DeviceCartPole(E, seed=1).attach_engine(eng)
        eng.env_reset()
        s = sentinel(eng)
        with pytest.raises(EngineError, match=msg):
            eng.env_rollout(1, resident=True)
        untouched(eng, s)
        eng.env_rollout(1)                                   # the chain takes these shapes
        eng.sync()
        eng.close()


# ------------------------------------------------------------------------------------------ 5: agent and command line
def test_ppo_trains_with_the_resident_rollout():
    """PPO(resident_rollout=True) on DeviceCartPole with a validation env, two iterations at T = E = 8: every rollout of either lane goes
    through mi_env_rollout_resident, the storage's mirrors are the device rings, the losses are finite."""
    from agents.ppo import PPO
    from common.env.vec_envs import DeviceCartPole
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    from mi355.engine import F_DONE, F_REW
    T, E = 8, 8
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    kw = RI.ENV_KW["cartpole"]
    env, env_v = DeviceCartPole(E, seed=4, **kw), DeviceCartPole(E, seed=5, **kw)
    policy = CategoricalPolicy(MLPModel(9, 4, 64, 64), False, 2)
    logger = Logger(E, None)
    agent = PPO(env, policy, logger, Storage((9,), 64, T, E, dev), dev, 1, env_valid=env_v, storage_valid=Storage((9,), 64, T, E, dev), n_steps=T,
                n_envs=E, epoch=2, n_minibatch=2, mini_batch_size=32, gamma=0.99, lmbda=0.95, learning_rate=1e-3, entropy_coef=0.01, seed=0,
                detect_nan=True, resident_rollout=True)
    assert agent.resident_rollout is True
    calls = []
    for eng in (agent.engine, agent.engine_valid):
        real = eng.env_rollout
        eng.env_rollout = lambda seed=0, resident=False, real=real, eng=eng: calls.append((eng, resident)) or real(seed, resident=resident)
    agent.train(2 * T * E)
    assert calls == [(agent.engine, True), (agent.engine_valid, True)] * 2
    for st, eng in ((agent.storage, agent.engine), (agent.storage_valid, agent.engine_valid)):
        rew, done = eng.read_field(F_REW), eng.read_field(F_DONE)
        assert np.array_equal(st._rew, rew) and np.array_equal(st._done, done)
        assert (rew == 1).all() and done.any() and set(np.unique(done)) <= {0.0, 1.0}
        obs = st.obs_batch.numpy()
        assert np.isfinite(obs).all() and (np.abs(obs[..., 0]) <= 0.06 + 0.05).all()      # x never far beyond h_range: the env really steps
    assert len(logger.rows) == 2
    for name in ("loss_total", "loss_pi", "loss_v", "loss_entropy"):
        assert np.isfinite([row[logger.columns.index(name)] for row in logger.rows]).all(), name
    agent.engine.close(); agent.engine_valid.close()


def test_train_cli_runs_the_mountain_car_with_the_resident_rollout(tmp_path):
    """`python train.py --env_name mountain_car --param_name mountain_car --device_env --resident_rollout` in a fresh child process: two
    iterations with the validation env, log rows and a checkpoint."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "--exp_name", "dev", "--env_name", "mountain_car", "--param_name", "mountain_car",
           "--n_envs", "8", "--n_steps", "16", "--mini_batch_size", "32", "--seed", "3", "--detect_nan", "--num_timesteps", "250",
           "--num_checkpoints", "1", "--device_env", "--resident_rollout"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "rollout: device-resident env, one kernel launch per rollout" in r.stdout
    runs = os.listdir(tmp_path / "logs" / "train" / "mountain_car" / "dev")
    assert len(runs) == 1 and runs[0].endswith("__seed_3")
    rd = tmp_path / "logs" / "train" / "mountain_car" / "dev" / runs[0]
    assert {"hyperparameters.npy", "config.npy", "log-append.csv", "model_256.pth"} <= set(os.listdir(rd))
    assert np.load(rd / "hyperparameters.npy", allow_pickle=True).item()["resident_rollout"] is True
    rows = open(rd / "log-append.csv").read().strip().splitlines()
    assert len(rows) == 3 and [float(row.split(",")[0]) for row in rows[1:]] == [128.0, 256.0]
