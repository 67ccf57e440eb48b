"""The device-resident mountain car (csrc/env_device.hip, mi_env_* in include/mi355ppo.h, common/env/vec_envs.py DeviceMountainCar,
train.py --device_env) against the reference's own class through the fixture tests/golden/g17_mountain_car.npz, and against a CPU replay
that drives MountainCarVec.step with the numpy restatement of the device env's Philox reset stream (tests/mountain_car_inputs.py).

Every comparison of a done flag is preceded by a CPU check on every compared row (ReplayMountainCar.margin_ok): the float64 post-step
position is at least 1e-9 away from goal_position and the velocity from goal_velocity, or the value is a clipped or zeroed constant that
is exact on both sides -- so a last-digit difference of cos cannot flip a flag."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mountain_car_inputs as MI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "train-procgen-pytorch_amd")
SMALL = dict(max_steps=5, **MI.VALID)       # truncations after 5 steps; the validation ranges, whose start draws are rejected 5 times in 24


def _engine(T, E, max_batch=None, **kw):
    from mi355.engine import Engine
    return Engine("mlp", T, E, 3, max_batch or E, obs_dim=5, mlp_depth=4, mlp_width=64, out_dim=64, **kw)


def _params(eng, seed=11):
    flat = (0.2 * np.random.default_rng(seed).standard_normal(eng.n_params)).astype(np.float32)
    eng.set_params(flat)
    return flat


def _device_env(eng, seed, **kw):
    from common.env.vec_envs import DeviceMountainCar
    env = DeviceMountainCar(eng.E, seed=seed, **kw)
    env.attach_engine(eng)
    return env


# ------------------------------------------------------------------------------------------ 1: one teacher-forced step, E = 70
def _one_step(sparse):
    c = MI.one_step_case(sparse)
    E = MI.ONE_STEP_E
    rp = MI.ReplayMountainCar(E, seed=c["seed"], **c["kw"])
    rp.load(c["state"], c["n_steps"], c["episode"])
    rp.step(c["act"])
    eng = _engine(2, E)
    env = _device_env(eng, c["seed"], **c["kw"])
    ring = np.random.default_rng(1).standard_normal((3, E, 5)).astype(np.float32)
    for t in range(3):
        eng.put_obs(t, ring[t])
    eng.env_set_state(c["state"], c["n_steps"], c["episode"])
    back = eng.env_state()
    obs, rew, done, info = env.step(c["act"])
    state, n_steps, episode = eng.env_state()
    ring_after = np.stack([eng.get_obs(t) for t in range(3)])
    low, high = env.low.copy(), env.high.copy()
    eng.close()
    return dict(c=c, margin_ok=rp.margin_ok(), back=back, obs=obs, rew=rew, done=done, info=info, state=state, n_steps=n_steps,
                episode=episode, ring=ring, ring_after=ring_after, low=low, high=high)


@pytest.fixture(scope="module")
def one_step_sparse():
    return _one_step(True)


@pytest.mark.parametrize("sparse", [True, False])
def test_one_teacher_forced_step_matches_the_reference(sparse, one_step_sparse):
    """E = 70 (a full wave + a 6-row tail), cases (b) and (c) of the fixture = the reference's own step.  Done flags exact; position and
    velocity of rows that go on within 1e-13 absolute (values at most 5 in magnitude, ulp(5) ~ 9e-16, at most three roundings on the
    position path, cos within a few ulp times gravity <= 0.0025: ~1e-15, two orders of margin), clipped / zeroed values exact, the three
    parameter columns bit-identical; the dense reward within 1 float32 ulp, the sparse one exactly -1; ended rows start episode + 1 inside
    [low, high] with goal_position <= right_boundary; the observation is float32(state); the rings are not touched."""
    r = one_step_sparse if sparse else _one_step(False)
    c = r["c"]
    assert r["margin_ok"].all(), np.nonzero(~r["margin_ok"])[0]
    for got, want in zip(r["back"], (c["state"], c["n_steps"], c["episode"])):
        assert np.array_equal(got, want)                                          # set_state / get_state round trip
    done = c["done"]
    assert set(np.nonzero(done)[0]) == MI.ONE_STEP_ENDED
    assert r["done"].dtype == np.float32 and np.array_equal(r["done"], done.astype(np.float32))
    go = ~done
    err = np.abs(r["state"][go, :2] - c["out_state"][go, :2]).max()
    print("max |device - reference| over position and velocity:", err)
    assert err <= 1e-13, err
    assert r["state"][go, 2:].tobytes() == c["state"][go, 2:].tobytes()
    assert (r["state"][54:56, :2] == (-1.2, 0.0)).all() and r["state"][57, 0] == 1.0                # the left wall, the right wall
    assert r["state"][58, 1] == 0.07 and r["state"][59, 1] == -0.07                                 # +-max_speed
    exact = np.array([54, 55, 58, 59])
    assert np.array_equal(r["state"][exact, 1], c["out_state"][exact, 1])
    assert np.array_equal(r["n_steps"][go], c["n_steps"][go] + 1) and np.array_equal(r["episode"][go], c["episode"][go])
    assert (r["n_steps"][done] == 0).all() and np.array_equal(r["episode"][done], c["episode"][done] + 1)
    fresh = r["state"][done]
    assert (fresh >= r["low"]).all() and (fresh <= r["high"]).all() and (fresh[:, 4] <= fresh[:, 3]).all() and (fresh[:, 1] == 0).all()
    assert r["obs"].dtype == np.float32 and np.array_equal(r["obs"], r["state"].astype(np.float32))
    want = c["rew"].astype(np.float32)
    if sparse:
        assert np.array_equal(r["rew"], np.full(MI.ONE_STEP_E, -1, np.float32)) and np.array_equal(want, r["rew"])
    else:
        ulps = np.abs(r["rew"] - want) / np.spacing(np.abs(want))
        print("dense reward: max float32 ulps from the reference:", ulps.max())
        assert r["rew"].dtype == np.float32 and (ulps <= 1).all(), ulps.max()
        assert len(np.unique(r["rew"])) > 60
    assert r["info"].has("env_reward") and np.array_equal(r["info"].column("env_reward"), r["rew"]) and len(r["info"]) == MI.ONE_STEP_E
    assert np.array_equal(r["ring_after"], r["ring"])                              # mi_env_step goes through its staging slot


# ------------------------------------------------------------------------------------------ 2: fresh states
def test_fresh_states_are_the_philox_restatement(one_step_sparse):
    """The rows that ended in the one-step case, and all rows after mi_env_reset at E = 6 with the validation ranges, are the CPU
    restatement's (attempt counter included) to 4 ulp (FMA contraction only).  Seeds 7 and 3 are chosen so that rows need a second, third
    and sixth attempt (shown below on the CPU).  The same seed gives identical states, another seed others."""
    r, c = one_step_sparse, one_step_sparse["c"]
    ended = np.nonzero(c["done"])[0]
    want, _ = MI.fresh_state(r["low"], r["high"], c["seed"], ended, c["episode"][ended] + 1)
    assert MI.within_ulp(r["state"][ended], want, 4).all(), np.abs(r["state"][ended] - want).max()
    got, most = {}, 0
    for name, seed in (("a", 7), ("b", 7), ("c", 3)):
        eng = _engine(2, 6)
        env = _device_env(eng, seed, **SMALL)
        first = env.reset()
        s1, n1, e1 = eng.env_state()
        env.reset()
        s2, n2, e2 = eng.env_state()
        eng.close()
        assert (e1 == 1).all() and (e2 == 2).all() and (n1 == 0).all() and (n2 == 0).all()
        assert np.array_equal(first, s1.astype(np.float32))
        for s, ep in ((s1, 1), (s2, 2)):
            want, attempts = MI.fresh_state(env.low, env.high, seed, np.arange(6), ep)
            assert (attempts > 1).any() or (seed, ep) == (3, 1)                     # (seed 3 rejects nothing in episode 1, a lot in 2)
            most = max(most, attempts.max())
            assert MI.within_ulp(s, want, 4).all(), (seed, ep)
            assert (s >= env.low).all() and (s <= env.high).all() and (s[:, 4] <= s[:, 3]).all() and (s[:, 1] == 0).all()
        got[name] = (s1, s2)
    assert most >= 6
    assert np.array_equal(got["a"][0], got["b"][0]) and np.array_equal(got["a"][1], got["b"][1])
    cols = [0, 2, 3, 4]                                                            # (velocity: low == high == 0)
    assert (got["a"][0][:, cols] != got["c"][0][:, cols]).all() and (got["a"][0][:, cols] != got["a"][1][:, cols]).all()


# ------------------------------------------------------------------------------------------ 3: a whole rollout against the CPU replay
def test_rollout_matches_the_cpu_replay_and_a_step_by_step_engine():
    """T = 8, E = 6, max_steps = 5: a termination, truncations and resets inside one mi_env_rollout.  Env 0 starts 1e-3 below its goal at
    max_speed: whatever the action its velocity stays above 0.07 - 0.001 - 0.0025 > 1e-3, so it is beyond the goal (or on the right wall
    at the goal) after step 1 with velocity >= goal_velocity = 0.  Env 1 starts at rest in the valley: 5 steps at no more than 0.07 cannot
    bring it from -0.5 to a goal >= 0.6, so it is truncated.  The replay is MountainCarVec.step on the device's actions with the Philox
    restatement for resets.  A second engine fed the ring's observations slot by slot reproduces act / logp / value bit for bit: the
    rollout's policy steps are mi_policy_step's."""
    from mi355.engine import F_ACT, F_DONE, F_LOGP, F_REW, F_VALUE
    T, E, env_seed, seed = 8, 6, 21, 77
    eng = _engine(T, E)
    flat = _params(eng)
    env = _device_env(eng, env_seed, **SMALL)
    env.reset()
    s0, n0, e0 = eng.env_state()
    s0[0, :2] = (s0[0, 4] - 1e-3, 0.07)
    s0[1, :2] = (-0.5, 0.0)
    eng.env_set_state(s0, n0, e0)
    eng.env_rollout(seed)
    rew, done, logp, value = (eng.read_field(f) for f in (F_REW, F_DONE, F_LOGP, F_VALUE))
    act = eng.read_field(F_ACT).astype(np.int64)
    obs = np.stack([eng.get_obs(t) for t in range(T + 1)])
    s1, n1, e1 = eng.env_state()
    eng.close()
    assert set(np.unique(act)) <= {0, 1, 2}
    rp = MI.ReplayMountainCar(E, seed=env_seed, **SMALL)
    robs, rrew, rdone, reached, ok = MI.replay(rp, s0, n0, e0, act)
    print("terminations", int((rdone & reached).sum()), "truncations", int((rdone & ~reached).sum()))
    assert ok.all(), np.argwhere(~ok)
    assert np.array_equal(done, rdone.astype(np.float32))
    assert np.array_equal(rew, rrew.astype(np.float32)) and (rew == -1).all()
    want = robs.astype(np.float32)
    assert (np.abs(obs - want) <= 1e-6 * np.abs(want)).all(), np.abs(obs - want).max()
    assert rdone[0, 0] and reached[0, 0] and rdone[4, 1] and not reached[4, 1] and not rdone[:4, 1].any()
    assert np.array_equal(obs[T], s1.astype(np.float32))                           # the ring observation is float32(state)
    assert np.array_equal(n1, rp.n_steps.astype(np.int32)) and np.array_equal(e1, rp.episode)
    assert np.isfinite(value).all() and np.isfinite(logp).all()
    eng2 = _engine(T, E)
    eng2.set_params(flat)
    for t in range(T + 1):
        eng2.put_obs(t, obs[t])
        a, lp, v = eng2.policy_step(t, seed=seed)
        assert v.tobytes() == value[t].tobytes(), t
        if t < T:
            assert np.array_equal(a, act[t]) and lp.tobytes() == logp[t].tobytes(), t
    eng2.close()


# ------------------------------------------------------------------------------------------ 4: refusals
def test_create_names_the_field_and_calls_without_an_env_are_refused():
    from mi355.engine import Engine, EngineError
    from common.env.vec_envs import DeviceCartPole, DeviceMountainCar
    eng = _engine(2, 4)
    with pytest.raises(EngineError, match="no env"):
        eng.env_rollout(1)
    with pytest.raises(EngineError, match="no env"):
        eng.env_reset()
    with pytest.raises(EngineError, match="no env"):
        eng.env_state()
    env = _device_env(eng, 0)
    with pytest.raises(EngineError, match="already has an env"):
        DeviceMountainCar(4, seed=1).attach_engine(eng)
    with pytest.raises(EngineError, match="0, 1 or 2"):
        env.step(np.array([0, 1, 2, 3]))
    with pytest.raises(EngineError, match="0, 1 or 2"):
        env.step(np.array([0, -1, 2, 1]))
    obs, rew, done, _ = env.step(np.array([0, 1, 2, 2]))                            # 2 is legal here
    assert obs.shape == (4, 5) and (rew == -1).all()
    eng.close()
    for mk, word in ((lambda: Engine("mlp", 2, 4, 3, 4, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64), "obs_dim"),
                     (lambda: Engine("mlp", 2, 4, 2, 4, obs_dim=5, mlp_depth=4, mlp_width=64, out_dim=64), "n_actions"),
                     (lambda: Engine("impala", 2, 4, 3, 4, out_dim=64), "arch")):
        eng = mk()
        with pytest.raises(EngineError, match=word):
            DeviceMountainCar(4).attach_engine(eng)
        eng.close()
    eng = Engine("mlp", 2, 4, 2, 4, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64)   # a cart-pole context keeps its own rules
    cp = DeviceCartPole(4)
    cp.attach_engine(eng)
    with pytest.raises(EngineError, match="obs_dim"):                               # (the width is checked before the occupancy)
        DeviceMountainCar(4).attach_engine(eng)
    with pytest.raises(EngineError, match="0 or 1"):
        cp.step(np.array([0, 1, 2, 0]))
    assert eng.env_state()[0].shape == (4, 9)
    eng.close()


# ------------------------------------------------------------------------------------------ 5: the agent
def _agent(T, E, env_seed=4, valid=False, **kw):
    from agents.ppo import PPO
    from common.env.vec_envs import DeviceMountainCar
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    env = DeviceMountainCar(E, seed=env_seed, **SMALL)
    env_v = DeviceMountainCar(E, seed=env_seed + 1, **SMALL) if valid else None
    policy = CategoricalPolicy(MLPModel(5, 4, 64, 64), False, 3)
    storage = Storage((5,), 64, T, E, dev)
    storage_v = Storage((5,), 64, T, E, dev) if valid else None
    logger = Logger(E, None)
    agent = PPO(env, policy, logger, storage, dev, 1, env_valid=env_v, storage_valid=storage_v, n_steps=T, n_envs=E, epoch=2, n_minibatch=2,
                mini_batch_size=32, gamma=0.99, lmbda=0.95, learning_rate=1e-3, entropy_coef=0.01, seed=0, **kw)
    return agent, env, env_v, logger


def test_ppo_trains_on_the_device_env():
    """PPO.train, two iterations at T = E = 8 with a validation env (both rollouts one mi_env_rollout each): the storage's mirrors are the
    device rings, every reward is -1, the losses are finite."""
    from mi355.engine import F_DONE, F_REW
    T, E = 8, 8
    agent, env, env_v, logger = _agent(T, E, valid=True, detect_nan=True)
    assert env.engine is agent.engine and env_v.engine is agent.engine_valid
    calls = []
    real = agent._collect_device
    agent._collect_device = lambda *a: calls.append(a[0]) or real(*a)
    agent.train(2 * T * E)
    assert calls == [env, env_v, env, env_v]
    for st, eng in ((agent.storage, agent.engine), (agent.storage_valid, agent.engine_valid)):
        rew, done = eng.read_field(F_REW), eng.read_field(F_DONE)
        assert np.array_equal(st._rew, rew) and np.array_equal(st._done, done)
        assert (rew == -1).all() and done.any() and set(np.unique(done)) <= {0.0, 1.0}
        assert st.step == 0 and len(st.info_batch) == T
        obs = st.obs_batch.numpy()
        assert obs.shape == (T + 1, E, 5) and np.isfinite(obs).all()
        assert (obs[..., 0] >= np.float32(-1.2)).all() and (obs[..., 0] <= obs[..., 3]).all() and (np.abs(obs[..., 1]) <= np.float32(0.07)).all()
        assert (obs[..., 1] != 0).any()                                             # the env really steps
    assert len(logger.rows) == 2
    for name in ("loss_total", "loss_pi", "loss_v", "loss_entropy"):
        assert np.isfinite([row[logger.columns.index(name)] for row in logger.rows]).all(), name
    assert logger.rows[-1][logger.columns.index("num_episodes")] > 0
    agent.engine.close(); agent.engine_valid.close()


# ------------------------------------------------------------------------------------------ 6: lifetime
def test_env_buffers_go_back_with_the_context():
    import gc
    from mi355.engine import live_resources
    gc.collect()
    base = live_resources()
    for _ in range(2):
        eng = _engine(4, 6)
        _params(eng)
        plain = live_resources()
        env = _device_env(eng, 1, **SMALL)
        assert live_resources()[0] == plain[0] + 7 and live_resources()[1:] == plain[1:]      # state, n_steps, episode + the staging slot's four
        env.reset()
        eng.env_rollout(3)
        eng.sync()
        eng.close()
        assert live_resources() == base, (live_resources(), base)


# ------------------------------------------------------------------------------------------ 7: the command line
@pytest.mark.parametrize("flag", [["--device_env"], []])
def test_train_cli_runs_the_mountain_car(tmp_path, flag):
    """`python train.py --env_name mountain_car --param_name mountain_car [--device_env]`: two iterations with the validation env, log rows
    and a checkpoint in the reference's format -- on the device env and on the host's MountainCarVec."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "--exp_name", "dev", "--env_name", "mountain_car", "--param_name", "mountain_car",
           "--n_envs", "8", "--n_steps", "16", "--mini_batch_size", "32", "--seed", "3", "--detect_nan", "--num_timesteps", "250",
           "--num_checkpoints", "1"] + flag
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ("rollout: device-resident env" if flag else "rollout: serial steps") in r.stdout
    runs = os.listdir(tmp_path / "logs" / "train" / "mountain_car" / "dev")
    assert len(runs) == 1 and runs[0].endswith("__seed_3")
    rd = tmp_path / "logs" / "train" / "mountain_car" / "dev" / runs[0]
    assert {"hyperparameters.npy", "config.npy", "log-append.csv", "model_256.pth"} <= set(os.listdir(rd))
    ck = torch.load(rd / "model_256.pth", map_location="cpu", weights_only=True)
    assert ck["t"] == 256 and ck["model_state_dict"]["fc_policy.weight"].shape == (3, 64)
    rows = open(rd / "log-append.csv").read().strip().splitlines()
    assert len(rows) == 3 and rows[0].startswith("timesteps,wall_time,num_episodes,max_episode_rewards")
    assert [float(row.split(",")[0]) for row in rows[1:]] == [128.0, 256.0]
