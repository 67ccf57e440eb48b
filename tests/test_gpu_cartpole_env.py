"""The device-resident cart-pole (csrc/env_device.hip, mi_env_* in include/mi355ppo.h, common/env/vec_envs.py DeviceCartPole, train.py
--device_env) against CartPoleVec, the project's float64 restatement of the reference env, and against a CPU replay that drives
CartPoleVec.step with the numpy restatement of the device env's Philox reset stream (tests/cartpole_inputs.py).

Every comparison of a done flag is preceded by a CPU check that the float64 post-step x / theta is at least 1e-9 away from its
threshold, so a last-digit difference of sin / cos cannot flip a flag."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cartpole_inputs as CI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "train-procgen-pytorch_amd")
SMALL = dict(max_steps=5, h_range=0.06)      # truncations after 5 steps, terminations when x drifts 1 cm beyond the start range


def _engine(T, E, max_batch=None, **kw):
    from mi355.engine import Engine
    return Engine("mlp", T, E, 2, max_batch or E, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64, **kw)


def _params(eng, seed=11):
    flat = (0.2 * np.random.default_rng(seed).standard_normal(eng.n_params)).astype(np.float32)
    eng.set_params(flat)
    return flat


def _device_env(eng, seed, **kw):
    from common.env.vec_envs import DeviceCartPole
    env = DeviceCartPole(eng.E, seed=seed, **kw)
    env.attach_engine(eng)
    return env


# ------------------------------------------------------------------------------------------ 1 + 2: one teacher-forced step, E = 70
@pytest.fixture(scope="module")
def one_step():
    """One mi_env_step from the states of cartpole_inputs.one_step_case, next to CartPoleVec.step from the same states."""
    from common.env.vec_envs import CartPoleVec
    c = CI.one_step_case()
    E = CI.ONE_STEP_E
    ref = CartPoleVec(E, **c["kw"])
    ref.state, ref.n_steps, ref.terminated = c["state"].copy(), c["n_steps"].astype(np.float64), np.full(E, False)
    rp = CI.ReplayCartPole(E, seed=CI.ONE_STEP_SEED, **c["kw"])
    rp.load(c["state"], c["n_steps"], c["episode"])
    rp.step(c["act"])
    margin = rp.margin()
    ref_state, _, ref_done, _ = ref.step(c["act"])
    eng = _engine(2, E)
    env = _device_env(eng, CI.ONE_STEP_SEED, **c["kw"])
    ring = np.random.default_rng(1).standard_normal((3, E, 9)).astype(np.float32)
    for t in range(3):
        eng.put_obs(t, ring[t])
    eng.env_set_state(c["state"], c["n_steps"], c["episode"])
    back = eng.env_state()
    obs, rew, done, info = env.step(c["act"])
    state, n_steps, episode = eng.env_state()
    ring_after = np.stack([eng.get_obs(t) for t in range(3)])
    low, high = env.low.copy(), env.high.copy()
    eng.close()
    return dict(c=c, margin=margin, ref_state=ref_state.copy(), ref_done=ref_done.copy(), back=back, obs=obs, rew=rew, done=done, info=info,
                state=state, n_steps=n_steps, episode=episode, ring=ring, ring_after=ring_after, low=low, high=high)


def test_one_teacher_forced_step_matches_cartpolevec(one_step):
    """E = 70 (a full wave + a 6-row tail): random interior rows with both actions, rows landing 1e-6 inside / outside each of the four
    thresholds, rows one and two steps short of max_steps.  Done flags exact; the four dynamic columns of rows that go on within 1e-12
    absolute of CartPoleVec.step (magnitudes below ~1e2 after the tau scaling, ~40 fp64 roundings plus sin / cos within a few ulp give
    ~1e-14; two orders of margin for FMA contraction and a different libm), their five parameter columns bit-identical; ended rows
    start episode + 1 inside [low, high]; the observation is float32(state), the reward exactly 1; the rings are not touched."""
    r, c = one_step, one_step["c"]
    assert r["margin"] >= 1e-9, r["margin"]
    for got, want in zip(r["back"], (c["state"], c["n_steps"], c["episode"])):
        assert np.array_equal(got, want)                                          # set_state / get_state round trip
    done = r["ref_done"]
    assert set(np.nonzero(done)[0]) == {51, 53, 55, 57, 58, 59}                    # just outside x 2 signs x 2 variables, two truncations
    assert r["done"].dtype == np.float32 and np.array_equal(r["done"], done.astype(np.float32))
    go = ~done
    err = np.abs(r["state"][go, :4] - r["ref_state"][go, :4]).max()
    print("max |device - CartPoleVec| over the dynamic columns:", err)
    assert err <= 1e-12, err
    assert r["state"][go, 4:].tobytes() == c["state"][go, 4:].tobytes()
    assert np.array_equal(r["n_steps"][go], c["n_steps"][go] + 1) and np.array_equal(r["episode"][go], c["episode"][go])
    assert (r["n_steps"][done] == 0).all() and np.array_equal(r["episode"][done], c["episode"][done] + 1)
    assert (r["state"][done] >= r["low"]).all() and (r["state"][done] <= r["high"]).all()
    assert r["obs"].dtype == np.float32 and np.array_equal(r["obs"], r["state"].astype(np.float32))
    assert np.array_equal(r["rew"], np.ones(CI.ONE_STEP_E, np.float32))
    assert r["info"].has("env_reward") and np.array_equal(r["info"].column("env_reward"), r["rew"]) and len(r["info"]) == CI.ONE_STEP_E
    assert np.array_equal(r["ring_after"], r["ring"])                              # mi_env_step goes through its staging slot


def test_fresh_states_are_the_philox_restatement(one_step):
    """The rows that ended in the one-step case, and all rows after mi_env_reset at E = 6, are low + (high - low) * philox_u53(seed,
    env, episode) of the CPU restatement to 4 ulp (FMA contraction only); the same seed gives identical states, another seed others."""
    r, c = one_step, one_step["c"]
    ended = np.nonzero(r["ref_done"])[0]
    want = CI.fresh_state(r["low"], r["high"], CI.ONE_STEP_SEED, ended, c["episode"][ended] + 1)
    assert CI.within_ulp(r["state"][ended], want, 4).all(), np.abs(r["state"][ended] - want).max()
    got = {}
    for name, seed in (("a", 5), ("b", 5), ("c", 6)):
        eng = _engine(2, 6)
        env = _device_env(eng, seed)
        first = env.reset()
        s1, n1, e1 = eng.env_state()
        env.reset()
        s2, n2, e2 = eng.env_state()
        eng.close()
        assert (e1 == 1).all() and (e2 == 2).all() and (n1 == 0).all() and (n2 == 0).all()
        assert np.array_equal(first, s1.astype(np.float32))
        for s, ep in ((s1, 1), (s2, 2)):
            assert CI.within_ulp(s, CI.fresh_state(env.low, env.high, seed, np.arange(6), ep), 4).all()
            assert (s >= env.low).all() and (s <= env.high).all()
        got[name] = (s1, s2)
    assert np.array_equal(got["a"][0], got["b"][0]) and np.array_equal(got["a"][1], got["b"][1])
    assert (got["a"][0][:, :8] != got["c"][0][:, :8]).all() and (got["a"][0][:, :8] != got["a"][1][:, :8]).all()      # (force_mag: low == high)


# ------------------------------------------------------------------------------------------ 3: a whole rollout against the CPU replay
def test_rollout_matches_the_cpu_replay_and_a_step_by_step_engine():
    """T = 8, E = 6, max_steps = 5, h_range = 0.06: truncations, terminations and resets inside one mi_env_rollout.  Env 0 starts at
    x = 0.055 with x_dot = 0.5 (beyond the threshold after one step whatever the action), env 1 at rest in the middle (cannot reach a
    threshold in 5 steps: 0.02 * 0.16 * (0 + 1 + 2 + 3 + 4) = 0.032 < 0.06, so it is truncated).  The replay is CartPoleVec.step on
    the device's actions with the Philox restatement for resets.  A second engine fed the ring's observations slot by slot reproduces
    act / logp / value bit for bit: the rollout's policy steps are mi_policy_step's."""
    from mi355.engine import F_ACT, F_DONE, F_LOGP, F_REW, F_VALUE
    T, E, env_seed, seed = 8, 6, 21, 77
    eng = _engine(T, E)
    flat = _params(eng)
    env = _device_env(eng, env_seed, **SMALL)
    env.reset()
    s0, n0, e0 = eng.env_state()
    s0[0, :4] = (0.055, 0.5, 0.0, 0.0)
    s0[1, :4] = 0.0
    eng.env_set_state(s0, n0, e0)
    eng.env_rollout(seed)
    rew, done, logp, value = (eng.read_field(f) for f in (F_REW, F_DONE, F_LOGP, F_VALUE))
    act = eng.read_field(F_ACT).astype(np.int64)
    obs = np.stack([eng.get_obs(t) for t in range(T + 1)])
    s1, n1, e1 = eng.env_state()
    eng.close()
    assert set(np.unique(act)) <= {0, 1}
    rp = CI.ReplayCartPole(E, seed=env_seed, **SMALL)
    robs, rdone, beyond, margin = CI.replay(rp, s0, n0, e0, act)
    print("threshold margin of the replay:", margin, "terminations", int((rdone & beyond).sum()), "truncations", int((rdone & ~beyond).sum()))
    assert margin >= 1e-9, margin
    assert np.array_equal(done, rdone.astype(np.float32)) and np.array_equal(rew, np.ones((T, E), np.float32))
    want = robs.astype(np.float32)
    assert (np.abs(obs - want) <= 1e-6 * np.abs(want)).all(), np.abs(obs - want).max()
    assert (rdone & beyond).any() and (rdone & ~beyond).any()
    assert rdone[0, 0] and beyond[0, 0] and rdone[4, 1] and not beyond[4, 1]
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


def test_rollout_is_refused_without_an_env_and_create_names_the_field():
    from mi355.engine import Engine, EngineError
    from common.env.vec_envs import DeviceCartPole
    eng = _engine(2, 4)
    with pytest.raises(EngineError, match="no env"):
        eng.env_rollout(1)
    with pytest.raises(EngineError, match="no env"):
        eng.env_reset()
    env = _device_env(eng, 0)
    with pytest.raises(EngineError, match="already has an env"):
        DeviceCartPole(4, seed=1).attach_engine(eng)
    with pytest.raises(EngineError, match="0 or 1"):
        env.step(np.array([0, 1, 2, 0]))
    eng.close()
    for mk, word in ((lambda: Engine("mlp", 2, 4, 2, 4, obs_dim=8, mlp_depth=4, mlp_width=64, out_dim=64), "obs_dim"),
                     (lambda: Engine("mlp", 2, 4, 3, 4, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64), "n_actions"),
                     (lambda: Engine("impala", 2, 4, 2, 4, out_dim=64), "arch")):
        eng = mk()
        with pytest.raises(EngineError, match=word):
            DeviceCartPole(4).attach_engine(eng)
        eng.close()


# ------------------------------------------------------------------------------------------ 4: the VecEnv protocol path
def _agent(T, E, env_seed=4, valid=False, **kw):
    from agents.ppo import PPO
    from common.env.vec_envs import DeviceCartPole
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    env = DeviceCartPole(E, seed=env_seed, **SMALL)
    env_v = DeviceCartPole(E, seed=env_seed + 1, **SMALL) if valid else None
    policy = CategoricalPolicy(MLPModel(9, 4, 64, 64), False, 2)
    storage = Storage((9,), 64, T, E, dev)
    storage_v = Storage((9,), 64, T, E, dev) if valid else None
    logger = Logger(E, None)
    agent = PPO(env, policy, logger, storage, dev, 1, env_valid=env_v, storage_valid=storage_v, n_steps=T, n_envs=E, epoch=2, n_minibatch=2,
                mini_batch_size=32, gamma=0.99, lmbda=0.95, learning_rate=1e-3, entropy_coef=0.01, seed=0, **kw)
    return agent, env, env_v, logger


def test_protocol_reset_and_step_agree_with_the_replay():
    """DeviceCartPole.reset() / .step(act) over 12 steps (max_steps = 5: every env is reset at least twice) against the CPU replay."""
    E, env_seed = 6, 9
    eng = _engine(2, E)
    env = _device_env(eng, env_seed, **SMALL)
    obs0 = env.reset()
    s0, n0, e0 = eng.env_state()
    acts = np.random.default_rng(3).integers(0, 2, (12, E))
    outs = [env.step(a) for a in acts]
    eng.close()
    rp = CI.ReplayCartPole(E, seed=env_seed, **SMALL)
    robs, rdone, beyond, margin = CI.replay(rp, s0, n0, e0, acts)
    assert margin >= 1e-9, margin
    assert np.array_equal(obs0, s0.astype(np.float32))
    assert rdone.sum() >= 2 * E
    for t, (o, r, d, info) in enumerate(outs):
        want = robs[t + 1].astype(np.float32)
        assert (np.abs(o - want) <= 1e-6 * np.abs(want)).all(), t
        assert np.array_equal(d, rdone[t].astype(np.float32)) and np.array_equal(r, np.ones(E, np.float32)), t
        assert np.array_equal(info.column("env_reward"), r) and info[0] == {"env_reward": 1.0}


def test_public_predict_and_store_loop_runs_on_the_device_env():
    """The reference's own loop (agents/ppo.py:225-236): env.reset(), agent.predict, env.step, storage.store, ..., store_last."""
    T, E = 8, 6
    agent, env, _, _ = _agent(T, E)
    storage = agent.storage
    obs = env.reset()
    hidden, done = np.zeros((E, storage.hidden_state_size)), np.zeros(E)
    seen_obs, seen_act, seen_done = [obs], [], []
    for _ in range(T):
        act, logp, value, nh = agent.predict(obs, hidden, done)
        nobs, rew, done, info = env.step(act)
        storage.store(obs, hidden, act, rew, done, info, logp, value)
        obs, hidden = nobs, nh
        seen_obs.append(obs); seen_act.append(act); seen_done.append(done)
    _, _, last_val, hidden = agent.predict(obs, hidden, done)
    storage.store_last(obs, hidden, last_val)
    assert np.array_equal(storage.obs_batch.numpy(), np.stack(seen_obs))
    assert np.array_equal(storage.act_batch.numpy(), np.stack(seen_act).astype(np.float32))
    assert np.array_equal(storage.done_batch.numpy(), np.stack(seen_done)) and (storage.rew_batch.numpy() == 1).all()
    assert np.stack(seen_done).any()
    rew_b, done_b, _ = storage.fetch_log_data()
    assert rew_b.shape == (T, E) and np.array_equal(done_b, np.stack(seen_done))
    storage.compute_estimates(0.99, 0.95, True, True)
    assert np.isfinite(storage.adv_batch.numpy()).all()
    agent.engine.close()


# ------------------------------------------------------------------------------------------ 5: the agent
def test_ppo_trains_on_the_device_env():
    """PPO.train, two iterations at T = E = 8 with a validation env (both rollouts one mi_env_rollout each): the storage's mirrors are the
    device rings, fetch_log_data is what a plain Storage fed the same arrays returns, the losses are finite."""
    from common.env.vec_envs import StepInfo
    from common.storage import Storage
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
        assert (rew == 1).all() and done.any() and set(np.unique(done)) <= {0.0, 1.0}
        assert st.step == 0 and len(st.info_batch) == T
        plain = Storage((9,), 64, T, E, torch.device("cuda", 0))
        for t in range(T):
            plain.note_stored(rew[t], done[t], StepInfo(E, {"env_reward": rew[t]}))
        for got, want in zip(st.fetch_log_data(), plain.fetch_log_data()):
            assert np.array_equal(got, want, equal_nan=True)
        obs = st.obs_batch.numpy()
        assert np.isfinite(obs).all() and (np.abs(obs[..., 0]) <= 0.06 + 0.05).all()      # x never far beyond h_range: the env really steps
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
        assert all(p > b for p, b in zip(plain, base))
        env = _device_env(eng, 1, **SMALL)
        assert live_resources()[0] == plain[0] + 7 and live_resources()[1:] == plain[1:]      # state, n_steps, episode + the staging slot's four
        env.reset()
        eng.env_rollout(3)
        eng.sync()
        eng.close()
        assert live_resources() == base, (live_resources(), base)


# ------------------------------------------------------------------------------------------ 7: the command line
def test_train_cli_runs_with_device_env(tmp_path):
    """`python train.py --env_name cartpole --param_name cartpole --device_env`: two iterations with the validation env, log rows and a
    checkpoint in the reference's format."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "--exp_name", "dev", "--env_name", "cartpole", "--param_name", "cartpole", "--device_env",
           "--n_envs", "8", "--n_steps", "16", "--mini_batch_size", "32", "--seed", "3", "--detect_nan", "--num_timesteps", "250",
           "--num_checkpoints", "1"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "rollout: device-resident env" in r.stdout
    runs = os.listdir(tmp_path / "logs" / "train" / "cartpole" / "dev")
    assert len(runs) == 1 and runs[0].endswith("__seed_3")
    rd = tmp_path / "logs" / "train" / "cartpole" / "dev" / runs[0]
    assert {"hyperparameters.npy", "config.npy", "log-append.csv", "model_256.pth"} <= set(os.listdir(rd))
    ck = torch.load(rd / "model_256.pth", map_location="cpu", weights_only=True)
    assert ck["t"] == 256 and ck["model_state_dict"]["fc_policy.weight"].shape == (2, 64)
    rows = open(rd / "log-append.csv").read().strip().splitlines()
    assert len(rows) == 3 and rows[0].startswith("timesteps,wall_time,num_episodes,max_episode_rewards")
    assert [float(row.split(",")[0]) for row in rows[1:]] == [128.0, 256.0]
