"""The device-resident swing-up cart-pole (csrc/env_physics.h `CartPoleSwing`, mi_env_cartpole_swing_create and mi_env_* in
include/mi355ppo.h, common/env/vec_envs.py DeviceCartPoleSwing, train.py --env_name cartpole_swing --device_env [--resident_rollout]) against
CartPoleSwingVec -- which tests/test_cartpole_swing_host.py pins bit for bit to the reference's own class through the fixture
tests/golden/g18_cartpole_swing.npz -- and against a CPU replay that drives CartPoleSwingVec.step with the numpy restatement of the device
env's Philox reset stream (tests/cartpole_swing_inputs.py).

Every comparison of a done flag is preceded by a CPU check that the float64 post-step x is at least 1e-9 away from +-h_range, so a
last-digit difference of sin / cos cannot flip a flag.  Rewards are compared by value (a row that ends beyond the edge with the reward
clamp on yields -0.0 on both sides)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cartpole_inputs as CI
import cartpole_swing_inputs as SI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "train-procgen-pytorch_amd")


def _engine(T, E, max_batch=None, **kw):
    from mi355.engine import Engine
    return Engine("mlp", T, E, 2, max_batch or E, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64, **kw)


def _params(eng, seed=11):
    flat = (0.2 * np.random.default_rng(seed).standard_normal(eng.n_params)).astype(np.float32)
    eng.set_params(flat)
    return flat


def _device_env(eng, seed, **kw):
    from common.env.vec_envs import DeviceCartPoleSwing
    env = DeviceCartPoleSwing(eng.E, seed=seed, **kw)
    env.attach_engine(eng)
    return env


def _read(eng):
    from mi355.engine import F_ACT, F_DONE, F_LOGP, F_REW, F_VALUE
    r = dict(rew=eng.read_field(F_REW), done=eng.read_field(F_DONE), logp=eng.read_field(F_LOGP), value=eng.read_field(F_VALUE),
             act=eng.read_field(F_ACT).astype(np.int64), obs=np.stack([eng.get_obs(t) for t in range(eng.T + 1)]))
    r["state"], r["n_steps"], r["episode"] = eng.env_state()
    return r


# ------------------------------------------------------------------------------------------ 1 + 2: one teacher-forced step, E = 70
@pytest.fixture(scope="module")
def one_step():
    """One mi_env_step from the states of the fixture's case (b), next to CartPoleSwingVec.step from the same states."""
    from common.env.vec_envs import CartPoleSwingVec
    c = SI.one_step_case()
    E = SI.ONE_STEP_E
    ref = CartPoleSwingVec(E, seed=c["seed"], **c["kw"])
    ref.state, ref.n_steps, ref.terminated = c["state"].copy(), c["n_steps"].astype(np.float64), np.full(E, False)
    rp = SI.ReplayCartPoleSwing(E, seed=c["seed"], **c["kw"])
    rp.load(c["state"], c["n_steps"], c["episode"])
    rp.step(c["act"])
    margin = rp.margin()
    ref_state, ref_rew, ref_done, _ = ref.step(c["act"])
    eng = _engine(2, E)
    env = _device_env(eng, c["seed"], **c["kw"])
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
    return dict(c=c, margin=margin, ref_state=ref_state.copy(), ref_rew=ref_rew.copy(), ref_done=ref_done.copy(), back=back, obs=obs, rew=rew,
                done=done, info=info, state=state, n_steps=n_steps, episode=episode, ring=ring, ring_after=ring_after, low=low, high=high)


def test_one_teacher_forced_step_matches_cartpoleswingvec(one_step):
    """E = 70 (a full wave + a 6-row tail), all 70 rows: random interior rows over several turns of theta with both actions, rows landing
    1e-6 inside / outside +-h_range, rows landing 1e-6 either side of +-pi/2 (the reward clamp), rows at theta = +-0.3 (no angle
    threshold: they go on), rows one and two steps short of max_steps.  Done flags exact; the four dynamic columns of rows that go on
    within 1e-12 absolute of CartPoleSwingVec.step -- the cart-pole test's bound and reasoning: |theta_dot| <= 8 keeps the accelerations
    below 1e2, so magnitudes stay below ~1e2 after the tau scaling, ~40 fp64 roundings plus sin / cos within a few ulp give ~1e-14; two
    orders of margin for a different libm --, their five parameter columns bit-identical; the reward within 1 float32 ulp of
    float32(host reward) and 0 wherever the host's is 0; ended rows start episode + 1 inside [low, high]; the observation is
    float32(state); the rings are not touched.
    Measured on an MI355X: see profiles/cartpole_swing_device_env.md."""
    r, c = one_step, one_step["c"]
    E = SI.ONE_STEP_E
    assert r["margin"] >= 1e-9, r["margin"]
    assert np.array_equal(r["ref_state"], c["out_state"]) and np.array_equal(r["ref_rew"], c["rew"])      # the host step IS the reference's
    for got, want in zip(r["back"], (c["state"], c["n_steps"], c["episode"])):
        assert np.array_equal(got, want)                                          # set_state / get_state round trip
    done = r["ref_done"]
    assert set(np.nonzero(done)[0]) == SI.ONE_STEP_ENDED and not done[58:60].any()
    assert r["done"].shape == (E,) and r["done"].dtype == np.float32 and np.array_equal(r["done"], done.astype(np.float32))
    go = ~done
    err = np.abs(r["state"][go, :4] - r["ref_state"][go, :4]).max()
    print("max |device - CartPoleSwingVec| over the dynamic columns:", err)
    assert err <= 1e-12, err
    assert r["state"][go, 4:].tobytes() == c["state"][go, 4:].tobytes()
    assert np.array_equal(r["n_steps"][go], c["n_steps"][go] + 1) and np.array_equal(r["episode"][go], c["episode"][go])
    assert (r["n_steps"][done] == 0).all() and np.array_equal(r["episode"][done], c["episode"][done] + 1)
    assert (r["state"][done] >= r["low"]).all() and (r["state"][done] <= r["high"]).all()
    assert r["obs"].dtype == np.float32 and np.array_equal(r["obs"], r["state"].astype(np.float32))
    want = r["ref_rew"]
    w32 = want.astype(np.float32)
    nz = w32 != 0
    ulps = np.abs(r["rew"][nz].astype(np.float64) - w32[nz]) / np.spacing(np.abs(w32[nz]))
    print("reward: max float32 ulps from float32(host reward):", ulps.max(), "rows with reward 0:", int((want == 0).sum()))
    assert r["rew"].shape == (E,) and r["rew"].dtype == np.float32 and SI.within_f32_ulp(r["rew"], want, 1).all(), np.nonzero(~SI.within_f32_ulp(r["rew"], want, 1))[0]
    assert (r["rew"][want == 0] == 0).all() and (want == 0).sum() >= 20 and (r["rew"] > 0).sum() >= 20
    for row, clamped in SI.CLAMP_ROWS.items():
        assert (r["rew"][row] == 0) if clamped else (0 < r["rew"][row] < 2e-6), row
    assert r["info"].has("env_reward") and np.array_equal(r["info"].column("env_reward"), r["rew"]) and len(r["info"]) == E
    assert np.array_equal(r["ring_after"], r["ring"])                              # mi_env_step goes through its staging slot


def test_fresh_states_are_the_philox_restatement(one_step):
    """The rows that ended in the one-step case, and all rows after mi_env_reset at E = 6, are low + (high - low) * philox_u53(seed, env,
    episode) of the cart-pole's CPU restatement with the swing-up's ranges to 4 ulp; they lie inside [low, high] (the pole hangs: theta in
    pi -+ 0.05); the same seed gives identical states, another seed others."""
    r, c = one_step, one_step["c"]
    ended = np.nonzero(r["ref_done"])[0]
    want = CI.fresh_state(r["low"], r["high"], c["seed"], ended, c["episode"][ended] + 1)
    assert CI.within_ulp(r["state"][ended], want, 4).all(), np.abs(r["state"][ended] - want).max()
    assert (r["state"][ended] >= r["low"]).all() and (r["state"][ended] <= r["high"]).all()
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
            assert (s >= env.low).all() and (s <= env.high).all() and (np.abs(s[:, 2] - np.pi) <= 0.05).all()
        got[name] = (s1, s2)
    assert np.array_equal(got["a"][0], got["b"][0]) and np.array_equal(got["a"][1], got["b"][1])
    assert (got["a"][0][:, :8] != got["c"][0][:, :8]).all() and (got["a"][0][:, :8] != got["a"][1][:, :8]).all()      # (force_mag: low == high)


# ------------------------------------------------------------------------------------------ 3: a whole rollout against the CPU replay
def test_rollout_matches_the_cpu_replay_and_a_step_by_step_engine():
    """T = 8, E = 6, max_steps = 5: a termination, truncations and resets inside one mi_env_rollout.  Env 0 starts at x = h_range - 0.005
    with x_dot = 0.5 (beyond the edge after one step whatever the action), env 1 upright at rest (theta = 0.01: rewards above 0.9,
    truncated at step 5), env 2 at theta = 0.3 (beyond the balance task's 12 degrees: it must not end before step 5), the others hang
    (reward 0).  The replay is CartPoleSwingVec.step on the device's actions with the Philox restatement for resets.  A second engine fed
    the ring's observations slot by slot reproduces act / logp / value bit for bit: the rollout's policy steps are mi_policy_step's."""
    T, E, env_seed, seed = 8, 6, 21, 77
    eng = _engine(T, E)
    flat = _params(eng)
    env = _device_env(eng, env_seed, **SI.SMALL)
    env.reset()
    s0, n0, e0 = eng.env_state()
    s0 = SI.plant(s0)
    eng.env_set_state(s0, n0, e0)
    eng.env_rollout(seed)
    g = _read(eng)
    eng.close()
    act, rew, done, obs = g["act"], g["rew"], g["done"], g["obs"]
    assert set(np.unique(act)) <= {0, 1}
    rp = SI.ReplayCartPoleSwing(E, seed=env_seed, **SI.SMALL)
    robs, rrew, rdone, beyond, margin = SI.replay(rp, s0, n0, e0, act)
    print("threshold margin of the replay:", margin, "terminations", int((rdone & beyond).sum()), "truncations", int((rdone & ~beyond).sum()))
    assert margin >= SI.ENV_MARGIN, margin
    assert np.array_equal(done, rdone.astype(np.float32))
    assert SI.within_f32_ulp(rew, rrew, 1).all(), np.argwhere(~SI.within_f32_ulp(rew, rrew, 1))
    want = robs.astype(np.float32)
    assert (np.abs(obs - want) <= 1e-6 * np.abs(want)).all(), np.abs(obs - want).max()
    assert done[0, 0] == 1 and beyond[0, 0] and rew[0, 0] == 0 and beyond.sum() == 1                  # env 0: over the edge at step 1
    assert (rew[:5, 1] > 0.9).all() and done[4, 1] == 1 and not beyond[4, 1] and not done[:4, 1].any()  # env 1: upright, truncated
    assert not done[:4, 2].any() and done[4, 2] == 1 and (rew[:5, 2] > 0.5).all()                      # env 2: no angle threshold
    assert (rew[:, 3:] == 0).all() and (rew[5:, :3] == 0).all() and (rew[1:, 0] == 0).all()            # hanging poles earn nothing
    assert np.array_equal(obs[T], g["state"].astype(np.float32))                   # the ring observation is float32(state)
    assert np.array_equal(g["n_steps"], rp.n_steps.astype(np.int32)) and np.array_equal(g["episode"], rp.episode)
    assert np.isfinite(g["value"]).all() and np.isfinite(g["logp"]).all()
    eng2 = _engine(T, E)
    eng2.set_params(flat)
    for t in range(T + 1):
        eng2.put_obs(t, obs[t])
        a, lp, v = eng2.policy_step(t, seed=seed)
        assert v.tobytes() == g["value"][t].tobytes(), t
        if t < T:
            assert np.array_equal(a, act[t]) and lp.tobytes() == g["logp"][t].tobytes(), t
    eng2.close()


# ------------------------------------------------------------------------------------------ 4: refusals
def test_create_refusals_are_raised_by_name():
    from mi355.engine import Engine, EngineError
    from common.env.vec_envs import DeviceCartPole, DeviceCartPoleSwing
    for mk, word in ((lambda: Engine("mlp", 2, 4, 2, 4, obs_dim=8, mlp_depth=4, mlp_width=64, out_dim=64), "mi_env_cartpole_swing_create: obs_dim must be 9"),
                     (lambda: Engine("mlp", 2, 4, 3, 4, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64), "mi_env_cartpole_swing_create: n_actions must be 2"),
                     (lambda: Engine("impala", 2, 4, 2, 4, out_dim=64), "mi_env_cartpole_swing_create: arch")):
        eng = mk()
        with pytest.raises(EngineError, match=word):
            DeviceCartPoleSwing(4).attach_engine(eng)
        eng.close()
    eng = _engine(2, 4)                                                            # a GRU context
    H, rng = 64, np.random.default_rng(9)
    eng.set_gru(*(0.1 * rng.standard_normal(n).astype(np.float32) for n in (3 * H * H, 3 * H * H, 3 * H, 3 * H)))
    with pytest.raises(EngineError, match="mi_env_cartpole_swing_create: a recurrent context"):
        DeviceCartPoleSwing(4).attach_engine(eng)
    eng.close()
    for h_range in (0.0, -2.4, float("nan")):                                      # the reward divides by x_threshold
        eng = _engine(2, 4)
        with pytest.raises(EngineError, match="mi_env_cartpole_swing_create: x_threshold must be positive"):
            DeviceCartPoleSwing(4, h_range=h_range).attach_engine(eng)
        with pytest.raises(EngineError, match="no env"):                           # a refused create leaves no env behind
            eng.env_reset()
        eng.close()
    eng = _engine(2, 4)
    with pytest.raises(EngineError, match="mi_env_cartpole_swing_create: max_steps"):
        DeviceCartPoleSwing(4, max_steps=0).attach_engine(eng)
    with pytest.raises(EngineError, match="no env.*mi_env_cartpole_swing_create"):
        eng.env_rollout(1)
    env = _device_env(eng, 0)
    with pytest.raises(EngineError, match="mi_env_cartpole_swing_create: this context already has an env"):
        DeviceCartPoleSwing(4, seed=1).attach_engine(eng)
    with pytest.raises(EngineError, match="mi_env_cartpole_create: this context already has an env"):
        DeviceCartPole(4, seed=1).attach_engine(eng)
    env.reset()
    with pytest.raises(EngineError, match="0 or 1"):
        env.step(np.array([0, 1, 2, 0]))
    obs, rew, done, _ = env.step(np.array([0, 1, 1, 0]))                            # (the poles hang: reward 0)
    assert obs.shape == (4, 9) and (rew == 0).all() and not done.any() and eng.env_state()[0].shape == (4, 9)
    eng.close()


# ------------------------------------------------------------------------------------------ 5: the agent and the command line
def _agent(T, E, env_seed=4, **kw):
    from agents.ppo import PPO
    from common.env.vec_envs import DeviceCartPoleSwing
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    env, env_v = DeviceCartPoleSwing(E, seed=env_seed, **SI.SMALL), DeviceCartPoleSwing(E, seed=env_seed + 1, **SI.SMALL)
    policy = CategoricalPolicy(MLPModel(9, 4, 64, 64), False, 2)
    logger = Logger(E, None)
    agent = PPO(env, policy, logger, Storage((9,), 64, T, E, dev), dev, 1, env_valid=env_v, storage_valid=Storage((9,), 64, T, E, dev), n_steps=T,
                n_envs=E, epoch=2, n_minibatch=2, mini_batch_size=32, gamma=0.99, lmbda=0.95, learning_rate=1e-3, entropy_coef=0.01, seed=0, **kw)
    return agent, env, env_v, logger


def test_ppo_trains_on_the_device_env():
    """PPO.train, two iterations at T = E = 8 with a validation env (both rollouts one mi_env_rollout each): the storage's mirrors are the
    device rings, the poles hang (reward 0, theta near pi) and are truncated after 5 steps, the losses are finite."""
    from mi355.engine import F_DONE, F_REW
    T, E = 8, 8
    agent, env, env_v, logger = _agent(T, E, detect_nan=True)
    assert env.engine is agent.engine and env_v.engine is agent.engine_valid
    calls = []
    real = agent._collect_device
    agent._collect_device = lambda *a: calls.append(a[0]) or real(*a)
    agent.train(2 * T * E)
    assert calls == [env, env_v, env, env_v]
    for st, eng in ((agent.storage, agent.engine), (agent.storage_valid, agent.engine_valid)):
        rew, done = eng.read_field(F_REW), eng.read_field(F_DONE)
        assert np.array_equal(st._rew, rew) and np.array_equal(st._done, done)
        assert (rew == 0).all() and done.any() and set(np.unique(done)) <= {0.0, 1.0}
        assert st.step == 0 and len(st.info_batch) == T
        obs = st.obs_batch.numpy()
        assert obs.shape == (T + 1, E, 9) and np.isfinite(obs).all()
        assert (np.abs(obs[..., 2] - np.pi) < 0.5).all() and (np.abs(obs[..., 0]) < 0.2).all() and (np.abs(obs[..., 1]) > 0.05).any()      # the env really steps
    assert len(logger.rows) == 2
    for name in ("loss_total", "loss_pi", "loss_v", "loss_entropy"):
        assert np.isfinite([row[logger.columns.index(name)] for row in logger.rows]).all(), name
    assert logger.rows[-1][logger.columns.index("num_episodes")] > 0
    agent.engine.close(); agent.engine_valid.close()


@pytest.mark.parametrize("flags", [[], ["--device_env"], ["--device_env", "--resident_rollout"]])
def test_train_cli_runs_the_swing_up(tmp_path, flags):
    """`python train.py --env_name cartpole_swing --param_name mlpmodel [--device_env [--resident_rollout]]` in a fresh child process -- the
    host env with the serial collector, the device chain, the resident rollout: two iterations with the validation env, log rows with
    finite losses and a checkpoint in the reference's format."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "--exp_name", "dev", "--env_name", "cartpole_swing", "--param_name", "mlpmodel",
           "--n_envs", "8", "--n_steps", "16", "--mini_batch_size", "32", "--seed", "3", "--detect_nan", "--num_timesteps", "250",
           "--num_checkpoints", "1"] + flags
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert ("rollout: serial steps", "rollout: device-resident env, one call per rollout",
            "rollout: device-resident env, one kernel launch per rollout")[len(flags)] in r.stdout
    runs = os.listdir(tmp_path / "logs" / "train" / "cartpole_swing" / "dev")
    assert len(runs) == 1 and runs[0].endswith("__seed_3")
    rd = tmp_path / "logs" / "train" / "cartpole_swing" / "dev" / runs[0]
    assert {"hyperparameters.npy", "config.npy", "log-append.csv", "model_256.pth"} <= set(os.listdir(rd))
    assert bool(np.load(rd / "hyperparameters.npy", allow_pickle=True).item().get("resident_rollout", False)) is (len(flags) == 2)
    ck = torch.load(rd / "model_256.pth", map_location="cpu", weights_only=True)
    assert ck["t"] == 256 and ck["model_state_dict"]["fc_policy.weight"].shape == (2, 64)
    assert ck["model_state_dict"]["embedder.model.0.weight"].shape == (256, 9)
    rows = open(rd / "log-append.csv").read().strip().splitlines()
    assert len(rows) == 3 and rows[0].startswith("timesteps,wall_time,num_episodes,max_episode_rewards")
    assert [float(row.split(",")[0]) for row in rows[1:]] == [128.0, 256.0]
    cols = rows[0].split(",")
    for name in ("loss_total", "loss_pi", "loss_v", "loss_entropy"):
        assert np.isfinite([float(row.split(",")[cols.index(name)]) for row in rows[1:]]).all(), name


# ------------------------------------------------------------------------------------------ 6: the resident rollout beside the chain
def test_resident_rollout_beside_the_chain():
    """E = 70 (four 16-env tiles and a 6-row tail), T = 8, from one saved state with the three planted rows: mi_env_rollout, then
    mi_env_rollout_resident.  Same actions, rewards, dones, observations and env state (the env arithmetic is the same code; the case's
    uniforms are clear of every CDF edge, checked on the CPU in tests/test_cartpole_swing_host.py); value / logp within
    test_resident_rollout_beside_the_chain's bound of each other: 16 x the error of torch's own float32 CPU evaluation of the same network
    on the same observations against float64 (resident_inputs.torch_errors: the bound comes from torch, never from the kernel)."""
    import policy_inputs as PI
    import resident_inputs as RI
    c = SI.RESIDENT_CASE
    T, E = c["T"], c["E"]
    flat = RI.params_of(c)
    start = SI.resident_start(c)
    o = SI.oracle_rollout(c)
    eng = _engine(T, E)
    eng.set_params(flat)
    _device_env(eng, c["env_seed"], **SI.SMALL).reset()
    first = eng.env_state()
    eng.env_set_state(*start)                       # (reset() left episode 1 of every env; the planted rows and exactly the replay's bits)
    eng.env_rollout(c["seed"])
    chain = _read(eng)
    eng.env_set_state(*start)
    eng.env_rollout(c["seed"], resident=True)
    res = _read(eng)
    eng.close()
    assert CI.within_ulp(first[0][3:], start[0][3:], 4).all() and (first[2] == 1).all()
    for k in ("act", "rew", "done", "obs", "state", "n_steps", "episode"):
        assert np.array_equal(chain[k], res[k]), k
    assert np.array_equal(res["act"], o["act"]) and np.array_equal(res["done"], o["done"].astype(np.float32)) and o["margin"] >= SI.ENV_MARGIN
    assert SI.within_f32_ulp(res["rew"], o["rew"], 1).all()
    assert res["done"][0, 0] == 1 and (res["rew"][:5, 1] > 0.9).all() and not res["done"][:4, 1:].any() and res["done"][4, 1:].all()
    assert (res["rew"][:, 3:] == 0).all() and (res["rew"][:5, 2] > 0.5).all()
    terr_v, terr_lp = RI.torch_errors(c, flat, res["obs"])
    dv, dl = PI.rel_l2(res["value"].astype(np.float64), chain["value"].astype(np.float64)), PI.rel_l2(res["logp"].astype(np.float64), chain["logp"].astype(np.float64))
    print(f"resident against the chain: value {dv:.3e} = {dv / terr_v:.2f} x torch float32's error, logp {dl:.3e} = {dl / terr_lp:.2f} x (bound: 16 x)")
    assert dv <= 16 * terr_v and dl <= 16 * terr_lp
