"""Host side of the swing-up cart-pole (common/env/vec_envs.py CartPoleSwingVec / DeviceCartPoleSwing / create_cartpole_swing /
create_vector_env, train.py): the numpy env against trajectories of the reference's own class (tests/golden/g18_cartpole_swing.npz), the
balance class's step against the reference's (a pin), what `--env_name cartpole_swing` builds, the ranges, and the replay the GPU tests
compare against.  Rewards are compared by value: a row that ends beyond the edge with the clamp on yields -0.0 on both sides."""
import argparse
import os
import re

import numpy as np
import pytest

import cartpole_inputs as CI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "train-procgen-pytorch_amd")


def _args(extra):
    import train
    return train.add_training_args(argparse.ArgumentParser()).parse_args(extra)


# ------------------------------------------------------------------------------------------ the reference's trajectories, bit for bit
@pytest.mark.parametrize("is_valid", [False, True])
def test_cartpoleswingvec_reproduces_the_reference_trajectory(is_valid):
    """(a): constructor -> reset() -> 40 steps at n_envs = 6, max_steps = 5 (every env is reset 8 times).  Every observation, reward and
    done of the reference's class: that includes the generator's position across the constructor's own draw, the caller's reset and every
    block reset."""
    import cartpole_swing_inputs as SI
    from common.env.vec_envs import create_cartpole_swing
    z, p = SI.golden(), "a_valid/" if is_valid else "a_train/"
    env = create_cartpole_swing({"n_envs": 6, "max_steps": 5}, is_valid, seed=int(z["seeds"][0]))
    obs0 = env.reset()
    assert obs0.dtype == np.float64 and np.array_equal(obs0, z[p + "obs0"])
    assert (np.abs(obs0[:, 2] - np.pi) <= 0.05).all() and (np.abs(obs0[:, [0, 1, 3]]) <= 0.05).all()
    for t, a in enumerate(z[p + "act"]):
        obs, rew, done, info = env.step(a)
        assert obs.dtype == np.float64 and np.array_equal(obs, z[p + "obs"][t]), t
        assert rew.dtype == np.float64 and np.array_equal(rew, z[p + "rew"][t]), t
        assert done.dtype == bool and np.array_equal(done, z[p + "done"][t]), t
        assert info.has("env_reward") and np.array_equal(info.column("env_reward"), rew) and info[0] == {"env_reward": rew[0]}
    assert z[p + "done"].sum() == 48 and (z[p + "rew"] == 0).all()      # the pole stays below the horizontal for 5 steps


def test_cartpoleswingvec_reproduces_the_teacher_forced_step():
    """(b): one step at E = 70 from assigned states -- interior rows over several turns of theta with both actions, rows 1e-6 inside /
    outside +-h_range, rows 1e-6 either side of +-pi/2 (the reward clamp), rows at theta = +-0.3 that the balance task would end, rows
    one and two steps short of max_steps -- state (the reset rows too: the same generator position), reward and done."""
    import cartpole_swing_inputs as SI
    from common.env.vec_envs import CartPoleSwingVec
    c = SI.one_step_case()
    env = CartPoleSwingVec(SI.ONE_STEP_E, seed=c["seed"], **c["kw"])
    env.state, env.n_steps, env.terminated = c["state"].copy(), c["n_steps"].astype(np.float64), np.full(SI.ONE_STEP_E, False)
    before = c["state"].copy()
    obs, rew, done, info = env.step(c["act"])
    assert np.array_equal(before, c["state"])
    assert obs.dtype == np.float64 and np.array_equal(obs, c["out_state"])
    assert rew.dtype == np.float64 and np.array_equal(rew, c["rew"]) and np.array_equal(info.column("env_reward"), rew)
    assert np.array_equal(done, c["done"]) and set(np.nonzero(done)[0]) == SI.ONE_STEP_ENDED and not done[58:60].any()
    assert (rew > 0).sum() >= 20 and (rew == 0).sum() >= 20 and (rew[~done] >= 0).all() and (rew <= 1).all()
    assert (rew[[51, 53]] < 0).all() and (rew[[51, 53]] > -1e-6).all()      # just beyond the edge with the pole up: rx is just below 0
    for row, clamped in SI.CLAMP_ROWS.items():
        assert (rew[row] == 0) if clamped else (0 < rew[row] < 2e-6), row
    assert rew[58] == rew[59] == np.cos(0.3)


def test_cartpolevec_step_reproduces_the_reference_balance_class():
    """(c), a pin: CartPoleVec.step on cartpole_inputs.one_step_case() against the reference's CartPoleVecEnv -- done equal, and the rows
    that go on bit for bit (the ended rows hold each class's own block draw: CartPoleVec's constructor draws no block, the reference's
    one, so the generators stand at different positions)."""
    import cartpole_swing_inputs as SI
    from common.env.vec_envs import CartPoleVec
    z, c = SI.golden(), CI.one_step_case()
    env = CartPoleVec(CI.ONE_STEP_E, **c["kw"])
    env.state, env.n_steps, env.terminated = c["state"].copy(), c["n_steps"].astype(np.float64), np.full(CI.ONE_STEP_E, False)
    obs, _, done, _ = env.step(c["act"])
    assert np.array_equal(done, z["c/done"]) and set(np.nonzero(done)[0]) == {51, 53, 55, 57, 58, 59}
    assert np.array_equal(obs[~done], z["c/out_state"][~done])


# ------------------------------------------------------------------------------------------ construction
def test_create_cartpole_swing_ranges_and_overrides():
    """The reference's param_range (cartpole_swing_pre_vec.py:313-327): create_cartpole's ten mass / length / gravity / force ranges and
    h_range [2.4], no `degrees`; max_steps 1000 unless the hyper-parameters give one; the pole hangs down."""
    from common.env.vec_envs import CARTPOLE_PARAM_RANGE, CARTPOLE_SWING_PARAM_RANGE, CartPoleSwingVec, create_cartpole_swing
    assert CARTPOLE_SWING_PARAM_RANGE == {"h_range": [2.4], "min_gravity": [9.8, 10.4], "max_gravity": [10.4, 24.8], "min_pole_length": [0.5, 1.0],
                                          "max_pole_length": [1.0, 2.0], "min_cart_mass": [1.0, 2.], "max_cart_mass": [1.5, 3.],
                                          "min_pole_mass": [0.1, .2], "max_pole_mass": [0.2, .4], "min_force_mag": [10.], "max_force_mag": [10.]}
    assert {k: v for k, v in CARTPOLE_PARAM_RANGE.items() if k != "degrees"} == CARTPOLE_SWING_PARAM_RANGE
    tr, va = create_cartpole_swing({}, False, seed=1, n_envs=4), create_cartpole_swing({}, True, seed=1, n_envs=4)
    assert type(tr) is CartPoleSwingVec and tr.n_envs == 4 and tr.max_steps == va.max_steps == 1000 and tr.x_threshold == va.x_threshold == 2.4
    assert np.array_equal(tr.low, [-0.05, -0.05, np.pi - 0.05, -0.05, 9.8, 0.5, 1.0, 0.1, 10.])
    assert np.array_equal(tr.high, [0.05, 0.05, np.pi + 0.05, 0.05, 10.4, 1.0, 1.5, 0.2, 10.])
    assert np.array_equal(va.low, [-0.05, -0.05, np.pi - 0.05, -0.05, 10.4, 1.0, 2., .2, 10.])
    assert np.array_equal(va.high, [0.05, 0.05, np.pi + 0.05, 0.05, 24.8, 2.0, 3., .4, 10.])
    for e in (tr, va):
        assert e.low[2] == np.pi - 0.05 and e.low.dtype == e.high.dtype == np.float64 and not hasattr(e, "theta_threshold")
        assert e.observation_space.shape == (9,) and e.action_space.n == 2
    assert create_cartpole_swing({"n_envs": 16}, False).n_envs == 16 and create_cartpole_swing({}, False).n_envs == 32
    hp = {"max_steps": 77, "h_range": 1.0, "h_range_v": 1.8, "max_gravity_v": 12.0, "degrees": 9}
    tr, va = create_cartpole_swing(hp, False, n_envs=4), create_cartpole_swing(hp, True, n_envs=4)
    assert tr.max_steps == va.max_steps == 77 and (tr.x_threshold, va.x_threshold) == (1.0, 1.8) and tr.high[4] == 10.4 and va.high[4] == 12.0
    with pytest.raises(Exception, match="n_envs"):
        create_cartpole_swing({}, False, n_envs=1)


@pytest.mark.parametrize("is_valid", [False, True])
@pytest.mark.parametrize("hp", [{}, "mlpmodel", {"max_steps": 123, "h_range": 1.5, "min_pole_length_v": 1.25}])
def test_host_and_device_class_carry_the_same_parameters(hp, is_valid):
    import train
    from common.env.vec_envs import CartPoleSwingVec, DeviceCartPoleSwing, create_cartpole_swing
    if hp == "mlpmodel":
        hp = train.get_hyperparams("mlpmodel")
        assert hp["n_envs"] == 1024 and hp["n_steps"] == 256 and "max_steps" not in hp
    host = create_cartpole_swing(hp, is_valid, seed=3, n_envs=6)
    dev = create_cartpole_swing(hp, is_valid, seed=3, n_envs=6, device=True)
    assert type(host) is CartPoleSwingVec and type(dev) is DeviceCartPoleSwing and dev.on_device is True and not getattr(host, "on_device", False)
    assert dev.low.dtype == np.float64 and dev.low.tobytes() == host.low.tobytes() and dev.high.tobytes() == host.high.tobytes()
    assert dev.low[2] == np.pi - 0.05 and dev.high[2] == np.pi + 0.05
    assert np.float64(dev.x_threshold).tobytes() == np.float64(host.x_threshold).tobytes()
    assert dev.max_steps == host.max_steps == hp.get("max_steps", 1000) and dev.n_envs == host.n_envs == 6 and dev.seed == 3
    assert dev.observation_space.shape == host.observation_space.shape == (9,) and dev.action_space.n == host.action_space.n == 2
    with pytest.raises(RuntimeError, match="attach"):
        dev.reset()


# ------------------------------------------------------------------------------------------ train.py
def test_make_env_builds_the_swing_up_under_its_name():
    """`--env_name cartpole_swing` builds the swing-up, on the host and with --device_env, for the training and the validation ranges, never
    as env groups; max_steps is the class's 1000 unless the hyper-parameters give one.  (Before create_vector_env the name fell into the
    cartpole* row and built CartPoleVec, the balance task.)"""
    import train
    from common.env import vec_envs
    from common.env.vec_envs import EnvGroups
    hp = train.get_hyperparams("mlpmodel")
    base = ["--env_name", "cartpole_swing", "--param_name", "mlpmodel"]
    for flag, name in (([], "CartPoleSwingVec"), (["--device_env"], "DeviceCartPoleSwing")):
        assert type(train.make_env("cartpole_swing", 16, 1, 2, _args(base + flag), hp)).__name__ == name      # (not CartPoleVec / DeviceCartPole)
        cls = getattr(vec_envs, name)
        args = _args(base + flag)
        for valid in (False, True):
            env = train.make_env("cartpole_swing", 16, 1, 2, args, hp, is_valid=valid)
            assert type(env) is cls and env.n_envs == 16 and not hasattr(env, "env_groups") and not isinstance(env, EnvGroups)
            assert env.max_steps == 1000 and env.low[2] == np.pi - 0.05 and env.high[4] == (24.8 if valid else 10.4)
            assert train.make_env("cartpole_swing", 16, 1, 2, args, dict(hp, max_steps=50), is_valid=valid).max_steps == 50
        for groups in ("4", "0", "2"):
            env = train.make_env("cartpole_swing", 256, 1, 2, _args(base + flag + ["--rollout_groups", groups]), hp)
            assert type(env) is cls and not isinstance(env, EnvGroups)


def test_every_other_cartpole_name_still_builds_the_balance_task():
    import train
    from common.env.vec_envs import CartPoleVec, DeviceCartPole, MountainCarVec, create_vector_env, vector_env
    hp = train.get_hyperparams("cartpole")
    for name in ("cartpole", "cartpole_position", "cartpole-cont", "cartpole_swing_up", "cartpole_swing2"):
        assert type(train.make_env(name, 16, 1, 2, _args(["--env_name", name]), hp)) is CartPoleVec, name
        assert type(train.make_env(name, 16, 1, 2, _args(["--env_name", name, "--device_env"]), hp, is_valid=True)) is DeviceCartPole, name
        assert type(create_vector_env(name, hp, n_envs=4)) is CartPoleVec
    assert type(create_vector_env("mountain_car", {}, n_envs=4)) is MountainCarVec
    assert vector_env("cartpole_swing").label == "the cart-pole (cartpole*)"           # the table itself is as it was


def test_train_reaches_the_env_construction_with_the_flags(monkeypatch):
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    class Reached(Exception):
        pass

    def built(env_name, *a, **k):
        raise Reached(env_name)
    monkeypatch.setattr(train, "make_env", built)
    for flags in ([], ["--device_env"], ["--device_env", "--resident_rollout"]):
        with pytest.raises(Reached, match="cartpole_swing"):
            train.train_ppo(_args(["--env_name", "cartpole_swing", "--param_name", "mlpmodel"] + flags))


# ------------------------------------------------------------------------------------------ the device side, as far as the CPU sees it
def test_names_in_header_exports_and_engine():
    from mi355 import engine
    header = open(os.path.join(ROOT, "include", "mi355ppo.h")).read()
    assert re.search(r"int mi_env_cartpole_swing_create\(mi_ctx\* ctx, const mi_cartpole_swing_params\* params, uint64_t seed\);", header)
    assert "mi_env_cartpole_swing_create" in engine.EXPORTS
    src = open(os.path.join(PKG, "mi355", "engine.py")).read()
    assert "self.lib.mi_env_cartpole_swing_create" in src and hasattr(engine.Engine, "env_cartpole_swing_create")
    fields = dict(engine._CartPoleSwingParams._fields_)
    assert list(f for f, _ in engine._CartPoleSwingParams._fields_) == ["low", "high", "x_threshold", "max_steps"] and fields["low"]._length_ == 9


def test_replay_env_is_cartpoleswingvec_until_the_first_reset():
    """The CPU replay the GPU tests use is CartPoleSwingVec.step itself: on the one-step case it gives the fixture's numbers on every row
    that goes on, and its resets are cartpole_inputs.fresh_state -- the cart-pole's Philox stream -- with the swing-up's ranges."""
    import cartpole_swing_inputs as SI
    c = SI.one_step_case()
    rp = SI.ReplayCartPoleSwing(SI.ONE_STEP_E, seed=c["seed"], **c["kw"])
    assert (rp.episode == 1).all()
    first = CI.fresh_state(rp.low, rp.high, c["seed"], np.arange(SI.ONE_STEP_E), 1)
    assert np.array_equal(rp.state, first) and (np.abs(first[:, 2] - np.pi) <= 0.05).all() and (first >= rp.low).all() and (first <= rp.high).all()
    rp.load(c["state"], c["n_steps"], c["episode"])
    s, rew, done, _ = rp.step(c["act"])
    go = ~done
    assert np.array_equal(done, c["done"]) and np.array_equal(s[go], c["out_state"][go]) and np.array_equal(rew, c["rew"])
    assert np.array_equal(rp.post[go], c["out_state"][go]) and rp.margin() >= 0.9e-6      # rows 50-53 land 1e-6 from +-h_range
    ended = np.nonzero(done)[0]
    assert np.array_equal(rp.episode[ended], c["episode"][ended] + 1) and np.array_equal(rp.episode[go], c["episode"][go])
    assert np.array_equal(s[ended], CI.fresh_state(rp.low, rp.high, c["seed"], ended, c["episode"][ended] + 1)) and (rp.n_steps[ended] == 0).all()


def test_the_planted_rollout_case_on_the_cpu():
    """The rollout case of the GPU tests (T = 8, E = 6 and E = 70, max_steps = 5, env seeds 21) on random actions: env 0 ends at step 1
    whatever the action, env 1 earns more than 0.9 a step and is truncated at step 5, env 2 (theta = 0.3) goes on until step 5, every other
    env hangs and earns 0; every post-step x keeps ENV_MARGIN from +-h_range."""
    import cartpole_swing_inputs as SI
    for E, act_seed in ((6, 0), (6, 1), (70, 2)):
        rp = SI.ReplayCartPoleSwing(E, seed=21, **SI.SMALL)
        s0 = SI.plant(rp.state)
        act = np.random.default_rng(act_seed).integers(0, 2, (8, E))
        obs, rew, done, beyond, margin = SI.replay(rp, s0, np.zeros(E, np.int32), np.ones(E, np.int64), act)
        assert margin >= SI.ENV_MARGIN
        assert done[0, 0] and beyond[0, 0] and rew[0, 0] == 0
        assert (rew[:5, 1] > 0.9).all() and done[4, 1] and not beyond[4, 1] and not done[:4, 1].any()
        assert not done[:4, 2].any() and done[4, 2] and (rew[:5, 2] > 0.5).all()
        assert (rew[:, 3:] == 0).all() and (rew[5:, :3] == 0).all() and done[4, 3:].all() and beyond.sum() == 1


def test_the_resident_case_is_clear_of_sampler_edges_on_the_cpu():
    """The float64 rollout of the resident-beside-the-chain case: no sampler uniform within resident_inputs.U_CLEAR of a CDF edge (two fp32
    evaluations of the policy pick the same actions), both actions occur, the planted rows behave as planted, the margin holds."""
    import cartpole_swing_inputs as SI
    import resident_inputs as RI
    o = SI.oracle_rollout()
    assert o["udist"].min() >= RI.U_CLEAR, o["udist"].min()
    assert o["margin"] >= SI.ENV_MARGIN and sorted(np.unique(o["act"])) == [0, 1]
    assert o["done"][0, 0] and o["beyond"][0, 0] and o["beyond"].sum() == 1
    assert (o["rew"][:5, 1] > 0.9).all() and o["done"][4, 1:].all() and not o["done"][:4, 1:].any()
    assert (o["rew"][:, 3:] == 0).all() and (o["rew"][:5, 2] > 0.5).all()
