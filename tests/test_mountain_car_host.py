"""Host side of the mountain car (common/env/vec_envs.py MountainCarVec / DeviceMountainCar / create_mountain_car, train.py): the numpy
env against trajectories of the reference's own class (tests/golden/g17_mountain_car.npz), the ranges and overrides, the acceptance
rule, the flag and its refusals, and the numpy restatement of the device env's reset stream that the GPU tests compare against."""
import argparse

import numpy as np
import pytest

import mountain_car_inputs as MI


def _args(extra):
    import train
    return train.add_training_args(argparse.ArgumentParser()).parse_args(extra)


# ------------------------------------------------------------------------------------------ the reference's trajectories, bit for bit
@pytest.mark.parametrize("is_valid", [False, True])
def test_mountaincarvec_reproduces_the_reference_trajectory(is_valid):
    """(a): constructor -> reset() -> 40 steps at n_envs = 6, max_steps = 5 (every env is reset 8 times).  Every observation, reward and
    done of the reference's class, bit for bit: that includes the generator's position across the constructor's own draw, the caller's
    reset and every block reset, and -- validation ranges -- the rejection sampling of the start space."""
    from common.env.vec_envs import create_mountain_car
    z, p = MI.golden(), "a_valid/" if is_valid else "a_train/"
    env = create_mountain_car({"n_envs": 6, "max_steps": 5}, is_valid, seed=int(z["seeds"][0]))
    obs0 = env.reset()
    assert obs0.dtype == np.float64 and obs0.tobytes() == z[p + "obs0"].tobytes()
    assert (obs0[:, 1] == 0).all() and (obs0[:, 4] <= obs0[:, 3]).all()
    for t, a in enumerate(z[p + "act"]):
        obs, rew, done, info = env.step(a)
        assert np.ascontiguousarray(obs).tobytes() == z[p + "obs"][t].tobytes(), t
        assert np.asarray(rew, np.float64).tobytes() == z[p + "rew"][t].tobytes(), t
        assert done.dtype == bool and np.array_equal(done, z[p + "done"][t]), t
        assert info.has("env_reward") and np.array_equal(info.column("env_reward"), rew) and info[0] == {"env_reward": -1.0}
    assert z[p + "done"].sum() == 48


@pytest.mark.parametrize("sparse", [True, False])
def test_mountaincarvec_reproduces_the_teacher_forced_step(sparse):
    """(b) / (c): one step at E = 70 from assigned states -- interior rows with all three actions, rows 1e-6 inside / outside the goal,
    a row beyond the goal below goal_velocity, rows on the left wall, rows clipped at the right wall and at +-max_speed, rows one and two
    steps short of max_steps -- state (the reset rows too: the same generator position), reward and done bit for bit."""
    from common.env.vec_envs import MountainCarVec
    c = MI.one_step_case(sparse)
    env = MountainCarVec(MI.ONE_STEP_E, seed=c["seed"], **c["kw"])
    env.state, env.n_steps, env.terminated = c["state"].copy(), c["n_steps"].astype(np.float64), np.full(MI.ONE_STEP_E, False)
    before = c["state"].copy()
    obs, rew, done, info = env.step(c["act"])
    assert np.array_equal(before, c["state"])
    assert np.ascontiguousarray(obs).tobytes() == c["out_state"].tobytes()
    assert np.asarray(rew, np.float64).tobytes() == c["rew"].tobytes() and np.array_equal(info.column("env_reward"), rew)
    assert np.array_equal(done, c["done"]) and set(np.nonzero(done)[0]) == MI.ONE_STEP_ENDED
    assert ((rew == -1).all() if sparse else (rew > -1).all() and (rew < 0.01).all())
    assert obs[57, 0] == 1.0 and (obs[54:56, :2] == (-1.2, 0.0)).all() and obs[58, 1] == 0.07 and obs[59, 1] == -0.07


# ------------------------------------------------------------------------------------------ construction
def test_create_mountain_car_ranges_and_overrides():
    """The reference's param_range (mountain_car_pre_vec.py:312-328): first values for training, second for validation; `<name>` /
    `<name>_v` override them; max_steps and sparse_rewards come from the hyper-parameters; the three range assertions are kept."""
    from common.env.vec_envs import MOUNTAIN_CAR_PARAM_RANGE, MountainCarVec, create_mountain_car
    assert MOUNTAIN_CAR_PARAM_RANGE == {"goal_velocity": [0], "left_boundary": [-1.2], "min_right_boundary": [0.6, 1.], "max_right_boundary": [1., 5.],
                                        "max_speed": [0.07], "min_goal_position": [0, 0.6], "max_goal_position": [0.6, 3], "force": [0.001],
                                        "min_gravity": [0.001, 0.0015], "max_gravity": [0.0015, 0.0025], "sparse_rewards": [True]}
    tr, va = create_mountain_car({}, False, seed=1, n_envs=4), create_mountain_car({}, True, seed=1, n_envs=4)
    assert type(tr) is MountainCarVec and tr.n_envs == 4 and tr.max_steps == 500 and tr.sparse_rewards is True
    assert np.array_equal(tr.low, [-0.6, 0, 0.001, 0.6, 0]) and np.array_equal(tr.high, [-0.4, 0, 0.0015, 1.0, 0.6])
    assert np.array_equal(va.low, [-0.6, 0, 0.0015, 1.0, 0.6]) and np.array_equal(va.high, [-0.4, 0, 0.0025, 5.0, 3])
    for e in (tr, va):
        assert (e.goal_velocity, e.left_boundary, e.max_speed, e.force) == (0, -1.2, 0.07, 0.001)
        assert e.observation_space.shape == (5,) and e.action_space.n == 3 and e.low.dtype == np.float64
    assert create_mountain_car({"n_envs": 16}, False).n_envs == 16 and create_mountain_car({}, False).n_envs == 32
    hp = {"max_steps": 77, "sparse_rewards": False, "max_speed": 0.05, "max_speed_v": 0.06, "max_gravity_v": 0.002, "force_v": 0.002}
    tr, va = create_mountain_car(hp, False, n_envs=4), create_mountain_car(hp, True, n_envs=4)
    assert tr.max_steps == va.max_steps == 77 and tr.sparse_rewards is False and va.sparse_rewards is True      # (`sparse_rewards_v` would set it)
    assert (tr.max_speed, va.max_speed, tr.force, va.force) == (0.05, 0.06, 0.001, 0.002)
    assert tr.high[2] == 0.0015 and va.high[2] == 0.002
    for bad, word in (({"left_boundary": -0.5}, "min_start_position"), ({"min_right_boundary": -0.5, "min_goal_position": -1.0}, "max_start_position"),
                      ({"max_goal_position": 1.5}, "max_goal_position")):
        with pytest.raises(AssertionError, match=word):
            create_mountain_car(bad, False, n_envs=4)
    with pytest.raises(Exception, match="n_envs"):
        create_mountain_car({}, False, n_envs=1)


@pytest.mark.parametrize("is_valid", [False, True])
@pytest.mark.parametrize("hp", [{}, "mountain_car", {"max_steps": 123, "goal_velocity": 0.01, "max_speed_v": 0.05, "sparse_rewards": False}])
def test_create_mountain_car_device_carries_the_host_envs_parameters(hp, is_valid):
    import train
    from common.env.vec_envs import DeviceMountainCar, MountainCarVec, create_mountain_car
    if hp == "mountain_car":
        hp = train.get_hyperparams("mountain_car")
        assert hp["n_envs"] == 16 and hp["n_steps"] == 16
    host = create_mountain_car(hp, is_valid, seed=3, n_envs=6)
    dev = create_mountain_car(hp, is_valid, seed=3, n_envs=6, device=True)
    assert type(host) is MountainCarVec and type(create_mountain_car(hp, is_valid, seed=3, n_envs=6, device=False)) is MountainCarVec
    assert type(dev) is DeviceMountainCar and dev.on_device is True and not getattr(host, "on_device", False)
    assert dev.low.dtype == np.float64 and dev.low.tobytes() == host.low.tobytes() and dev.high.tobytes() == host.high.tobytes()
    for name in ("left_boundary", "max_speed", "force", "goal_velocity"):
        assert np.float64(getattr(dev, name)).tobytes() == np.float64(getattr(host, name)).tobytes(), name
    assert dev.max_steps == host.max_steps and dev.sparse_rewards is host.sparse_rewards and dev.n_envs == host.n_envs == 6 and dev.seed == 3
    assert dev.observation_space.shape == host.observation_space.shape == (5,) and dev.action_space.n == host.action_space.n == 3
    with pytest.raises(RuntimeError, match="attach"):
        dev.reset()


def test_acceptance_probability_and_its_refusal():
    """P(goal_position <= right_boundary) in closed form against a Monte-Carlo estimate; 1 for the training ranges, 19/24 for the
    validation ranges; a range set below 1/2 is refused by name by both classes, at construction."""
    from common.env.vec_envs import DeviceMountainCar, MountainCarVec, mountain_car_acceptance
    assert mountain_car_acceptance(0, 0.6, 0.6, 1.0) == pytest.approx(1.0, abs=1e-12)
    assert mountain_car_acceptance(0.6, 3, 1.0, 5.0) == pytest.approx(19 / 24, abs=1e-12)
    assert mountain_car_acceptance(2, 3, 0.6, 1.0) == 0 and mountain_car_acceptance(0.5, 0.5, 0.6, 0.6) == 1 and mountain_car_acceptance(0.7, 0.7, 0.6, 0.6) == 0
    assert mountain_car_acceptance(0.5, 0.5, 0.0, 1.0) == pytest.approx(0.5) and mountain_car_acceptance(0.0, 1.0, 0.25, 0.25) == pytest.approx(0.25)
    rng = np.random.default_rng(0)
    for a, b, c, d in ((0.6, 3, 1, 5), (0, 4, 1, 3), (1, 2, 0, 5), (0, 1, 0, 1), (0.5, 3, 0.6, 5)):
        mc = (rng.uniform(a, b, 400000) <= rng.uniform(c, d, 400000)).mean()
        assert abs(mountain_car_acceptance(a, b, c, d) - mc) < 4e-3, (a, b, c, d)      # (binomial sigma <= 8e-4)
    for cls in (MountainCarVec, DeviceMountainCar):
        cls(4)                                                                           # the constructor defaults: 0.5 .. 3 against 0.6 .. 5
        with pytest.raises(ValueError, match="mountain_car.*goal_position <= right_boundary.*max_goal_position 4.9"):
            cls(4, min_goal_position=3.0, max_goal_position=4.9, min_right_boundary=0.6, max_right_boundary=5)
        with pytest.raises(ValueError, match="probability"):
            cls(4, min_goal_position=2.0, max_goal_position=3.0, min_right_boundary=0.6, max_right_boundary=3.0)      # (the reference: for ever)


# ------------------------------------------------------------------------------------------ train.py
def test_make_env_builds_the_mountain_car():
    import train
    from common.env.vec_envs import DeviceMountainCar, MountainCarVec
    hp = train.get_hyperparams("mountain_car")
    for flag, cls in (([], MountainCarVec), (["--device_env"], DeviceMountainCar)):
        args = _args(["--env_name", "mountain_car", "--param_name", "mountain_car"] + flag)
        for valid in (False, True):
            env = train.make_env("mountain_car", 16, 1, 3, args, hp, is_valid=valid)
            assert type(env) is cls and env.n_envs == 16 and not hasattr(env, "env_groups")
    args = _args(["--env_name", "mountain_car", "--param_name", "mountain_car", "--rollout_groups", "4"])
    assert type(train.make_env("mountain_car", 256, 1, 3, args, hp)) is MountainCarVec      # no env groups: the serial single env


def test_train_device_env_admits_mountain_car_and_still_refuses_others(monkeypatch):
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    train.check_device_env("mountain_car", {}, "ppo")
    train.check_device_env("cartpole_swing", {}, "ppo-pure")
    for name in ("coinrun", "acrobot", "synthetic"):
        with pytest.raises(NotImplementedError, match=name):
            train.check_device_env(name, {}, "ppo")
    mc = ["--env_name", "mountain_car", "--param_name", "mountain_car", "--device_env"]

    class Reached(Exception):
        pass

    def built(env_name, *a, **k):
        raise Reached(env_name)
    monkeypatch.setattr(train, "make_env", built)
    with pytest.raises(Reached, match="mountain_car"):                                   # past every refusal, at the env's construction
        train.train_ppo(_args(mc))
    monkeypatch.setattr(train, "make_env", lambda *a, **k: pytest.fail("an env was built"))
    with pytest.raises(NotImplementedError, match="coinrun"):
        train.train_ppo(_args(["--env_name", "coinrun", "--param_name", "hard-500", "--device_env"]))
    base = train.get_hyperparams
    monkeypatch.setattr(train, "get_hyperparams", lambda name: dict(base(name), recurrent=True))
    with pytest.raises(NotImplementedError, match="recurrent"):
        train.train_ppo(_args(mc))
    monkeypatch.setattr(train, "get_hyperparams", base)
    with pytest.raises(NotImplementedError, match="IPL"):
        train.train_ppo(_args(mc + ["--algo", "IPL"]))
    with pytest.raises(NotImplementedError, match="sae"):
        train.train_ppo(_args(mc + ["--algo", "sae"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        train.train_ppo(_args(mc))


# ------------------------------------------------------------------------------------------ the device env's reset stream, restated
def test_reset_stream_restatement():
    """philox_u53 with the attempt counter is built on the oracle's Philox; fresh_state draws attempts until goal <= right wall, counts
    them, and after MAX_ATTEMPTS rejected attempts keeps the last draw with goal_position = right_boundary."""
    from oracle.philox import philox4x32_10
    seed = 0x0123456789abcdef
    env, ep = np.repeat(np.arange(64), 8), np.tile(np.arange(8), 64)
    u = MI.philox_u53(seed, env, ep, 0)
    assert u.shape == (512, 5) and u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53)) and len(np.unique(u)) == u.size
    assert (MI.philox_u53(seed, env, ep, 1) != u).all() and (MI.philox_u53(seed + 1, env, ep, 0) != u).all()
    w = philox4x32_10([[5, 7, 2, 3 * 4 + 2]], [[seed & 0xffffffff, seed >> 32]])[0]      # env 5, episode 2^33 + 7, attempt 4, block 2
    assert MI.philox_u53(seed, 5, 2 ** 33 + 7, 4)[0, 4] == ((int(w[0]) >> 5) * 2 ** 26 + (int(w[1]) >> 6)) / 2.0 ** 53
    w = philox4x32_10([[5, 7, 0, 1]], [[seed & 0xffffffff, seed >> 32]])[0]              # attempt 0, block 1: columns 2 and 3
    assert MI.philox_u53(seed, 5, 7, 0)[0, 3] == ((int(w[2]) >> 5) * 2 ** 26 + (int(w[3]) >> 6)) / 2.0 ** 53
    va = MI.ReplayMountainCar(4, seed=1, **MI.VALID)
    s, att = MI.fresh_state(va.low, va.high, seed, env, ep)
    assert (s >= va.low).all() and (s <= va.high).all() and (s[:, 1] == 0).all() and (s[:, 4] <= s[:, 3]).all()
    assert att.min() == 1 and att.max() >= 3 and 0.12 < (att > 1).mean() < 0.30                 # 5 / 24 of the first attempts are rejected
    first = va.low + (va.high - va.low) * u
    one = att == 1
    assert np.array_equal(s[one], first[one]) and (first[~one, 4] > first[~one, 3]).all()
    two = att == 2
    assert np.array_equal(s[two], (va.low + (va.high - va.low) * MI.philox_u53(seed, env, ep, 1))[two])
    low, high = np.array([-0.6, 0, 0.001, 0.6, 2.0]), np.array([-0.4, 0, 0.002, 1.0, 3.0])      # never accepted: the bounded fallback
    s, att = MI.fresh_state(low, high, seed, np.arange(3), 1)
    last = low + (high - low) * MI.philox_u53(seed, np.arange(3), 1, MI.MAX_ATTEMPTS - 1)
    assert (att == MI.MAX_ATTEMPTS).all() and np.array_equal(s[:, :4], last[:, :4]) and np.array_equal(s[:, 4], last[:, 3])
    s3, att3 = MI.fresh_state(low, high, seed, np.arange(3), 1, max_attempts=3)
    assert (att3 == 3).all() and np.array_equal(s3[:, :4], (low + (high - low) * MI.philox_u53(seed, np.arange(3), 1, 2))[:, :4])


def test_replay_env_is_mountaincarvec_until_the_first_reset():
    """The CPU replay the GPU tests use is MountainCarVec.step itself: on the one-step case it gives the fixture's numbers bit for bit
    on every row that goes on (both reward modes), the margin rule holds on every row, and its resets are the Philox restatement's."""
    from common.env.vec_envs import MountainCarVec
    for sparse in (True, False):
        c = MI.one_step_case(sparse)
        rp = MI.ReplayMountainCar(MI.ONE_STEP_E, seed=c["seed"], **c["kw"])
        assert (rp.episode == 1).all()
        rp.load(c["state"], c["n_steps"], c["episode"])
        s, rew, done, _ = rp.step(c["act"])
        go = ~done
        assert np.array_equal(done, c["done"]) and np.array_equal(s[go], c["out_state"][go]) and np.array_equal(rew, c["rew"])
        assert rp.margin_ok().all()
        ended = np.nonzero(done)[0]
        assert set(ended) == MI.ONE_STEP_ENDED
        assert np.array_equal(rp.episode[ended], c["episode"][ended] + 1) and np.array_equal(rp.episode[go], c["episode"][go])
        want, _ = MI.fresh_state(rp.low, rp.high, c["seed"], ended, c["episode"][ended] + 1)
        assert np.array_equal(s[ended], want) and (rp.n_steps[ended] == 0).all()
    a = MI.ReplayMountainCar(6, seed=3, max_steps=50, **MI.VALID)
    b = MountainCarVec(6, seed=3, max_steps=50, **MI.VALID)
    b.state = a.state.copy()
    for act in np.random.default_rng(1).integers(0, 3, (40, 6)):
        (sa, ra, da, _), (sb, rb, db, _) = a.step(act), b.step(act)
        assert np.array_equal(sa, sb) and np.array_equal(ra, rb) and not da.any() and not db.any()
