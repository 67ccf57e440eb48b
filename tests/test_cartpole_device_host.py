"""Host side of the device-resident cart-pole (train.py --device_env, common/env/vec_envs.py DeviceCartPole): the flag, the refusals,
the parameters the device env is created with, and the numpy restatement of its reset stream that the GPU tests compare against."""
import argparse

import numpy as np
import pytest

import cartpole_inputs as CI


def _args(extra):
    import train
    return train.add_training_args(argparse.ArgumentParser()).parse_args(extra)


def test_device_env_flag_parses():
    assert _args([]).device_env is False
    assert _args(["--env_name", "cartpole", "--param_name", "cartpole", "--device_env"]).device_env is True


def test_train_refuses_by_name_before_any_env(monkeypatch):
    """Everything the device env does not cover ends train.py by name before an env, a log directory or an engine exists."""
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(train, "make_env", lambda *a, **k: pytest.fail("an env was built"))
    monkeypatch.setattr(train, "create_logdir_train", lambda *a, **k: pytest.fail("a log directory was made"))
    cart = ["--env_name", "cartpole", "--param_name", "cartpole", "--device_env"]
    with pytest.raises(NotImplementedError, match="coinrun"):
        train.train_ppo(_args(["--env_name", "coinrun", "--param_name", "hard-500", "--device_env"]))
    with pytest.raises(NotImplementedError, match="synthetic"):
        train.train_ppo(_args(["--env_name", "synthetic", "--param_name", "cartpole", "--device_env"]))
    base = train.get_hyperparams
    monkeypatch.setattr(train, "get_hyperparams", lambda name: dict(base(name), recurrent=True))
    with pytest.raises(NotImplementedError, match="recurrent"):
        train.train_ppo(_args(cart))
    monkeypatch.setattr(train, "get_hyperparams", base)
    with pytest.raises(NotImplementedError, match="IPL"):
        train.train_ppo(_args(["--env_name", "cartpole", "--param_name", "ipl_cartpole", "--device_env"]))
    with pytest.raises(NotImplementedError, match="sae"):
        train.train_ppo(_args(cart + ["--algo", "sae"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        train.train_ppo(_args(cart))


@pytest.mark.parametrize("is_valid", [False, True])
@pytest.mark.parametrize("hp", [{}, "cartpole", {"max_steps": 123, "degrees": 10, "h_range_v": 1.1, "min_gravity_v": 11.0}])
def test_create_cartpole_device_carries_the_host_envs_parameters(hp, is_valid):
    """create_cartpole(..., device=True) and the CartPoleVec of the same arguments: same ranges, thresholds (the same bits), max_steps and
    spaces -- for the training ranges, the validation ranges and the `cartpole` set's degrees_v / h_range_v."""
    import train
    from common.env.vec_envs import CartPoleVec, DeviceCartPole, create_cartpole
    if hp == "cartpole":
        hp = train.get_hyperparams("cartpole")
        assert hp["degrees_v"] == 9 and hp["h_range_v"] == 1.8
    host = create_cartpole(hp, is_valid, seed=3, n_envs=6)
    dev = create_cartpole(hp, is_valid, seed=3, n_envs=6, device=True)
    assert type(host) is CartPoleVec and type(create_cartpole(hp, is_valid, seed=3, n_envs=6, device=False)) is CartPoleVec
    assert type(dev) is DeviceCartPole and dev.on_device is True and not getattr(host, "on_device", False)
    assert np.array_equal(dev.low, host.low) and np.array_equal(dev.high, host.high)
    assert dev.low.dtype == np.float64 and dev.high.dtype == np.float64
    assert np.float64(dev.theta_threshold).tobytes() == np.float64(host.theta_threshold).tobytes()
    assert np.float64(dev.x_threshold).tobytes() == np.float64(host.x_threshold).tobytes()
    assert dev.max_steps == host.max_steps and dev.n_envs == host.n_envs == 6 and dev.seed == 3
    assert dev.observation_space.shape == host.observation_space.shape == (9,) and dev.action_space.n == host.action_space.n == 2
    if is_valid and "h_range_v" in hp:
        assert dev.x_threshold == hp["h_range_v"]
    with pytest.raises(RuntimeError, match="attach"):
        dev.reset()


def test_one_env_builds_the_device_env_only_with_the_flag():
    import train
    from common.env.vec_envs import CartPoleVec, DeviceCartPole
    hp = train.get_hyperparams("cartpole")
    for flag, cls in (([], CartPoleVec), (["--device_env"], DeviceCartPole)):
        args = _args(["--env_name", "cartpole", "--param_name", "cartpole"] + flag)
        assert type(train.make_env("cartpole", 8, 1, 2, args, hp)) is cls
        assert type(train.make_env("cartpole", 8, 1, 2, args, hp, is_valid=True)) is cls


def test_philox_u53_restatement():
    """The 53-bit uniform: in [0, 1), a multiple of 2^-53, reproducible, different between neighbouring envs, episodes and seeds, built on
    the oracle's Philox (the first uniform of a row is words 0 and 1 of block 0)."""
    from oracle.philox import philox4x32_10
    seed = 0x0123456789abcdef
    env, ep = np.repeat(np.arange(64), 8), np.tile(np.arange(8), 64)
    u = CI.philox_u53(seed, env, ep)
    assert u.shape == (512, 9) and u.dtype == np.float64
    assert (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))
    assert np.array_equal(u, CI.philox_u53(seed, env, ep))
    g = u.reshape(64, 8, 9)
    assert (g[1:] != g[:-1]).all() and (g[:, 1:] != g[:, :-1]).all()
    assert (CI.philox_u53(seed + 1, env, ep) != u).all()
    assert len(np.unique(u)) == u.size
    assert abs(u.mean() - 0.5) < 0.02
    w = philox4x32_10([[5, 7, 0, 0]], [[seed & 0xffffffff, seed >> 32]])[0]
    assert CI.philox_u53(seed, 5, 7)[0, 0] == ((int(w[0]) >> 5) * 2 ** 26 + (int(w[1]) >> 6)) / 2.0 ** 53
    hi = CI.philox_u53(seed, 3, 2 ** 33 + 6)                      # the episode's high word is part of the counter
    assert (hi != CI.philox_u53(seed, 3, 6)).all()
    w = philox4x32_10([[3, 6, 2, 4]], [[seed & 0xffffffff, seed >> 32]])[0]
    assert hi[0, 8] == ((int(w[0]) >> 5) * 2 ** 26 + (int(w[1]) >> 6)) / 2.0 ** 53


def test_replay_env_is_cartpolevec_until_the_first_reset():
    """The CPU replay the GPU tests use is CartPoleVec.step itself: from the same state it gives CartPoleVec's numbers bit for bit as long
    as no env ends, and its resets are the Philox restatement's."""
    from common.env.vec_envs import CartPoleVec
    c = CI.one_step_case()
    ref = CartPoleVec(CI.ONE_STEP_E, **c["kw"])
    ref.state, ref.n_steps, ref.terminated = c["state"].copy(), c["n_steps"].astype(np.float64), np.full(CI.ONE_STEP_E, False)
    rp = CI.ReplayCartPole(CI.ONE_STEP_E, seed=CI.ONE_STEP_SEED, **c["kw"])
    rp.load(c["state"], c["n_steps"], c["episode"])
    s0, _, d0, _ = ref.step(c["act"])
    s1, _, d1, _ = rp.step(c["act"])
    assert np.array_equal(d0, d1) and np.array_equal(s0[~d0], s1[~d1])
    assert rp.margin() >= 1e-9
    ended = np.nonzero(d1)[0]
    assert set(ended) == {51, 53, 55, 57, 58, 59}
    assert np.array_equal(rp.episode[ended], c["episode"][ended] + 1) and np.array_equal(rp.episode[~d1], c["episode"][~d1])
    assert np.array_equal(s1[ended], CI.fresh_state(rp.low, rp.high, CI.ONE_STEP_SEED, ended, c["episode"][ended] + 1))
    assert (s1[ended] >= rp.low).all() and (s1[ended] <= rp.high).all() and (rp.n_steps[ended] == 0).all()
