"""The table of pre-vectorised envs (common/env/vec_envs.py VECTOR_ENVS) and its three users in train.py: every row's host class and
device class describe the same env, and the env construction, the env-group exclusion and the --device_env check all accept the row's
name.  Host only."""
import argparse

import numpy as np
import pytest

from common.env.vec_envs import VECTOR_ENVS, EnvGroups, device_env_labels, vector_env

ROWS = sorted(VECTOR_ENVS)


def _args(extra):
    import train
    return train.add_training_args(argparse.ArgumentParser()).parse_args(extra)


def test_the_table_names_its_envs():
    assert vector_env("cartpole") is VECTOR_ENVS["cartpole*"] and vector_env("cartpole_swing") is VECTOR_ENVS["cartpole*"]
    assert vector_env("mountain_car") is VECTOR_ENVS["mountain_car"]
    for other in ("synthetic", "coinrun", "mountain_car_v2", "my_cartpole", ""):
        assert vector_env(other) is None
    assert device_env_labels().startswith("the cart-pole (cartpole*)") and " and " in device_env_labels()
    assert all(v.label in device_env_labels() for v in VECTOR_ENVS.values())


@pytest.mark.parametrize("is_valid", [False, True])
@pytest.mark.parametrize("pattern", ROWS)
def test_host_and_device_class_describe_the_same_env(pattern, is_valid):
    """For the same arguments -- through the row's creator and through the two constructors -- the host class and the device class
    report the same observation_space, action_space, low and high."""
    row = VECTOR_ENVS[pattern]
    hp = {"max_steps": 17}
    host, dev = row.create(hp, is_valid, seed=3, n_envs=6), row.create(hp, is_valid, seed=3, n_envs=6, device=True)
    assert type(host) is row.host_cls and type(dev) is row.device_cls and row.host_cls is not row.device_cls
    for a, b in ((host, dev), (row.host_cls(4, seed=1), row.device_cls(4, seed=1))):
        assert a.observation_space.shape == b.observation_space.shape and len(a.observation_space.shape) == 1
        assert a.action_space.n == b.action_space.n and a.action_space.n >= 2
        assert a.low.dtype == b.low.dtype == np.float64 and a.low.shape == a.high.shape == a.observation_space.shape
        assert a.low.tobytes() == b.low.tobytes() and a.high.tobytes() == b.high.tobytes()
        assert a.n_envs == b.n_envs and a.max_steps == b.max_steps
    assert dev.on_device is True and not getattr(host, "on_device", False)
    assert host.max_steps == 17


@pytest.mark.parametrize("pattern", ROWS)
def test_train_accepts_every_row(pattern, monkeypatch):
    """_one_env builds the row's class (the device class only with --device_env), make_env keeps the env out of the env groups whatever
    --rollout_groups says, and check_device_env lets the name through; a name outside the table gets the refusal."""
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    row, name = VECTOR_ENVS[pattern], pattern.replace("*", "")
    for flag, cls in (([], row.host_cls), (["--device_env"], row.device_cls)):
        args = _args(["--env_name", name, "--rollout_groups", "2"] + flag)
        assert type(train._one_env(name, 8, 1, None, args, {}, False)) is cls
        env = train.make_env(name, 8, 1, None, args, {})
        assert type(env) is cls and not isinstance(env, EnvGroups)
    for algo in ("ppo", "ppo-pure"):
        train.check_device_env(name, {}, algo)
    with pytest.raises(NotImplementedError, match=r"--device_env with env_name coinrun is not supported: only the cart-pole \(cartpole\*\) and mountain_car have a device-resident env$"):
        train.check_device_env("coinrun", {}, "ppo")
