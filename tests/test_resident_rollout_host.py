"""Host side of the one-launch rollout (train.py --resident_rollout, Engine.env_rollout(resident=True), mi_env_rollout_resident): the flag,
its refusal without --device_env, and the CPU oracle (tests/resident_inputs.py) on every case of tests/test_gpu_resident_rollout.py --
the oracle alone must leave no row out of the GPU comparison."""
import argparse

import numpy as np
import pytest

import resident_inputs as RI


def _args(extra):
    import train
    return train.add_training_args(argparse.ArgumentParser()).parse_args(extra)


def test_resident_rollout_flag_parses_and_defaults_to_false():
    assert _args([]).resident_rollout is False
    assert _args(["--env_name", "cartpole", "--param_name", "cartpole", "--device_env"]).resident_rollout is False
    assert _args(["--env_name", "cartpole", "--param_name", "cartpole", "--device_env", "--resident_rollout"]).resident_rollout is True


def test_train_refuses_the_flag_without_device_env_before_any_env(monkeypatch):
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(train, "make_env", lambda *a, **k: pytest.fail("an env was built"))
    monkeypatch.setattr(train, "create_logdir_train", lambda *a, **k: pytest.fail("a log directory was made"))
    for name in ("cartpole", "mountain_car"):
        with pytest.raises(NotImplementedError, match="--resident_rollout needs --device_env"):
            train.train_ppo(_args(["--env_name", name, "--param_name", name, "--resident_rollout"]))
    # with --device_env the flag passes the checks and reaches the agent as a hyper-parameter: the next thing train.py does is build the env
    seen = {}

    class Stop(Exception):
        pass

    def stop(*a, **k):
        seen["hp"] = a[5]
        raise Stop
    monkeypatch.setattr(train, "make_env", stop)
    with pytest.raises(Stop):
        train.train_ppo(_args(["--env_name", "cartpole", "--param_name", "cartpole", "--device_env", "--resident_rollout"]))
    assert seen["hp"]["resident_rollout"] is True
    with pytest.raises(Stop):
        train.train_ppo(_args(["--env_name", "cartpole", "--param_name", "cartpole", "--device_env"]))
    assert "resident_rollout" not in seen["hp"]              # nothing changes when the flag is absent


def test_the_agent_takes_the_flag_as_a_keyword():
    import inspect
    from agents.ppo import PPO
    src = inspect.getsource(PPO.__init__) + inspect.getsource(PPO._collect_device)
    assert 'kwargs.get("resident_rollout", False)' in src and "resident=self.resident_rollout" in src


@pytest.mark.parametrize("name", RI.TEST1 + RI.TEST2)
def test_the_oracle_alone_leaves_no_row_out(name):
    """Every replay margin holds, no uniform is within 1e-4 of a float64 CDF edge, and the two rollouts hold a termination, a truncation, a
    reset and every action value."""
    o = RI.oracle(name)
    c, (r1, r2) = o["c"], o["rollouts"]
    cov = RI.coverage(c, (r1, r2))
    print(name, cov)
    assert cov["margin_ok"]
    assert cov["min_udist"] >= RI.U_CLEAR, cov["min_udist"]
    assert cov["terminations"] >= 1 and cov["truncations"] >= 1 and cov["resets"] >= 1
    assert cov["actions"] == list(range(RI.ACTIONS[c["kind"]]))
    E, T, W = c["E"], c["T"], RI.WIDTH[c["kind"]]
    assert r1["obs"].shape == (T + 1, E, W) and r1["act"].shape == (T, E) and r1["value"].shape == (T + 1, E) and r1["udist"].shape == (T + 1, E)
    assert np.array_equal(r2["obs"][0], r1["obs"][T]) and np.array_equal(r1["obs"][T], r1["state"].astype(np.float32))
    if name in RI.TEST1:                                     # the planted rows of the existing rollout tests
        assert r1["done"][0, 0] and r1["terminated"][0, 0] and r1["done"][4, 1] and not r1["terminated"][4, 1] and not r1["done"][:4, 1].any()
    if c["kind"] == "mountain_car":
        dense = not RI.env_kwargs(c).get("sparse_rewards", True)
        assert (r1["rew"] != -1).any() if dense else (r1["rew"] == -1).all()
        # the validation ranges: some start draw of these rollouts was rejected (the reset restatement's attempt counter)
        ended = np.argwhere(np.concatenate([r1["done"], r2["done"]]))
        rp = RI.make_replay(c)
        assert (RI.MI.fresh_state(rp.low, rp.high, c["env_seed"], ended[:, 1], np.full(len(ended), 2))[1] > 1).any()


def test_forced_rollout_on_the_oracles_own_ring_is_the_oracle():
    """The stepwise rule of the GPU test (policy rows on a ring's own observations, env stepped on the ring's actions) applied to the oracle's
    rings reproduces the oracle."""
    o = RI.oracle("cartpole")
    r1 = o["rollouts"][0]
    f = RI.rollout(o["c"], o["flat"], *o["s0"], o["c"]["seed"], forced=(r1["obs"], r1["act"]))
    for k in ("obs", "act", "rew", "done", "state", "n_steps", "episode"):
        assert np.array_equal(f[k], r1[k]), k
    for k in ("logp", "value"):                              # (two float64 evaluations by a threaded BLAS need not agree in the last bit)
        assert np.allclose(f[k], r1[k], rtol=1e-12, atol=1e-14), k


def test_torch_error_is_measured_on_a_pool_for_small_cases():
    o = RI.oracle("shallow")
    ev, el = RI.torch_errors(o["c"], o["flat"], o["rollouts"][0]["obs"])
    assert 0 < ev < 1e-5 and 0 < el < 1e-5, (ev, el)
