"""Host side of the one-launch evaluation (mi_env_evaluate, Engine.env_evaluate, PPO.evaluate, evaluate.py): the CPU oracle
(tests/evaluate_inputs.py) on every case of tests/test_gpu_evaluate.py -- the oracle alone must leave nothing out of the GPU comparison --
the statistics function, the script's arguments and refusals, and the agent's refusal of a host env."""
import numpy as np
import pytest

import evaluate_inputs as EI
import resident_inputs as RI


# ------------------------------------------------------------------------------------------ the oracle's cases
def test_the_cases_are_the_shapes_the_kernel_can_go_wrong_at():
    shape = {n: (c["E"], c["K"], c["greedy"], c["depth"], c["lse"], c["starts"] is not None, c["env"]) for n, c in EI.CASES.items()}
    assert shape == {"cartpole_sampled": (18, 3, False, 4, 0, False, "cartpole"), "cartpole_greedy": (18, 3, True, 4, 0, False, "cartpole"),
                     "exact_tile": (16, 1, False, 4, 0, False, "cartpole"), "mountain_car_dense": (18, 2, False, 4, 0, False, "mountain_car"),
                     "swing_planted": (18, 2, True, 4, 0, True, "cartpole_swing"), "lse": (18, 2, False, 4, 1, False, "cartpole"),
                     "shallow": (16, 2, True, 2, 0, False, "cartpole"), "cartpole_starts": (18, 3, False, 4, 0, True, "cartpole")}
    for c in EI.CASES.values():
        assert c["width"] == 64 and c["out"] == 64 and EI.make_replay(c).max_steps == EI.MAX_STEPS
    assert EI.env_kwargs(EI.CASES["mountain_car_dense"])["sparse_rewards"] is False


@pytest.mark.parametrize("name", list(EI.CASES))
def test_the_oracle_alone_leaves_nothing_out(name):
    """Over the evaluated steps of the case: every env margin holds; sampled: no uniform within U_CLEAR of a float64 CDF edge; greedy: the
    two largest log-probabilities at least 1e-3 apart; every action value occurs; a termination and a truncation; dense rewards: at least
    half of the steps with |reward| >= 0.1."""
    o = EI.oracle(name)
    c, ev = o["c"], o["ev"]
    cov = EI.coverage(name, ev)
    print(name, cov)
    assert cov["margin_ok"]
    if c["greedy"]:
        assert cov["min_gap"] >= EI.GREEDY_GAP, cov["min_gap"]
    else:
        assert cov["min_udist"] >= EI.U_CLEAR, cov["min_udist"]
    assert cov["actions"] == list(range(RI.ACTIONS[c["kind"]]))
    assert cov["terminations"] >= 1 and cov["truncations"] >= 1
    if name in EI.DENSE:
        assert cov["dense_share"] >= 0.5, cov["dense_share"]
        assert len(np.unique(ev["rew"])) > len(ev["rew"]) // 2                     # (really a dense reward)
    else:
        assert (ev["rew"] == 1).all()
    assert EI.covered(name, cov)
    E, K, W = c["E"], c["K"], RI.WIDTH[c["kind"]]
    assert ev["ret"].shape == ev["length"].shape == ev["terminated"].shape == ev["value0"].shape == (E, K) and ev["start"].shape == (E, K, W)
    # the accounting: every episode has 1 .. max_steps steps, a shorter one was terminated, the steps used are the longest env's, and the
    # per-step arrays hold exactly the evaluated steps
    assert (ev["length"] >= 1).all() and (ev["length"] <= o["max_steps"]).all()
    assert (ev["terminated"][ev["length"] < o["max_steps"]] == 1).all()
    assert ev["steps"] == ev["length"].sum(axis=1).max() <= K * o["max_steps"]
    assert len(ev["act"]) == len(ev["rew"]) == ev["length"].sum()
    assert np.isclose(ev["rew"].sum(), ev["ret"].sum(), rtol=1e-12)


def test_the_starts_are_the_reset_stream_or_the_planted_rows():
    o = EI.oracle("cartpole_sampled")
    c, ev = o["c"], o["ev"]
    for e, i in ((0, 0), (17, 2), (5, 1)):
        assert np.array_equal(ev["start"][e, i], RI.fresh(c, e, EI.F_DEFAULT + i)[0])
    assert not np.array_equal(EI.stream_starts(c, 1), ev["start"])                 # another first_episode, other episodes
    p = EI.oracle("cartpole_starts")
    assert np.array_equal(p["ev"]["start"], p["starts"])
    # the planted rows of resident_inputs.initial_state: env 0 ends at its first step, env 1 is truncated, in every episode
    assert (p["ev"]["length"][0] == 1).all() and (p["ev"]["terminated"][0] == 1).all()
    assert (p["ev"]["length"][1] == p["max_steps"]).all() and (p["ev"]["terminated"][1] == 0).all()
    s = EI.oracle("swing_planted")
    assert s["ev"]["length"][0, 0] == 1 and s["ev"]["terminated"][0, 0] == 1 and (s["ev"]["ret"][:, 1] > 0.5 * s["ev"]["length"][:, 1]).all()


def test_the_oracle_follows_the_mode_the_seed_and_the_first_episode():
    o = EI.oracle("cartpole_sampled")
    c, flat, ev = o["c"], o["flat"], o["ev"]
    again = EI.evaluate(c, flat)
    for k in ("ret", "length", "terminated", "start", "act"):
        assert np.array_equal(again[k], ev[k]), k
    assert not np.array_equal(EI.evaluate(c, flat, seed=c["seed"] + 1)["act"], ev["act"])
    assert not np.array_equal(EI.evaluate(c, flat, first_episode=7)["start"], ev["start"])
    g = EI.evaluate(c, flat, greedy=True)
    assert np.array_equal(g["act"], EI.evaluate(c, flat, greedy=True, seed=123)["act"])      # greedy: the sampler's seed does not matter


# ------------------------------------------------------------------------------------------ evaluation_stats
def test_evaluation_stats_against_direct_numpy():
    from common.logger import EPISODE_KEYS, EVALUATION_KEYS, SimpleLogger, evaluation_stats
    assert EVALUATION_KEYS == EPISODE_KEYS[:9] and len(SimpleLogger.STAT_NAMES) == len(EPISODE_KEYS)
    ret = np.array([[3.0, -1.0, 0.0], [5.0, 2.5, -4.0]])
    length = np.array([[3, 5, 1], [5, 4, 5]], np.int32)
    s = evaluation_stats(ret, length, 5)
    assert list(s) == EVALUATION_KEYS and all(isinstance(v, float) for v in s.values())
    want = [5.0, np.mean(ret), np.median(ret), -4.0, 5.0, np.mean(length), 1.0, 3 / 6, (3 + 5 + 4) / 3]
    assert list(s.values()) == [float(w) for w in want]
    assert s["median_episode_rewards"] == 1.25 and s["mean_timeouts"] == 0.5 and s["mean_episode_len_pos_reward"] == 4.0
    # no positive return: the conditional mean is NaN, nothing else is
    s = evaluation_stats(-ret * (ret > 0), length, 5)
    assert np.isnan(s["mean_episode_len_pos_reward"]) and np.isfinite([v for k, v in s.items() if k != "mean_episode_len_pos_reward"]).all()
    # the whole record of an oracle evaluation: the means are over all K * E episodes
    ev = EI.oracle("mountain_car_dense")["ev"]
    s = evaluation_stats(ev["ret"], ev["length"], 5)
    assert s["mean_episode_rewards"] == float(ev["ret"].reshape(-1).mean()) and s["mean_timeouts"] == float((ev["length"] == 5).mean())
    for bad in ((np.zeros(0), np.zeros(0)), (np.zeros(3), np.zeros(4))):
        with pytest.raises(ValueError, match="evaluation_stats"):
            evaluation_stats(*bad, 5)


# ------------------------------------------------------------------------------------------ evaluate.py
def test_evaluate_py_parses_its_flags():
    import evaluate
    a = evaluate.parse_args([])
    assert (a.model_file, a.env_name, a.param_name, a.n_envs, a.seed, a.episodes, a.greedy, a.valid, a.both) == (None, "cartpole", "cartpole", None, 0, 10, False, False, False)
    a = evaluate.parse_args(["--model_file", "m.pth", "--env_name", "mountain_car", "--param_name", "mountain_car", "--n_envs", "16", "--seed", "4",
                             "--episodes", "3", "--greedy", "--both"])
    assert (a.model_file, a.env_name, a.param_name, a.n_envs, a.seed, a.episodes, a.greedy, a.valid, a.both) == ("m.pth", "mountain_car", "mountain_car", 16, 4, 3, True, False, True)
    assert evaluate.parse_args(["--valid"]).valid is True
    with pytest.raises(SystemExit):
        evaluate.parse_args(["--valid", "--both"])


def test_evaluate_py_refuses_a_missing_model_file_and_a_name_without_a_device_env(tmp_path, monkeypatch):
    import evaluate
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(train, "initialize_model", lambda *a, **k: pytest.fail("a model was built"))
    with pytest.raises(ValueError, match="--model_file is required"):
        evaluate.evaluate(evaluate.parse_args(["--env_name", "cartpole", "--param_name", "cartpole"]))
    with pytest.raises(FileNotFoundError, match="--model_file .*nothing.pth: no such file"):
        evaluate.evaluate(evaluate.parse_args(["--model_file", str(tmp_path / "nothing.pth")]))
    ck = tmp_path / "model_1.pth"
    ck.write_bytes(b"")
    with pytest.raises(NotImplementedError, match="--device_env with env_name coinrun is not supported"):
        evaluate.evaluate(evaluate.parse_args(["--model_file", str(ck), "--env_name", "coinrun", "--param_name", "easy-200"]))
    hp, env_name = evaluate.check_args(evaluate.parse_args(["--model_file", str(ck), "--param_name", "mountain_car", "--env_name", "mountain_car", "--n_envs", "32"]))
    assert env_name == "mountain_car" and hp["n_envs"] == 32 and hp["architecture"] == "mlpmodel"
    assert not (tmp_path / "evaluation.npz").exists() and not (tmp_path / "evaluation.csv").exists()


# ------------------------------------------------------------------------------------------ the agent and the engine
def test_ppo_evaluate_refuses_a_host_env_by_name():
    import inspect
    from agents.base_agent import BaseAgent
    from agents.ppo import PPO
    from agents.ppo_pure import PPOPure
    from common.env.vec_envs import CartPoleVec
    assert PPO.evaluate is not BaseAgent.evaluate and PPOPure.evaluate is PPO.evaluate
    assert list(inspect.signature(PPO.evaluate).parameters) == ["self", "episodes", "greedy", "valid", "seed", "starts"]
    agent = PPO.__new__(PPO)                                 # (no engine: the refusal comes before anything touches one)
    agent.env, agent.engine, agent.env_valid, agent.engine_valid = CartPoleVec(4), object(), None, None
    with pytest.raises(NotImplementedError, match="--device_env"):
        agent.evaluate(episodes=2)
    with pytest.raises(ValueError, match="validation env"):
        agent.evaluate(episodes=2, valid=True)


def test_the_engine_has_the_method_and_the_export():
    import inspect
    from mi355 import engine
    assert "mi_env_evaluate" in engine.EXPORTS
    sig = inspect.signature(engine.Engine.env_evaluate)
    assert list(sig.parameters) == ["self", "episodes", "seed", "greedy", "first_episode", "starts"]
    assert sig.parameters["first_episode"].default == 1 << 40 == EI.F_DEFAULT and sig.parameters["greedy"].default is False
