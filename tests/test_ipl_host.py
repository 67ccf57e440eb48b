"""The IPL agent (`algo: IPL`; reference agents/IPL.py), host side: the float64 restatement of tests/ipl_inputs.py against fixture G16
(tests/golden/make_golden_ipl.py ran the reference), IPLStorage's index stream, the accumulation schedule, the logger's columns, every
refusal by name and train.py's argument handling.  CPU only.

Bounds of the restatement against the fixture: the golden's terms are float32 numbers of the reference (magnitudes up to 30), the
restatement is float64, so 1e-6 x max(1, |term|) -- one part in 1e6 of the term, 8 float32 ulps -- and 1e-5 relative L2 for the gradients
of the first minibatch."""
import argparse

import numpy as np
import pytest
import torch

import ipl_inputs as II
import sae_inputs as SI
from conftest import load_npz

torch.set_num_threads(8)


@pytest.fixture(scope="module")
def z():
    return load_npz("g16_ipl.npz")


@pytest.mark.parametrize("name", list(II.CASES))
def test_restatement_reproduces_the_golden(z, name):
    c, roll, params, idx = II.load_case(z, name)
    row, pred, grads = II.minibatch(c, params, roll, idx[0])
    ref = z[f"{name}/terms"][0]
    for j, k in enumerate(II.TERMS):
        if np.isnan(ref[j]):
            assert np.isnan(row[j]) and k == "alpha_loss"
        else:
            assert abs(row[j] - ref[j]) < 1e-6 * max(1.0, abs(ref[j])), (k, row[j], ref[j])
    assert np.abs(pred - z[f"{name}/pred0"]).max() < 1e-6 * max(1.0, np.abs(pred).max())
    for n, g in grads.items():
        assert SI.tensor_error(g, z, f"{name}/g0/", n) < 1e-5, n
    # the returned summary is the mean of the per-minibatch terms, in the reference's key order
    np.testing.assert_allclose(z[f"{name}/summary"], z[f"{name}/terms"].mean(0), rtol=1e-12, equal_nan=True)
    # every other minibatch in front of the first optimizer step runs on the same parameters
    for k in range(1, II.step_schedule(c)[0]):
        row, _, _ = II.minibatch(c, params, roll, idx[k])
        ref = z[f"{name}/terms"][k]
        ok = ~np.isnan(ref)
        assert (np.abs(row[ok] - ref[ok]) < 1e-6 * np.maximum(1.0, np.abs(ref[ok]))).all(), (k, row, ref)


def test_next_only_restatement_has_no_obs_side_gradient(z):
    """alpha = 0 and a detached obs-side value: fc_policy's gradient is exactly zero, the embedder and fc_value receive theirs through
    obs[t + 1] alone."""
    c, roll, params, idx = II.load_case(z, "b")
    _, _, g = II.minibatch(c, params, roll, idx[0], next_only=True)
    assert not g["fc_policy.weight"].any() and not g["fc_policy.bias"].any() and np.linalg.norm(g["fc_value.weight"]) > 0


def test_index_stream_is_the_references_draw(z):
    from common.storage import IPLStorage
    for name, c in II.CASES.items():
        mbs, _ = II.accumulation(c)
        st = IPLStorage((3, 64, 64) if c["arch"] == "impala" else (9,), c["T"], c["E"], None)
        torch.manual_seed(c["seed"] + 100)
        got = [idx for _ in range(c["epoch"]) for idx in st.minibatch_index_stream(mbs, False)]
        assert np.array_equal(np.stack(got), z[f"{name}/idx"]), name


class _FakeEngine:
    """Counts what IPL.optimize asks of the engine."""

    def __init__(self):
        self.calls = []

    def ipl_hparams(self, *a, **k):
        return ("hp", a)

    def ipl_minibatch(self, idx, n_global, hp):
        assert len(idx) == n_global
        self.calls.append("mb")

    def optimizer_step(self, lr, clip, step, want_norm=False):
        self.calls.append("step")
        return 0.0

    def loss_log(self, reset=True):
        n = self.calls.count("mb")
        return np.tile(np.arange(8, dtype=np.float32), (n, 1))

    def ipl_read_pred(self, n):
        return np.zeros(n, np.float32), np.ones(n, np.float32)


def _fake_agent(c):
    from agents.ipl import IPL
    from common.storage import IPLStorage
    from mi355.optim import DeviceAdam
    o = II.opts(c)
    agent = IPL.__new__(IPL)
    agent.engine = _FakeEngine()
    agent.storage = IPLStorage((9,), c["T"], c["E"], None)
    agent.n_steps, agent.n_envs, agent.epoch, agent.n_minibatch, agent.mini_batch_size = c["T"], c["E"], c["epoch"], c["n_minibatch"], c["mini_batch_size"]
    agent.gamma, agent.alpha, agent.entropy_coef = c["gamma"], o["alpha"], o["entropy_coef"]
    agent.entropy_modified, agent.reward_incentive, agent.adv_incentive = o["entropy_modified"], o["reward_incentive"], o["adv_incentive"]
    agent.accumulate_all_grads, agent.grad_clip_norm, agent.detect_nan, agent.optimizer_steps = o["accumulate_all_grads"], 0.5, False, 0
    opt = DeviceAdam.__new__(DeviceAdam)
    opt.engine, opt.step_count = agent.engine, 0
    opt.policy = type("P", (), {"mark_device_updated": lambda self: None})()
    opt._adam = type("A", (), {"param_groups": [{"lr": 5e-4}]})()
    agent.optimizer = opt
    return agent


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_accumulation_schedule(z, name):
    """Optimizer steps of one optimize(): the float rule cnt % (batch_size / mini_batch_size) == 0 (b: every second minibatch), one step
    per epoch with accumulate_all_grads (c) -- counted, and at the positions the reference stepped (the fixture's step count)."""
    c = II.CASES[name]
    agent = _fake_agent(c)
    torch.manual_seed(c["seed"] + 100)
    summary = agent.optimize()
    calls = agent.engine.calls
    at = [calls[:i].count("mb") for i, x in enumerate(calls) if x == "step"]
    assert at == II.step_schedule(c) and len(at) == len(z[f"{name}/step_norms"]) == int(z[f"{name}/adam_step"]) == agent.optimizer_steps
    assert {"a": [1], "b": [2, 4, 6, 8], "c": [2, 4]}[name] == at
    assert list(summary) == list(II.SUMMARY_KEYS)
    assert np.isnan(summary["Loss/alpha"]) and summary["Loss/gamma"] == c["gamma"] and summary["alpha"] == II.opts(c)["alpha"]
    assert summary["Loss/entropy"] == 0.0 and summary["Loss/pred_reward"] == 7.0
    assert agent.last_predicted_reward.shape == agent.last_reward.shape == (len(z[f"{name}/idx"][-1]),)


def test_logger_columns_for_ipl(tmp_path):
    from common.logger import Logger
    cols = Logger(4, str(tmp_path), algo="IPL").columns
    # the reference's list for algo == "IPL" (common/logger.py:67-69), typed here as names
    want = ["entropy", "mutual_info", "loss_total", "rew_corr", "gamma", "loss_alpha", "alpha", "pred_reward"]
    i0 = cols.index("ema_rewards") + 1
    assert cols[i0:-1] == want and cols[-1] == "learning_rate" and cols[:3] == ["timesteps", "wall_time", "num_episodes"]
    ppo = Logger(4, str(tmp_path), algo="ppo").columns
    assert ppo[i0:-1] == ["loss_pi", "loss_v", "loss_entropy", "loss_x_entropy", "atn_entropy", "atn_entropy2", "loss_sparsity",
                          "loss_feature_sparsity", "loss_total"]
    assert Logger(4, str(tmp_path), algo="ppo-pure").columns[i0:-1] == ["loss_pi", "loss_v", "loss_entropy", "loss_x_entropy", "loss_total"]


def _policy(recurrent=False, lse=False):
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(1)
    return CategoricalPolicy(MLPModel(9, 4, 64, 64), recurrent, 2, logsumexp_logits_is_v=lse)


def test_refusals_name_their_option(monkeypatch):
    from agents.ipl import IPL, check_supported
    from common.storage import IPLStorage
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    check_supported({"learned_gamma": False}, _policy())
    st = IPLStorage((9,), 4, 4, None)
    mk = lambda pol=None, **kw: IPL(None, pol or _policy(), None, st, torch.device("cpu"), 1, n_steps=4, n_envs=4, **kw)
    for kw, word in ((dict(learned_gamma=True), "learned_gamma"), (dict(learned_temp=True), "learned_temp"),
                     (dict(env_greedy=object()), "use_greedy_env"), (dict(storage_greedy=object()), "greedy")):
        with pytest.raises(NotImplementedError, match=word):
            mk(**kw)
    with pytest.raises(NotImplementedError, match="recurrent"):
        mk(_policy(recurrent=True))
    with pytest.raises(NotImplementedError, match="logsumexp_logits_is_v"):
        mk(_policy(lse=True))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        mk()
    with pytest.raises(NotImplementedError, match="recurrent"):
        next(st.fetch_train_generator(4, recurrent=True))


def _args(extra, algo=("--algo", "IPL")):
    import train
    return train.add_training_args(argparse.ArgumentParser()).parse_args(list(algo) + ["--env_name", "synthetic"] + extra)


def test_cli_and_hyperparameter_sets(monkeypatch):
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert _args(["--param_name", "hard-500-ipl"]).algo == "IPL"
    hard, cart = train.get_hyperparams("hard-500-ipl"), train.get_hyperparams("ipl_cartpole")
    assert hard == dict(algo="IPL", n_envs=256, n_steps=256, epoch=3, n_minibatch=8, mini_batch_size=8192, gamma=0.999, lmbda=0.95,
                        learning_rate=0.0005, grad_clip_norm=0.5, normalize_adv=True, normalize_rew=True, architecture="impala",
                        recurrent=False, output_dim=256, latent_dim=32)
    assert cart == dict(algo="IPL", n_envs=256, n_steps=256, epoch=3, n_minibatch=16, mini_batch_size=8192, gamma=0.99, lmbda=0.95,
                        learning_rate=0.0005, grad_clip_norm=0.5, normalize_adv=True, normalize_rew=False, architecture="mlpmodel",
                        recurrent=False, depth=4, latent_size=64, mid_weight=256)
    assert train.get_hyperparams("hard-500")["algo"] == "ppo" and train.get_hyperparams("sae")["algo"] == "sae"
    with pytest.raises(KeyError):
        train.get_hyperparams("ipl_icm_cartpole")


def test_train_refuses_before_any_engine(monkeypatch):
    """Everything outside the built scope ends train.py by name before an env, a log directory or an engine exists."""
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(train, "make_env", lambda *a, **k: pytest.fail("an env was built"))
    for extra, word in ((["--learned_gamma"], "learned_gamma"), (["--use_greedy_env"], "use_greedy_env")):
        with pytest.raises(NotImplementedError, match=word):
            train.train_ppo(_args(["--param_name", "hard-500-ipl"] + extra))
    base = train.get_hyperparams
    for key, word in (("learned_temp", "learned_temp"), ("recurrent", "recurrent"), ("logsumexp_logits_is_v", "logsumexp_logits_is_v")):
        monkeypatch.setattr(train, "get_hyperparams", lambda name, key=key: dict(base(name), **{key: True}))
        with pytest.raises(NotImplementedError, match=word):
            train.train_ppo(_args(["--param_name", "hard-500-ipl"]))
    monkeypatch.setattr(train, "get_hyperparams", lambda name: dict(base(name), algo="IPL_ICM"))
    with pytest.raises(NotImplementedError, match="IPL_ICM"):
        train.train_ppo(_args(["--param_name", "hard-500-ipl"], algo=()))
    monkeypatch.setattr(train, "get_hyperparams", base)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        train.train_ppo(_args(["--param_name", "ipl_cartpole"]))
