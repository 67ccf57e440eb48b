"""Host side of GRU training (algo ppo-pure): the CLI flag, the logger columns, the recurrent minibatch generator, and the torch
restatement of a recurrent ppo-pure minibatch (tests/bptt_inputs.py) against fixture G13 case (a) -- which checks the fixture and
the mask convention (m[t] = 1 - done[t], the done stored with step t) without the reference."""
import argparse
import json
from collections import OrderedDict

import numpy as np
import pytest
import torch

import bptt_inputs as BI
from conftest import load_npz, npz_json
from oracle import ppo_oracle as O


def _args(*argv):
    import train
    return train.add_training_args(argparse.ArgumentParser()).parse_args(list(argv))


def test_algo_flag_parses_and_merges():
    import train
    a = _args("--param_name", "hard-rec", "--algo", "ppo-pure")
    assert a.algo == "ppo-pure"
    hp = train.merge_hyperparameters(train.get_hyperparams("hard-rec"), a)
    assert hp["algo"] == "ppo-pure" and hp["recurrent"] is True
    a = _args("--param_name", "hard-rec")
    assert a.algo is None
    assert train.merge_hyperparameters(train.get_hyperparams("hard-rec"), a)["algo"] == "ppo"      # the file's value stays
    with pytest.raises(SystemExit):
        _args("--algo", "espo")


def test_logger_columns():
    from common.logger import Logger, EPISODE_KEYS
    head = ["timesteps", "wall_time", "num_episodes"] + EPISODE_KEYS + ["val_" + k for k in EPISODE_KEYS] + ["ema_rewards"]
    # the reference's list for algo in ['ppo-pure', 'espo'] (common/logger.py:65-66)
    pure = ["loss_pi", "loss_v", "loss_entropy", "loss_x_entropy", "loss_total"]
    assert Logger(4, None, algo="ppo-pure").columns == head + pure + ["learning_rate"]
    default = ["loss_pi", "loss_v", "loss_entropy", "loss_x_entropy", "atn_entropy", "atn_entropy2", "loss_sparsity", "loss_feature_sparsity",
               "loss_total"]
    assert Logger(4, None).columns == head + default + ["learning_rate"]
    assert Logger(4, None, algo="ppo").columns == head + default + ["learning_rate"]


def test_ppo_pure_surface():
    import inspect
    from agents.ppo import PPO
    from agents.ppo_pure import PPOPure
    assert issubclass(PPOPure, PPO)
    ref = ["self", "env", "policy", "logger", "storage", "device", "n_checkpoints", "env_valid", "storage_valid", "n_steps", "n_envs", "epoch",
           "n_minibatch", "mini_batch_size", "gamma", "lmbda", "learning_rate", "grad_clip_norm", "eps_clip", "value_coef", "entropy_coef",
           "x_entropy_coef", "normalize_adv", "normalize_rew", "use_gae", "entropy_scaling", "increasing_lr", "sparsity_coef", "fs_coef", "kwargs"]
    assert list(inspect.signature(PPOPure.__init__).parameters) == ref          # agents/ppo_pure.py:12-41
    # hard-rec: E = 256, T = 256, 8 minibatches -> 32 envs x 256 steps per minibatch, one optimizer step each
    assert PPOPure.rec_plan(256, 256, 8, 8192) == (8192, 32, 1.0)
    assert PPOPure.rec_plan(8, 8, 2, 16) == (16, 2, 2.0)                       # two accumulated minibatches of 2 envs per step
    with pytest.raises(ValueError):
        PPOPure._check_recurrent(8, 8, 2, 12)                                   # not whole trajectories


@pytest.mark.parametrize("seed,T,E,B", [(0, 8, 16, 32), (9, 8, 16, 32), (123, 4, 8, 8), (5, 8, 8, 32)])
def test_recurrent_generator_consumes_rng_like_the_index_stream(seed, T, E, B):
    from common.storage import Storage
    st = Storage((9,), 6, T, E, torch.device("cpu"))
    st._hidden[:] = np.random.default_rng(1).standard_normal(st._hidden.shape).astype(np.float32)
    torch.manual_seed(seed)
    ref = [idx for idx in st.minibatch_index_stream(B, recurrent=True)]
    state_ref = torch.get_rng_state()
    torch.manual_seed(seed)
    got = list(st.recurrent_minibatch_stream(B))
    assert torch.equal(torch.get_rng_state(), state_ref)
    assert len(got) == len(ref)
    for (envs, h0), idx in zip(got, ref):
        assert envs.dtype == np.int64 and np.array_equal(envs, idx[:len(idx) // T] % E)
        assert np.array_equal((np.arange(T)[:, None] * E + envs[None, :]).reshape(-1), idx)       # time-major rows t*n + i
        assert h0.dtype == np.float32 and np.array_equal(h0, st._hidden[0, envs])
    assert np.array_equal(np.sort(np.concatenate([e for e, _ in got])), np.arange(E))


# ---------------------------------------------------------------------------------------------- fixture G13, case (a)
@pytest.fixture(scope="module")
def g13():
    return load_npz("g13_bptt.npz")


def test_g13_inputs_and_seeded_init(g13):
    r = BI.rollout_a()
    for k, v in r.items():
        assert np.array_equal(g13["a/in/" + k], v), k
    d = r["done"]
    assert d[0].any() and d[-1].any() and (d.sum(0) == 0).any() and 0 < d.mean() < 1
    assert np.abs(r["h0"]).min() > 0
    assert BI.sha(BI.rollout_b()["frames"]) == bytes(g13["b/frames_sha"]).decode()
    for case in ("a", "b"):
        assert BI.flat_sha(BI.build_policy(case)) == bytes(g13[f"{case}/sha"]).decode(), "seeded init differs from the reference's"
    torch.manual_seed(5)
    assert np.array_equal(torch.randperm(BI.CASE_A["E"]).numpy(), g13["a/envs"])


def _minibatch_args(r, adv, ret, envs):
    T = r["done"].shape[0]
    return dict(obs=r["frames"][:T][:, envs], h0=r["h0"][envs], done=r["done"][:, envs], act=r["act"][:, envs], old_logp=r["logp"][:, envs],
                old_value=r["val"][:T][:, envs], ret=ret[:, envs], adv=adv[:, envs])


@pytest.mark.parametrize("dtype,loss_tol,grad_tol", [(torch.float32, 1e-6, 1e-5), (torch.float64, 1e-6, 1e-5)])
def test_twin_reproduces_g13_case_a(g13, dtype, loss_tol, grad_tol):
    """Both minibatches of the un-clipped run: minibatch 1 at the seeded parameters, minibatch 2 after one Adam step (the oracle's
    restated Adam on the fixture's own step-1 gradients).  The reference in fp32 against itself in fp64 differs by at most 6e-8 in
    the losses and 3e-7 relative L2 in the gradients on this shape, so the bounds leave a factor of 15 and more."""
    r = BI.rollout_a()
    adv, ret = O.compute_estimates(torch.from_numpy(r["rew"]), torch.from_numpy(r["done"]), torch.from_numpy(r["val"]), 0.999, 0.95)
    assert np.abs(adv.numpy() - g13["a/adv"]).max() < 1e-5 and np.array_equal(ret.numpy(), g13["a/ret"])
    adv, ret = g13["a/adv"], g13["a/ret"]
    params = BI.host_params(BI.build_policy("a"))
    envs = g13["a/envs"]
    losses = []
    for k in (1, 2):
        L, g = BI.rec_minibatch(params, "mlp", dtype=dtype, **_minibatch_args(r, adv, ret, envs[4 * (k - 1):4 * k]))
        losses.append(L)
        ref = {n: g13[f"a/raw/g{k}/g/{n}"] for n in params}
        assert set(g) == set(ref) and len(ref) == 16
        for n in ref:
            err = BI.rel_l2(g[n].numpy(), ref[n])
            print(f"minibatch {k} {n}: rel L2 {err:.2e}")
            assert err < grad_tol, (k, n, err)
        tot = float(np.sqrt(sum(float((v.double() ** 2).sum()) for v in g.values())))
        assert abs(tot - float(g13[f"a/raw/total_norm{k}"])) < 1e-5 * float(g13[f"a/raw/total_norm{k}"])
        if k == 1:                                  # the reference's optimizer step 1 (clip 1e9: un-clipped), lr 5e-4
            p = OrderedDict((n, torch.from_numpy(v.copy())) for n, v in params.items())
            m = OrderedDict((n, torch.zeros_like(v)) for n, v in p.items())
            v2 = OrderedDict((n, torch.zeros_like(v)) for n, v in p.items())
            O.adam_step(p, OrderedDict((n, torch.from_numpy(ref[n].copy())) for n in p), m, v2, 1, 5e-4)
            params = OrderedDict((n, v.numpy()) for n, v in p.items())
    s = npz_json(g13, "a/raw/summary")
    mean = lambda key: float(np.mean([L[key] for L in losses]))
    got = {'Loss/pi': -mean("pi_loss"), 'Loss/v': -mean("value_loss"), 'Loss/entropy': mean("entropy"), 'Loss/x_entropy': mean("x_ent"),
           'Loss/total': mean("total")}
    assert list(s) == list(got)
    for key in s:
        print(f"{key}: {got[key]:.9f} vs {s[key]:.9f}")
        assert abs(got[key] - s[key]) < loss_tol, key


def test_mask_convention_is_pinned(g13):
    """Masking step t with the done of step t - 1 (the rollout's convention) must NOT reproduce the fixture."""
    r = BI.rollout_a()
    envs = g13["a/envs"][:4]
    a = _minibatch_args(r, g13["a/adv"], g13["a/ret"], envs)
    a["done"] = np.concatenate([np.zeros_like(a["done"][:1]), a["done"][:-1]])
    _, g = BI.rec_minibatch(BI.host_params(BI.build_policy("a")), "mlp", **a)
    assert BI.rel_l2(g["gru.gru.weight_hh_l0"].numpy(), g13["a/raw/g1/g/gru.gru.weight_hh_l0"]) > 1e-2
