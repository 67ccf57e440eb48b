"""Host side of the fused MLP minibatch pass (train.py --fused_update, PPO(fused_update=True), Engine.minibatch_fused, mi_minibatch_fused):
the float64 reference of tests/fused_update_inputs.py against the reference's own numbers, the margins of every case, the flag and its
refusals, the agent's refusals and the C declaration.  CPU only."""
import argparse
import os
import re
import types

import numpy as np
import pytest
import torch

import fused_update_inputs as FI
import policy_inputs as PI
from conftest import ROOT, npz_json

torch.set_num_threads(8)


def _args(extra):
    import train
    return train.add_training_args(argparse.ArgumentParser()).parse_args(extra)


def test_reference_reproduces_the_reference_projects_minibatch():
    """g4_mlp_lossgrad.npz, tag raw: the losses and every gradient tensor of the reference's own PPO.optimize, to the tolerances
    tests/test_oracle_golden.py::test_g4_loss_and_grads holds the oracle to on that fixture."""
    z, c, b, hp = FI.g4_case()
    r = FI.reference(c, b, hp=hp)
    rec, ref = r["loss"]["records"][0], npz_json(z, "raw/summary")
    for k, mine in (("Loss/pi", -rec["pi_loss"]), ("Loss/v", -rec["value_loss"]), ("Loss/entropy", rec["entropy"]), ("Loss/x_entropy", rec["x_ent"]),
                    ("Loss/total", rec["total"])):
        assert abs(float(mine) - ref[k]) < 2e-6, (k, float(mine), ref[k])
    g = r["grads"]
    total = float(np.sqrt(sum((t ** 2).sum() for t in g.values())))
    assert abs(total - float(z["raw/grad_total_norm"])) < 1e-5 * max(1.0, total)
    for k, (nrm, _) in npz_json(z, "raw/grad_stats").items():
        mine = float(np.sqrt((g[k] ** 2).sum()))
        assert abs(mine - nrm) < 1e-5 * max(1.0, nrm) + 1e-7, (k, mine, nrm)
    seen = 0
    for k in z.files:
        if k.startswith("raw/g/"):
            np.testing.assert_allclose(g[k[len("raw/g/"):]], z[k], rtol=1e-4, atol=2e-6)
            seen += 1
    assert seen == len(g) == 2 * c["depth"] + 4


@pytest.mark.parametrize("name", list(FI.CASES))
def test_every_case_keeps_its_margins(name):
    """No sample within 1e-3 of a clip edge or a vs1 == vs2 tie (so the exclusion cap is 0), every regime present from 64 rows on, the
    segments add up, the indices are in range, and the scattered case is unsorted with repeats."""
    c = FI.CASES[name]
    b, r = FI.case(c), FI.ref64(c)["loss"]
    assert b["idx"].shape == (c["n"],) and b["idx"].min() >= 0 and b["idx"].max() < b["T"] * b["E"]
    assert sum(b["seg_n"]) == c["n"] and min(b["seg_n"]) >= 1
    excluded = PI.loss_excluded(r, FI.HP, margin=FI.MARGIN)
    assert not excluded.any(), f"{name}: rows {np.flatnonzero(excluded)[:8]} lie within {FI.MARGIN} of a decision"
    if c["n"] >= 64:
        present = PI.loss_regimes(r, FI.HP).any(axis=1)
        assert present.all(), [q for q, on in zip(PI.REGIMES, present) if not on]
    if c.get("scattered"):
        assert (np.diff(b["idx"]) < 0).any() and len(np.unique(b["idx"])) == c["n"] - 3
    else:
        assert (np.diff(b["idx"]) > 0).all()
    z = FI.ref64(c)["hout"][:, :c["A"]]
    assert np.ptp(z, axis=1).max() > 0.5, "the logits are all alike"
    terr, eps_q = FI.torch_errors(c)
    g = FI.ref64(c)["grads"]
    assert set(terr) - {"abs"} | set(terr["abs"]) == set(g) and all((g[k].size < FI.SMALL) == (k in terr["abs"]) for k in g)
    assert all(0 < FI.tensor_error(terr, k, g[k]) < 1e-4 for k in g if np.any(g[k])), terr
    if c["lse"]:
        assert not np.any(FI.ref64(c)["grads"]["fc_value.weight"]) and not np.any(FI.ref64(c)["grads"]["fc_value.bias"])
    assert all(v > 0 for v in eps_q.values())


def test_the_shapes_cover_both_sides_of_every_tile():
    ns = sorted(c["n"] for k, c in FI.CASES.items() if k.startswith("base"))
    assert ns == [1, 15, 16, 17, 31, 32, 33, 1039]
    assert FI.CASES["segments"]["seg_n"] == (1, 63, 64, 65, 130, 1) and FI.CASES["segments"]["n_global"] == 200 and FI.CASES["segments"]["n"] == 324
    m = FI.CASES["max"]
    assert (m["width"], m["out"], m["obs_dim"]) == (512, 512, 16) and FI.CASES["odd"]["A"] + 1 == 16


def test_the_flag_is_known_and_off_by_default():
    assert _args([]).fused_update is False
    assert _args(["--fused_update"]).fused_update is True


def test_check_fused_update_refuses_by_name(monkeypatch):
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ok = dict(architecture="mlpmodel")
    train.check_fused_update(ok, "ppo")
    train.check_fused_update(dict(ok, x_entropy_coef=0.0, fs_coef=0.0, recurrent=False), "ppo-pure")
    for hp, algo, word in ((dict(architecture="impala"), "ppo", "architecture impala"), ({}, "ppo", "architecture impala"),
                           (dict(ok, recurrent=True), "ppo", "recurrent: True"), (ok, "IPL", "algo: IPL"), (ok, "sae", "algo: sae"),
                           (dict(ok, x_entropy_coef=0.05), "ppo", "x_entropy_coef"), (dict(ok, fs_coef=0.5), "ppo", "fs_coef")):
        with pytest.raises(NotImplementedError, match="--fused_update.*" + word):
            train.check_fused_update(hp, algo)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="--fused_update.*WORLD_SIZE = 2"):
        train.check_fused_update(ok, "ppo")


def test_train_refuses_before_an_env_exists(monkeypatch):
    """train.train_ppo with --fused_update: past every refusal it reaches make_env with hp["fused_update"] set, with or without
    --device_env; every refusal comes before make_env."""
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cp = ["--env_name", "cartpole", "--param_name", "cartpole", "--fused_update"]

    class Reached(Exception):
        pass

    def built(env_name, n_envs, seed, A, args, hp, *a, **k):
        raise Reached(f"{env_name} fused_update={hp.get('fused_update')}")
    monkeypatch.setattr(train, "make_env", built)
    for extra in ([], ["--device_env"], ["--device_env", "--resident_rollout"]):
        with pytest.raises(Reached, match="cartpole fused_update=True"):
            train.train_ppo(_args(cp + extra))
    with pytest.raises(Reached, match="mountain_car fused_update=True"):
        train.train_ppo(_args(["--env_name", "mountain_car", "--param_name", "mountain_car", "--fused_update"]))
    with pytest.raises(Reached, match="cartpole fused_update=None"):                       # without the flag nothing is set
        train.train_ppo(_args(cp[:-1]))
    monkeypatch.setattr(train, "make_env", lambda *a, **k: pytest.fail("an env was built"))
    with pytest.raises(NotImplementedError, match="--fused_update with architecture impala"):
        train.train_ppo(_args(["--env_name", "coinrun", "--param_name", "hard-500", "--fused_update"]))
    with pytest.raises(NotImplementedError, match="--fused_update with algo: IPL"):
        train.train_ppo(_args(cp + ["--algo", "IPL"]))
    with pytest.raises(NotImplementedError, match="--fused_update with algo: sae"):
        train.train_ppo(_args(cp + ["--algo", "sae"]))
    with pytest.raises(NotImplementedError, match="--fused_update with x_entropy_coef = 0.05"):
        train.train_ppo(_args(cp + ["--x_entropy_coef", "0.05"]))
    with pytest.raises(NotImplementedError, match="--fused_update with fs_coef = 0.5"):
        train.train_ppo(_args(cp + ["--fs_coef", "0.5"]))
    base = train.get_hyperparams
    monkeypatch.setattr(train, "get_hyperparams", lambda name: dict(base(name), recurrent=True))
    with pytest.raises(NotImplementedError, match="--fused_update with recurrent: True"):
        train.train_ppo(_args(cp))
    monkeypatch.setattr(train, "get_hyperparams", base)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="--fused_update runs on a single GPU"):
        train.train_ppo(_args(cp))


def _fake_policy(arch="mlp", recurrent=False):
    return types.SimpleNamespace(arch=arch, is_recurrent=lambda: recurrent)


def test_the_agents_refuse_by_name(monkeypatch):
    """PPO.__init__ (and PPOPure through it) with fused_update=True: every refusal is raised before an engine is created."""
    import agents.ppo as P
    from agents.ppo_pure import PPOPure
    monkeypatch.setattr(P, "Engine", lambda *a, **k: pytest.fail("an engine was created"))
    mk = lambda cls, policy, **kw: cls(None, policy, None, None, torch.device("cpu"), 1, n_steps=8, n_envs=16, fused_update=True, **kw)
    for cls in (P.PPO, PPOPure):
        with pytest.raises(ValueError, match="fused_update needs an mlpmodel policy"):
            mk(cls, _fake_policy("impala"))
        with pytest.raises(ValueError, match="fused_update needs x_entropy_coef == 0"):
            mk(cls, _fake_policy(), x_entropy_coef=0.05)
    with pytest.raises(ValueError, match="fused_update needs fs_coef == 0"):      # (ppo-pure has no such term: it passes fs_coef = 0 on)
        mk(P.PPO, _fake_policy(), fs_coef=0.5)
    with pytest.raises(ValueError, match="fused_update does not support a recurrent policy"):
        mk(P.PPO, _fake_policy(recurrent=True))
    with pytest.raises((ValueError, NotImplementedError), match="recurrent"):
        mk(PPOPure, types.SimpleNamespace(arch="mlp", is_recurrent=lambda: True, logsumexp_logits_is_v=False), n_minibatch=1, mini_batch_size=128)
    monkeypatch.setattr(P, "Collective", lambda: types.SimpleNamespace(active=True, world=2, rank=0))
    with pytest.raises(ValueError, match="fused_update runs on one rank only"):
        mk(P.PPO, _fake_policy())


def test_the_header_declares_the_entry_and_the_engine_binds_it():
    text = open(os.path.join(ROOT, "include", "mi355ppo.h")).read()
    assert re.search(r"int mi_minibatch_fused\(mi_ctx\* ctx, const int64_t\* idx, int32_t n_idx, const int32_t\* seg_n, int32_t n_seg, int32_t n_global,\s*"
                     r"const mi_hparams\* hp\);", text)
    from mi355 import engine
    assert "mi_minibatch_fused" in engine.EXPORTS and callable(engine.Engine.minibatch_fused)
