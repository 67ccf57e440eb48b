"""The fused MLP minibatch pass on the MI355X (csrc/mlp_fused.hip, mi_minibatch_fused, Engine.minibatch_fused, PPO(fused_update=True),
train.py --fused_update) against the reference project's own minibatch, the float64 reference of tests/fused_update_inputs.py, the
chain of launches it stands beside, and itself.  Bounds: fused_update_inputs' docstring."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fused_update_inputs as FI
import policy_inputs as PI
from conftest import PKG, ROOT, npz_json
from oracle import ppo_oracle as O

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)


def _engine(c, b, max_batch=None, **kw):
    """an engine of case c's network with b's rings loaded"""
    from mi355 import engine as M
    cfg = dict(obs_dim=c["obs_dim"], mlp_depth=c["depth"], mlp_width=c["width"], out_dim=c["out"], value_from_logits=bool(c["lse"]))
    cfg.update(kw)
    eng = M.Engine("mlp", b["T"], b["E"], c["A"], max(max_batch or b["n"], b["E"]), **cfg)
    eng.set_params(b["flat"])
    for t in range(b["T"] + 1):
        eng.put_obs(t, b["obs"][t])
    eng.write_field(M.F_ACT, b["act"].astype(np.float32)); eng.write_field(M.F_LOGP, b["old_logp"]); eng.write_field(M.F_VALUE, b["old_value"])
    eng.write_field(M.F_ADV, b["adv"]); eng.write_field(M.F_RET, b["ret"])
    eng.sync()
    return eng


def _hp(eng, hp=None):
    return eng.hparams(**(FI.HP if hp is None else hp))


def _stats_rows(eng, k):
    """the first k 32-float rows of the statistics ring"""
    from mi355 import engine as M
    from mi355.dist import DevicePointerTensor
    eng.sync()
    p, n = eng.device_ptr(M.PTR_STATS_RING)
    return DevicePointerTensor(p, n).tensor(0)[:32 * k].cpu().numpy().reshape(k, 32).copy()


def _run(c, b, fused=True, eng=None):
    """one pass on a fresh engine (or eng) -> (gradient vector, statistics rows, log records)"""
    own = eng is None
    eng = _engine(c, b) if own else eng
    if fused:
        eng.minibatch_fused(b["idx"], b["seg_n"], b["n_global"], _hp(eng))
    elif len(b["seg_n"]) > 1:
        eng.minibatch_multi(b["idx"], b["seg_n"], b["n_global"], _hp(eng))
    else:
        eng.minibatch(b["idx"], b["n_global"], _hp(eng))
    out = eng.get_grads(), _stats_rows(eng, len(b["seg_n"])), eng.loss_log()
    if own:
        eng.close()
    return out


def _check_records(stats, log, c, ref, what):
    _, eps_q = FI.torch_errors(c)
    assert log.shape == (len(ref["loss"]["seg"]), 8)
    return max(PI.check_record(stats[k], log[k], ref["loss"], k, c["A"], FI.HP, eps_q, what=what) for k in range(len(log)))


# ------------------------------------------------------------------------------------------ 1: the reference's own numbers
def _check_grads(flat_g, shapes, ref_grads, rtol=1e-3):
    """tests/test_gpu_engine.py's rule: every tensor within rtol of the reference tensor's norm"""
    from mi355 import layout
    g = layout.unflatten(shapes, flat_g)
    for k, r in ref_grads.items():
        r = np.asarray(r, dtype=np.float64)
        err = np.sqrt(((g[k].astype(np.float64) - r) ** 2).sum()) / (np.sqrt((r ** 2).sum()) + 1e-7)
        assert err < rtol, (k, err)


def test_g4_loss_and_grads_golden_through_the_fused_pass():
    """The mlp / raw leg of tests/test_gpu_engine.py::test_g4_loss_and_grads_golden through Engine.minibatch_fused, same assertions: one
    minibatch of B = 32 against what the reference's PPO.optimize produced, then clip + Adam step 1 against the oracle's."""
    from mi355 import engine as M, layout
    z, c, b, hp = FI.g4_case()
    T, E = b["T"], b["E"]
    shapes = FI.shapes_of(c)
    eng = M.Engine("mlp", T, E, 2, T * E, obs_dim=9, mlp_depth=4, mlp_width=256, out_dim=64)
    eng.set_params(b["flat"])
    for t in range(T + 1):
        eng.put_obs(t, z["in/frames"][t])
    for t in range(T):
        eng.put_step(t, z["in/rew"][t], z["in/done"][t])
    eng.write_field(M.F_ACT, z["in/act"].astype(np.float32)); eng.write_field(M.F_LOGP, z["in/logp"]); eng.write_field(M.F_VALUE, z["in/val"])
    eng.compute_estimates(0.999, 0.95, True, True)
    np.testing.assert_allclose(eng.read_field(M.F_ADV), z["adv"], rtol=0, atol=2e-6)
    assert np.array_equal(eng.read_field(M.F_RET), z["ret"])
    eng.minibatch_fused(np.random.default_rng(0).permutation(T * E), [T * E], T * E, eng.hparams(0.2, 0.5, 0.01, 0.0, 1.0, 0.0))
    rec = eng.loss_log()[0]
    ref = npz_json(z, "raw/summary")
    assert abs(-rec[0] - ref["Loss/pi"]) < 1e-5
    assert abs(-rec[1] - ref["Loss/v"]) < 1e-5 * max(1.0, abs(ref["Loss/v"]))
    assert abs(rec[2] - ref["Loss/entropy"]) < 1e-5
    assert abs(rec[3] - ref["Loss/x_entropy"]) < 1e-5
    assert abs(rec[4] - ref["Loss/total"]) < 1e-5 * max(1.0, abs(ref["Loss/total"]))
    flat_g = eng.get_grads()
    g = layout.unflatten(shapes, flat_g)
    for k, (nrm, _) in npz_json(z, "raw/grad_stats").items():
        mine = float(np.sqrt((g[k].astype(np.float64) ** 2).sum()))
        assert abs(mine - nrm) < 1e-3 * nrm + 1e-7, (k, mine, nrm)
    _check_grads(flat_g, shapes, {k[len("raw/g/"):]: z[k] for k in z.files if k.startswith("raw/g/")})
    total = float(np.sqrt((flat_g.astype(np.float64) ** 2).sum()))
    assert abs(total - float(z["raw/grad_total_norm"])) < 1e-4 * total
    params = layout.unflatten(shapes, b["flat"])
    p0 = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    gr = {k: torch.from_numpy(g[k].copy()) for k in p0}
    m0 = {k: torch.zeros_like(v) for k, v in p0.items()}
    v0 = {k: torch.zeros_like(v) for k, v in p0.items()}
    nrm, coef = O.clip_grad_norm(gr, 0.5)
    O.adam_step(p0, gr, m0, v0, 1, 5e-4)
    gn = eng.optimizer_step(5e-4, 0.5, 1, want_norm=True)
    assert abs(gn - nrm) < 1e-5 * nrm
    newp = layout.unflatten(shapes, eng.get_params())
    for k in p0:
        np.testing.assert_allclose(newp[k], p0[k].numpy(), rtol=0, atol=2e-6)
    m1 = layout.unflatten(shapes, eng.get_adam_state()[0])
    for k in p0:
        np.testing.assert_allclose(m1[k], m0[k].numpy(), rtol=1e-3, atol=1e-9)
    assert not eng.get_grads().any()          # zero_grad
    eng.close()


# ------------------------------------------------------------------------------------------ 2: against float64, per case
@pytest.mark.parametrize("name", list(FI.CASES))
def test_fused_pass_against_float64(name):
    """Every gradient tensor within 8 x torch's float32 error of the float64 reference, every segment's statistics row and log record
    within policy_inputs.record_bounds."""
    c = FI.CASES[name]
    b, ref = FI.case(c), FI.ref64(c)
    terr, _ = FI.torch_errors(c)
    grads, stats, log = _run(c, b)
    worst = _check_records(stats, log, c, ref, name)
    print(f"{name}: records: largest error / bound {worst:.3f}")
    FI.check_grads(grads, c, ref["grads"], terr, what=name)


# ------------------------------------------------------------------------------------------ 3: accumulation
def test_gradients_accumulate_until_the_optimizer_step():
    """Two different passes without a step in between: the buffer holds the float64 sum of both references.  After optimizer_step the
    buffer is zero and a third pass stands alone (against the float64 reference at the stepped parameters)."""
    c = FI.CASES["base1039"]
    b = FI.case(c)
    terr, _ = FI.torch_errors(c)
    sub = lambda lo, hi, **kw: dict(b, idx=b["idx"][lo:hi], seg_n=(hi - lo,), n_global=hi - lo, n=hi - lo, **kw)
    b1, b2 = sub(0, 500), sub(500, 1039)
    eng = _engine(c, b)
    eng.minibatch_fused(b1["idx"], b1["seg_n"], b1["n_global"], _hp(eng))
    eng.minibatch_fused(b2["idx"], b2["seg_n"], b2["n_global"], _hp(eng))
    r1, r2 = FI.reference(c, b1), FI.reference(c, b2)
    both = {k: r1["grads"][k] + r2["grads"][k] for k in r1["grads"]}
    FI.check_grads(eng.get_grads(), c, both, terr, what="two passes")
    assert eng.loss_log().shape == (2, 8)
    eng.optimizer_step(1e-6, 0.5, 1)            # (a step of 1e-6 per parameter: every sample keeps its regime)
    assert not eng.get_grads().any()
    b3 = sub(7, 40, flat=eng.get_params())
    eng.minibatch_fused(b3["idx"], b3["seg_n"], b3["n_global"], _hp(eng))
    r3 = FI.reference(c, b3)
    assert not PI.loss_excluded(r3["loss"], FI.HP, margin=FI.MARGIN / 2).any()
    terr3, _ = FI.torch_errors(dict(c, n=33))
    FI.check_grads(eng.get_grads(), c, r3["grads"], terr3, what="third pass")
    eng.close()


# ------------------------------------------------------------------------------------------ 4: beside the chain
@pytest.mark.parametrize("name", ("wide", "segments", "lse"))
def test_fused_pass_beside_the_chain(name):
    """A twin engine with the same parameters and rings runs mi_minibatch / mi_minibatch_multi: the gradient tensors of the two paths lie
    within 16 x torch's float32 error of each other (the two-path bound of tests/test_gpu_resident_rollout.py), and the records of both
    satisfy the same check."""
    from mi355 import layout
    c = FI.CASES[name]
    b, ref = FI.case(c), FI.ref64(c)
    terr, _ = FI.torch_errors(c)
    gf, sf, lf = _run(c, b)
    gc, sc, lc = _run(c, b, fused=False)
    chain = layout.unflatten(FI.shapes_of(c), gc)
    FI.check_grads(gc, c, ref["grads"], terr, factor=float("inf"), what=name + " (for the record) the chain against float64")
    FI.check_grads(gf, c, {k: v.astype(np.float64) for k, v in chain.items()}, terr, factor=16, what=name + " fused against the chain")
    print(f"{name}: records, largest error / bound: fused {_check_records(sf, lf, c, ref, name + ' fused'):.3f}, chain {_check_records(sc, lc, c, ref, name + ' chain'):.3f}")


# ------------------------------------------------------------------------------------------ 5: determinism
@pytest.mark.parametrize("name", ("base1039", "segments"))
def test_two_fresh_engines_give_the_same_bits(name):
    c = FI.CASES[name]
    b = FI.case(c)
    a1, a2 = _run(c, b), _run(c, b)
    for x, y, what in zip(a1, a2, ("gradients", "statistics rows", "records")):
        assert np.array_equal(x, y), what
    assert a1[0].any() and np.isfinite(a1[0]).all()


# ------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_by_name_change_nothing():
    """Each refusal of mi_minibatch_fused by its words; after a refused call get_grads(), loss_log() and the next accepted pass's result
    are what they are without it."""
    from mi355 import engine as M
    c = FI.CASES["base33"]
    b = FI.case(c)
    n, idx, TE = b["n"], b["idx"], b["T"] * b["E"]
    p1, p2 = (idx[:20], (20,), 20), (idx[5:33], (10, 18), 28)
    ctl = _engine(c, b)
    ctl.minibatch_fused(*p1, _hp(ctl))
    g1, l1 = ctl.get_grads(), ctl.loss_log(reset=False)
    ctl.minibatch_fused(*p2, _hp(ctl))
    g2, l2 = ctl.get_grads(), ctl.loss_log(reset=False)
    ctl.close()
    assert g1.any() and l1.shape == (1, 8) and l2.shape == (3, 8)

    eng = _engine(c, b)
    eng.minibatch_fused(*p1, _hp(eng))

    def refused(msg, call):
        with pytest.raises(M.EngineError, match="mi_minibatch_fused: " + msg):
            call()
        assert np.array_equal(eng.get_grads(), g1) and np.array_equal(eng.loss_log(reset=False), l1), msg

    hp = _hp(eng)
    refused("x_entropy_coef and fs_coef must be 0", lambda: eng.minibatch_fused(idx, [n], n, _hp(eng, dict(FI.HP, x_entropy_coef=0.05))))
    refused("x_entropy_coef and fs_coef must be 0", lambda: eng.minibatch_fused(idx, [n], n, eng.hparams(fs_coef=0.5)))
    refused("n_idx must be in", lambda: eng.minibatch_fused(idx[:0], [1], 1, hp))
    refused("n_idx must be in", lambda: eng.minibatch_fused(np.concatenate([idx, idx]), [2 * n], 2 * n, hp))
    refused("n_global must be at least 1", lambda: eng.minibatch_fused(idx, [n], 0, hp))
    refused("every segment needs at least one sample", lambda: eng.minibatch_fused(idx, [0, n], n, hp))
    refused("segments do not add up to n_idx", lambda: eng.minibatch_fused(idx, [n - 1], n, hp))
    refused("1 .. 16 segments", lambda: eng.minibatch_fused(idx, [1] * 17 + [n - 17], n, hp))
    bad = idx.copy(); bad[-1] = TE
    refused("minibatch index out of range", lambda: eng.minibatch_fused(bad, [n], n, hp))
    bad[-1] = -1
    refused("minibatch index out of range", lambda: eng.minibatch_fused(bad, [n], n, hp))
    eng.set_multirank(1)
    refused("multirank mode must be 0", lambda: eng.minibatch_fused(idx, [n], n, hp))
    eng.set_multirank(2)
    refused("multirank mode must be 0", lambda: eng.minibatch_fused(idx, [n], n, hp))
    eng.set_multirank(0)
    eng.minibatch_fused(*p2, hp)                 # the next accepted pass: the control's bits
    assert np.array_equal(eng.get_grads(), g2) and np.array_equal(eng.loss_log(reset=False), l2)
    # a full loss log (4096 records)
    eng.optimizer_step(1e-6, 0.5, 1)
    eng.loss_log()
    one = idx[:1]
    for _ in range(4096 // 16):
        eng.minibatch_fused(np.repeat(one, 16), [1] * 16, 1, hp)
    g_full, l_full = eng.get_grads(), eng.loss_log(reset=False)
    assert l_full.shape == (4096, 8)
    with pytest.raises(M.EngineError, match="mi_minibatch_fused: loss log full"):
        eng.minibatch_fused(one, [1], 1, hp)
    assert np.array_equal(eng.get_grads(), g_full) and np.array_equal(eng.loss_log(), l_full)
    # a pending minibatch of multirank mode 1
    eng.set_multirank(1)
    eng.minibatch(idx[:8], 8, hp)
    eng.set_multirank(0)
    with pytest.raises(M.EngineError, match="mi_minibatch_fused: previous multirank minibatch not finished"):
        eng.minibatch_fused(idx, [n], n, hp)
    eng.set_multirank(1); eng.minibatch_finish(); eng.set_multirank(0)
    eng.loss_log()
    # an initialised communicator
    eng.comm_init(eng.comm_unique_id(), 0, 1)
    with pytest.raises(M.EngineError, match="mi_minibatch_fused: an armed or in-flight gradient exchange or an initialised communicator"):
        eng.minibatch_fused(idx, [n], n, hp)
    assert eng.loss_log().shape == (0, 8)
    eng.close()
    # a recurrent context
    eng = _engine(c, b)
    H, rng = c["out"], np.random.default_rng(9)
    eng.set_gru(*(0.1 * rng.standard_normal(k).astype(np.float32) for k in (3 * H * H, 3 * H * H, 3 * H, 3 * H)))
    with pytest.raises(M.EngineError, match="mi_minibatch_fused: a recurrent context"):
        eng.minibatch_fused(idx, [n], n, _hp(eng))
    assert not eng.get_grads().any() and eng.loss_log().shape == (0, 8)
    eng.close()
    # an IMPALA context
    eng = M.Engine("impala", 2, 4, 15, 8)
    with pytest.raises(M.EngineError, match="mi_minibatch_fused: the context's arch must be MI_ARCH_MLP"):
        eng.minibatch_fused(np.arange(8), [8], 8, eng.hparams())
    assert not eng.get_grads().any() and eng.loss_log().shape == (0, 8)
    eng.close()
    # shapes outside the list: the chain takes them
    T, E = 2, 8
    for kw, A, msg in ((dict(mlp_width=72), 2, "mlp_width must be a multiple of 16 and at most 512"), (dict(mlp_width=528), 2, "mlp_width must be a multiple of 16 and at most 512"),
                       (dict(out_dim=40), 2, "out_dim must be a multiple of 16 and at most 512"), (dict(mlp_depth=17), 2, "mlp_depth must be at least 2 and at most 16"),
                       (dict(), 16, "n_actions must be at most 15"), (dict(obs_dim=17), 2, "obs_dim must be at most 16")):
        cfg = dict(dict(obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64), **kw)
        eng = M.Engine("mlp", T, E, A, T * E, **cfg)
        eng.set_params((0.1 * rng.standard_normal(eng.n_params)).astype(np.float32))
        for t in range(T + 1):
            eng.put_obs(t, rng.standard_normal((E, cfg["obs_dim"])).astype(np.float32))
        eng.write_field(M.F_ACT, rng.integers(0, A, (T, E)).astype(np.float32))
        for f in (M.F_LOGP, M.F_ADV, M.F_RET):
            eng.write_field(f, rng.standard_normal((T, E)).astype(np.float32))
        with pytest.raises(M.EngineError, match="mi_minibatch_fused: " + msg):
            eng.minibatch_fused(np.arange(T * E), [T * E], T * E, eng.hparams())
        assert not eng.get_grads().any() and eng.loss_log().shape == (0, 8)
        eng.minibatch(np.arange(T * E), T * E, eng.hparams())
        assert eng.get_grads().any() and np.isfinite(eng.loss_log()).all()
        eng.close()


# ------------------------------------------------------------------------------------------ 7: agent and command line
def test_ppo_updates_through_the_fused_pass():
    """PPO(fused_update=True) on DeviceCartPole (E 16, T 8, a 4 x 64 -> 64 MLP) beside PPO(fused_update=False), from the same parameters,
    the same rollout rings and the same permutation: one optimize() goes through minibatch_fused only (two merged passes of two
    minibatches each), the other never; every entry of the logged loss summary agrees with the chain's within 1e-5 relative."""
    from agents.ppo import PPO
    from common.env.vec_envs import DeviceCartPole
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    from mi355.engine import F_ADV, F_LOGP
    T, E = 8, 16
    dev = torch.device("cuda", 0)
    out = {}
    for fused in (True, False):
        torch.manual_seed(0)
        policy = CategoricalPolicy(MLPModel(9, 4, 64, 64), False, 2)
        agent = PPO(DeviceCartPole(E, seed=4, max_steps=5, h_range=0.06), policy, Logger(E, None), Storage((9,), 64, T, E, dev), dev, 1, n_steps=T, n_envs=E,
                    epoch=1, n_minibatch=2, mini_batch_size=32, gamma=0.99, lmbda=0.95, learning_rate=1e-3, entropy_coef=0.01, seed=0, detect_nan=True,
                    fused_update=fused)
        assert agent.fused_update is fused
        calls = {"minibatch_fused": 0, "minibatch": 0, "minibatch_multi": 0}
        for name in calls:
            real = getattr(agent.engine, name)
            setattr(agent.engine, name, lambda *a, name=name, real=real: calls.__setitem__(name, calls[name] + 1) or real(*a))
        real_opt, seen = agent.optimize, {}

        def optimize(real_opt=real_opt, agent=agent, seen=seen):
            seen["rings"] = (agent.engine.read_field(F_ADV), agent.engine.read_field(F_LOGP))
            seen["summary"] = real_opt()
            return seen["summary"]
        agent.optimize = optimize
        torch.manual_seed(1)
        agent.train(T * E)
        out[fused] = (calls, seen, agent.engine.get_params())
        agent.engine.close()
    (cf, sf, pf), (cc, sc, pc) = out[True], out[False]
    assert cf == {"minibatch_fused": 2, "minibatch": 0, "minibatch_multi": 0}, cf
    assert cc["minibatch_fused"] == 0 and cc["minibatch"] + cc["minibatch_multi"] == 2, cc
    for x, y in zip(sf["rings"], sc["rings"]):
        assert np.array_equal(x, y)
    for k in ("Loss/pi", "Loss/v", "Loss/entropy", "Loss/x_entropy", "Loss/total"):
        a, r = sf["summary"][k], sc["summary"][k]
        print(f"{k}: fused {a!r} chain {r!r}")
        assert np.isfinite(a) and abs(a - r) <= 1e-5 * abs(r), (k, a, r)
    assert np.isfinite(pf).all() and np.isfinite(pc).all()


def test_train_cli_runs_the_cartpole_with_the_fused_update(tmp_path):
    """`python train.py --env_name cartpole --param_name cartpole --device_env --resident_rollout --fused_update` in a fresh child process:
    two iterations, log rows, a checkpoint, and the banner names the fused update."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "--exp_name", "dev", "--env_name", "cartpole", "--param_name", "cartpole",
           "--n_envs", "8", "--n_steps", "16", "--mini_batch_size", "32", "--seed", "3", "--detect_nan", "--num_timesteps", "250",
           "--num_checkpoints", "1", "--device_env", "--resident_rollout", "--fused_update"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "update: fused MLP minibatch pass, two kernel launches per minibatch (--fused_update)" in r.stdout
    assert "rollout: device-resident env, one kernel launch per rollout" in r.stdout
    runs = os.listdir(tmp_path / "logs" / "train" / "cartpole" / "dev")
    assert len(runs) == 1 and runs[0].endswith("__seed_3")
    rd = tmp_path / "logs" / "train" / "cartpole" / "dev" / runs[0]
    assert {"hyperparameters.npy", "config.npy", "log-append.csv", "model_256.pth"} <= set(os.listdir(rd))
    assert np.load(rd / "hyperparameters.npy", allow_pickle=True).item()["fused_update"] is True
    rows = open(rd / "log-append.csv").read().strip().splitlines()
    assert len(rows) == 3 and [float(row.split(",")[0]) for row in rows[1:]] == [128.0, 256.0]
    assert np.isfinite([float(v) for row in rows[1:] for v in row.split(",") if v not in ("", "nan")]).all()
