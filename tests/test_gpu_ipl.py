"""The IPL agent on the MI355X (`algo: IPL`; csrc/ipl.hip, mi_ipl_minibatch, agents/ipl.py): the loss kernels against float64 autograd
per element, the reference's own IPL.optimize (fixture G16) through the engine in fp32 and bf16, the gradient path through obs[t + 1] on
its own, and the agent / CLI end to end.  Every test here calls symbols that exist only with the feature.

Bounds.  Per-sample quantities (dY, g_next, pred): atol 2e-6, the value the existing loss tests use.  Record terms: 1e-5 * max(1, |ref|),
as G4.  First-backward gradients: per tensor relative L2 < 1e-3 (_check_grads' measure, on the fixture's whole tensors / sketches).
Parameters and Adam moments: the per-step bounds of test_g56_optimize_trajectory on every tensor's norm (2e-6 / 1e-4 / 5e-3 x max(1, norm)
after optimizer step 1 / 2 / 3..8)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ipl_inputs as II
import sae_inputs as SI
from conftest import PKG, ROOT, load_npz, npz_json

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

FLAG_SETS = [(em, ri, ai) for em in (False, True) for ri in (False, True) for ai in (False, True)]
STEP_TOL = {1: 2e-6, 2: 1e-4}          # optimizer step -> bound on a tensor's norm (x max(1, norm)); later steps 5e-3


@pytest.fixture(scope="module")
def op_engine():
    from mi355.engine import Engine
    eng = Engine("mlp", 2, 2, 2, 4, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64)
    yield eng
    eng.close()


def _engine(c, max_batch, precision="fp32"):
    from mi355.engine import Engine
    if c["arch"] == "impala":
        return Engine("impala", c["T"], c["E"], c["A"], max_batch, precision=precision)
    return Engine("mlp", c["T"], c["E"], c["A"], max_batch, obs_dim=9, mlp_depth=4, mlp_width=256, out_dim=64)


def _shapes(c):
    from mi355 import layout
    return layout.impala_param_shapes(c["A"]) if c["arch"] == "impala" else layout.mlp_param_shapes(c["A"], 9, 4, 256, 64)


def _load(eng, c, roll, params):
    from mi355 import engine as M, layout
    eng.set_params(layout.flatten(_shapes(c), params))
    for t in range(c["T"] + 1):
        eng.put_obs(t, roll["frames"][t])
    for t in range(c["T"]):
        eng.put_step(t, roll["rew"][t], roll["done"][t])
    eng.write_field(M.F_ACT, roll["act"].astype(np.float32))
    eng.write_field(M.F_VALUE, roll["value"])
    eng.sync()


def _hp(eng, c, **over):
    o = dict(II.opts(c), **over)
    return eng.ipl_hparams(c["gamma"], o["alpha"], o["entropy_coef"], o["entropy_modified"], o["reward_incentive"], o["adv_incentive"],
                           debug_zero_obs_seed=o.get("debug_zero_obs_seed", False))


def _terms_close(mine, ref, tol=1e-5, corr_tol=1e-5):
    for j, k in enumerate(II.TERMS):
        if np.isnan(ref[j]):
            assert np.isnan(mine[j]), (k, mine[j])
        else:
            bound = corr_tol if k == "rew_corr" else tol * max(1.0, abs(ref[j]))
            assert abs(mine[j] - ref[j]) < bound, (k, mine[j], ref[j])


# ------------------------------------------------------------------------------------------------ the kernels alone
def _op_reference(hout, nv_raw, act, rew, done, gamma, alpha, ec, em, ri, ai):
    h = torch.from_numpy(hout.astype(np.float64)).requires_grad_(True)
    nv = torch.from_numpy(nv_raw.astype(np.float64)).requires_grad_(True)
    A = hout.shape[1] - 1
    lp = torch.log_softmax(h[:, :A], dim=1)
    lp = lp - lp.logsumexp(dim=-1, keepdim=True)
    o = dict(alpha=alpha, entropy_coef=ec, entropy_modified=em, reward_incentive=ri, adv_incentive=ai)
    loss, pred, terms = II.ipl_terms(lp, h[:, A], nv, torch.from_numpy(act), torch.from_numpy(rew.astype(np.float64)),
                                     torch.from_numpy(done.astype(np.float64)), gamma, o)
    loss.backward()
    return II.terms_row(terms, gamma, alpha), h.grad.numpy(), nv.grad.numpy(), pred.detach().numpy()


@pytest.mark.parametrize("A", [2, 9, 15])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_op_ipl_loss_against_float64_autograd(op_engine, n, A):
    """mi_op_ipl_loss (next value, loss + finaliser, next-side seed) on random head rows, ~25 % done rows, all 8 flag combinations,
    per element against float64 autograd.  rew_corr: max(1e-5, 10 x floor); the floor -- the reference's float32 corrcoef stored in
    G16 against the float64 recomputation from the stored pred / rew -- measured 3.4e-8 (a), 1.3e-8 (b), 2.5e-8 (c), so 1e-5."""
    rng = np.random.default_rng(1000 * n + A)
    hout = rng.standard_normal((n, A + 1)).astype(np.float32)
    nv_raw, rew = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    done = (rng.random(n) < 0.25).astype(np.float32)
    act = rng.integers(0, A, size=n).astype(np.int64)
    gamma, alpha, ec = 0.99, 0.7, 0.02
    for em, ri, ai in FLAG_SETS:
        hp = op_engine.ipl_hparams(gamma, alpha, ec, em, ri, ai)
        rec, dY, gn, pred = op_engine.op_ipl_loss(hout, nv_raw, act, rew, done, hp)
        ref_rec, ref_dY, ref_gn, ref_pred = _op_reference(hout, nv_raw, act, rew, done, gamma, alpha, ec, em, ri, ai)
        tag = (n, A, em, ri, ai)
        print(tag, "dY", np.abs(dY - ref_dY).max(), "g_next", np.abs(gn - ref_gn).max(), "pred", np.abs(pred - ref_pred).max(),
              "terms", np.nanmax(np.abs(rec - ref_rec)))
        assert np.abs(dY - ref_dY).max() < 2e-6, tag
        assert np.abs(gn - ref_gn).max() < 2e-6, tag
        assert np.abs(pred - ref_pred).max() < 2e-6, tag
        assert (gn[done > 0] == 0).all() and (ref_gn[done > 0] == 0).all(), tag
        _terms_close(rec, ref_rec)


def test_op_ipl_ties_take_the_lower_index(op_engine):
    """Rows whose two largest logits are equal: the greedy action and the max term pick the lower index (torch.max / argmax); forward
    values only."""
    rng = np.random.default_rng(5)
    n, A = 70, 9
    hout = rng.standard_normal((n, A + 1)).astype(np.float32)
    lo, hi = rng.integers(0, A - 1, size=n), None
    hi = np.array([rng.integers(l + 1, A) for l in lo])
    top = hout[:, :A].max(1) + np.float32(0.5)
    hout[np.arange(n), lo] = top
    hout[np.arange(n), hi] = top
    assert np.array_equal(op_engine.op_ipl_greedy(hout), lo.astype(np.int32))
    nv_raw, rew = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    done, act = (rng.random(n) < 0.25).astype(np.float32), rng.integers(0, A, size=n).astype(np.int64)
    rec, _, _, pred = op_engine.op_ipl_loss(hout, nv_raw, act, rew, done, op_engine.ipl_hparams(0.99, 1.0, 0.0, False, False, True))
    ref_rec, _, _, ref_pred = _op_reference(hout, nv_raw, act, rew, done, 0.99, 1.0, 0.0, False, False, True)
    assert np.abs(pred - ref_pred).max() < 2e-6
    _terms_close(rec, ref_rec)


# ------------------------------------------------------------------------------------------------ G16 through the engine
def _run_case(name, precision="fp32"):
    z = load_npz("g16_ipl.npz")
    c, roll, params, idx = II.load_case(z, name)
    eng = _engine(c, len(idx[0]), precision)
    _load(eng, c, roll, params)
    hp = _hp(eng, c)
    steps = set(II.step_schedule(c))
    out = dict(z=z, c=c, norms=[], g0=None, pred0=None, params0=params, roll=roll, idx=idx)
    from mi355 import layout
    nstep = 0
    for k, ix in enumerate(idx):
        eng.ipl_minibatch(ix, len(ix), hp)
        if k == 0:
            out["g0"] = layout.unflatten(_shapes(c), eng.get_grads())
            out["pred0"], out["rew0"] = eng.ipl_read_pred(len(ix))
        if k + 1 in steps:
            nstep += 1
            eng.optimizer_step(II.LR, II.CLIP, nstep)
            p = layout.unflatten(_shapes(c), eng.get_params())
            m, v = (layout.unflatten(_shapes(c), a) for a in eng.get_adam_state())
            out["norms"].append([{n: float(np.linalg.norm(d[n].astype(np.float64))) for n in d} for d in (p, m, v)])
    out["pred_last"], _ = eng.ipl_read_pred(len(idx[-1]))
    out["log"] = eng.loss_log()
    out["params"], (out["m"], out["v"]) = layout.unflatten(_shapes(c), eng.get_params()), [layout.unflatten(_shapes(c), a) for a in eng.get_adam_state()]
    eng.close()
    return out


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_g16_fp32(name):
    r = _run_case(name)
    z = r["z"]
    ref_terms = z[f"{name}/terms"]
    assert r["log"].shape == ref_terms.shape
    first_step = II.step_schedule(r["c"])[0]
    for k in range(len(ref_terms)):
        print(name, k, np.nanmax(np.abs(r["log"][k] - ref_terms[k])))
    for k in range(first_step):
        _terms_close(r["log"][k], ref_terms[k])
    # pred against the golden's float32 pred: the reference's own error against float64 is 3.3e-6 on these rows (case a, |pred| up to 10;
    # measured with ipl_inputs.minibatch), so 2e-5 = 6 x that
    print(name, "pred0", np.abs(r["pred0"] - z[f"{name}/pred0"]).max(), "pred_last", np.abs(r["pred_last"] - z[f"{name}/pred_last"]).max())
    assert np.abs(r["pred0"] - z[f"{name}/pred0"]).max() < 2e-5
    assert np.array_equal(r["rew0"], z[f"{name}/rew0"])
    for n in r["g0"]:
        err = SI.tensor_error(r["g0"][n], z, f"{name}/g0/", n)
        print(name, "g0", n, err)
        assert err < 1e-3, (n, err)
    names = npz_json(z, f"{name}/tensor_names")
    ref_norms = z[f"{name}/step_norms"]
    assert len(r["norms"]) == len(ref_norms)
    for s, per in enumerate(r["norms"]):
        tol = STEP_TOL.get(s + 1, 5e-3)
        for q, what in enumerate(("param", "exp_avg", "exp_avg_sq")):
            for j, n in enumerate(names):
                assert abs(per[q][n] - ref_norms[s, q, j]) < tol * max(1.0, ref_norms[s, q, j]), (s + 1, what, n, per[q][n], ref_norms[s, q, j])
    for k in range(first_step, len(ref_terms)):
        _terms_close(r["log"][k], ref_terms[k])
    # The last minibatch's pred.  With no optimizer step in front of it (case a) the single-pass bound.  Behind steps: mi_optimizer_step is
    # the PPO path's, whose Adam kernel forms 1 - beta2 in fp32 (1.3e-5 off in exp_avg_sq, csrc/optim.hip; pinned as it is) -- every
    # update is off by up to that fraction of itself, so pred by up to 1.3e-5 x how far the steps moved it (float64 replay), on top
    _, moved_to = II.replay(r["c"], r["params0"], r["roll"], r["idx"])
    _, stayed, _ = II.minibatch(r["c"], r["params0"], r["roll"], r["idx"][-1])
    last_tol = 2e-5 + 1.3e-5 * float(np.abs(moved_to - stayed).max())
    print(name, "pred_last bound", last_tol)
    assert np.abs(r["pred_last"] - z[f"{name}/pred_last"]).max() < last_tol
    for n in ("fc_policy.weight", "fc_value.weight", "fc_value.bias"):
        np.testing.assert_allclose(r["params"][n], z[f"{name}/p/{n}"], rtol=0, atol=1.5e-2)


def test_next_obs_path_carries_gradient():
    """alpha = 0, no entropy / max term and the obs-side value detached in the float64 restatement: the whole gradient arrives through
    obs[t + 1].  The engine with alpha = 0 and the obs-side seed zeroed (MI_IPL_DEBUG_ZERO_OBS_SEED) must give that gradient -- and not
    zero.  Cases b (MLP) and c (IMPALA, n = 8): per tensor relative L2 < 1e-3, the first-backward bound.  Case a (IMPALA, n = 32): this
    part is 0.3 - 0.5 % of block 1's full gradient there (float64), and the first-backward bound pins the engine's passes to 1e-3 of the
    FULL gradient, which is all this summand of it can be asked to meet: 1e-3 x the norm of the fixture's g0 tensor, for every tensor."""
    from mi355 import layout
    z = load_npz("g16_ipl.npz")
    for name in ("a", "b", "c"):
        c, roll, params, idx = II.load_case(z, name)
        eng = _engine(c, len(idx[0]))
        _load(eng, c, roll, params)
        eng.ipl_minibatch(idx[0], len(idx[0]), _hp(eng, c, alpha=0.0, entropy_coef=0.0, adv_incentive=False, debug_zero_obs_seed=True))
        g = layout.unflatten(_shapes(c), eng.get_grads())
        eng.close()
        _, _, ref = II.minibatch(c, params, roll, idx[0], next_only=True)
        _, _, full = II.minibatch(c, params, roll, idx[0])
        assert float(np.linalg.norm(ref["fc_value.weight"])) > 1e-3 and not ref["fc_policy.weight"].any()
        for n, rg in ref.items():
            if not rg.any():                                # fc_policy: no path from obs[t + 1]
                assert not g[n].any(), (name, n)
                continue
            scale = np.linalg.norm(full[n]) if name == "a" else np.linalg.norm(rg)
            err = float(np.linalg.norm(g[n].astype(np.float64) - rg) / (scale + 1e-7))
            print(name, n, err, "of its own norm", float(np.linalg.norm(g[n].astype(np.float64) - rg) / (np.linalg.norm(rg) + 1e-7)))
            assert err < 1e-3, (name, n, err)
            assert np.linalg.norm(g[n]) > 0.5 * np.linalg.norm(rg), (name, n)
        for n in g:
            if n not in ref:
                assert not g[n].any(), n


def test_update_sized_bf16_pass_does_not_depend_on_the_side_stream():
    """n = 1024 in bf16 is where a backward pass takes the update-sized kernels and sums its weight-gradient slabs on the side stream
    beside block1.conv's launch; an IPL minibatch runs two such passes back to back into one gradient buffer.  The gradient, the record and
    pred are the same bits with the side stream switched off (mi_debug_flags bit 4) and on a second run: nothing depends on timing."""
    from mi355 import engine as M, layout
    from mi355.engine import Engine
    T, E, A, n = 4, 256, 15, 1024
    c = II.CASES["a"]
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(T + 1, E, 64, 64, 3), dtype=np.uint8)
    rew, done = rng.standard_normal((T, E)).astype(np.float32), (rng.random((T, E)) < 0.2).astype(np.float32)
    act = rng.integers(0, A, size=(T, E)).astype(np.float32)
    idx = rng.permutation(T * E)[:n]
    flat = layout.flatten(layout.impala_param_shapes(A), II.initial_params(c))
    runs = []
    for flags in (0, 16, 0):
        eng = Engine("impala", T, E, A, n, precision="bf16")
        eng.debug_flags(flags)
        eng.set_params(flat)
        for t in range(T + 1):
            eng.put_obs(t, frames[t])
        for t in range(T):
            eng.put_step(t, rew[t], done[t])
        eng.write_field(M.F_ACT, act)
        eng.ipl_minibatch(idx, n, eng.ipl_hparams(0.999, 1.0, 0.01, True, True, True))
        runs.append((eng.get_grads(), eng.loss_log()[0], eng.ipl_read_pred(n)[0]))
        eng.close()
    g, rec, pred = runs[0]
    assert np.isfinite(g).all() and np.linalg.norm(g) > 0 and np.isfinite(rec[[0, 1, 2, 3, 7]]).all()
    for g2, rec2, pred2 in runs[1:]:
        assert np.array_equal(g, g2) and np.array_equal(rec, rec2, equal_nan=True) and np.array_equal(pred, pred2)


def test_engine_refusals_name_the_thing():
    from mi355.engine import Engine, EngineError
    idx = np.arange(4)
    eng = Engine("mlp", 2, 4, 2, 4, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64)
    hp = eng.ipl_hparams()
    with pytest.raises(EngineError, match="max_batch"):
        eng.ipl_minibatch(np.arange(5), 5, hp)
    with pytest.raises(EngineError, match="no mi_ipl_minibatch has run"):
        eng.ipl_read_pred(4)
    eng.set_multirank(1)
    with pytest.raises(EngineError, match="multirank"):
        eng.ipl_minibatch(idx, 4, hp)
    eng.set_multirank(0)
    eng.ipl_minibatch(idx, 4, hp)                              # (and it runs once the mode is back)
    with pytest.raises(EngineError, match="n != the last minibatch's size"):
        eng.ipl_read_pred(3)
    H = 64
    eng.set_gru(np.zeros((3 * H, H), np.float32), np.zeros((3 * H, H), np.float32), np.zeros(3 * H, np.float32), np.zeros(3 * H, np.float32))
    with pytest.raises(EngineError, match="recurrent"):
        eng.ipl_minibatch(idx, 4, hp)
    with pytest.raises(EngineError, match="recurrent"):
        eng.predict_greedy(np.zeros((4, 9), np.float32))
    eng.close()
    eng = Engine("mlp", 2, 4, 2, 4, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64, value_from_logits=True)
    with pytest.raises(EngineError, match="value_from_logits"):
        eng.ipl_minibatch(idx, 4, hp)
    eng.close()


def _ppo_bf16_g4_errors():
    """Per-tensor relative L2 error of the bf16 PPO pass on G4 (IMPALA, 'raw' case) against that golden: the yardstick of the bf16 bound."""
    from mi355 import engine as M, layout
    from mi355.engine import Engine
    z, z3 = load_npz("g4_impala_lossgrad.npz"), load_npz("g3_impala_forward.npz")
    T, E, A = 4, 8, 15
    shapes = layout.impala_param_shapes(A)
    eng = Engine("impala", T, E, A, T * E, precision="bf16")
    eng.set_params(layout.flatten(shapes, {k[2:]: z3[k] for k in z3.files if k.startswith("p/")}))
    for t in range(T + 1):
        eng.put_obs(t, z["in/frames"][t])
    for t in range(T):
        eng.put_step(t, z["in/rew"][t], z["in/done"][t])
    eng.write_field(M.F_ACT, z["in/act"].astype(np.float32)); eng.write_field(M.F_LOGP, z["in/logp"]); eng.write_field(M.F_VALUE, z["in/val"])
    eng.compute_estimates(0.999, 0.95, True, True)
    eng.minibatch(np.arange(T * E), T * E, eng.hparams(0.2, 0.5, 0.01, 0.0, 1.0, 0.0))      # (one minibatch of all rows, as test_g4_loss_and_grads_golden)
    g = layout.unflatten(shapes, eng.get_grads())
    eng.close()
    ref = {k[len("raw/g/"):]: z[k] for k in z.files if k.startswith("raw/g/")}
    return {k: float(np.linalg.norm(g[k].astype(np.float64) - r) / (np.linalg.norm(r.astype(np.float64)) + 1e-7)) for k, r in ref.items()}


def test_g16_case_a_bf16():
    """Case a in bf16 against the same golden: Loss/total within 2 % (the margin tests/test_gpu_bf16.py gives Loss/v), entropy / mutual_info
    within 1e-3, pred_reward within 2e-3 * max(1, |ref|).  Gradients: the per-tensor relative L2 error, worst tensor, within twice that of the
    bf16 PPO pass on G4 against its golden (_check_grads' measure and return value), measured in the same process -- IPL sums two
    backward passes through the same kernels.  Measured on the MI355X: IPL 0.089 (embedder.block1.res1.conv1.weight), PPO 0.272
    (embedder.block1.res1.conv1.bias).  Tensor by tensor the comparison does not hold for fc_policy.bias (IPL 5.0e-3, PPO 1.9e-5): G4's
    policy is the 0.01-gain initialisation, whose softmax is uniform whatever the features are, so that gradient does not feel the bf16
    features at all, while G16's logits (fc_policy.weight x 600) do -- its error there is that of fc_policy.weight (6.9e-3, PPO 6.1e-3)."""
    r = _run_case("a", "bf16")
    z = r["z"]
    ref, mine = z["a/terms"][0], r["log"][0]
    print("bf16 terms", mine, ref)
    assert abs(mine[2] - ref[2]) < 0.02 * abs(ref[2])
    assert abs(mine[0] - ref[0]) < 1e-3 and abs(mine[1] - ref[1]) < 1e-3
    assert abs(mine[7] - ref[7]) < 2e-3 * max(1.0, abs(ref[7]))
    ppo = _ppo_bf16_g4_errors()
    ipl = {n: SI.tensor_error(r["g0"][n], z, "a/g0/", n) for n in r["g0"]}
    for n in ipl:
        print("bf16 g0", n, "ipl", ipl[n], "ppo on G4", ppo.get(n))
    print("bf16 worst per-tensor error: ipl", max(ipl.values()), "ppo on G4", max(ppo.values()))
    assert max(ipl.values()) < 2 * max(ppo.values()), (max(ipl, key=ipl.get), max(ipl.values()), max(ppo.values()))


# ------------------------------------------------------------------------------------------------ agent level
def _agent(tmp_path, arch="mlp", T=4, E=8, greedy_scale=40.0, **kw):
    from agents.ipl import IPL
    from common.env.vec_envs import SyntheticFrames, create_cartpole
    from common.logger import Logger
    from common.model import ImpalaModel, MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import IPLStorage
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    if arch == "impala":
        A, env, emb, shape = 9, SyntheticFrames(E, 9, 1), ImpalaModel(3), (3, 64, 64)
    else:
        A, env, emb, shape = 2, create_cartpole({}, False, seed=1, n_envs=E), MLPModel(9, 4, 64, 64), (9,)
    pol = CategoricalPolicy(emb, False, A)
    with torch.no_grad():
        pol.fc_policy.weight.mul_(greedy_scale)
    agent = IPL(env, pol, Logger(E, str(tmp_path), algo="IPL"), IPLStorage(shape, T, E, dev), dev, 1, n_steps=T, n_envs=E, epoch=2,
                n_minibatch=2, mini_batch_size=8, learning_rate=5e-4, seed=3, **kw)
    return agent, env


@pytest.mark.parametrize("arch", ["mlp", "impala"])
def test_predict_greedy_is_argmax_of_forward(tmp_path, arch):
    agent, env = _agent(tmp_path, arch)
    obs = env.reset()
    from common.model import as_device_obs
    act, value = agent.predict(obs, greedy=True)
    lp, v = agent.engine.forward(as_device_obs(obs, arch))
    assert np.array_equal(act, lp.argmax(-1)) and np.allclose(value, v, atol=1e-6)
    act2, _ = agent.predict(obs, greedy=False)
    assert act2.shape == act.shape
    agent.engine.close()


def test_collect_optimize_checkpoint_roundtrip(tmp_path):
    agent, env = _agent(tmp_path, "mlp", entropy_coef=0.01, reward_incentive=True)
    obs = env.reset()
    obs = agent.collect_data(obs, agent.storage, env)
    before = agent.engine.get_params().copy()
    summary = agent.optimize()
    assert list(summary) == list(II.SUMMARY_KEYS)
    assert np.isnan(summary["Loss/alpha"]) and all(np.isfinite(v) for k, v in summary.items() if k not in ("Loss/alpha", "Loss/rew_corr"))
    assert agent.optimizer_steps == 4 and agent.last_predicted_reward.shape == agent.last_reward.shape == (8,)
    assert np.abs(agent.engine.get_params() - before).max() > 0
    # greedy rollout through the reference's loop, then the 6-tuple for outside consumers
    obs = agent.collect_data(obs, agent.storage, env, greedy=True)
    sample = next(iter(agent.storage.fetch_train_generator(8)))
    assert [tuple(t.shape) for t in sample] == [(8, 9), (8, 9), (8,), (8,), (8,), (8,)]
    ck = tmp_path / "model.pth"
    torch.save({"model_state_dict": agent.policy.state_dict(), "optimizer_state_dict": agent.optimizer.state_dict()}, ck)
    params, (m, v) = agent.engine.get_params().copy(), agent.engine.get_adam_state()
    agent.engine.close()
    agent2, _ = _agent(tmp_path / "b", "mlp")
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    agent2.policy.load_state_dict(sd["model_state_dict"])
    agent2.optimizer.load_state_dict(sd["optimizer_state_dict"])
    assert np.array_equal(agent2.engine.get_params(), params)
    m2, v2 = agent2.engine.get_adam_state()
    assert np.array_equal(m2, m) and np.array_equal(v2, v) and agent2.optimizer.step_count == 4
    agent2.engine.close()


def _run_cli(tmp_path, extra):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "--algo", "IPL", "--seed", "3", "--n_envs", "8", "--n_steps", "8", "--mini_batch_size", "16",
           "--num_timesteps", "130", "--num_checkpoints", "1", "--exp_name", "ipl"] + extra
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


@pytest.mark.parametrize("env_name,param_name,A", [("cartpole", "ipl_cartpole", 2), ("synthetic", "hard-500-ipl", 9)])
def test_cli_writes_ipl_columns_and_checkpoint(tmp_path, env_name, param_name, A):
    """`train.py --algo IPL` for three iterations: the CSV has the IPL loss columns, the checkpoint loads into a stock torch policy."""
    import csv
    _run_cli(tmp_path, ["--env_name", env_name, "--param_name", param_name])
    base = tmp_path / "logs" / "train" / env_name / "ipl"
    rd = base / os.listdir(base)[0]
    with open(rd / "log-append.csv") as f:
        rows = list(csv.reader(f))
    from common.logger import LOSS_KEYS_IPL
    i0 = rows[0].index("entropy")
    assert rows[0][i0:i0 + 8] == LOSS_KEYS_IPL and rows[0][-1] == "learning_rate" and len(rows) == 4
    assert all(np.isfinite(float(rows[k][i0 + 2])) for k in (1, 2, 3))
    cks = [f for f in os.listdir(rd) if f.startswith("model_")]
    assert cks, os.listdir(rd)
    ck = torch.load(rd / cks[0], map_location="cpu", weights_only=True)
    assert set(ck) >= {"model_state_dict", "optimizer_state_dict"}
    assert ck["model_state_dict"]["fc_policy.weight"].shape[0] == A and len(ck["optimizer_state_dict"]["state"]) > 0
