"""GRU training on the MI355X (algo ppo-pure, BPTT): the sequence kernels through mi_debug_gru_seq against float64 autograd, the
reference's recurrent PPOPure.optimize through mi_gru_train + mi_minibatch_rec + mi_optimizer_step (fixture G13), the bf16 mode
teacher-forced against the float64 twin of tests/bptt_inputs.py, the untouched frozen path, and the agent / CLI end to end."""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import bptt_inputs as BI
import width_inputs as WI
from conftest import PKG, ROOT, load_npz, npz_json

pytestmark = pytest.mark.gpu

HP_KW = dict(eps_clip=0.2, value_coef=0.5, entropy_coef=0.01, x_entropy_coef=0.0)


class _Log:
    episode_reward_buffer = [0.0]
    logdir = "/tmp"


@pytest.fixture(scope="module")
def hook_engine():
    from mi355.engine import Engine
    eng = Engine("mlp", 2, 2, 2, 8, obs_dim=4, mlp_depth=2, mlp_width=8, out_dim=8)      # mi_debug_gru_seq is independent of the context's sizes
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def g13():
    return load_npz("g13_bptt.npz")


# ---------------------------------------------------------------------------------------------- 1. the op
def _seq_inputs(T, n, H, seed=0):
    rng = np.random.default_rng(1000 * H + 10 * T + n + seed)
    k = 1.0 / np.sqrt(H)                                                    # nn.GRU's own initialisation range
    u = lambda *s: rng.uniform(-k, k, size=s).astype(np.float32)
    x = (0.5 * rng.standard_normal((T, n, H))).astype(np.float32)
    h0 = (0.5 * rng.standard_normal((n, H))).astype(np.float32)
    mask = (rng.random((T, n)) < 0.7).astype(np.float32)
    mask[0, 0] = 0.0
    mask[T - 1, n - 1] = 0.0
    if T * n > 2:
        mask[T - 1, 0] = 1.0                                                # zeros AND ones present
    d_out = rng.standard_normal((T, n, H)).astype(np.float32)
    return x, h0, mask, (u(3 * H, H), u(3 * H, H), u(3 * H), u(3 * H)), d_out


def _torch_seq(x, h0, mask, w, d_out, dtype):
    t = lambda a: torch.from_numpy(a).to(dtype)
    xl = t(x).requires_grad_(True)
    wl = [t(a).requires_grad_(True) for a in w]
    h = BI.gru_sequence(xl, t(h0), t(mask), *wl)
    (h * t(d_out)).sum().backward()
    return [h.detach().numpy(), xl.grad.numpy()] + [a.grad.numpy() for a in wl]        # h, dX, dW_ih, dW_hh, db_ih, db_hh


NAMES = ("h", "dX", "dW_ih", "dW_hh", "db_ih", "db_hh")


@pytest.mark.parametrize("T,n", [(1, 1), (7, 19), (5, 33)])
@pytest.mark.parametrize("H", [64, 256, 320])
def test_gru_seq_matches_float64_autograd(hook_engine, H, T, n):
    """forward h within 2e-6 * T absolute (2e-6: the one-step bound of the fused-step test), every gradient within 1e-5 relative L2;
    torch's own fp32 error on the same inputs must sit 8x under each bound, else the inputs are too hard to tell anything."""
    x, h0, mask, w, d_out = _seq_inputs(T, n, H)
    assert mask.min() == 0.0 and (T * n <= 2 or mask.max() == 1.0) and np.abs(h0).min() > 0
    ref = _torch_seq(x, h0, mask, w, d_out, torch.float64)
    t32 = _torch_seq(x, h0, mask, w, d_out, torch.float32)
    got = hook_engine.debug_gru_seq(x, h0, mask, *w, d_out=d_out)
    fwd_only = hook_engine.debug_gru_seq(x, h0, mask, *w)
    assert np.array_equal(fwd_only, got[0])
    for name, g, r, t in zip(NAMES, got, ref, t32):
        if name == "h":
            bound, err, terr = 2e-6 * T, float(np.abs(g - r).max()), float(np.abs(t - r).max())
        else:
            bound, err, terr = 1e-5, BI.rel_l2(g, r), BI.rel_l2(t, r)
        print(f"H={H} T={T} n={n} {name}: kernel {err:.3e}  torch fp32 {terr:.3e}  bound {bound:.1e}")
        assert bound >= 8 * terr, (name, "inputs too hard for the bound", terr)
        assert err < bound, (name, err)


def test_gru_seq_rows_do_not_depend_on_tile_or_neighbours(hook_engine):
    """Rows of the n = 33 launch (three tiles, the last with one row) equal the same rows launched alone and at another offset, bit for bit."""
    for H, with_dx in ((256, False), (64, True)):       # (dX comes from a GEMM behind the kernel: bit-stable per row while its K = 3H stays unsplit)
        T, n = 5, 33
        x, h0, mask, w, d_out = _seq_inputs(T, n, H, seed=7)
        full = hook_engine.debug_gru_seq(x, h0, mask, *w, d_out=d_out)
        for row in (0, 15, 16, 21, 32):
            alone = hook_engine.debug_gru_seq(x[:, row:row + 1], h0[row:row + 1], mask[:, row:row + 1], *w, d_out=d_out[:, row:row + 1])
            assert np.array_equal(alone[0][:, 0], full[0][:, row]), (H, row)
            sel = [3, 30, 8, 2, 11, 9, row, 4]                               # the row at offset 6 among other neighbours
            moved = hook_engine.debug_gru_seq(x[:, sel], h0[sel], mask[:, sel], *w, d_out=d_out[:, sel])
            assert np.array_equal(moved[0][:, 6], full[0][:, row]), (H, row)
            if with_dx:
                assert np.array_equal(alone[1][:, 0], full[1][:, row]) and np.array_equal(moved[1][:, 6], full[1][:, row]), (H, row)


def test_gru_seq_mask_acts(hook_engine):
    x, h0, _, w, _ = _seq_inputs(2, 1, 64, seed=3)
    ones = hook_engine.debug_gru_seq(x, h0, np.ones((2, 1), np.float32), *w)
    cut = hook_engine.debug_gru_seq(x, h0, np.array([[1.0], [0.0]], np.float32), *w)
    assert np.array_equal(ones[0], cut[0])                                   # step 0 does not see the mask of step 1
    assert np.abs(ones[1] - cut[1]).max() > 1e-2


@pytest.mark.parametrize("H", [32, 96, 576])
def test_gru_seq_refuses_unsupported_width(hook_engine, H):
    from mi355.engine import EngineError
    x, h0, mask, w, _ = _seq_inputs(2, 2, H)
    with pytest.raises(EngineError, match="multiple of 64"):
        hook_engine.debug_gru_seq(x, h0, mask, *w)


# ---------------------------------------------------------------------------------------------- engines on the G13 cases
def _engine(case, precision="fp32", train=True):
    """-> (engine, policy, rollout): the case's seeded policy on a fresh engine, rollout ring filled, GRU training on."""
    from mi355 import engine as M, layout
    c = BI.CASE_A if case == "a" else BI.CASE_B
    r = BI.rollout_a() if case == "a" else BI.rollout_b()
    T, E = c["T"], c["E"]
    policy = BI.build_policy(case)
    mb = T * E // c["n_minibatch"]
    if case == "a":
        eng = M.Engine("mlp", T, E, c["A"], mb, obs_dim=c["obs"], mlp_depth=c["depth"], mlp_width=c["width"], out_dim=c["H"])
    else:
        eng = M.Engine("impala", T, E, c["A"], mb, out_dim=c["H"], precision=precision)
    host = BI.host_params(policy)
    eng.set_params(layout.flatten(policy.param_shapes(), {k: v for k, v in host.items() if not k.startswith("gru.")}))
    eng.set_gru(*(host[k] for k in BI.GRU_KEYS))
    if train:
        eng.gru_train(True)
    for t in range(T + 1):
        eng.put_obs(t, r["frames"][t])
    eng.sync()
    eng.write_field(M.F_ACT, r["act"].astype(np.float32)); eng.write_field(M.F_LOGP, r["logp"]); eng.write_field(M.F_VALUE, r["val"])
    eng.write_field(M.F_REW, r["rew"]); eng.write_field(M.F_DONE, r["done"])
    eng.compute_estimates(0.999, 0.95, True, True)
    return eng, policy, r


def _all_grads(eng, policy):
    from mi355 import layout
    g = OrderedDict(layout.unflatten(policy.param_shapes(), eng.get_grads()))
    g.update(zip(BI.GRU_KEYS, eng.get_gru_grads()))
    return g


def _all_params(eng, policy):
    from mi355 import layout
    p = OrderedDict(layout.unflatten(policy.param_shapes(), eng.get_params()))
    p.update(zip(BI.GRU_KEYS, eng.get_gru()))
    return p


def _total_norm(g):
    return float(np.sqrt(sum((np.asarray(v, np.float64) ** 2).sum() for v in g.values())))


def _summary(log):
    return {'Loss/pi': float(np.mean(-log[:, 0])), 'Loss/v': float(np.mean(-log[:, 1])), 'Loss/entropy': float(np.mean(log[:, 2])),
            'Loss/x_entropy': float(np.mean(log[:, 3])), 'Loss/total': float(np.mean(log[:, 4]))}


def _check_estimates(eng, z, case):
    from mi355 import engine as M
    assert np.abs(eng.read_field(M.F_ADV) - z[f"{case}/adv"]).max() < 1e-5 and np.abs(eng.read_field(M.F_RET) - z[f"{case}/ret"]).max() < 1e-5


def _check_params(p, z, prefix, tol=2e-6):
    """whole tensors: max abs error; sketched ones: norm, sum / sqrt(n) and every projection move by at most ||a - r|| <= sqrt(n) * tol"""
    seen = 0
    for k in z.files:
        if k.startswith(prefix + "g/"):
            name = k[len(prefix) + 2:]
            err = float(np.abs(p[name] - z[k]).max())
            assert err < tol, (prefix, name, err)
            seen += 1
        elif k.startswith(prefix + "norm/"):
            name = k[len(prefix) + 5:]
            a = np.asarray(p[name], np.float64).ravel()
            errs = [abs(np.linalg.norm(a) - float(z[k])), abs(a.sum() - float(z[prefix + "sum/" + name])) / np.sqrt(a.size),
                    float(np.abs(WI.sketch(a) - z[prefix + "sketch/" + name]).max())]
            assert max(errs) < np.sqrt(a.size) * tol, (prefix, name, errs)
            seen += 1
    assert seen == len(p)


# ---------------------------------------------------------------------------------------------- 2. golden case (a)
def test_golden_case_a_gradients_and_losses(g13):
    eng, policy, r = _engine("a")
    _check_estimates(eng, g13, "a")
    envs, hp = g13["a/envs"], eng.hparams(**HP_KW)
    assert eng.n_params + eng.gru_count() == sum(v.size for v in BI.host_params(policy).values())
    first = None
    for k in (1, 2):
        e = envs[4 * (k - 1):4 * k]
        eng.minibatch_rec(e, r["h0"][e], 32, hp)
        g = _all_grads(eng, policy)
        first = first or g
        assert len(g) == 16
        for name, v in g.items():
            err = BI.rel_l2(v, g13[f"a/raw/g{k}/g/{name}"])
            print(f"minibatch {k} {name}: rel L2 {err:.2e}")
            assert err < 1e-3, (k, name, err)
        want = float(g13[f"a/raw/total_norm{k}"])
        assert abs(_total_norm(g) - want) < 1e-4 * want
        gn = eng.optimizer_step(5e-4, 1e9, k, want_norm=True)
        assert abs(gn - want) < 1e-4 * want                                   # the reported norm is the global one, GRU included
        assert not eng.get_grads().any() and not any(v.any() for v in eng.get_gru_grads())      # both zeroed
    got, want = _summary(eng.loss_log()), npz_json(g13, "a/raw/summary")
    for key in want:
        print(f"{key}: {got[key]:.8f} vs {want[key]:.8f}")
        assert abs(got[key] - want[key]) < 1e-5, key
    eng.close()
    # row order within a minibatch does not matter
    eng, policy, r = _engine("a")
    e = envs[:4][[2, 0, 3, 1]]
    eng.minibatch_rec(e, r["h0"][e], 32, hp)
    for name, v in _all_grads(eng, policy).items():
        assert BI.rel_l2(v, first[name]) < 1e-6, name
    eng.close()


def test_golden_case_a_clipped_adam_steps(g13):
    eng, policy, r = _engine("a")
    envs, hp = g13["a/envs"], eng.hparams(**HP_KW)
    for k in (1, 2):
        e = envs[4 * (k - 1):4 * k]
        eng.minibatch_rec(e, r["h0"][e], 32, hp)
        gn = eng.optimizer_step(5e-4, 0.5, k, want_norm=True)
        want = float(g13[f"a/clip/norm{k}"])
        print(f"step {k}: reported norm {gn:.8f} vs {want:.8f}")
        assert abs(gn - want) < 1e-5 * want
        _check_params(_all_params(eng, policy), g13, f"a/clip/p{k}/")
    m, v = eng.get_gru_adam_state()
    assert m.shape == (eng.gru_count(),) and np.abs(m).max() > 0 and v.min() >= 0 and v.max() > 0
    eng.close()


# ---------------------------------------------------------------------------------------------- 3. golden case (b)
def test_golden_case_b_impala(g13):
    eng, policy, r = _engine("b")
    _check_estimates(eng, g13, "b")
    envs, hp = g13["b/envs"], eng.hparams(**HP_KW)
    eng.minibatch_rec(envs, r["h0"][envs], 16, hp)
    g = _all_grads(eng, policy)
    errs = WI.grad_errors(g, g13, prefix="b/raw/g1/")
    assert len(errs) == len(g) == 40
    for name, err in errs.items():
        print(f"{name}: {err:.2e}")
        assert err < 1e-3, (name, err)
    got, want = _summary(eng.loss_log()), npz_json(g13, "b/raw/summary")
    for key in want:
        assert abs(got[key] - want[key]) < 1e-5, (key, got[key], want[key])
    eng.close()
    # the clipped run: two epochs of one minibatch, an Adam step after each
    eng, policy, r = _engine("b")
    torch.manual_seed(5)
    for k in (1, 2):
        e = torch.randperm(4).numpy()
        eng.minibatch_rec(e, r["h0"][e], 16, hp)
        gn = eng.optimizer_step(5e-4, 0.5, k, want_norm=True)
        want = float(g13[f"b/clip/norm{k}"])
        assert abs(gn - want) < 1e-5 * want, (k, gn, want)
        _check_params(_all_params(eng, policy), g13, f"b/clip/p{k}/")
    eng.close()


# ---------------------------------------------------------------------------------------------- 4. bf16 mode, teacher-forced
def test_bf16_mode_teacher_forced():
    """Everything downstream of the embedder output is fp32 in both modes: from the engine's own features the float64 twin must give
    the engine's losses (1e-5) and its head / GRU gradients and dX (1e-4 relative L2)."""
    eng, policy, r = _engine("b", precision="bf16")
    from mi355 import engine as M
    T, E, H = 4, 4, 128
    envs = np.array([2, 0, 3, 1])
    eng.minibatch_rec(envs, r["h0"][envs], T * E, eng.hparams(**HP_KW))
    x = eng.debug_read(100, T * E).reshape(T, E, H)
    assert x.min() >= 0 and (x == 0).any() and (x > 0).any()                 # the embedder's final ReLU
    adv, ret = eng.read_field(M.F_ADV), eng.read_field(M.F_RET)
    L, g = BI.rec_minibatch(BI.host_params(policy), "impala", None, r["h0"][envs], r["done"][:, envs], r["act"][:, envs], r["logp"][:, envs],
                            r["val"][:T][:, envs], ret[:, envs], adv[:, envs], x_override=x)
    rec = eng.loss_log()[0]
    for j, key in enumerate(("pi_loss", "value_loss", "entropy", "x_ent", "total")):
        print(f"{key}: {rec[j]:.8f} vs {L[key]:.8f}")
        assert abs(rec[j] - L[key]) < 1e-5, key
    mine = _all_grads(eng, policy)
    for name in ("fc_policy.weight", "fc_policy.bias", "fc_value.weight", "fc_value.bias") + BI.GRU_KEYS:
        err = BI.rel_l2(mine[name], g[name].numpy())
        print(f"{name}: rel L2 {err:.2e}")
        assert err < 1e-4, (name, err)
    dx = eng.debug_read(102, T * E).reshape(T, E, H)
    want = g["x"].numpy() * (x > 0)                                          # the ReLU mask moved from the heads to dX
    assert BI.rel_l2(dx, want) < 1e-4
    h = eng.debug_read(101, T * E).reshape(T, E, H)
    t64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    hp64 = BI.gru_sequence(t64(x), t64(r["h0"][envs]), 1.0 - t64(r["done"][:, envs]), *(t64(BI.host_params(policy)[k]) for k in BI.GRU_KEYS))
    assert np.abs(h - hp64.numpy()).max() < 2e-6 * T
    eng.close()


# ---------------------------------------------------------------------------------------------- 5. frozen path untouched
def test_frozen_gru_path_is_untouched():
    """A GRU set but never trained: an ordinary minibatch + optimizer step gives the flat parameters of an engine that never saw any
    of the new calls, bit for bit, and the GRU reads back as uploaded."""
    from mi355 import layout
    eng, policy, r = _engine("a", train=False)
    plain, _, _ = _engine("a", train=False)
    host = BI.host_params(policy)
    idx = np.random.default_rng(0).permutation(64)[:32]
    outs = []
    for e in (eng, plain):
        e.minibatch(idx, 32, e.hparams(**HP_KW))
        gn = e.optimizer_step(5e-4, 0.5, 1, want_norm=True)
        outs.append((e.get_params(), gn, e.loss_log()))
    for w, k in zip(eng.get_gru(), BI.GRU_KEYS):
        assert np.array_equal(w, host[k])
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and np.array_equal(outs[0][2], outs[1][2])
    assert not np.array_equal(outs[0][0], layout.flatten(policy.param_shapes(), {k: v for k, v in host.items() if not k.startswith("gru.")}))
    eng.close(); plain.close()


def test_refusals():
    from mi355.engine import EngineError
    eng, policy, r = _engine("a", train=False)
    envs, hp = np.arange(4), eng.hparams(**HP_KW)
    with pytest.raises(EngineError, match="GRU training is off"):
        eng.minibatch_rec(envs, r["h0"][envs], 32, hp)
    eng.gru_train(True)
    with pytest.raises(EngineError, match="fs_coef must be 0"):
        eng.minibatch_rec(envs, r["h0"][envs], 32, eng.hparams(fs_coef=0.5, **HP_KW))
    with pytest.raises(EngineError, match="max_batch"):
        eng.minibatch_rec(np.arange(5), r["h0"][:5], 40, hp)
    for mode in (1, 2):
        eng.set_multirank(mode)
        with pytest.raises(EngineError, match="single rank"):
            eng.minibatch_rec(envs, r["h0"][envs], 32, hp)
    eng.set_multirank(0)
    eng.minibatch_rec(envs, r["h0"][envs], 32, hp)                            # and it runs once the state is clean again
    assert len(eng.loss_log()) == 1
    eng.close()
    from mi355.engine import Engine
    bare = Engine("mlp", 2, 2, 2, 8, obs_dim=4, mlp_depth=2, mlp_width=8, out_dim=64)
    with pytest.raises(EngineError, match="mi_set_gru"):
        bare.gru_train(True)
    bare.close()


# ---------------------------------------------------------------------------------------------- 6. agent and CLI
def _agent(cls, T=8, E=8, D=64, seed=6033, valid=True, **kw):
    from common.env.vec_envs import SyntheticFrames
    from common.model import ImpalaModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    dev = torch.device("cuda", 0)
    torch.manual_seed(seed)
    policy = CategoricalPolicy(ImpalaModel(3, output_dim=D), True, 15)
    st, stv = Storage((3, 64, 64), D, T, E, dev), (Storage((3, 64, 64), D, T, E, dev) if valid else None)
    from common.logger import Logger
    agent = cls(SyntheticFrames(E, 15, seed=3), policy, Logger(E, None, algo="ppo" if cls.__name__ == "PPO" else "ppo-pure"), st, dev, 1, env_valid=SyntheticFrames(E, 15, seed=4) if valid else None,
                storage_valid=stv, n_steps=T, n_envs=E, epoch=2, n_minibatch=2, mini_batch_size=T * E // 2, gamma=0.999, lmbda=0.95,
                learning_rate=5e-4, seed=0, **kw)
    return agent, policy


def test_agent_trains_the_gru_and_checkpoints_it(tmp_path):
    from agents.ppo import PPO
    from agents.ppo_pure import PPOPure
    T, E, D = 8, 8, 64
    agent, policy = _agent(PPOPure)
    before = [t.detach().clone() for t in policy.gru.parameters()]
    agent.train(2 * T * E)
    assert len(agent.logger.rows) == 2 and np.isfinite(agent.logger.rows[-1][agent.logger.columns.index("loss_total")])
    sd = policy.state_dict()
    assert all(not torch.equal(a, b) for a, b in zip(before, policy.gru.parameters()))           # the recurrence is learnt ...
    for w, k in zip(agent.engine.get_gru(), BI.GRU_KEYS):
        assert np.array_equal(sd[k].numpy(), w)                                                    # ... and state_dict() pulls it
    agent.engine_valid.copy_params_from(agent.engine)                                             # the validation twin acts with the trained GRU
    for a, b in zip(agent.engine_valid.get_gru(), agent.engine.get_gru()):
        assert np.array_equal(a, b)
    assert np.array_equal(agent.engine_valid.get_params(), agent.engine.get_params())
    # checkpoint: Adam state for all 36 + 4 tensors in torch's layout, through a stock torch.optim.Adam and back
    osd = agent.optimizer.state_dict()
    assert len(osd["param_groups"][0]["params"]) == 40 and len(osd["state"]) == 40 and float(osd["state"][39]["step"]) == 8.0
    path = str(tmp_path / "model.pth")
    torch.save({'model_state_dict': sd, 'optimizer_state_dict': osd}, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert list(ck["model_state_dict"])[-4:] == list(BI.GRU_KEYS)
    stock = torch.optim.Adam([torch.nn.Parameter(v.clone()) for v in ck["model_state_dict"].values()], lr=5e-4, eps=1e-5)
    stock.load_state_dict(ck["optimizer_state_dict"])
    assert [tuple(s["exp_avg"].shape) for s in stock.state_dict()["state"].values()] == [tuple(v.shape) for v in ck["model_state_dict"].values()]
    agent2, policy2 = _agent(PPOPure, seed=1, valid=False)
    policy2.load_state_dict(ck["model_state_dict"])
    agent2.optimizer.load_state_dict(stock.state_dict())
    for a, b in zip(agent2.engine.get_gru(), agent.engine.get_gru()):
        assert np.array_equal(a, b)
    for a, b in zip(agent2.engine.get_gru_adam_state() + agent2.engine.get_adam_state(), agent.engine.get_gru_adam_state() + agent.engine.get_adam_state()):
        assert np.array_equal(a, b)
    assert agent2.optimizer.step_count == 8
    # under algo ppo the same policy keeps its GRU frozen and stateless
    frozen, fpolicy = _agent(PPO, valid=False)
    fbefore = [t.detach().clone() for t in fpolicy.gru.parameters()]
    frozen.train(T * E)
    fpolicy.state_dict()
    assert all(torch.equal(a, b) for a, b in zip(fbefore, fpolicy.gru.parameters())) and len(frozen.optimizer.state_dict()["state"]) == 36


def test_train_cli_ppo_pure_runs_and_resumes(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    base = [sys.executable, os.path.join(PKG, "train.py"), "--exp_name", "pure", "--env_name", "synthetic", "--param_name", "hard-local-dev-rec",
            "--algo", "ppo-pure", "--n_envs", "8", "--n_steps", "16", "--mini_batch_size", "32", "--seed", "3", "--detect_nan"]
    r = subprocess.run(base + ["--num_timesteps", "250", "--num_checkpoints", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    runs = os.listdir(tmp_path / "logs" / "train" / "synthetic" / "pure")
    rd = tmp_path / "logs" / "train" / "synthetic" / "pure" / runs[0]
    ck = torch.load(rd / "model_256.pth", map_location="cpu", weights_only=True)
    assert ck["t"] == 256 and len(ck["model_state_dict"]) == 40 and len(ck["optimizer_state_dict"]["state"]) == 40
    rows = open(rd / "log-append.csv").read().strip().splitlines()
    assert len(rows) == 3 and rows[0].endswith("ema_rewards,loss_pi,loss_v,loss_entropy,loss_x_entropy,loss_total,learning_rate")
    r = subprocess.run(base + ["--num_timesteps", "500", "--num_checkpoints", "1", "--model_file", "auto"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ck2 = torch.load(rd / "model_512.pth", map_location="cpu", weights_only=True)
    steps = float(ck["optimizer_state_dict"]["state"][39]["step"])
    assert ck2["t"] == 512 and float(ck2["optimizer_state_dict"]["state"][39]["step"]) == 2 * steps          # continued, GRU state included
    assert not torch.equal(ck2["model_state_dict"][BI.GRU_KEYS[1]], ck["model_state_dict"][BI.GRU_KEYS[1]])
