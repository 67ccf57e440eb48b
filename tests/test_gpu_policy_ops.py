"""The arithmetic that decides what the policy does and which gradient it gets, one launch sequence at a time on caller data: the heads at
update size (csrc/heads.hip heads_fwd_kernel, heads_bwd_kernel) through mi_op_heads, the three sampling kernels through mi_op_sample, the
PPO loss (csrc/loss.hip, csrc/policy_math.h) through mi_op_ppo_loss -- per sample, per 64-sample block and per segment against float64.
Inputs, references and every bound's derivation are in tests/policy_inputs.py; tests/test_policy_host.py checks those on the CPU.

Every hook call goes through the production launchers into poisoned outputs followed by canary bands.  The bit-for-bit assertions are the
kernels' own documented claims (the comment above heads_sample_kernel, batch invariance of heads_bwd_kernel).  One documented claim did not
hold when first tested -- heads_fwd_kernel's logits are NOT heads_sample_kernel's bits at H = 256: the compiler fuses the four products of
a step in one kernel and not in the other -- and is pinned as what does hold (test_samplers); the comment in csrc/heads.hip says so now."""
import numpy as np
import pytest
import torch

import policy_inputs as PI

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)


@pytest.fixture(scope="module")
def hook_engine():
    from mi355.engine import Engine
    eng = Engine("mlp", 2, 2, 2, 8, obs_dim=4, mlp_depth=2, mlp_width=8, out_dim=8)          # the hooks are independent of the context's sizes
    yield eng
    eng.close()


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------------------------------------ heads forward
@pytest.mark.parametrize("O", PI.FWD_O)
def test_heads_forward(hook_engine, O):
    """heads_fwd_kernel against the float64 product, d = 256; the last two rows (the clamped tail loads of a partial workgroup) on their own"""
    for n in PI.FWD_N:
        c = PI.heads_case(n, 256, O)
        got = hook_engine.op_heads_fwd(c["feat"], c["Wh"], c["bh"])
        r = PI.heads_fwd_reference(c["feat"], c["Wh"], c["bh"])
        worst = PI.check_sum(got, r, f"heads_fwd n={n} O={O}")
        for row in {n - 1, max(n - 2, 0)}:
            PI.check_sum(got[row:row + 1], PI.heads_fwd_reference(c["feat"][row:row + 1], c["Wh"], c["bh"]), f"heads_fwd n={n} O={O} row {row}")
        print(f"heads_fwd n={n} O={O}: worst err/bound {worst:.3f}")
        assert _same(got, hook_engine.op_heads_fwd(c["feat"], c["Wh"], c["bh"]))


def test_heads_refusals(hook_engine):
    """what the kernels do not support is an error before any launch, and the context still works"""
    from mi355.engine import EngineError
    c = PI.heads_case(4, 256, 16)
    w17 = np.zeros((17, 256), np.float32)
    with pytest.raises(EngineError, match="at most 16 outputs"):
        hook_engine.op_heads_fwd(c["feat"], w17, np.zeros(17, np.float32))
    with pytest.raises(EngineError, match="at most 16 outputs"):
        hook_engine.op_heads_bwd(np.zeros((4, 17), np.float32), c["feat"], w17, 1, w17, np.zeros(17, np.float32))
    with pytest.raises(EngineError, match="H == 256"):
        hook_engine.op_heads_fwd(c["feat"][:, :64], c["Wh"][:, :64], c["bh"])
    with pytest.raises(EngineError, match="H == 256"):
        hook_engine.op_heads_bwd(np.zeros((4, 2), np.float32), np.zeros((4, 260), np.float32), np.zeros((2, 260), np.float32), 1, np.zeros((2, 260), np.float32), np.zeros(2, np.float32))
    PI.check_sum(hook_engine.op_heads_fwd(c["feat"], c["Wh"], c["bh"]), PI.heads_fwd_reference(c["feat"], c["Wh"], c["bh"]))


# ------------------------------------------------------------------------------------------------ heads backward
@pytest.mark.parametrize("relu_mask", (0, 1))
@pytest.mark.parametrize("H,O", PI.BWD_HO)
def test_heads_backward(hook_engine, H, O, relu_mask):
    """heads_bwd_kernel + its slab sum: dfeat (d = O), gW / gb from non-zero starting values (d = rows of a chunk + the slab sum's depth).
    n > 8192: chunk = 17 rows, so the 8-rows-in-flight loop and the scalar tail run in one workgroup, and trailing workgroups own no rows."""
    for n in PI.BWD_N:
        c = PI.heads_case(n, H, O)
        args = (c["dY"], c["feat"], c["Wh"], relu_mask, c["gW0"], c["gb0"])
        got = hook_engine.op_heads_bwd(*args)
        refs = PI.heads_bwd_reference(*args)
        worst = [PI.check_sum(g, r, f"heads_bwd n={n} H={H} O={O} mask={relu_mask} {name}") for g, r, name in zip(got, refs, ("dfeat", "gW", "gb"))]
        if relu_mask:
            assert not got[0][~(c["feat"] > 0)].any()          # exact zeros, negative zeros and negative features
        print(f"heads_bwd n={n} H={H} O={O} mask={relu_mask}: worst err/bound dfeat {worst[0]:.3f} gW {worst[1]:.3f} gb {worst[2]:.3f}")
        again = hook_engine.op_heads_bwd(*args)
        assert all(_same(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("H,O", PI.BWD_HO)
def test_heads_backward_batch_invariance(hook_engine, H, O):
    """dfeat of one n = 8193 launch (17-row chunks) is, bit for bit, that of the same rows launched 16 at a time"""
    n = 8193
    c = PI.heads_case(n, H, O)
    whole = hook_engine.op_heads_bwd(c["dY"], c["feat"], c["Wh"], 1, c["gW0"], c["gb0"])[0]
    parts = [hook_engine.op_heads_bwd(c["dY"][s:s + 16], c["feat"][s:s + 16], c["Wh"], 1, c["gW0"], c["gb0"])[0] for s in range(0, n, 16)]
    held = _same(whole, np.concatenate(parts))
    print(f"heads_bwd batch invariance H={H} O={O}: {'held' if held else 'BROKEN'}")
    assert held


# ------------------------------------------------------------------------------------------------ samplers
_SAMPLE_ERR = {}


def _sampler_torch_errors(H, A, spread, lse):
    """torch's float32 error of lp / logp / value on the 256-row inputs of this (H, A, spread), computed once"""
    key = (H, A, spread, lse)
    if key not in _SAMPLE_ERR:
        c = PI.sample_case(256, H, A, spread)
        r64, r32 = PI.sample_reference(**c, lse=lse), PI.sample_reference(**c, lse=lse, dtype=torch.float32)
        keep = ~r64["edge"]
        _SAMPLE_ERR[key] = {k: PI.rel_l2(r32[k][keep], r64[k][keep]) for k in ("lp", "logp", "value")}
    return _SAMPLE_ERR[key]


def _check_sampler(eng, c, A, lse, terr, what, seed=0, counter=0, philox=False):
    out = eng.op_sample(c["feat"], c["Wh"], c["bh"], None if philox else c["u"], seed=seed, counter=counter, value_from_logits=lse)
    n = c["feat"].shape[0]
    act, logp, val = out["fused"]
    claims = {
        # heads_sample_kernel's comment: given the same logits, its numbers are those of sample_kernel's sequential walk
        "sample_kernel == fused": all(_same(a, b) for a, b in zip(out["fused"], out["sample"])),
        "logp == table[act]": _same(logp, out["table"][np.arange(n), np.clip(act, 0, A - 1)]),
        "pack == arrays": _same(out["pack"], np.stack([act.astype(np.float32), logp, val], axis=1)),
        "logp_all value == value": _same(out["table_value"], val),
    }
    assert ((act >= 0) & (act < A)).all(), what
    r = PI.sample_reference(c["feat"], c["Wh"], c["bh"], c["u"], lse)
    share = PI.check_cap(r["edge"], what)
    PI.check_actions(act, r["act"], r["edge"], A, what)
    keep = ~r["edge"]
    w_h = PI.check_sum(out["hout"], r["hout"], what + " hout")          # d = H; the value head's column included
    e_lp = PI.check_measured(out["table"], r["lp"], terr["lp"], None, what + " table")
    e_logp = PI.check_measured(logp, r["logp"], terr["logp"], keep, what + " logp")
    e_v = PI.check_measured(val, r["value"], terr["value"], None, what + " value") if lse else (0.0, 0.0)
    if not lse:
        assert _same(val, out["hout"][:, A])
    print(f"{what}: hout err/bound {w_h:.3f}  table {e_lp[0]:.2e} (torch {terr['lp']:.2e}, row max {e_lp[1]:.1e})  logp {e_logp[0]:.2e} (torch {terr['logp']:.2e})"
          f"  value {e_v[0]:.2e} (torch {terr['value']:.2e})  excluded {share:.2%}  " + "  ".join(f"[{k}: {'held' if v else 'BROKEN'}]" for k, v in claims.items()))
    assert all(claims.values()), claims
    return out


@pytest.mark.parametrize("H", PI.SAMPLE_H)
@pytest.mark.parametrize("A", PI.SAMPLE_A)
def test_samplers(hook_engine, A, H):
    """heads_sample_kernel in each of its five staging branches, sample_kernel and logp_all_kernel on its logits: the bit-for-bit claims
    within one call, the actions and numbers against float64.  At H = 256 and A <= 15 heads_fwd_kernel's logits of the same rows: not the
    same bits (see the comment above heads_fwd_kernel), but within 138 * 2^-24 * sum|terms| of the fused kernel's -- a step's term differs
    by at most 8 roundings of its products (fused: one product and three fused multiply-adds; unfused: four products and three additions),
    each of the 64 additions and the bias's by one more rounding in either kernel -- about half of what two results that are each
    within the d = 256 bound of float64 could differ by."""
    for i, n in enumerate(PI.SAMPLE_N):
        spread = PI.SPREADS[(i + A + H) % 3]
        c = PI.sample_case(n, H, A, spread)
        for lse in (False, True):
            out = _check_sampler(hook_engine, c, A, lse, _sampler_torch_errors(H, A, spread, lse), f"sample A={A} H={H} n={n} lse={int(lse)} spread={spread}")
        if H == 256 and A <= 15:
            fwd = hook_engine.op_heads_fwd(c["feat"], c["Wh"], c["bh"])
            diff = np.abs(fwd.astype(np.float64) - out["hout"].astype(np.float64))
            bound = 138 * PI.U * PI.heads_fwd_reference(c["feat"], c["Wh"], c["bh"]).sum_abs
            print(f"sample A={A} H=256 n={n}: heads_fwd hout against fused hout: {int((diff > 0).sum())} of {diff.size} elements differ, largest difference "
                  f"{diff.max():.2e} = {float((diff / np.maximum(bound, 1e-300)).max()):.3f} of the bound")
            assert (diff <= bound).all()


def test_sampler_philox(hook_engine):
    """the kernels' own uniforms: Philox(seed, counter + row), the same draw in both kernels, the oracle's generator as the reference"""
    from oracle import philox
    n, H, A, seed, counter = 100, 256, 15, 0x1234567890, (1 << 32) - 40          # (the counter's low word wraps inside the batch)
    c = PI.sample_case(n, H, A, 4.0)
    c["u"] = philox.uniform(seed, counter + np.arange(n, dtype=np.uint64))
    _check_sampler(hook_engine, c, A, False, _sampler_torch_errors(H, A, 4.0, False), "sample philox", seed=seed, counter=counter, philox=True)


# ------------------------------------------------------------------------------------------------ PPO loss
_LOSS_REF = {}


def _loss_refs(n, A, lse, xc, seg=None, n_global=None):
    """(case, float64 reference, excluded rows, torch's float32 dY error, eps_q), computed once.  Fewer than 256 rows: torch's errors are
    those of the 1088-row case of the same distribution."""
    key = (n, A, lse, xc, seg, n_global)
    if key not in _LOSS_REF:
        hp = dict(PI.HP, x_entropy_coef=xc)
        c = PI.loss_case(n, A, lse)
        r64 = PI.loss_reference(c, hp, n_global, seg)
        if n >= 256:
            r32 = PI.loss_reference(c, hp, n_global, seg, dtype=torch.float32)
            keep = ~PI.loss_excluded(r64, hp)
            terr, eps_q = PI.rel_l2(r32["dY"][keep], r64["dY"][keep]), PI.term_errors(r32, r64)
        else:
            terr, eps_q = _loss_refs(PI.POOL_N, A, lse, xc)[3:]
        _LOSS_REF[key] = (c, r64, PI.loss_excluded(r64, hp), terr, eps_q)
    return _LOSS_REF[key]


def _check_loss(eng, mode, n, A, lse, xc, seg=None, n_global=None):
    hp = dict(PI.HP, x_entropy_coef=xc)
    c, r, excl, terr, eps_q = _loss_refs(n, A, lse, xc, seg, n_global)
    what = f"loss mode={mode} A={A} n={n} lse={int(lse)} xc={xc}" + (f" seg={list(seg)} n_global={n_global}" if seg else "")
    ehp = eng.hparams(hp["eps_clip"], hp["value_coef"], hp["entropy_coef"], xc, hp["entropy_multiplier"], 0.0)
    dY, partial, stats, log = eng.op_ppo_loss(mode, c["hout"], c["idx"], c["act"], c["old_logp"], c["old_value"], c["ret"], c["adv"], ehp, lse, n_global, seg)
    share = PI.check_cap(excl, what)
    e_dy = PI.check_measured(dY, r["dY"], terr, ~excl, what + " dY")
    if lse:
        assert not dY[:, A].any(), what + ": the value column of dY must be exact zeros under value_from_logits"
    want = PI.block_partials(r, A, eps_q)
    assert partial.shape == (want["pi"].want.shape[0], 8 + A)
    w_p = max(PI.check_sum(partial[:, j], want[q], f"{what} partial {q}") for j, q in ((0, "pi"), (1, "vm"), (2, "H")))
    w_p = max(w_p, PI.check_sum(partial[:, 8:8 + A], want["p"], what + " partial p"))
    w_r = max(PI.check_record(stats[k], log[k], r, k, A, hp, eps_q, what) for k in range(len(r["seg"])) if r["seg"][k])
    print(f"{what}: dY {e_dy[0]:.2e} (torch {terr:.2e}, bound {8 * terr:.2e}, ratio {e_dy[0] / terr:.2f}, row max {e_dy[1]:.1e})  partial err/bound {w_p:.3f}"
          f"  record err/bound {w_r:.3f}  excluded {share:.2%}")
    return dY, partial


@pytest.mark.parametrize("lse", (False, True), ids=("value-head", "lse"))
@pytest.mark.parametrize("A", PI.LOSS_A)
def test_ppo_loss(hook_engine, A, lse):
    """sample_terms / loss_bwd_sample per sample in all nine regimes, the 64-sample block sums and the finalised record: the two-phase path
    with and without the cross-batch entropy, the one-pass path, and -- without batch-level terms -- the same dY bits from both"""
    for n in PI.LOSS_N:
        dY0, p0 = _check_loss(hook_engine, 0, n, A, lse, 0.0)
        _check_loss(hook_engine, 0, n, A, lse, 0.05)
        dY1, p1 = _check_loss(hook_engine, 1, n, A, lse, 0.0, seg=(n,))
        held = _same(dY0, dY1)
        print(f"loss A={A} n={n} lse={int(lse)}: [two-phase dY == one-pass dY: {'held' if held else 'BROKEN'}]")
        assert held


@pytest.mark.parametrize("lse", (False, True), ids=("value-head", "lse"))
@pytest.mark.parametrize("A", PI.LOSS_A)
def test_ppo_loss_segments(hook_engine, A, lse):
    """seg_of_block and loss_finalize_seg_kernel over segments of 0, 1, 63, 64, 65, 130 and 0 samples with n_global != n: every sample's
    gradient, every block's partial row and every non-empty segment's record; the same samples one segment per call give the same dY bits"""
    n = sum(PI.SEG_N)
    dY, _ = _check_loss(hook_engine, 1, n, A, lse, 0.0, seg=PI.SEG_N, n_global=200)
    c = _loss_refs(n, A, lse, 0.0, PI.SEG_N, 200)[0]
    ehp = hook_engine.hparams(PI.HP["eps_clip"], PI.HP["value_coef"], PI.HP["entropy_coef"], 0.0, PI.HP["entropy_multiplier"], 0.0)
    s0 = 0
    for k in PI.SEG_N:
        if k:
            one = hook_engine.op_ppo_loss(0, c["hout"][s0:s0 + k], c["idx"][s0:s0 + k], c["act"], c["old_logp"], c["old_value"], c["ret"], c["adv"], ehp, lse, 200)[0]
            assert _same(one, dY[s0:s0 + k]), f"segment of {k} samples at {s0}"
        s0 += k


def test_ppo_loss_refusals(hook_engine):
    from mi355.engine import EngineError
    c = PI.loss_case(8, 2, False)
    args = (c["hout"], c["idx"], c["act"], c["old_logp"], c["old_value"], c["ret"], c["adv"])
    with pytest.raises(EngineError, match="x_entropy_coef == 0"):
        hook_engine.op_ppo_loss(1, *args, hook_engine.hparams(0.2, 0.5, 0.01, 0.05, 1.0, 0.0), seg_n=(8,))
    with pytest.raises(EngineError, match="fs_coef must be 0"):
        hook_engine.op_ppo_loss(0, *args, hook_engine.hparams(0.2, 0.5, 0.01, 0.0, 1.0, 0.1))
    with pytest.raises(EngineError, match="add up"):
        hook_engine.op_ppo_loss(1, *args, hook_engine.hparams(0.2, 0.5, 0.01, 0.0, 1.0, 0.0), seg_n=(3, 4))


# ------------------------------------------------------------------------------------------------ context level: 1 and 16 actions
def _context_params(A, H, obs):
    """a freshly initialised MLP policy with fc_policy.weight scaled to logits of standard deviation 1 on obs"""
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from oracle import ppo_oracle as O
    torch.manual_seed(6033 + A + H)
    p = {k: v.detach().numpy().copy() for k, v in torch.nn.Module.state_dict(CategoricalPolicy(MLPModel(9, 4, 64, H), False, A)).items()}
    with torch.no_grad():
        feat = O.mlp_embed({k: torch.as_tensor(v) for k, v in p.items()}, torch.as_tensor(obs)).numpy()
    raw = feat @ p["fc_policy.weight"].T + p["fc_policy.bias"]
    p["fc_policy.weight"] = p["fc_policy.weight"] * np.float32(1.0 / max(float(raw.std()), float(np.abs(raw).mean())))
    return p


@pytest.mark.parametrize("A", (1, 16, 15))
def test_context_with_1_and_16_actions(A):
    """What the hooks cannot reach: a context of n_actions 1 / 16 (15 is the control).  One 1040-sample minibatch of an MLP with a 256-wide
    latent -- at 16 actions the heads forward and backward take the GEMM route (A + 1 > 16), at 1 and 15 heads_fwd_kernel / heads_bwd_kernel
    -- against the float64 network (losses 1e-5, every gradient tensor 1e-3 of its norm: the bounds of
    test_update_sized_heads_and_partial_loss_block), and a rollout step of heads_sample_kernel against forward()."""
    from mi355 import engine as M, layout
    from mi355.engine import Engine
    from oracle import ppo_oracle as O
    T_, n, H = 8, 130, 256
    rng = np.random.default_rng(80 + A)
    obs = rng.standard_normal((T_ + 1, n, 9)).astype(np.float32)
    params = _context_params(A, H, obs[0])
    shapes = layout.mlp_param_shapes(A, 9, 4, 64, H)
    eng = Engine("mlp", T_, n, A, T_ * n, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=H)
    try:
        eng.set_params(layout.flatten(shapes, {k: params[k] for k in shapes}))
        for t in range(T_ + 1):
            eng.put_obs(t, obs[t])
        # a rollout step: the fused heads + sample kernel against forward()'s log-probabilities and values
        u = rng.random(n).astype(np.float32)
        u[0], u[-1] = 0.0, np.float32(1 - 2.0 ** -24)
        act, logp, val = eng.rollout_step(0, seed=0, u=u)
        lp_f, v_f = eng.forward(obs[0])
        cdf = np.cumsum(np.exp(lp_f.astype(np.float64)), axis=1)
        edge = (np.abs(cdf[:, :A - 1] - u[:, None]) < PI.U_MARGIN).any(axis=1)
        PI.check_cap(edge, f"context A={A}")
        a_ref = np.minimum((cdf <= u[:, None]).sum(axis=1), A - 1)
        PI.check_actions(act, a_ref, edge, A, f"context A={A} rollout step")
        np.testing.assert_allclose(logp[~edge], lp_f[np.arange(n), a_ref][~edge], rtol=0, atol=1e-6)
        np.testing.assert_allclose(val, v_f, rtol=0, atol=1e-6)
        # one update-sized minibatch against the float64 network
        own = np.stack([eng.forward(obs[t])[1] for t in range(T_ + 1)])
        r = dict(act=rng.integers(0, A, (T_, n)), logp=(np.log(1 / A) + 0.3 * rng.standard_normal((T_, n))).astype(np.float32),
                 val=(own + 0.25 * rng.standard_normal((T_ + 1, n))).astype(np.float32), rew=rng.standard_normal((T_, n)).astype(np.float32),
                 done=(rng.random((T_, n)) < 0.1).astype(np.float32))
        eng.write_field(M.F_ACT, r["act"].astype(np.float32)); eng.write_field(M.F_LOGP, r["logp"]); eng.write_field(M.F_VALUE, r["val"])
        eng.write_field(M.F_REW, r["rew"]); eng.write_field(M.F_DONE, r["done"])
        eng.compute_estimates(0.999, 0.95, True, True)
        adv, ret = eng.read_field(M.F_ADV), eng.read_field(M.F_RET)
        idx = rng.permutation(T_ * n)
        eng.loss_log()
        eng.minibatch(idx, T_ * n, eng.hparams(0.2, 0.5, 0.01, 0.0, 1.0, 0.0))
        rec, g = eng.loss_log()[0], layout.unflatten(shapes, eng.get_grads())
        p = {k: torch.as_tensor(params[k]).double().requires_grad_(True) for k in shapes}
        f = lambda a: torch.as_tensor(np.asarray(a).reshape(-1)[idx])
        lp, v = O.heads(p, O.mlp_embed(p, torch.as_tensor(obs[:-1].reshape(-1, 9)[idx]).double()))
        L = O.ppo_loss(lp, v, f(r["act"]), f(r["logp"]).double(), f(r["val"][:-1]).double(), f(ret).double(), f(adv).double(), float(np.float32(0.2)), 0.5,
                       float(np.float32(0.01)), 0.0, 1.0)
        L["total"].backward()
        for j, k in enumerate(("pi_loss", "value_loss", "entropy", "x_ent", "total")):
            want = float(L[k].detach())
            print(f"context A={A} {k}: {float(rec[j])!r} vs {want!r}")
            assert abs(rec[j] - want) < 1e-5 * max(1.0, abs(want)), (k, rec[j], want)
        for k in shapes:
            want = p[k].grad.numpy()
            if A == 1 and k.startswith("fc_policy"):          # one action: the log-probability is the constant 0, its gradient exactly zero
                assert np.abs(want).max() < 1e-15 and not g[k].any(), (k, np.abs(g[k]).max())
                continue
            e = PI.rel_l2(g[k], want)
            print(f"context A={A} {k}: rel l2 {e:.2e}")
            assert e < 1e-3, (k, e)
    finally:
        eng.close()
