"""The sparse-autoencoder agent on the MI355X (`algo: sae`; csrc/sae.hip, agents/sae.py): the two minibatch ops against float64 autograd
of the reference's expressions, row independence of the codes, the reference's updates through SAE.optimize_sae /
SAE.optimize_linear_model (fixture G15), mi_sae_step against mi_forward, the probe sampler's law, the untouched PPO path, and the
CLI end to end.

Bound rule (tests/test_gpu_bptt.py): a quantity's bound is 8 x the error of torch's own fp32 run on the same inputs against float64 --
the margin between "same arithmetic, another summation order" and a defect.  Errors are relative L2 errors.
A quantity needs enough numbers for torch's error to be an estimate of anything: the fp32 error of ONE number is not -- torch's float is
the correctly rounded float64 value in one case in a few (4e-9 where one ulp is 1e-7: seen on the MI355X runs of these tests), and a
bound of 8 x that asks for correct rounding, which no fp32 forward pass delivers, torch's own included.  So each loss is measured on its
own over several minibatches of the same ring -- recon, KL and total of the SAE pass, value, logit and total of the probe pass: one
8-vector each in the op test, in G15 the per-minibatch values of that loss with the summary entry that is their mean; losses of
different scale never share a norm -- and every gradient tensor on its own, except the one-element fc_value.bias, which is measured
together with fc_value.weight as the gradient of the affine map [W | b] (S + 1 numbers)."""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import sae_inputs as SI
from conftest import PKG, ROOT, load_npz

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
D = SI.D


def _policy(A, scale=1.0, seed=6033):
    from common.model import ImpalaModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(seed)
    pol = CategoricalPolicy(ImpalaModel(3), False, A)
    with torch.no_grad():
        pol.fc_policy.weight.mul_(scale)
    return pol


def _engine(T, E, A, max_batch, S=None, precision="fp32", scale=1.0):
    from mi355 import layout
    from mi355.engine import Engine
    eng = Engine("impala", T, E, A, max_batch, precision=precision)
    pol = _policy(A, scale)
    eng.set_params(layout.flatten(layout.impala_param_shapes(A), {k: v.detach().numpy() for k, v in pol.state_dict().items()}))
    if S is not None:
        eng.sae_create(S, SI.RHO)
    return eng


def rel_l2(a, r):
    a, r = np.asarray(a, np.float64).ravel(), np.asarray(r, np.float64).ravel()
    return float(np.linalg.norm(a - r) / (np.linalg.norm(r) + 1e-300))


def _flat(d, keys):
    return np.concatenate([np.asarray(d[k], np.float32).ravel() for k in keys])


def _joint_value_head(d):
    """name -> tensor with fc_value.weight / fc_value.bias replaced by their concatenation 'fc_value [W | b]' (see the module docstring)."""
    out = OrderedDict((k, np.asarray(v)) for k, v in d.items() if not k.startswith("fc_value."))
    if "fc_value.weight" in d:
        out["fc_value [W | b]"] = np.concatenate([np.asarray(d["fc_value.weight"]).ravel(), np.asarray(d["fc_value.bias"]).ravel()])
    return out


def _unflat(flat, shapes, keys):
    out, o = OrderedDict(), 0
    for k in keys:
        n = int(np.prod(shapes[k]))
        out[k] = flat[o:o + n].reshape(shapes[k])
        o += n
    return out


# ---------------------------------------------------------------------------------------------- 1. the ops
T1, E1 = 5, 8                                  # 40 ring rows


def _op_inputs(n, S, A):
    """Ring contents and parameters for one call on n rows.  Features: non-negative, half of them zero.  Encoder: b_e = 0.1 and weights
    sized so that w . x has a standard deviation of 0.02 (n = 1: every unit of the single row must be active, or rho_hat = 0) or 0.15
    (a quarter of the (row, unit) pairs silent: the ReLU masks act; all n rows of a unit silent: 0.25^19).  Stored values = 3 x the
    probe's own initial value prediction + noise + 2: correlated with it, so that the reference's pairwise value loss (which ignores
    the pairing) differs from the per-sample one."""
    rng = np.random.default_rng(1000 * n + S + A)
    c = dict(S=S, A=A)
    sh = SI.shapes(c)
    x = np.maximum(rng.standard_normal((T1 + 1, E1, D)), 0.0).astype(np.float32) * np.float32(0.25)
    sd = 0.02 if n == 1 else 0.15
    P = OrderedDict()
    w = rng.standard_normal(sh["encoder.0.weight"])
    w -= w.mean(axis=1, keepdims=True)          # blind to the features' common mean: a unit's pre-activations then scatter around b_e on every row
    P["encoder.0.weight"] = (w * sd / np.sqrt(D * x.var())).astype(np.float32)
    P["encoder.0.bias"] = (0.1 + 0.01 * rng.standard_normal(S)).astype(np.float32)
    P["decoder.0.weight"] = (rng.standard_normal(sh["decoder.0.weight"]) / np.sqrt(S)).astype(np.float32)
    P["decoder.0.bias"] = (0.05 * rng.standard_normal(D)).astype(np.float32)
    P["fc_policy.weight"] = (rng.standard_normal(sh["fc_policy.weight"]) * 6.0 / np.sqrt(S)).astype(np.float32)
    P["fc_policy.bias"] = (0.1 * rng.standard_normal(A)).astype(np.float32)
    P["fc_value.weight"] = (rng.standard_normal(sh["fc_value.weight"]) * 6.0 / np.sqrt(S)).astype(np.float32)
    P["fc_value.bias"] = (0.1 * rng.standard_normal(1)).astype(np.float32)
    z = 1.5 * rng.standard_normal((T1, E1, A))
    logits = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    enc = np.maximum(x.reshape(-1, D).astype(np.float64) @ P["encoder.0.weight"].T.astype(np.float64) + P["encoder.0.bias"], 0.0)
    vhat = (enc @ P["fc_value.weight"].T.astype(np.float64) + P["fc_value.bias"]).reshape(T1 + 1, E1)
    value = (3.0 * vhat + 0.3 * rng.standard_normal((T1 + 1, E1)) + 2.0).astype(np.float32)
    idx = rng.permutation(T1 * E1)[:n].astype(np.int64)
    return P, x, logits, value, idx


def _more_idx(n, k=7):
    """k further minibatches of n rows of the same ring (the losses are measured over 1 + k of them: see the module docstring)."""
    rng = np.random.default_rng(77 + n)
    return [rng.permutation(T1 * E1)[:n].astype(np.int64) for _ in range(k)]


def _torch_ops(P, x, logits, value, idx, coef, dtype):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    Pt = OrderedDict((k, t(v).requires_grad_(True)) for k, v in P.items())
    xs = t(x[:T1].reshape(-1, D))[idx]
    recon, kl, rho_hat = SI.sae_losses(Pt, xs)
    (recon + coef * kl).backward()
    sae = dict(losses=[float(recon.detach()), float(kl.detach()), float((recon + coef * kl).detach())],
               grads=OrderedDict((k, Pt[k].grad.numpy().copy()) for k in SI.SAE_KEYS), rho_hat=rho_hat.detach().numpy())
    vl, ll, per = SI.probe_losses(Pt, Pt, xs, t(logits.reshape(-1, logits.shape[-1]))[idx], t(value[:T1].reshape(-1))[idx])
    (ll + vl).backward()
    probe = dict(losses=[float(vl.detach()), float(ll.detach()), float((ll + vl).detach())],
                 grads=OrderedDict((k, Pt[k].grad.numpy().copy()) for k in SI.PROBE_KEYS), per_sample=float(per.detach()))
    return sae, probe


@pytest.mark.parametrize("S,A", [(64, 15), (192, 9), (64, 9), (192, 15)])
@pytest.mark.parametrize("n", [1, 19, 33])
def test_minibatch_ops_match_float64_autograd(n, S, A):
    """mi_sae_minibatch and mi_sae_probe_minibatch on n rows written through the ring: losses and every gradient against float64
    autograd of the reference's expressions (tests/sae_inputs.sae_losses / probe_losses, the pairwise value loss included)."""
    coef = 0.05
    P, x, logits, value, idx = _op_inputs(n, S, A)
    sh = SI.shapes(dict(S=S, A=A))
    ref_s, ref_p = _torch_ops(P, x, logits, value, idx, coef, torch.float64)
    t32_s, t32_p = _torch_ops(P, x, logits, value, idx, coef, torch.float32)
    assert (ref_s["rho_hat"] > 0).all() and (ref_s["rho_hat"] < 1).all()
    more = _more_idx(n)
    more64 = [_torch_ops(P, x, logits, value, j, coef, torch.float64) for j in more]
    more32 = [_torch_ops(P, x, logits, value, j, coef, torch.float32) for j in more]
    assert all((r[0]["rho_hat"] > 0).all() and (r[0]["rho_hat"] < 1).all() for r in more64)
    if n > 1:
        assert 0.05 < (np.maximum(x[:T1].reshape(-1, D)[idx].astype(np.float64) @ P["encoder.0.weight"].T.astype(np.float64) + P["encoder.0.bias"], 0) == 0).mean() < 0.5
    if n == 33:      # the pairwise form is not the per-sample form on these values
        assert abs(ref_p["losses"][0] - ref_p["per_sample"]) > 0.05 * ref_p["per_sample"], (ref_p["losses"][0], ref_p["per_sample"])
    eng = _engine(T1, E1, A, 64, S)
    try:
        eng.sae_set_params(eng.SAE, _flat(P, SI.SAE_KEYS))
        eng.sae_set_params(eng.PROBE, _flat(P, SI.PROBE_KEYS))
        for t in range(T1 + 1):
            eng.sae_put_ring(t, x[t], logits[t] if t < T1 else None)
            eng.put_policy_outputs(t, None, None, value[t])
        assert np.array_equal(eng.sae_get_hidden(2), x[2]) and np.array_equal(eng.sae_get_logits(3), logits[3])
        assert np.array_equal(eng.sae_get_params(eng.SAE), _flat(P, SI.SAE_KEYS)) and np.array_equal(eng.sae_get_params(eng.PROBE), _flat(P, SI.PROBE_KEYS))
        log_s = eng.sae_minibatch(idx, coef)
        g_s = _unflat(eng.sae_get_grads(eng.SAE), sh, SI.SAE_KEYS)
        log_p = eng.sae_probe_minibatch(idx)
        g_p = _unflat(eng.sae_get_grads(eng.PROBE), sh, SI.PROBE_KEYS)
        assert np.array_equal(eng.sae_get_grads(eng.SAE), _flat(g_s, SI.SAE_KEYS))          # the probe pass leaves the SAE's gradient alone
        logs_s = np.stack([log_s] + [eng.sae_minibatch(j, coef) for j in more])
        logs_p = np.stack([log_p] + [eng.sae_probe_minibatch(j) for j in more])
    finally:
        eng.close()
    stack = lambda first, rest, k: np.array([first[k]["losses"]] + [r[k]["losses"] for r in rest])
    checks = []
    for op, logs, k, names in (("sae", logs_s, 0, ("recon", "KL", "total")), ("probe", logs_p, 1, ("value", "logit", "total"))):
        r64, r32 = stack((ref_s, ref_p), more64, k), stack((t32_s, t32_p), more32, k)
        checks += [(f"{op} loss {nm} over 8 minibatches", logs[:, j], r64[:, j], r32[:, j]) for j, nm in enumerate(names)]
    checks += [(f"d {k}", g_s[k], ref_s["grads"][k], t32_s["grads"][k]) for k in SI.SAE_KEYS]
    jg, jr, jt = _joint_value_head(g_p), _joint_value_head(ref_p["grads"]), _joint_value_head(t32_p["grads"])
    checks += [(f"d {k}", jg[k], jr[k], jt[k]) for k in jg]
    bad = []
    for name, got, ref, t32 in checks:
        err, terr = rel_l2(got, ref), rel_l2(t32, ref)
        print(f"n={n} S={S} A={A} {name}: kernel {err:.3e}  torch fp32 {terr:.3e}  bound {8 * terr:.3e}")
        if not err <= 8 * terr:
            bad.append((name, err, terr))
    assert not bad, bad


def test_rho_hat_of_one_or_more_gives_nan_like_torch():
    """rho_hat_j >= 1 is not clamped: log((1 - rho + eps) / (1 - rho_hat + eps)) of a negative number is NaN in torch and here."""
    S, A = 64, 9
    P, x, logits, value, idx = _op_inputs(19, S, A)
    P["encoder.0.bias"][5] = 3.0
    ref, _ = _torch_ops(P, x, logits, value, idx, 0.05, torch.float32)
    assert np.isnan(ref["losses"][1])
    eng = _engine(T1, E1, A, 64, S)
    try:
        eng.sae_set_params(eng.SAE, _flat(P, SI.SAE_KEYS))
        for t in range(T1):
            eng.sae_put_ring(t, x[t], logits[t])
        log = eng.sae_minibatch(idx, 0.05)
    finally:
        eng.close()
    assert np.isfinite(log[0]) and np.isnan(log[1]) and np.isnan(log[2])


# ---------------------------------------------------------------------------------------------- 2. row independence
def test_codes_do_not_depend_on_batch_size_or_neighbours():
    """enc / rec rows of an n = 33 call equal the same ring rows launched alone and at another offset among other neighbours, bit for bit."""
    for S in (64, 192):
        P, x, logits, value, idx = _op_inputs(33, S, 9)
        eng = _engine(T1, E1, 9, 64, S)
        try:
            eng.sae_set_params(eng.SAE, _flat(P, SI.SAE_KEYS))
            for t in range(T1):
                eng.sae_put_ring(t, x[t], logits[t])
            enc, rec = eng.sae_debug_forward(idx)
            assert np.isfinite(enc).all() and (enc > 0).any() and (enc == 0).any()
            for k in (0, 15, 16, 21, 32):
                e1, r1 = eng.sae_debug_forward(idx[k:k + 1])
                assert np.array_equal(e1[0], enc[k]) and np.array_equal(r1[0], rec[k]), (S, k)
                sel = idx[[3, 30, 8, 2, 11, 9, k, 4]]
                e8, r8 = eng.sae_debug_forward(sel)
                assert np.array_equal(e8[6], enc[k]) and np.array_equal(r8[6], rec[k]), (S, k)
        finally:
            eng.close()


# ---------------------------------------------------------------------------------------------- 3. G15
class _Log:
    logdir = "/tmp"


@pytest.mark.parametrize("name", list(SI.CASES))
def test_g15_updates_through_the_agent(name):
    """The reference's optimize_sae and optimize_linear_model (fixture G15) through SAE.optimize_sae / SAE.optimize_linear_model on the
    engine: summaries, per-minibatch losses, first-minibatch gradients, final parameters and Adam moments against the fixture, each
    within 8 x the error of the torch fp32 replay (tests/sae_inputs.replay) against the float64 replay."""
    from agents.sae import SAE
    from common.storage import SAEStorage
    z = load_npz("g15_sae.npz")
    c, roll, idx_sae, idx_probe = SI.load_case(z, name)
    T, E, A, S = c["T"], c["E"], c["A"], c["S"]
    pol = _policy(A)
    storage = SAEStorage((3, 64, 64), D, T, E, torch.device("cuda", 0), act_shape=A)
    torch.manual_seed(c["seed"])
    agent = SAE(None, pol, _Log(), storage, torch.device("cuda", 0), 1, n_steps=T, n_envs=E, epoch=c["epoch"],
                mini_batch_per_epoch=c["mini_batch_per_epoch"], mini_batch_size=c["mini_batch_size"], learning_rate=SI.LR,
                grad_clip_norm=SI.CLIP, sae_dim=S, rho=SI.RHO, sparse_coef=c["sparse_coef"])
    eng = agent.engine
    try:
        init = {k: v.detach().numpy().copy() for m in (agent.sae, agent.linear_model) for k, v in m.state_dict().items()}
        frames, zero = np.zeros((E, 64, 64, 3), np.uint8), np.zeros(E, np.float32)
        for t in range(T):
            storage.store(frames, roll["hidden"][t], roll["act"][t], zero, zero, [{}] * E, roll["logits"][t], roll["value"][t])
        storage.store_last(frames, roll["hidden"][T], roll["value"][T])
        assert np.array_equal(storage.hidden_batch.numpy(), roll["hidden"]) and np.array_equal(storage.logit_batch.numpy(), roll["logits"])
        assert np.array_equal(storage.value_batch.numpy(), roll["value"]) and np.array_equal(storage.act_batch.numpy(), roll["act"])
        got = {}
        for stage, which, fn, opt, model, off, call in (("sae", eng.SAE, agent.optimize_sae, agent.optimizer, agent.sae, 100, "sae_minibatch"),
                                                        ("probe", eng.PROBE, agent.optimize_linear_model, agent.l_optimizer, agent.linear_model, 200, "sae_probe_minibatch")):
            logs, g0, idxs, inner = [], [], [], getattr(eng, call)

            def spy(idx, *a, inner=inner, which=which):
                out = inner(idx, *a)
                idxs.append(np.asarray(idx))
                logs.append(np.array(out, np.float64))
                if not g0:
                    g0.append(eng.sae_get_grads(which))
                return out
            setattr(eng, call, spy)
            torch.manual_seed(c["seed"] + off)
            summary = fn()
            setattr(eng, call, inner)
            assert np.array_equal(np.stack(idxs), z[f"{name}/idx_{stage}"])
            opt.pull_params()
            st = opt.state_dict()["state"]
            keys = SI.SAE_KEYS if stage == "sae" else SI.PROBE_KEYS
            assert float(st[0]["step"]) == float(z[f"{name}/{stage}/adam_step"])
            got[stage] = dict(summary=np.array(list(summary.values())), summary_keys=list(summary), losses=np.stack(logs),
                              g0=_unflat(g0[0], SI.shapes(c), keys), params=OrderedDict((k, v.numpy()) for k, v in model.state_dict().items()),
                              m=OrderedDict((k, st[i]["exp_avg"].numpy()) for i, k in enumerate(keys)),
                              v=OrderedDict((k, st[i]["exp_avg_sq"].numpy()) for i, k in enumerate(keys)))
    finally:
        eng.close()
    r64 = SI.replay(c, init, roll, idx_sae, idx_probe, torch.float64)
    r32 = SI.replay(c, init, roll, idx_sae, idx_probe, torch.float32)
    bad = []

    def check(label, err, terr):
        print(f"G15 {name} {label}: engine {err:.3e}  torch fp32 {terr:.3e}  bound {8 * terr:.3e}")
        if not err <= 8 * terr:
            bad.append((label, err, terr))

    for stage in ("sae", "probe"):
        pre, g = f"{name}/{stage}/", got[stage]
        assert g["summary_keys"] == (["Loss/total", "Loss/recon", "Loss/sparsity"] if stage == "sae" else ["Loss/total_linear", "Loss/value", "Loss/logit"])
        # loss column j of the per-minibatch records (order: first term, second term, total) is summary entry [1, 2, 0][j]
        for j, nm in enumerate(("recon", "KL", "total") if stage == "sae" else ("value", "logit", "total")):
            col = lambda losses, summary: np.concatenate([np.asarray(losses, np.float64)[:, j], [np.asarray(summary, np.float64)[[1, 2, 0][j]]]])
            check(f"{stage} loss {nm} (per minibatch + summary)", rel_l2(col(g["losses"], g["summary"]), col(z[pre + "losses"], z[pre + "summary"])),
                  rel_l2(col(r32[stage]["losses"], r32[stage]["losses"].mean(0)[[2, 0, 1]]), col(r64[stage]["losses"], r64[stage]["losses"].mean(0)[[2, 0, 1]])))
        np.testing.assert_allclose(g["summary"], g["losses"].mean(0)[[2, 0, 1]], rtol=1e-12)
        for kind, key in (("g0", "g0/"), ("params", "p/"), ("m", "m/"), ("v", "v/")):
            for k, a in g[kind].items():
                if k.startswith("fc_value."):
                    continue
                check(f"{stage} {kind} {k}", SI.tensor_error(a, z, pre + key, k), SI.tensor_error_pair(r32[stage][kind][k], r64[stage][kind][k]))
            if stage == "probe":
                fix = {k: z[f"{pre}{key}g/{k}"] for k in ("fc_value.weight", "fc_value.bias")}
                j = [_joint_value_head(d)["fc_value [W | b]"] for d in (g[kind], fix, r32[stage][kind], r64[stage][kind])]
                check(f"{stage} {kind} fc_value [W | b]", rel_l2(j[0], j[1]), rel_l2(j[2], j[3]))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 4. mi_sae_step
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_step_stores_what_forward_computes(precision):
    """Stored hidden, logits and value of mi_sae_step equal mi_forward's block-3 features (ReLU), log-softmax and value bit for bit;
    acting from the probe leaves the stored logits the policy's; store = 0 changes no ring byte and still advances the sampler."""
    from mi355 import engine as M, layout
    T, E, A, S = 3, 16, 15, 64
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(E, 64, 64, 3), dtype=np.uint8)
    P = _op_inputs(19, S, A)[0]
    eng = _engine(T, E, A, E, S, precision=precision, scale=150.0)
    try:
        eng.sae_set_params(eng.SAE, _flat(P, SI.SAE_KEYS))
        eng.sae_set_params(eng.PROBE, _flat(P, SI.PROBE_KEYS))
        lp, val = eng.forward(frames)
        feat = layout.features_from_device(np.maximum(eng.debug_read(8 * 2 + 4, E), 0.0).reshape(E, D))
        assert (feat > 0).any() and np.exp(lp).max(1).mean() > 1.5 / A
        u = rng.random(E).astype(np.float32)

        def rings():
            return ([eng.sae_get_hidden(t) for t in range(T + 1)] + [eng.sae_get_logits(t) for t in range(T)]
                    + [eng.read_field(f) for f in (M.F_VALUE, M.F_ACT, M.F_REW, M.F_DONE)] + [eng.get_obs(t) for t in range(T + 1)])

        act, v = eng.sae_step(1, frames, act_from_probe=False, store=True, u=u)
        assert np.array_equal(eng.sae_get_hidden(1), feat) and np.array_equal(eng.sae_get_logits(1), lp)
        assert np.array_equal(v, val) and np.array_equal(eng.read_field(M.F_VALUE)[1], val)
        assert np.array_equal(eng.read_field(M.F_ACT)[1], act.astype(np.float32)) and np.array_equal(eng.get_obs(1), frames)
        cdf = np.cumsum(np.exp(lp.astype(np.float64)), 1)
        want = np.minimum((cdf <= u[:, None]).sum(1), A - 1)
        sure = np.abs(cdf - u[:, None]).min(1) > 1e-5
        assert sure.sum() >= E - 2 and np.array_equal(act[sure], want[sure])
        # acting from the probe: Categorical(logits = probe(encode(hidden))); the stored logits stay the policy's
        act_p, v_p = eng.sae_step(2, frames, act_from_probe=True, store=True, u=u)
        assert np.array_equal(eng.sae_get_logits(2), lp) and np.array_equal(eng.sae_get_hidden(2), feat) and np.array_equal(v_p, val)
        enc = np.maximum(feat.astype(np.float64) @ P["encoder.0.weight"].T.astype(np.float64) + P["encoder.0.bias"], 0.0)
        zl = enc @ P["fc_policy.weight"].T.astype(np.float64) + P["fc_policy.bias"]
        pp = np.exp(zl - zl.max(1, keepdims=True)); pp /= pp.sum(1, keepdims=True)
        cdf_p = np.cumsum(pp, 1)
        want_p = np.minimum((cdf_p <= u[:, None]).sum(1), A - 1)
        sure_p = np.abs(cdf_p - u[:, None]).min(1) > 1e-4
        assert sure_p.sum() >= E - 3 and np.array_equal(act_p[sure_p], want_p[sure_p])
        assert np.array_equal(eng.read_field(M.F_ACT)[2], act_p.astype(np.float32))
        # the bootstrap step stores hidden and value only
        before = rings()
        eng.sae_step(T, frames, store=True, u=u)
        after = rings()
        changed = [i for i, (a, b) in enumerate(zip(before, after)) if not np.array_equal(a, b)]
        assert set(changed) <= {T, 2 * T + 1, 2 * T + 5 + T} and np.array_equal(eng.sae_get_hidden(T), feat)
        assert np.array_equal(eng.read_field(M.F_VALUE)[T], val)
        # store = 0: no ring byte changes, the unstored step's outputs are readable, the sampler counter moves on
        other = rng.integers(0, 256, size=(E, 64, 64, 3), dtype=np.uint8)
        before = rings()
        a1, _ = eng.sae_step(0, other, store=False, seed=9)
        a2, _ = eng.sae_step(0, other, store=False, seed=9)
        a3, _ = eng.sae_step(0, other, act_from_probe=True, store=False, seed=9)
        assert all(np.array_equal(a, b) for a, b in zip(before, rings()))
        lp_o, _ = eng.forward(other)
        assert np.array_equal(eng.sae_get_logits(-1), lp_o)
        assert np.array_equal(eng.sae_get_hidden(-1), layout.features_from_device(np.maximum(eng.debug_read(20, E), 0.0).reshape(E, D)))
        assert not np.array_equal(a1, a2)
    finally:
        eng.close()


def _chi2_critical(dof, p=1e-4):
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p, dof))
    except ImportError:
        return {8: 31.828, 14: 42.579}[dof]          # upper 1e-4 points of chi^2


def test_probe_actions_follow_the_probe_distribution():
    """Categorical(logits = probe(encode(hidden))).sample() (agents/sae.py:81-84) through the production path: 200 envs that all see the same
    frame -- one fixed probe distribution -- x 100 steps = 20 000 draws from the engine's Philox stream; Pearson chi^2 of the action
    counts against softmax(probe logits) (float64, from the stored hidden), A - 1 degrees of freedom, at the 1e-4 level."""
    from mi355 import engine as M
    T, E, A, S, R = 1, 200, 15, 64, 100
    rng = np.random.default_rng(11)
    frames = np.repeat(rng.integers(0, 256, size=(1, 64, 64, 3), dtype=np.uint8), E, axis=0)
    P = _op_inputs(19, S, A)[0]
    eng = _engine(T, E, A, E, S)
    try:
        eng.sae_set_params(eng.SAE, _flat(P, SI.SAE_KEYS))
        eng.sae_step(0, frames, act_from_probe=True, store=True, seed=77)
        hid = eng.sae_get_hidden(0).astype(np.float64)
        assert np.array_equal(hid, np.repeat(hid[:1], E, axis=0))
        # a probe whose distribution over this one code vector is spread: no cell below 1 %
        enc = np.maximum(hid[0] @ P["encoder.0.weight"].T.astype(np.float64) + P["encoder.0.bias"], 0.0)
        target = np.log(rng.dirichlet(np.full(A, 8.0)))
        P["fc_policy.weight"] = (np.outer(target - target.mean(), enc) / (enc @ enc)).astype(np.float32)
        P["fc_policy.bias"] = np.zeros(A, np.float32)
        eng.sae_set_params(eng.PROBE, _flat(P, SI.PROBE_KEYS))
        zl = enc @ P["fc_policy.weight"].T.astype(np.float64) + P["fc_policy.bias"]
        p = np.exp(zl - zl.max()); p /= p.sum()
        assert p.min() > 0.01 and p.max() < 0.5
        counts = np.zeros(A, np.int64)
        for r in range(R):
            act, _ = eng.sae_step(0, frames, act_from_probe=True, store=(r % 2 == 0), seed=77)
            counts += np.bincount(act, minlength=A)
        a_pol, _ = eng.sae_step(0, frames, act_from_probe=False, store=False, seed=77)
    finally:
        eng.close()
    exp = R * E * p
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    crit = _chi2_critical(A - 1)
    print(f"chi2 {chi2:.2f} on {A - 1} dof (1e-4 point {crit:.2f}); smallest expected count {exp.min():.0f}")
    assert counts.sum() == R * E and chi2 < crit, (chi2, crit, counts.tolist())
    assert len(np.unique(a_pol)) > 1


# ---------------------------------------------------------------------------------------------- 5. the PPO path
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ppo_path_is_untouched_by_an_sae_context(precision):
    """With an SAE created (and used) on the engine, a policy step, the estimates, a mi_minibatch and the optimizer step give the bits of
    an engine without one."""
    from mi355 import engine as M
    T, E, A, B = 4, 8, 15, 16
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, size=(T + 1, E, 64, 64, 3), dtype=np.uint8)
    u = rng.random((T + 1, E)).astype(np.float32)
    rew, done = rng.standard_normal((T, E)).astype(np.float32), (rng.random((T, E)) < 0.2).astype(np.float32)
    idx = rng.permutation(T * E)[:B]
    outs = []
    for with_sae in (False, True):
        eng = _engine(T, E, A, B, 64 if with_sae else None, precision=precision)
        try:
            if with_sae:
                P = _op_inputs(19, 64, A)[0]
                eng.sae_set_params(eng.SAE, _flat(P, SI.SAE_KEYS))
                eng.sae_set_params(eng.PROBE, _flat(P, SI.PROBE_KEYS))
                for t in range(T + 1):
                    eng.sae_step(t, frames[(t + 1) % (T + 1)], act_from_probe=bool(t & 1), store=True, seed=4)
                j = rng.permutation(T * E)[:8]
                eng.sae_minibatch(j, 0.01); eng.sae_probe_minibatch(j)
                eng.sae_optimizer_step(eng.SAE, 1e-3, 0.5, 1); eng.sae_optimizer_step(eng.PROBE, 1e-3, 0.5, 1)
            res = []
            for t in range(T + 1):
                eng.put_obs(t, frames[t])
                out = eng.policy_step(t, seed=1, u=u[t])
                res += list(out) if t < T else [out[2]]          # (the bootstrap step returns a value only)
                if t < T:
                    eng.put_step(t, rew[t], done[t])
            eng.compute_estimates(0.999, 0.95, True, True)
            res += [eng.read_field(M.F_ADV), eng.read_field(M.F_RET)]
            eng.minibatch(idx, B, eng.hparams())
            res += [eng.get_grads(), eng.loss_log()]
            eng.optimizer_step(5e-4, 0.5, 1)
            res += [eng.get_params()]
            outs.append(res)
        finally:
            eng.close()
    assert len(outs[0]) == len(outs[1])
    for k, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------- 6. end to end
def test_agent_trains_both_stages_and_leaves_the_policy_alone(tmp_path):
    """SAE.train in process on the synthetic env (training + validation env): both stages update their model, the losses are finite,
    and the frozen policy's parameters on the device are the bits they were."""
    from agents.sae import SAE
    from common.env.vec_envs import SyntheticFrames
    from common.logger import SimpleLogger
    from common.storage import SAEStorage
    T, E, A, S, N = 8, 8, 9, 64, 128
    dev = torch.device("cuda", 0)
    mk = lambda: SAEStorage((3, 64, 64), D, T, E, dev, act_shape=A)
    agent = SAE(SyntheticFrames(E, A, 1), _policy(A, 50.0), SimpleLogger(E, str(tmp_path)), mk(), dev, 2, env_valid=SyntheticFrames(E, A, 2),
                storage_valid=mk(), n_steps=T, n_envs=E, epoch=2, mini_batch_per_epoch=4, mini_batch_size=8, learning_rate=5e-4, sae_dim=S,
                anneal_lr=False, seed=3)
    try:
        before = agent.engine.get_params()
        p0 = [agent.engine.sae_get_params(w) for w in (0, 1)]
        agent.train(N)
        assert agent.t == 2 * N
        assert np.array_equal(agent.engine.get_params(), before)
        p1 = [agent.engine.sae_get_params(w) for w in (0, 1)]
        assert all(np.isfinite(b).all() and not np.array_equal(a, b) for a, b in zip(p0, p1))
        assert all(np.isfinite(v) for k, v in agent.logger.last.items() if k.startswith("Loss/"))
    finally:
        agent.engine.close()
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["linear_192.pth", "sae_128.pth"]


def test_train_cli_ppo_checkpoint_then_sae(tmp_path):
    """`train.py --algo ppo` for one iteration on the synthetic env writes a checkpoint; `--algo sae --param_name sae --model_file <it>`
    then runs both stages as a fresh child process and writes sae_<t>.pth / linear_<t>.pth that load into stock torch modules with
    the reference's keys (common/model.py:1623-1667)."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    common = [sys.executable, os.path.join(PKG, "train.py"), "--env_name", "synthetic", "--n_envs", "8", "--n_steps", "8", "--seed", "3"]
    r = subprocess.run(common + ["--exp_name", "pol", "--param_name", "debug", "--mini_batch_size", "16", "--num_timesteps", "60", "--num_checkpoints", "1"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    base = tmp_path / "logs" / "train" / "synthetic"
    rd = base / "pol" / os.listdir(base / "pol")[0]
    ck = rd / "model_64.pth"
    assert ck.exists(), os.listdir(rd)
    r = subprocess.run(common + ["--exp_name", "sae", "--algo", "sae", "--param_name", "sae", "--model_file", str(ck), "--num_timesteps", "128",
                                 "--num_checkpoints", "2"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Loading agent from" in r.stdout and "Loss/sparsity" in r.stdout and "Loss/logit" in r.stdout
    # the device held the checkpoint's policy when training started, and the same bits when it ended
    import hashlib
    import re
    from mi355 import layout
    pol = torch.load(ck, map_location="cpu", weights_only=True)["model_state_dict"]
    want = hashlib.sha256(layout.flatten(layout.impala_param_shapes(9), {k: v.numpy() for k, v in pol.items()}).tobytes()).hexdigest()
    assert re.findall(r"policy parameters on the device[^:]*: ([0-9a-f]{64})", r.stdout) == [want, want], r.stdout[-1500:]
    sd = base / "sae" / os.listdir(base / "sae")[0]
    files = set(os.listdir(sd))
    assert {"sae_128.pth", "linear_192.pth"} <= files and "log-append.csv" not in files, files
    A, S = 9, 1024
    sae = torch.nn.Module()
    sae.encoder = torch.nn.Sequential(torch.nn.Linear(D, S), torch.nn.ReLU(inplace=True))
    sae.decoder = torch.nn.Sequential(torch.nn.Linear(S, D))
    probe = torch.nn.Module()
    probe.fc_policy, probe.fc_value = torch.nn.Linear(S, A), torch.nn.Linear(S, 1)
    for f, model in (("sae_128.pth", sae), ("linear_192.pth", probe)):
        c = torch.load(sd / f, map_location="cpu", weights_only=True)
        assert list(c["model_state_dict"]) == list(model.state_dict())
        model.load_state_dict(c["model_state_dict"])
        torch.optim.Adam(model.parameters(), lr=5e-4, eps=1e-5).load_state_dict(c["optimizer_state_dict"])
        assert all(torch.isfinite(v).all() for v in c["model_state_dict"].values())
