"""Cases, float64 reference and bounds of the fused MLP minibatch pass (csrc/mlp_fused.hip, mi_minibatch_fused, train.py --fused_update):
tests/test_fused_update_host.py on the CPU, tests/test_gpu_fused_update.py on the GPU.  Nothing here touches a GPU.

A case is a network (depth, width, out, obs_dim, A, value_from_logits), rollout rings of T x E rows and the n gathered indices of one
pass in segments seg_n, every segment a global minibatch of n_global samples.  The parameters are the project's own initialisation of
MLPModel + CategoricalPolicy at a fixed torch seed with the policy head scaled up (its gain of 0.01 leaves every logit within 1e-2 of
zero: the softmax would be exercised at one point only); observations, actions, advantages and returns are random.  old_logp and
old_value are built FROM THE FLOAT64 FORWARD of the sample's own row, by policy_inputs.loss_case's scheme: sample s is in ratio regime
s % 3 (below / inside / above the clip), advantage sign (s // 3) % 2 and value regime (s // 6) % 3 (delta inside the clip / outside with
vs1 larger / outside with vs2 larger), with every draw at least 0.03 away from a clip edge or a vs1 == vs2 tie.  So no sample lies within
MARGIN = 1e-3 of a decision that float32 could take the other way, nothing is excluded from any comparison (the cap is 0), and every
regime of policy_inputs.REGIMES is present in every case of 64 rows or more: test_fused_update_host.py asserts all three.

Reference.  The whole pass in float64 torch: the MLP and the heads as oracle.ppo_oracle.mlp_embed / heads have them (raw head rows
[fc_policy; fc_value], test_fused_update_host.py pins this restatement to the reference's own numbers of g4_mlp_lossgrad.npz),
policy_inputs.loss_reference for the loss, its dY and the per-segment records, and autograd from dY back to every parameter.  The same
in float32 on the CPU gives torch's own error per gradient tensor and per kind of loss term; for a case of fewer than 256 rows that
error is measured on a 1088-row case of the same network and distribution (policy_inputs' rule: a few numbers do not estimate an error),
and for a tensor of fewer than 256 elements it is torch's absolute error over 16 draws of the case's own shape (torch_errors).

Bounds.  A gradient tensor: relative L2 <= 8 x torch's float32 error of that tensor (policy_inputs.check_measured).  A record:
policy_inputs.check_record, whose chain length d = 6 + ceil(blocks / 8) + 8 is the fused reduction's own documented order (64-sample
blocks by wave_sum, then loss_finalize_body: the chain's order, csrc/mlp_fused.hip)."""
import numpy as np
import torch
import torch.nn.functional as F

import policy_inputs as PI
from conftest import load_npz, npz_params
from mi355 import layout
from oracle import ppo_oracle as O

MARGIN = 1e-3
HP = dict(PI.HP)
POOL_N = PI.POOL_N
POLICY_GAIN = 150.0      # fc_policy is initialised with gain 0.01: x 150 gives logits a spread of about 1

_BASE = dict(depth=4, width=64, out=64, obs_dim=9, A=2, lse=0)
CASES = {f"base{n}": dict(_BASE, n=n) for n in (1, 15, 16, 17, 31, 32, 33, 1039)}
CASES.update({
    "wide": dict(depth=4, width=256, out=64, obs_dim=9, A=2, lse=0, n=130),
    "shallow": dict(depth=2, width=64, out=64, obs_dim=5, A=3, lse=0, n=65),
    "odd": dict(depth=3, width=48, out=80, obs_dim=9, A=15, lse=0, n=100),
    "max": dict(depth=2, width=512, out=512, obs_dim=16, A=2, lse=0, n=33),
    "lse": dict(_BASE, lse=1, n=65),
    "segments": dict(_BASE, n=324, seg_n=(1, 63, 64, 65, 130, 1), n_global=200),
    "scattered": dict(_BASE, n=65, scattered=True),
})
_cache = {}


def net_key(c):
    return tuple(c[k] for k in ("depth", "width", "out", "obs_dim", "A", "lse"))


def shapes_of(c):
    return layout.mlp_param_shapes(c["A"], c["obs_dim"], c["depth"], c["width"], c["out"])


def params_of(c, seed=1234):
    """flat float32 parameters in parameters() order: MLPModel + CategoricalPolicy as train.py builds them, at a fixed seed"""
    key = ("params",) + net_key(c)[:5]
    if key not in _cache:
        from common.model import MLPModel
        from common.policy import CategoricalPolicy
        gen = torch.random.get_rng_state()
        torch.manual_seed(seed)
        policy = CategoricalPolicy(MLPModel(c["obs_dim"], c["depth"], c["width"], c["out"]), False, c["A"])
        torch.random.set_rng_state(gen)
        p = {k: v.detach().numpy().copy() for k, v in policy.state_dict().items()}
        p["fc_policy.weight"] = p["fc_policy.weight"] * np.float32(POLICY_GAIN)
        p["fc_policy.bias"] = (0.3 * np.random.default_rng(seed).standard_normal(c["A"])).astype(np.float32)
        _cache[key] = layout.flatten(shapes_of(c), p)
    return _cache[key]


def head_rows(c, p, obs):
    """hout (n, A + 1) = [fc_policy; fc_value] on the MLP's output, in p's dtype: ReLU after every embedder layer but the last, none in
    front of the heads (oracle.ppo_oracle.mlp_embed / heads)"""
    x = obs
    names = ["embedder.model.0"] + [f"embedder.model.2.{2 * k}" for k in range(c["depth"] - 2)] + ["embedder.model.3"]
    for i, nm in enumerate(names):
        x = F.linear(x, p[nm + ".weight"], p[nm + ".bias"])
        if i + 1 < len(names):
            x = torch.relu(x)
    return torch.cat([F.linear(x, p["fc_policy.weight"], p["fc_policy.bias"]), F.linear(x, p["fc_value.weight"], p["fc_value.bias"])], dim=1)


def tensors(c, flat, dtype, grad=False):
    return {k: torch.as_tensor(v).to(dtype).requires_grad_(grad) for k, v in layout.unflatten(shapes_of(c), flat).items()}


def build(c, n=None, seed=0):
    """The rings and indices of case c (n rows; default c["n"]) -> dict(T, E, obs (T + 1, E, obs_dim), act, old_logp, old_value (T + 1, E),
    ret, adv (T, E), idx (n,), seg_n, n_global, flat)."""
    n = c["n"] if n is None else n
    A, W, lse = c["A"], c["obs_dim"], bool(c["lse"])
    rng = np.random.default_rng([53, n, seed] + [int(v) for v in net_key(c)])
    E = 8
    T = -(-(n + 37) // E)
    rows, eps = T * E, float(np.float32(HP["eps_clip"]))
    obs = rng.uniform(-1.5, 1.5, (T + 1, E, W)).astype(np.float32)
    idx = rng.permutation(rows)[:n].astype(np.int64)
    if not c.get("scattered"):
        idx = np.sort(idx)
    elif n >= 8:
        idx[3], idx[n - 1], idx[n // 2] = idx[1], idx[5], idx[1]
    flat = params_of(c)
    with torch.no_grad():
        hout = head_rows(c, tensors(c, flat, torch.float64), torch.as_tensor(obs[:T].reshape(rows, W)[idx]).double())
        lp, v = (t.numpy() for t in PI.policy_terms(hout, lse))
    act = rng.integers(0, A, rows).astype(np.int32)
    old_logp, old_v, ret = (rng.standard_normal(rows).astype(np.float32) for _ in range(3))
    adv = (rng.uniform(0.3, 2.0, rows) * rng.choice((-1.0, 1.0), rows)).astype(np.float32)
    seen = set()
    for s in range(n):
        g = int(idx[s])
        if g in seen:
            continue
        seen.add(g)
        rr, sign, vr = s % 3, (1.0 if (s // 3) % 2 == 0 else -1.0), (s // 6) % 3
        target = (rng.uniform(0.5, 0.75), rng.uniform(0.85, 1.15), rng.uniform(1.3, 1.8))[rr]
        old_logp[g] = lp[s, act[g]] - np.log(target)
        adv[g] = sign * rng.uniform(0.3, 2.0)
        sd = rng.choice((-1.0, 1.0))
        if vr == 0:
            old_v[g] = v[s] - sd * rng.uniform(0.0, 0.15)
            ret[g] = v[s] + rng.standard_normal()
        else:
            delta = sd * rng.uniform(0.3, 1.0)
            old_v[g] = v[s] - delta
            vclip = float(old_v[g]) + sd * eps
            ret[g] = (vclip - sd * rng.uniform(0.1, 1.0)) if vr == 1 else (v[s] + sd * rng.uniform(0.1, 1.0))
    value = np.concatenate([old_v, rng.standard_normal(E).astype(np.float32)]).reshape(T + 1, E)
    seg_n = tuple(c.get("seg_n", (n,))) if n == c["n"] else (n,)
    n_global = c.get("n_global", n) if n == c["n"] else n
    return dict(T=T, E=E, obs=obs, act=act.reshape(T, E), old_logp=old_logp.reshape(T, E), old_value=value, ret=ret.reshape(T, E),
                adv=adv.reshape(T, E), idx=idx, seg_n=seg_n, n_global=n_global, flat=flat, n=n)


def reference(c, b, dtype=torch.float64, hp=None):
    """The pass on rings b in dtype (hp: the loss's coefficients, default HP) -> dict(grads: {name: array}, loss: policy_inputs.loss_reference's dict, hout)"""
    p = tensors(c, b["flat"], dtype, grad=True)
    T, E, W = b["T"], b["E"], c["obs_dim"]
    obs = torch.as_tensor(b["obs"][:T].reshape(T * E, W)[b["idx"]]).to(dtype)
    hout = head_rows(c, p, obs)
    lc = dict(hout=hout.detach().numpy(), idx=b["idx"], act=b["act"].reshape(-1), old_logp=b["old_logp"].reshape(-1),
              old_value=b["old_value"][:T].reshape(-1), ret=b["ret"].reshape(-1), adv=b["adv"].reshape(-1), n=b["n"], A=c["A"], lse=bool(c["lse"]))
    r = PI.loss_reference(lc, HP if hp is None else hp, n_global=b["n_global"], seg_n=b["seg_n"], dtype=dtype)
    hout.backward(torch.as_tensor(r["dY"]).to(dtype))
    return dict(grads={k: t.grad.numpy().copy() for k, t in p.items()}, loss=r, hout=lc["hout"])


def rel_err(a, ref):
    ref = np.asarray(ref, np.float64)
    den = np.sqrt((ref ** 2).sum())
    return float(np.sqrt(((np.asarray(a, np.float64) - ref) ** 2).sum()) / den) if den > 0 else float(np.abs(a).max())


SMALL, DRAWS = 256, 16


def torch_errors(c):
    """(terr, eps_q) of case c: torch's float32 error per gradient tensor and policy_inputs.term_errors.
    A tensor of 256 elements or more: terr[name] = relative L2 of torch's float32 gradient against float64, measured on the case itself
    from 256 rows on, else on POOL_N rows of the same network and distribution.
    A tensor of fewer than SMALL = 256 elements (the biases, down to the one number of fc_value.bias): terr["abs"][name] = torch's
    ABSOLUTE L2 error as the root mean square over DRAWS = 16 independent draws of the case's own shape (same n, segments and n_global);
    check_grads divides it by the norm of the case's float64 tensor.  That is policy_inputs' rule that a few numbers do not estimate an
    error, applied to the columns as it is to the rows; and the error of a sum that cancels (fc_policy.bias: the two columns of a 2-action
    head are each other's negatives, and sum|terms| is 10 to 100 times the result) does not shrink with the result, so it is pooled as
    an absolute error and not relative to each draw's own result.  (One draw on the case itself put torch's float32 error of `wide`'s
    fc_policy.bias at 8.3e-9, a seventh of float32's own rounding 2^-24: from the float64 gradient the chain of launches is 62 x that
    figure away and the fused pass 43 x, on every other tensor both are 0.4 .. 3 x torch's error away.)"""
    key = ("terr",) + net_key(c) + (c["n"], c.get("seg_n"), c.get("n_global"), c.get("scattered"))
    if key not in _cache:
        named = any(v is c for v in CASES.values())
        b = (case(c) if named else build(c)) if c["n"] >= 256 else build(c, POOL_N)
        r64 = (ref64(c) if named else reference(c, b)) if c["n"] >= 256 else reference(c, b)
        r32 = reference(c, b, torch.float32)
        terr = {k: rel_err(r32["grads"][k], g) for k, g in r64["grads"].items() if g.size >= SMALL}
        eps_q = PI.term_errors(r32["loss"], r64["loss"])
        sq = {k: 0.0 for k, g in r64["grads"].items() if g.size < SMALL}
        for seed in range(DRAWS):
            d = build(c, seed=seed)
            d64, d32 = reference(c, d), reference(c, d, torch.float32)
            for k in sq:
                sq[k] += float(((d32["grads"][k].astype(np.float64) - d64["grads"][k]) ** 2).sum())
        terr["abs"] = {k: float(np.sqrt(v / DRAWS)) for k, v in sq.items()}
        _cache[key] = (terr, eps_q)
    return _cache[key]


def tensor_error(terr, k, ref):
    """torch's float32 error of tensor k relative to the float64 tensor ref (torch_errors)"""
    return terr["abs"][k] / float(np.sqrt((np.asarray(ref, np.float64) ** 2).sum())) if k in terr["abs"] else terr[k]


def _name(c):
    return next(k for k, v in CASES.items() if v is c)


def case(c):
    """the rings of a CASES entry, built once"""
    key = ("case", _name(c))
    if key not in _cache:
        _cache[key] = build(c)
    return _cache[key]


def ref64(c):
    """the float64 reference of a CASES entry, computed once and shared"""
    key = ("ref", _name(c))
    if key not in _cache:
        _cache[key] = reference(c, case(c))
    return _cache[key]


def check_grads(got_flat, c, ref_grads, terr, factor=8, what=""):
    """every gradient tensor: relative L2 <= factor x torch's float32 error of that tensor (a tensor whose float64 gradient is all zeros --
    fc_value under value_from_logits -- must be all zeros).  Every tensor is measured and printed before the one assertion at the end
    -> {name: error / torch's error}"""
    got = layout.unflatten(shapes_of(c), got_flat)
    out, failed = {}, []
    for k, r in ref_grads.items():
        if not np.any(r):
            assert not np.any(got[k]), f"{what} {k}: the float64 gradient is zero, got {np.abs(got[k]).max():.3e}"
            out[k] = 0.0
            continue
        te = tensor_error(terr, k, r)
        assert te > 0 and np.isfinite(got[k]).all(), (what, k)
        err = rel_err(got[k], r)
        out[k] = err / te
        try:
            if factor == 8:
                PI.check_measured(got[k], r, te, what=f"{what} {k}")
            else:
                assert err <= factor * te, f"{what} {k}: relative L2 error {err:.3e} > {factor} x torch's float32 error {te:.3e}"
        except AssertionError as e:
            failed.append(str(e))
    print(f"{what}: gradient error / torch float32's error (bound {factor}): " + ", ".join(f"{k} {v:.2f}" for k, v in out.items()))
    assert not failed, "\n".join(failed)
    return out


def g4_case():
    """the inputs of g4_mlp_lossgrad.npz (tests/test_oracle_golden.py, tests/test_gpu_engine.py) as a case of fused_update_inputs: the whole
    T * E = 32 batch as one minibatch -> (case, rings, hp)"""
    z = load_npz("g4_mlp_lossgrad.npz")
    T, E = 4, 8
    c = dict(depth=4, width=256, out=64, obs_dim=9, A=2, lse=0, n=T * E)
    adv, ret = O.compute_estimates(torch.from_numpy(z["in/rew"]), torch.from_numpy(z["in/done"]), torch.from_numpy(z["in/val"]), 0.999, 0.95, True, True)
    flat = layout.flatten(shapes_of(c), npz_params(load_npz("g7_mlp_forward.npz")))
    b = dict(T=T, E=E, obs=z["in/frames"], act=z["in/act"].astype(np.int32), old_logp=z["in/logp"], old_value=z["in/val"], ret=ret.numpy(), adv=adv.numpy(),
             idx=np.arange(T * E, dtype=np.int64), seg_n=(T * E,), n_global=T * E, flat=flat, n=T * E)
    hp = dict(eps_clip=0.2, value_coef=0.5, entropy_coef=0.01, x_entropy_coef=0.0, entropy_multiplier=1.0)
    return z, c, b, hp
