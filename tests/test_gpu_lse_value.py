"""CategoricalPolicy(logsumexp_logits_is_v=True) on the MI355X (mi_config.value_from_logits; reference: common/policy.py:77-78,
v = logits.logsumexp(-1)): the rollout heads, the loss and its backward, the saliency seeds and the agent, against fixture G14 (the
reference's own run, tests/golden/make_golden_lse.py) and the float64 restatement of tests/lse_inputs.py (pinned to G14 by
tests/test_lse_value_host.py).

Tolerances are the suite's: forward 2e-5, losses 1e-5, gradient tensors 1e-3 of their norm, the Adam step 2e-6, saliency 2e-3 of the
gradient's scale in fp32 and direction (cos > 0.9) with bf16 storage (tests/test_gpu_engine.py)."""
import os

import numpy as np
import pytest
import torch

import lse_inputs as LI
from conftest import npz_json
from width_inputs import grad_errors, sketch

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
T, E = LI.T, LI.E
ARCHS = ("impala", "mlp")


def make_engine(arch, T, E, A, max_batch, lse=True, precision="fp32", H=None):
    from mi355.engine import Engine
    if arch == "impala":
        return Engine("impala", T, E, A, max_batch, out_dim=H or 256, precision=precision, value_from_logits=lse)
    return Engine("mlp", T, E, A, max_batch, obs_dim=9, mlp_depth=4, mlp_width=256 if H is None else 64, out_dim=H or 64, value_from_logits=lse)


def shapes_for(arch, A, H=None):
    from mi355 import layout
    if arch == "impala":
        return layout.impala_param_shapes(A, output_dim=H or 256)
    return layout.mlp_param_shapes(A, 9, 4, 256 if H is None else 64, H or 64)


def seeded_params(arch, A, H, obs, recurrent=False):
    """Parameters of a freshly initialised policy (IMPALA of width H, or MLPModel(9, 4, 64, H)) with fc_policy.weight scaled so that the
    raw logits of `obs` (device layout) have a standard deviation of 1, as in G14: the 0.01-gain initialisation would leave the softmax
    uniform and the logsumexp at log A whatever the kernel does."""
    from common.model import ImpalaModel, MLPModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(6033 + A + H)
    emb = ImpalaModel(3, output_dim=H) if arch == "impala" else MLPModel(9, 4, 64, H)
    p = {k: v.detach().numpy().copy() for k, v in torch.nn.Module.state_dict(CategoricalPolicy(emb, recurrent, A, logsumexp_logits_is_v=True)).items()}
    feat = LI.forward(p, arch, LI.ref_obs(arch, obs))[2]
    raw = feat @ p["fc_policy.weight"].T + p["fc_policy.bias"]
    p["fc_policy.weight"] = p["fc_policy.weight"] * np.float32(1.0 / raw.std())
    return p


def flat_of(shapes, params):
    from mi355 import layout
    return layout.flatten(shapes, {k: params[k] for k in shapes})


def lse64(params, feat):
    """float64 logsumexp of fc_policy applied to (the engine's own) features."""
    z = feat.astype(np.float64) @ params["fc_policy.weight"].astype(np.float64).T + params["fc_policy.bias"].astype(np.float64)
    m = z.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))).reshape(-1), z


def dev_obs(arch, frames):
    f = np.asarray(frames)
    return f.reshape(-1, 64, 64, 3) if arch == "impala" else f.reshape(-1, f.shape[-1])


def load_case(eng, c):
    from mi355 import engine as M
    for t in range(T + 1):
        eng.put_obs(t, c["frames"][t])
    for t in range(T):
        eng.put_step(t, c["rew"][t], c["done"][t])
    eng.write_field(M.F_ACT, c["act"].astype(np.float32))
    eng.write_field(M.F_LOGP, c["logp"])
    eng.write_field(M.F_VALUE, c["val"])
    eng.sync()


@pytest.fixture(scope="module")
def cases():
    return {a: LI.case(a) for a in ARCHS}


@pytest.fixture(scope="module")
def twin64(cases):
    """float64 restatement of G14's minibatch (all 32 samples in index order): arch -> tag -> (losses, grads, names without gradient)."""
    out = {}
    f = lambda a: np.asarray(a).reshape(-1)
    for arch, c in cases.items():
        obs = LI.ref_obs(arch, c["frames"][:T])
        out[arch] = {tag: LI.loss_and_grads(c["params"], arch, obs, f(c["act"]), f(c["logp"]), f(c["val"][:T]), f(c["ret"]), f(c["adv"]),
                                            x_entropy_coef=xc, dtype=torch.float64) for tag, xc in (("raw", 0.0), ("xent", 0.05))}
    return out


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("arch", ARCHS)
def test_forward_matches_g14(cases, arch):
    c = cases[arch]
    z, A = c["z"], c["A"]
    obs = dev_obs(arch, c["frames"][:T])
    eng = make_engine(arch, T, E, A, T * E)
    eng.set_params(flat_of(shapes_for(arch, A), c["params"]))
    lp, v = eng.forward(obs)
    print("forward", arch, "max |lp - ref|", np.abs(lp - z[f"{arch}/logits"]).max(), "max |v - ref|", np.abs(v - z[f"{arch}/value"]).max())
    np.testing.assert_allclose(lp, z[f"{arch}/logits"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(v, z[f"{arch}/value"], rtol=0, atol=2e-5)
    eng.close()
    off = make_engine(arch, T, E, A, T * E, lse=False)         # flag off: the fc_value head, another number
    off.set_params(flat_of(shapes_for(arch, A), c["params"]))
    lp0, v0 = off.forward(obs)
    assert np.array_equal(lp0, lp) and np.abs(v0 - v).max() > 0.1
    off.close()


def test_engine_refuses_other_flag_values():
    import ctypes as C
    from mi355 import engine as M
    lib = M.load_library()
    cfg = M._Config(arch=M.ARCH_MLP, n_steps=2, n_envs=2, n_actions=2, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64, max_batch=4,
                    value_from_logits=2)
    ctx = C.c_void_p()
    assert lib.mi_create(C.byref(cfg), C.byref(ctx)) != 0 and b"value_from_logits" in lib.mi_last_error()


# ------------------------------------------------------------------------------------------------ 2. rollout heads
@pytest.mark.parametrize("A", [2, 9, 15])
@pytest.mark.parametrize("arch,H,precision", [("impala", 256, "fp32"), ("impala", 256, "bf16"), ("mlp", 64, "fp32"), ("impala", 512, "fp32")])
def test_rollout_heads_give_one_value(arch, H, precision, A):
    """The three staging branches of heads_sample_kernel (H = 256; H < 256; H > 256 in chunks) with one partial 16-env workgroup
    (E = 20), and the unfused kernels.  policy_step, predict_staged (sample_kernel) and forward (logp_all_kernel) read the same head
    outputs and return the same bits; rollout_step (heads_sample_kernel) takes the heads' dot products itself, in another order, so
    its logits -- with the flag off too -- are a few ulp away: like the others it is 2e-5 from a float64 logsumexp on the engine's
    own features, and what it returns is what it stores."""
    from mi355 import engine as M
    n = 20
    rng = np.random.default_rng(A + H)
    obs = rng.integers(0, 256, size=(n, 64, 64, 3), dtype=np.uint8) if arch == "impala" else rng.standard_normal((n, 9)).astype(np.float32)
    params = seeded_params(arch, A, H, obs)
    eng = make_engine(arch, 1, n, A, n, precision=precision, H=H)
    eng.set_params(flat_of(shapes_for(arch, A, H), params))
    eng.put_obs(0, obs)
    _, _, v_step = eng.policy_step(0, seed=3)
    ring_step = eng.read_field(M.F_VALUE)[0].copy()
    a_roll, lp_roll, v_roll = (x.copy() for x in eng.rollout_step(0, seed=3))
    ring_roll = eng.read_field(M.F_VALUE)[0].copy()
    a_st, lp_st, v_st = eng.predict_staged(obs, seed=3, counter=0)
    lp_all, v_fwd, feat = eng.forward(obs, want_feat=True)
    ref, z = lse64(params, feat)
    print("heads", arch, H, precision, A, "max |v - lse64|", np.abs(v_fwd - ref).max(), "spread of v", np.ptp(ref))
    for name, v in (("policy_step", v_step), ("predict_staged", v_st), ("ring/step", ring_step)):
        assert np.array_equal(v, v_fwd), name
    assert np.array_equal(ring_roll, v_roll)
    print("heads", arch, H, precision, A, "rollout_step: max |v - lse64|", np.abs(v_roll - ref).max())
    np.testing.assert_allclose(v_fwd, ref, rtol=0, atol=2e-5)
    np.testing.assert_allclose(v_roll, ref, rtol=0, atol=2e-5)
    assert np.ptp(ref) > 0.05 and np.abs(ref - np.log(A)).max() > 0.05                     # not the uniform softmax's log A
    # the distribution is what it was: the samplers' log-prob is that of the action they drew, log-probs of the twice-normalised softmax
    np.testing.assert_allclose(lp_roll, lp_all[np.arange(n), a_roll], rtol=0, atol=2e-5)
    np.testing.assert_allclose(lp_st, lp_all[np.arange(n), a_st], rtol=0, atol=2e-5)
    np.testing.assert_allclose(lp_all, z - ref[:, None], rtol=0, atol=2e-5)
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. pipelined groups
@pytest.mark.parametrize("arch,precision", [("impala", "bf16"), ("mlp", "fp32")])
def test_pipelined_groups_equal_serial_steps(arch, precision):
    from mi355 import engine as M
    n, G, T_, A, H = 32, 2, 2, (15 if arch == "impala" else 2), (256 if arch == "impala" else 64)
    rng = np.random.default_rng(5)
    obs = (rng.integers(0, 256, size=(T_ + 1, n, 64, 64, 3), dtype=np.uint8) if arch == "impala"
           else rng.standard_normal((T_ + 1, n, 9)).astype(np.float32))
    params = seeded_params(arch, A, H, obs[0])
    flat = flat_of(shapes_for(arch, A, H), params)
    rew = rng.standard_normal((T_, n)).astype(np.float32)
    done = (rng.random((T_, n)) < 0.3).astype(np.float32)
    ser = make_engine(arch, T_, n, A, n, precision=precision, H=H)
    ser.set_params(flat)
    for t in range(T_ + 1):
        ser.put_obs(t, obs[t])
        ser.rollout_step(t, rew[t - 1] if t else None, done[t - 1] if t else None, seed=5)
    want = {f: ser.read_field(f) for f in (M.F_VALUE, M.F_ACT, M.F_LOGP)}
    ser.close()
    pip = make_engine(arch, T_, n, A, n, precision=precision, H=H)
    pip.set_params(flat)
    pip.rollout_groups(G)
    ng = n // G
    stage = [[pip.pinned(obs[0, :ng].shape, obs.dtype) for _ in range(2)] for _ in range(G)]
    vals = np.zeros((T_ + 1, n), np.float32)
    for t in range(T_ + 1):
        for g in range(G):
            sl = slice(g * ng, (g + 1) * ng)
            if t:
                vals[t - 1, sl] = pip.rollout_wait(g)[2]
            stage[g][t & 1][...] = obs[t, sl]
            pip.rollout_submit(t, g, stage[g][t & 1], np.ascontiguousarray(rew[t - 1, sl]) if t else None,
                               np.ascontiguousarray(done[t - 1, sl]) if t else None, seed=5)
    for g in range(G):
        vals[T_, g * ng:(g + 1) * ng] = pip.rollout_wait(g)[2]
    for f, w in want.items():
        assert np.array_equal(pip.read_field(f), w), f
    assert np.array_equal(vals, want[M.F_VALUE]) and np.ptp(vals) > 0.05
    pip.close()


# ------------------------------------------------------------------------------------------------ 4. loss + gradients against G14
@pytest.mark.parametrize("tag,xc", [("raw", 0.0), ("xent", 0.05)])
@pytest.mark.parametrize("arch", ARCHS)
def test_loss_and_gradients_match_g14(cases, twin64, arch, tag, xc):
    from mi355 import engine as M, layout
    c = cases[arch]
    z, A = c["z"], c["A"]
    shapes = shapes_for(arch, A)
    eng = make_engine(arch, T, E, A, T * E)
    flat0 = flat_of(shapes, c["params"])
    eng.set_params(flat0)
    load_case(eng, c)
    eng.compute_estimates(0.999, 0.95, True, True)
    np.testing.assert_allclose(eng.read_field(M.F_ADV), c["adv"], rtol=0, atol=2e-6)
    assert np.array_equal(eng.read_field(M.F_RET), c["ret"])
    eng.minibatch(np.random.default_rng(0).permutation(T * E), T * E, eng.hparams(0.2, 0.5, 0.01, xc, 1.0, 0.0))
    rec = eng.loss_log()[0]
    ref = npz_json(z, f"{arch}/{tag}/summary")
    print("losses", arch, tag, [float(x) for x in rec[:5]], ref)
    assert abs(-rec[0] - ref["Loss/pi"]) < 1e-5
    assert abs(-rec[1] - ref["Loss/v"]) < 1e-5 * max(1.0, abs(ref["Loss/v"]))
    assert abs(rec[2] - ref["Loss/entropy"]) < 1e-5
    assert abs(rec[3] - ref["Loss/x_entropy"]) < 1e-5
    assert abs(rec[4] - ref["Loss/total"]) < 1e-5 * max(1.0, abs(ref["Loss/total"]))
    g = layout.unflatten(shapes, eng.get_grads())
    for k in LI.VALUE_KEYS:
        assert not g[k].any(), k                               # exactly zero: the value column of dY is zero
    err = grad_errors(g, LI.Sub(z, f"{arch}/{tag}/"), prefix="")          # the reference's tensors (large ones: norm / sum / sketch)
    assert sorted(err) == sorted(set(shapes) - set(LI.VALUE_KEYS))
    g64 = twin64[arch][tag][1]
    whole = {k: LI.rel_l2(g[k], g64[k]) for k in g64}           # every tensor whole against the float64 restatement
    print("gradients", arch, tag, "worst vs G14", max((v, k) for k, v in err.items()), "worst vs float64", max((v, k) for k, v in whole.items()))
    assert max(err.values()) < 1e-3, max((v, k) for k, v in err.items())
    assert max(whole.values()) < 1e-3, max((v, k) for k, v in whole.items())
    if tag == "raw":
        gn = eng.optimizer_step(5e-4, 0.5, 1, want_norm=True)
        assert abs(gn - float(z[f"{arch}/step/norm"])) < 1e-5 * gn
        after = layout.unflatten(shapes, eng.get_params())
        before = layout.unflatten(shapes, flat0)
        for k in LI.VALUE_KEYS:
            assert np.array_equal(after[k], before[k]), k       # bit-equal: zero gradient on zero moments is a zero update
        sub = LI.Sub(z, f"{arch}/step/")
        stored = [k[2:] for k in sub.files if k.startswith("g/")]
        for k in stored:
            np.testing.assert_allclose(after[k], sub["g/" + k], rtol=0, atol=2e-6, err_msg=k)
        twin_after, _ = LI.adam_first_step(c["params"], {k: g[k] for k in g64}, 0.5, 5e-4)       # the large tensors: torch's update on these gradients
        for k in set(shapes) - set(stored):
            np.testing.assert_allclose(after[k], twin_after[k], rtol=0, atol=2e-6, err_msg=k)
            # and against the reference's own parameters after its step, kept as norm and +-1 unit-vector projections: an elementwise
            # bound of 2e-6 means ||a - r|| <= 2e-6 sqrt(n), which bounds | ||a|| - ||r|| | and every |s . (a - r)|
            a = after[k].astype(np.float64).ravel()
            bound = 2e-6 * np.sqrt(a.size)
            d_sk, d_nrm = np.abs(sketch(a) - sub["sketch/" + k]).max(), abs(np.linalg.norm(a) - float(sub["norm/" + k]))
            print("adam step", arch, k, "sketch", d_sk, "norm", d_nrm, "bound", bound)
            assert d_sk < bound and d_nrm < bound, (k, d_sk, d_nrm, bound)
        m, v = (layout.unflatten(shapes, x) for x in eng.get_adam_state())
        assert not any(m[k].any() or v[k].any() for k in LI.VALUE_KEYS) and m["fc_policy.weight"].any()
        assert not eng.get_grads().any()
    eng.close()


def test_two_phase_loss_path_equals_the_one_pass(cases):
    """Multi-rank mode 1 runs the loss as loss_fwd_kernel, then (after the statistics exchange) loss_bwd_kernel: on one rank the
    record and the gradients are those of the single pass (loss_fwd_seg_kernel)."""
    c = cases["mlp"]
    A = c["A"]
    out = []
    for mode in (0, 1):
        eng = make_engine("mlp", T, E, A, T * E)
        eng.set_params(flat_of(shapes_for("mlp", A), c["params"]))
        load_case(eng, c)
        eng.compute_estimates(0.999, 0.95, True, True)
        eng.set_multirank(mode)
        eng.minibatch(np.arange(T * E), T * E, eng.hparams(0.2, 0.5, 0.01, 0.05, 1.0, 0.0))
        if mode:
            eng.minibatch_finish()
        out.append((eng.loss_log()[0], eng.get_grads()))
        eng.close()
    np.testing.assert_allclose(out[1][0][:5], out[0][0][:5], rtol=0, atol=2e-6)
    gn = float(np.linalg.norm(out[0][1].astype(np.float64)))
    assert np.abs(out[1][1] - out[0][1]).max() < 2e-7 * gn and gn > 0


# ------------------------------------------------------------------------------------------------ 5. update-sized head path
def _teacher_forced_heads(eng, arch, params, shapes, r, idx, n):
    """One minibatch on the engine, then the float64 restatement's heads + loss on the ENGINE's features of those samples."""
    from mi355 import layout
    eng.minibatch(idx, n, eng.hparams(0.2, 0.5, 0.01, 0.0, 1.0, 0.0))
    rec = eng.loss_log()[0]
    g = layout.unflatten(shapes, eng.get_grads())
    feat = eng.debug_read(100, n)
    f = lambda a: np.asarray(a).reshape(-1)[idx]
    L, g64, none = LI.loss_and_grads(params, arch, None, f(r["act"]), f(r["logp"]), f(r["val"][:-1]), f(r["ret"]), f(r["adv"]),
                                     dtype=torch.float64, feat=feat)
    return rec, g, L, g64


def _check_heads(rec, g, L, g64, label):
    for j, k in enumerate(("pi_loss", "value_loss", "entropy", "x_ent", "total")):
        print(label, k, float(rec[j]), L[k])
        assert abs(rec[j] - L[k]) < 1e-5 * max(1.0, abs(L[k])), (k, rec[j], L[k])
    for k in ("fc_policy.weight", "fc_policy.bias"):
        e = LI.rel_l2(g[k], g64[k])
        print(label, k, "rel l2", e)
        assert e < 1e-3, (k, e)
    for k in LI.VALUE_KEYS:
        assert k not in g64 and not g[k].any(), k


def _scalar_rollout(eng, rng, T_, n, A, obs):
    """Stored actions / log-probs / rewards / dones from the generator; old values = the engine's own logsumexp values + noise, so that
    the value clip acts on part of the samples."""
    from mi355 import engine as M
    for t in range(T_ + 1):
        eng.put_obs(t, obs[t])
    own = np.stack([eng.forward(obs[t])[1] for t in range(T_ + 1)])
    val = own + (0.25 * rng.standard_normal((T_ + 1, n))).astype(np.float32)
    r = dict(own=own, act=rng.integers(0, A, (T_, n)), logp=(np.log(1 / A) + 0.3 * rng.standard_normal((T_, n))).astype(np.float32), val=val.astype(np.float32),
             rew=rng.standard_normal((T_, n)).astype(np.float32), done=(rng.random((T_, n)) < 0.1).astype(np.float32))
    eng.write_field(M.F_ACT, r["act"].astype(np.float32)); eng.write_field(M.F_LOGP, r["logp"]); eng.write_field(M.F_VALUE, r["val"])
    eng.write_field(M.F_REW, r["rew"]); eng.write_field(M.F_DONE, r["done"])
    eng.compute_estimates(0.999, 0.95, True, True)
    r["adv"], r["ret"] = eng.read_field(M.F_ADV), eng.read_field(M.F_RET)
    return r


def test_update_sized_heads_and_partial_loss_block():
    """MLP with a 256-wide latent, 1040 samples in one minibatch: heads_fwd_kernel (n >= 1024, H = 256) feeds the loss, whose last
    64-sample block is partial (1040 = 16 * 64 + 16)."""
    # The route is chosen in csrc/engine.hip net_heads(): heads_fwd_kernel when H == 256, A + 1 <= 16 and the pass has >= 1024 samples,
    # the generic GEMM otherwise.  1040 = T_ * n is past that threshold with a remainder of 16 in the loss's 64-sample blocks; if the
    # threshold moves, move T_ * n with it (the comment at net_heads points back here).
    T_, n, A, H = 8, 130, 2, 256
    assert T_ * n >= 1024 and H == 256 and A + 1 <= 16 and (T_ * n) % 64
    rng = np.random.default_rng(8)
    obs = rng.standard_normal((T_ + 1, n, 9)).astype(np.float32)
    params = seeded_params("mlp", A, H, obs[0])
    shapes = shapes_for("mlp", A, H)
    eng = make_engine("mlp", T_, n, A, T_ * n, H=H)
    eng.set_params(flat_of(shapes, params))
    r = _scalar_rollout(eng, rng, T_, n, A, obs)
    idx = rng.permutation(T_ * n)
    rec, g, L, g64 = _teacher_forced_heads(eng, "mlp", params, shapes, r, idx, T_ * n)
    _check_heads(rec, g, L, g64, "mlp 1040")
    frac = float((np.abs(r["own"][:-1] - r["val"][:-1]) > 0.2).mean())          # both regimes of the value clip are in the minibatch
    assert 0.1 < frac < 0.9, frac
    eng.close()


def test_bf16_heads_teacher_forced(cases):
    """bf16 IMPALA at T = 4, E = 8 on G14's rollout: the heads and the loss are fp32 arithmetic on features that carry the bf16
    storage error, so they are checked on the engine's own features."""
    c = cases["impala"]
    A = c["A"]
    shapes = shapes_for("impala", A)
    eng = make_engine("impala", T, E, A, T * E, precision="bf16")
    eng.set_params(flat_of(shapes, c["params"]))
    load_case(eng, c)
    eng.compute_estimates(0.999, 0.95, True, True)
    from mi355 import engine as M
    idx = np.random.default_rng(1).permutation(T * E)
    r = dict(c, adv=eng.read_field(M.F_ADV), ret=eng.read_field(M.F_RET))
    rec, g, L, g64 = _teacher_forced_heads(eng, "impala", c["params"], shapes, r, idx, T * E)
    _check_heads(rec, g, L, g64, "impala bf16")
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. merged pass
def test_two_segments_in_one_pass_equal_two_minibatches(cases):
    """mi_minibatch_multi over two 16-sample segments against the same two minibatches one call each: same records, accumulated gradient
    equal up to the fp32 summation order (the bounds of test_accumulated_minibatches_in_one_pass_equal_one_by_one)."""
    c = cases["impala"]
    A = c["A"]
    idx = np.random.default_rng(2).permutation(T * E)
    out = []
    for merged in (False, True):
        eng = make_engine("impala", T, E, A, T * E)
        eng.set_params(flat_of(shapes_for("impala", A), c["params"]))
        load_case(eng, c)
        eng.compute_estimates(0.999, 0.95, True, True)
        hp = eng.hparams(0.2, 0.5, 0.01, 0.0, 1.0, 0.0)
        if merged:
            eng.minibatch_multi(idx, [16, 16], 16, hp)
        else:
            eng.minibatch(idx[:16], 16, hp); eng.minibatch(idx[16:], 16, hp)
        out.append((eng.loss_log(), eng.get_grads()))
        eng.close()
    (l0, g0), (l1, g1) = out
    assert l0.shape == l1.shape == (2, 8) and np.abs(l0[0, :5] - l0[1, :5]).max() > 1e-4
    np.testing.assert_allclose(l1[:, :5], l0[:, :5], rtol=0, atol=2e-6)
    gn = float(np.sqrt((g0.astype(np.float64) ** 2).sum()))
    print("merged pass: max |dg|", np.abs(g1 - g0).max(), "of", gn)
    assert np.abs(g1 - g0).max() < 2e-7 * gn, (np.abs(g1 - g0).max(), gn)


# ------------------------------------------------------------------------------------------------ 7. saliency
def _check_saliency(grad, ref, precision, label):
    assert np.abs(ref).max() > 0
    if precision == "fp32":
        print(label, "max |d|", np.abs(grad - ref).max(), "scale", np.abs(ref).max())
        assert np.abs(grad - ref).max() < 2e-3 * np.abs(ref).max(), (np.abs(grad - ref).max(), np.abs(ref).max())
    else:
        cos = float((grad * ref).sum() / (np.linalg.norm(grad) * np.linalg.norm(ref) + 1e-30))
        print(label, "cos", cos)
        assert cos > 0.9, cos


@pytest.mark.parametrize("arch,precision", [("impala", "fp32"), ("impala", "bf16"), ("mlp", "fp32")])
def test_value_saliency_matches_g14_and_autograd(cases, arch, precision):
    c = cases[arch]
    z, A = c["z"], c["A"]
    obs = dev_obs(arch, c["frames"][0])
    eng = make_engine(arch, 2, E, A, E, precision=precision)
    eng.set_params(flat_of(shapes_for(arch, A), c["params"]))
    act, logp, val, grad = eng.value_saliency(obs, seed=3)
    if arch == "impala":
        grad = grad.transpose(0, 3, 1, 2)
    v64, ref64, _ = LI.saliency(c["params"], arch, LI.ref_obs(arch, c["frames"][0]), torch.float64)
    if precision == "fp32":
        np.testing.assert_allclose(val, z[f"{arch}/value"][:E], rtol=0, atol=2e-5)
    _check_saliency(grad, z[f"{arch}/sal"], precision, f"saliency {arch} {precision} vs G14")
    _check_saliency(grad, ref64, precision, f"saliency {arch} {precision} vs float64")
    assert not np.any(eng.get_grads())                        # the pass's parameter gradients were discarded
    a2, l2, v2 = eng.predict_staged(obs, seed=3)
    assert np.array_equal(a2, act) and np.array_equal(l2, logp) and np.array_equal(v2, val)
    # the fc_value head's saliency is another gradient (the test is not vacuous)
    off = make_engine(arch, 2, E, A, E, lse=False, precision=precision)
    off.set_params(flat_of(shapes_for(arch, A), c["params"]))
    g0 = off.value_saliency(obs, seed=3)[3]
    g0 = g0.transpose(0, 3, 1, 2) if arch == "impala" else g0
    assert np.abs(g0 - ref64).max() > 0.1 * np.abs(ref64).max()
    off.close(); eng.close()


@pytest.mark.parametrize("arch,precision", [("impala", "fp32"), ("impala", "bf16"), ("mlp", "fp32")])
def test_value_saliency_through_the_gru_matches_autograd(cases, arch, precision):
    """Recurrent policy: value = logsumexp(fc_policy(h')), h' = GRU(embedder(obs), hidden (1 - done)): the seed into the cell differs from
    row to row (softmax(logits) W_pi).  One env has done = 1."""
    c = cases[arch]
    A, H = c["A"], c["H"]
    rng = np.random.default_rng(12)
    k = 1.0 / np.sqrt(H)
    gru = {n: rng.uniform(-k, k, s).astype(np.float32) for n, s in zip(LI.GRU_KEYS, ((3 * H, H), (3 * H, H), (3 * H,), (3 * H,)))}
    params = dict(c["params"], **gru)
    hid = (0.5 * rng.standard_normal((E, H))).astype(np.float32)
    done = np.array([0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    obs = dev_obs(arch, c["frames"][1])
    # the heads now sit on h' (|h'| < 1), not on the features G14's fc_policy.weight was scaled for: scale again, to raw logits of std 1
    h0 = LI.saliency(params, arch, LI.ref_obs(arch, c["frames"][1]), torch.float64, hidden=hid, done=done)[2]
    params["fc_policy.weight"] = params["fc_policy.weight"] * np.float32(1.0 / (h0 @ params["fc_policy.weight"].T.astype(np.float64)).std())
    eng = make_engine(arch, 2, E, A, E, precision=precision)
    eng.set_params(flat_of(shapes_for(arch, A), params))
    eng.set_gru(*(gru[n] for n in LI.GRU_KEYS))
    eng.rec_state(hid, done)
    act, logp, val, grad = eng.value_saliency(obs, seed=3)
    h_eng = eng.get_hidden()
    if arch == "impala":
        grad = grad.transpose(0, 3, 1, 2)
    v64, ref64, h64 = LI.saliency(params, arch, LI.ref_obs(arch, c["frames"][1]), torch.float64, hidden=hid, done=done)
    if precision == "fp32":
        np.testing.assert_allclose(val, v64, rtol=0, atol=2e-5)
        np.testing.assert_allclose(h_eng, h64, rtol=0, atol=2e-5)
    _check_saliency(grad, ref64, precision, f"recurrent saliency {arch} {precision}")
    assert np.ptp(v64) > 0.02 and not np.any(eng.get_grads())
    # the rows' seeds differ (one vector shared by all rows, the fc_value path's shape, would give another gradient)
    raw = h64 @ params["fc_policy.weight"].T.astype(np.float64) + params["fc_policy.bias"]
    sm1 = np.exp(raw - v64[:, None])
    assert np.abs(sm1 - sm1.mean(axis=0)).max() > 0.05
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. agent
class _Log:
    episode_reward_buffer = [0.0]
    logdir = "/tmp"


def test_agent_trains_checkpoints_and_resumes(cases, tmp_path):
    from agents.ppo import PPO
    from common.env.vec_envs import SyntheticFrames
    from common.logger import Logger
    from common.model import ImpalaModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    from mi355 import layout
    T_, n, A = 4, 8, 15
    dev = torch.device("cuda", 0)

    def build(seed, logger, env=None, env_valid=None):
        torch.manual_seed(seed)
        policy = CategoricalPolicy(ImpalaModel(3), False, A, logsumexp_logits_is_v=True)
        with torch.no_grad():
            policy.fc_policy.weight.mul_(100.0)
        st, stv = Storage((3, 64, 64), 256, T_, n, dev), Storage((3, 64, 64), 256, T_, n, dev)
        agent = PPO(env, policy, logger, st, dev, 1, env_valid=env_valid, storage_valid=stv, n_steps=T_, n_envs=n, epoch=1, n_minibatch=2,
                    mini_batch_size=16, gamma=0.999, lmbda=0.95, learning_rate=5e-4, seed=0, detect_nan=True)
        return agent, policy

    logger = Logger(n, str(tmp_path))
    agent, policy = build(1, logger, SyntheticFrames(n, A, seed=1), SyntheticFrames(n, A, seed=2))
    assert agent.engine.value_from_logits and agent.engine_valid.value_from_logits
    shapes = policy.param_shapes()
    before = layout.unflatten(shapes, agent.engine.get_params())
    agent.train(2 * T_ * n - 1)                                # two iterations, one checkpoint (written when t exceeds the mark)
    row = logger.rows[-1]
    assert all(np.isfinite(row[logger.columns.index(k)]) for k in ("loss_pi", "loss_v", "loss_entropy", "loss_total"))
    after = layout.unflatten(shapes, agent.engine.get_params())
    for k in LI.VALUE_KEYS:
        assert np.array_equal(after[k], before[k]), k
    assert not np.array_equal(after["fc_policy.weight"], before["fc_policy.weight"])
    # the validation twin follows the trained policy and computes the same values
    frames = np.random.default_rng(4).integers(0, 256, size=(n, 64, 64, 3), dtype=np.uint8)
    agent.engine_valid.copy_params_from(agent.engine)
    lp_m, v_m = agent.engine.forward(frames)
    lp_v, v_v = agent.engine_valid.forward(frames)
    assert np.array_equal(v_m, v_v) and np.array_equal(lp_m, lp_v) and np.ptp(v_m) > 0
    # the checkpoint: the optimizer state has the structure the reference wrote (G14): no entries for fc_value
    ck = [f for f in os.listdir(tmp_path) if f.endswith(".pth")]
    assert len(ck) == 1
    state = torch.load(os.path.join(tmp_path, ck[0]), map_location="cpu", weights_only=True)
    want = npz_json(cases["impala"]["z"], "impala/step/opt")
    desc = lambda t: [list(t.shape), str(t.dtype)]
    osd = state["optimizer_state_dict"]
    assert [[k, *desc(t)] for k, t in state["model_state_dict"].items()] == want["model"]
    got = [[int(i), [[k, *desc(t)] for k, t in s.items()]] for i, s in osd["state"].items()]
    assert got == [[i, fields] for i, fields, _ in want["opt_state"]] and len(got) == want["n_parameters"] - 2
    assert all(float(s["step"]) == 4.0 for s in osd["state"].values())              # 2 iterations x 2 optimizer steps
    assert osd["param_groups"][0]["params"] == want["param_groups"][0]["params"]
    for k in LI.VALUE_KEYS:
        assert np.array_equal(state["model_state_dict"][k].numpy(), before[k])
    # a resume from it runs: weights, moments and the step count come back, another update leaves fc_value alone
    agent2, policy2 = build(9, _Log())
    policy2.load_state_dict(state["model_state_dict"])
    agent2.optimizer.load_state_dict(osd)
    assert agent2.optimizer.step_count == 4 and np.array_equal(agent2.engine.get_params(), agent.engine.get_params())
    m1, v1 = agent.engine.get_adam_state(); m2, v2 = agent2.engine.get_adam_state()
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2)
    env = SyntheticFrames(n, A, seed=3)
    agent2._collect(env, agent2.engine, agent2.storage, env.reset(), np.zeros((n, 256), np.float32), np.zeros(n, np.float32))
    agent2.storage.compute_estimates(0.999, 0.95, True, True)
    summary = agent2.optimize()
    assert np.isfinite(summary["Loss/total"]) and agent2.optimizer.step_count == 6
    again = layout.unflatten(shapes, agent2.engine.get_params())
    assert all(np.array_equal(again[k], before[k]) for k in LI.VALUE_KEYS)


def test_non_recurrent_ppo_pure_runs_with_the_flag():
    from agents.ppo_pure import PPOPure
    from common.env.vec_envs import SyntheticFrames
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    T_, n, A = 4, 8, 2
    dev = torch.device("cuda", 0)
    torch.manual_seed(2)
    policy = CategoricalPolicy(MLPModel(9, 4, 64, 64), False, A, logsumexp_logits_is_v=True)
    st = Storage((9,), 64, T_, n, dev)
    agent = PPOPure(None, policy, _Log(), st, dev, 1, n_steps=T_, n_envs=n, epoch=1, n_minibatch=1, mini_batch_size=32, learning_rate=5e-4)
    from mi355 import engine as M
    eng, rng = agent.engine, np.random.default_rng(0)
    assert eng.value_from_logits
    for t in range(T_ + 1):
        eng.put_obs(t, rng.standard_normal((n, 9)).astype(np.float32))
    eng.write_field(M.F_ACT, rng.integers(0, A, (T_, n)).astype(np.float32)); eng.write_field(M.F_LOGP, np.full((T_, n), np.log(0.5), np.float32))
    eng.write_field(M.F_VALUE, rng.standard_normal((T_ + 1, n)).astype(np.float32)); eng.write_field(M.F_REW, rng.standard_normal((T_, n)).astype(np.float32))
    eng.write_field(M.F_DONE, np.zeros((T_, n), np.float32))
    st.compute_estimates(0.999, 0.95, True, True)
    summary = agent.optimize()
    assert set(summary) == {'Loss/pi', 'Loss/v', 'Loss/entropy', 'Loss/x_entropy', 'Loss/total'} and np.isfinite(summary['Loss/total'])
    assert len(agent.optimizer.state_dict()["state"]) == len(list(policy.parameters())) - 2
