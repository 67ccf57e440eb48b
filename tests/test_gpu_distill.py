"""Policy distillation on the MI355X (distill.py; csrc/distill.hip, mi_distill_label / _minibatch / _loss, mi_optimizer_step_eps): the
loss kernels against float64 autograd, the labels against mi_forward bit for bit, the reference's fit loop (fixture G19) through the
engine, an IMPALA minibatch in fp32 and bf16 against the oracles, the forward-only loss, determinism and refusals, and distill.py end to
end.  Every test here calls symbols that exist only with the feature.  Inputs, references and the derivation of the measured bounds:
tests/distill_inputs.py.

Bounds taken over from existing tests.  G19 (test_gpu_ipl.py's for G16): loss 1e-5 * max(1, |ref|); every gradient tensor relative
L2 < 1e-3; parameter and Adam-moment norms 2e-6 / 1e-4 / 5e-3 x max(1, norm) after optimizer step 1 / 2 / 3...  IMPALA fp32, n = 8:
relative L2 < 1e-3 per tensor against float64 autograd (test_gpu_engine.py _check_grads at G4's size; IPL's case c meets it at n = 8).
IMPALA bf16: test_gpu_bf16.py check_bf16_minibatch_against_oracle's -- teacher-forced backward 5e-3 per tensor and the loss 2e-6 *
max(1, |L|); end to end every tensor within 3 x the algorithm's own fp32-vs-fp64 floor + 1e-3."""
import csv
import os

import numpy as np
import pytest
import torch

import distill_inputs as DI
import ipl_inputs as II
from conftest import load_npz, npz_json

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
STEP_TOL = {1: 2e-6, 2: 1e-4}
INF = float("inf")


@pytest.fixture(scope="module")
def op_engine():
    from mi355.engine import Engine
    eng = Engine("mlp", 2, 2, 2, 4, obs_dim=9, mlp_depth=4, mlp_width=64, out_dim=64)
    yield eng
    eng.close()


def _mlp(T, E, A=2, max_batch=8, obs_dim=9, depth=4, width=64, out=64, **kw):
    from mi355.engine import Engine
    return Engine("mlp", T, E, A, max_batch, obs_dim=obs_dim, mlp_depth=depth, mlp_width=width, out_dim=out, **kw)


def _mlp_params(A=2, obs_dim=9, depth=4, width=64, out=64, seed=0, logit_scale=3.0):
    from mi355 import layout
    shapes = layout.mlp_param_shapes(A, obs_dim, depth, width, out)
    rng = np.random.default_rng(seed)
    p = {n: (rng.standard_normal(s) / np.sqrt(s[-1] if len(s) > 1 else 4.0)).astype(np.float32) for n, s in shapes.items()}
    p["fc_policy.weight"] *= np.float32(logit_scale)
    return shapes, p


def _fill(eng, rows):
    """rows (T * E, ...) -> observation slots 0 .. T - 1 (slot T: the first E rows again; no distillation pass reads it)."""
    E = eng.E
    for t in range(eng.T + 1):
        eng.put_obs(t, rows[(t % eng.T) * E:(t % eng.T + 1) * E])
    eng.sync()


# ------------------------------------------------------------------------------------------------ 1: the kernels alone
@pytest.mark.parametrize("A", DI.OP_A)
@pytest.mark.parametrize("n", DI.OP_N)
def test_op_distill_loss_against_float64_autograd(op_engine, n, A):
    """mi_op_distill_loss on random head rows (row 0 saturated at +-80, row 1 equal to its target) against float64 autograd of
    MSELoss(Categorical(logits=log_softmax(z)).logits, y), with n_global = n and n_global = 2 n + 1.
    Measured on the MI355X: worst dY error / torch's float32 error 3.51 (n = 257, A = 2, n_global = 515; the bound is 8), most cases
    0.4 .. 1.9; worst loss error / bound 0.089 (n = 1)."""
    hout, y = DI.op_case(n, A)
    terr, rms_q = DI.torch_errors(n, A)
    for n_global in (n, 2 * n + 1):
        rec, dY = op_engine.op_distill_loss(hout, y, n_global)
        ref_loss, ref_dY, terms = DI.mse(hout, y, n_global)
        err, bound = DI.rel_l2(dY, ref_dY), DI.loss_bound(ref_loss, terms, rms_q, n_global * A)
        print(f"n={n} A={A} n_global={n_global}: dY {err:.2e} (torch {terr:.2e}, ratio {err / terr:.2f})  loss {rec[0]:.6g} err/bound {abs(rec[0] - ref_loss) / bound:.3f}")
        assert np.isfinite(dY).all() and err <= 8 * terr, (n, A, n_global, err, terr)
        assert abs(float(rec[0]) - ref_loss) <= bound, (n, A, n_global, rec[0], ref_loss, bound)
        assert rec[4] == rec[0] and not rec[[1, 2, 3, 5, 6, 7]].any()
        assert not dY[:, A].any(), "the value column of dY must be exact zeros"
        if n >= 2:
            assert not dY[1].any(), "a row that equals its target has an exactly zero gradient"
            assert np.abs(dY[0, :A]).max() > 0
    (rec_a, dY_a), (rec_b, dY_b) = op_engine.op_distill_loss(hout, y, n), op_engine.op_distill_loss(hout, y, n)
    assert rec_a.tobytes() == rec_b.tobytes() and dY_a.tobytes() == dY_b.tobytes()


# ------------------------------------------------------------------------------------------------ 2: the labels
def _impala_pair(A=15):
    """(shapes, student params, teacher params): G3's IMPALA weights with scaled logits; the teacher's policy rows rolled and halved."""
    from mi355 import layout
    p = II.initial_params(II.CASES["a"])
    t = dict(p)
    t["fc_policy.weight"] = (0.5 * np.roll(p["fc_policy.weight"], 1, axis=0)).astype(np.float32)
    t["fc_policy.bias"] = np.roll(p["fc_policy.bias"], 1).astype(np.float32)
    return layout.impala_param_shapes(A), p, t


@pytest.mark.parametrize("arch,precision", [("mlp", "fp32"), ("impala", "fp32"), ("impala", "bf16")])
def test_labels_equal_mi_forward_bit_for_bit(arch, precision):
    """T = 3, E = 6 rows in the data ring, a teacher with max_batch = 4: four full chunks and a ragged one.  Then data == teacher
    (max_batch 7: 7 + 7 + 4)."""
    from mi355 import layout
    from mi355.engine import Engine
    T, E = 3, 6
    rng = np.random.default_rng(3)
    if arch == "mlp":
        A = 3
        shapes, tp = _mlp_params(A, seed=5)
        rows = rng.standard_normal((T * E, 9)).astype(np.float32)
        make = lambda t, e, nb: _mlp(t, e, A, nb)
    else:
        A = 15
        shapes, _, tp = _impala_pair(A)
        rows = load_npz("g4_impala_lossgrad.npz")["in/frames"][:3, :6].reshape(T * E, 64, 64, 3).copy()
        make = lambda t, e, nb: Engine("impala", t, e, A, nb, precision=precision)
    data, teacher = make(T, E, 6), make(1, 2, 4)
    assert teacher.max_batch == 4
    teacher.set_params(layout.flatten(shapes, tp))
    _fill(data, rows)
    data.distill_label(teacher)
    got = data.distill_targets()
    want = np.concatenate([teacher.forward(rows[r:r + 4])[0] for r in range(0, T * E, 4)])
    assert got.tobytes() == want.tobytes()
    assert np.abs(np.logaddexp.reduce(got.astype(np.float64), axis=1)).max() < 1e-5
    data.close(); teacher.close()
    both = make(T, E, 7)
    both.set_params(layout.flatten(shapes, tp))
    _fill(both, rows)
    both.distill_label(both)
    want = np.concatenate([both.forward(rows[r:r + 7])[0] for r in range(0, T * E, 7)])
    assert both.distill_targets().tobytes() == want.tobytes()
    both.close()


# ------------------------------------------------------------------------------------------------ 3: G19 through the engine
def test_g19_minibatches_and_optimizer_steps():
    from mi355 import layout
    z = DI.load()
    names, state_names = npz_json(z, "tensor_names"), npz_json(z, "state_names")
    shapes = layout.mlp_param_shapes(2, 9, 4, 64, 64)
    tshapes = layout.mlp_param_shapes(2, 9, 2, 32, 64)
    eng, teng = _mlp(12, 8, 2, 32), _mlp(1, 8, 2, 32, depth=2, width=32)
    start = DI.fixture_params(z, "student/")
    eng.set_params(layout.flatten(shapes, start))
    teng.set_params(layout.flatten(tshapes, DI.fixture_params(z, "teacher/")))
    _fill(eng, z["obs"])
    eng.distill_label(teng)
    y = eng.distill_targets()
    print("labels against the fixture's y_gold:", np.abs(y - z["y_gold"]).max())
    assert np.abs(y - z["y_gold"]).max() < 2e-6
    lr = float(z["lr"])
    nrm = lambda a: float(np.linalg.norm(np.asarray(a, np.float64)))
    for k, rows in DI.batches(z):
        eng.distill_minibatch(rows, len(rows))
        g = layout.unflatten(shapes, eng.get_grads())
        loss = eng.loss_log(reset=True)
        assert loss.shape == (1, 8) and loss[0, 4] == loss[0, 0] and not loss[0, [1, 2, 3, 5, 6, 7]].any()
        ref = float(z["loss"][k])
        print(f"step {k}: loss {loss[0, 0]:.7g} ref {ref:.7g}; worst gradient error",
              max(DI.rel_l2(g[n], z[f"g{k}/{n}"]) for n in state_names))
        assert abs(loss[0, 0] - ref) < 1e-5 * max(1.0, abs(ref)), (k, loss[0, 0], ref)
        for n in state_names:
            assert DI.rel_l2(g[n], z[f"g{k}/{n}"]) < 1e-3, (k, n)
        for n in ("fc_value.weight", "fc_value.bias"):
            assert not g[n].any(), (k, n)
        eng.optimizer_step_eps(lr, INF, 1e-8, k + 1)
        assert not eng.get_grads().any()
        p = layout.unflatten(shapes, eng.get_params())
        m, v = (layout.unflatten(shapes, a) for a in eng.get_adam_state())
        tol = STEP_TOL.get(k + 1, 5e-3)
        for n in names:
            r = nrm(z[f"p{k}/{n}"])
            assert abs(nrm(p[n]) - r) < tol * max(1.0, r), (k, "param", n)
        for q, mom in enumerate((m, v)):
            for j, n in enumerate(state_names):
                r = float(z["step_norms"][k, q, j])
                assert abs(nrm(mom[n]) - r) < tol * max(1.0, r), (k, ("exp_avg", "exp_avg_sq")[q], n)
        for n in ("fc_value.weight", "fc_value.bias"):
            assert p[n].tobytes() == start[n].tobytes() and not m[n].any() and not v[n].any(), (k, n)
    eng.close(); teng.close()


# ------------------------------------------------------------------------------------------------ 4: IMPALA, fp32 and bf16
def _impala_minibatch(precision):
    from mi355 import layout
    from mi355.engine import Engine
    A, n = 15, 8
    shapes, sp, tp = _impala_pair(A)
    frames = load_npz("g4_impala_lossgrad.npz")["in/frames"][0, :n].copy()
    eng, teng = Engine("impala", 1, n, A, n, precision=precision), Engine("impala", 1, n, A, n, precision=precision)
    eng.set_params(layout.flatten(shapes, sp)); teng.set_params(layout.flatten(shapes, tp))
    _fill(eng, frames)
    eng.distill_label(teng)
    y = eng.distill_targets()
    eng.distill_minibatch(np.arange(n), n)
    return eng, teng, shapes, sp, frames, y


def test_impala_minibatch_fp32_against_float64_autograd():
    from mi355 import layout
    eng, teng, shapes, sp, frames, y = _impala_minibatch("fp32")
    g, rec = layout.unflatten(shapes, eng.get_grads()), eng.loss_log()[0]
    loss, ref = DI.minibatch(sp, "impala", DI.O.frames_to_obs(frames), y)
    print("loss", rec[0], loss)
    assert abs(rec[0] - loss) < 1e-5 * max(1.0, abs(loss))
    for n, r in ref.items():
        err = DI.rel_l2(g[n], r)
        print(n, err)
        assert err < 1e-3, (n, err)
    assert set(g) - set(ref) == {"fc_value.weight", "fc_value.bias"} and not g["fc_value.weight"].any() and not g["fc_value.bias"].any()
    eng.close(); teng.close()


def test_impala_minibatch_bf16_against_the_bf16_oracle():
    from mi355 import layout
    from oracle import ppo_oracle_bf16 as OB
    eng, teng, shapes, sp, frames, y = _impala_minibatch("bf16")
    g, rec = layout.unflatten(shapes, eng.get_grads()), eng.loss_log()[0]
    n = len(frames)                 # what the pass stored (mi_debug_read): per block the pooled map, the residual tensors, the arg-max; the features
    acts = [dict(zip(("q", "a1", "y1", "a2", "y2", "arg"), (eng.debug_read(8 * b + j, n) for j in range(6)))) for b in range(3)]
    feat = eng.debug_read(100, n)
    Ltf, gtf = DI.minibatch_bf16(sp, frames, y, forward=OB.cache_from_engine(frames, acts, feat))
    assert abs(rec[0] - Ltf) < 2e-6 * max(1.0, abs(Ltf)), (rec[0], Ltf)           # same features in: fp32 loss arithmetic only
    worst_tf = max((DI.rel_l2(g[k], v), k) for k, v in gtf.items())
    L, go = DI.minibatch_bf16(sp, frames, y)
    L64, g64 = DI.minibatch_bf16(sp, frames, y, dtype=torch.float64)
    assert abs(rec[0] - L) < max(1e-4 * max(1.0, abs(L)), 3.0 * abs(L - L64)), (rec[0], L, L64)
    worst = (0.0, "", 0.0)
    for k, r in go.items():
        floor, e = DI.rel_l2(r, g64[k]), DI.rel_l2(g[k], r)
        worst = max(worst, (e, k, floor))
        assert e < 3.0 * floor + 1e-3, (k, e, floor)
    print(f"teacher-forced backward worst {worst_tf}; end to end worst (error, tensor, algorithm noise floor) {worst}")
    assert worst_tf[0] < 5e-3, worst_tf
    assert not g["fc_value.weight"].any() and not g["fc_value.bias"].any()
    eng.close(); teng.close()


# ------------------------------------------------------------------------------------------------ 5: the forward-only loss
def test_distill_loss_is_the_recombined_chunk_losses():
    """A student with max_batch = 32 on a data ring of 5 x 16 = 80 rows: chunks of 32, 32, 16.  Per chunk the head rows hout = fc(feat) +
    b (float64 on the host from Engine.forward's features, rounded to float32) go through mi_op_distill_loss; the chunk losses are
    recombined in float64 by their row counts.  mi_distill_loss must agree within the loss bound of test 1 -- the float64 loss of those
    rows bounds both -- and change neither the gradients nor the loss log."""
    from mi355 import layout
    A = 3
    shapes, sp = _mlp_params(A, seed=11)
    _, tp = _mlp_params(A, seed=12, logit_scale=6.0)
    eng, data = _mlp(2, 16, A, 32), _mlp(5, 16, A, 16)
    eng.set_params(layout.flatten(shapes, sp)); data.set_params(layout.flatten(shapes, tp))
    rng = np.random.default_rng(13)
    rows = rng.standard_normal((80, 9)).astype(np.float32)
    _fill(data, rows); _fill(eng, rows[:32])
    data.distill_label(data)
    eng.distill_label(data)
    eng.distill_minibatch(np.arange(32), 32)
    g0, log0 = eng.get_grads(), eng.loss_log(reset=False)
    got = eng.distill_loss(data)
    assert np.array_equal(eng.get_grads(), g0) and np.array_equal(eng.loss_log(reset=False), log0) and len(log0) == 1
    y = data.distill_targets()
    total, hout_all = 0.0, []
    for r0 in range(0, 80, 32):
        _, _, feat = eng.forward(rows[r0:r0 + 32], want_feat=True)
        h = feat.astype(np.float64) @ np.concatenate([sp["fc_policy.weight"], sp["fc_value.weight"]]).astype(np.float64).T
        h = (h + np.concatenate([sp["fc_policy.bias"], sp["fc_value.bias"]]).astype(np.float64)).astype(np.float32)
        hout_all.append(h)
        rec, _ = eng.op_distill_loss(h, y[r0:r0 + len(h)])
        total += float(rec[0]) * len(h) * A
    recombined = total / (80 * A)
    hout_all = np.concatenate(hout_all)
    ref, _, terms = DI.mse(hout_all, y)
    _, _, t32 = DI.mse(hout_all, y, dtype=torch.float32)
    rms_q = float(np.sqrt(np.mean((t32 - terms) ** 2)))
    bound = DI.loss_bound(ref, terms, rms_q, 80 * A)
    print(f"distill_loss {got:.8g} recombined {recombined:.8g} float64 {ref:.8g} bound {bound:.3g}")
    assert abs(got - ref) <= bound and abs(recombined - ref) <= bound and abs(got - recombined) <= 2 * bound
    eng.close(); data.close()


# ------------------------------------------------------------------------------------------------ 6: determinism, refusals
def test_same_calls_same_bits():
    from mi355 import layout
    A = 9
    shapes, sp = _mlp_params(A, width=256, seed=21)
    _, tp = _mlp_params(A, width=256, seed=22, logit_scale=6.0)
    rows = np.random.default_rng(23).standard_normal((4 * 80, 9)).astype(np.float32)
    idx = np.random.default_rng(24).permutation(320)[:257]
    runs = []
    for _ in range(2):
        eng, teng = _mlp(4, 80, A, 257, width=256), _mlp(1, 80, A, 100, width=256)
        eng.set_params(layout.flatten(shapes, sp)); teng.set_params(layout.flatten(shapes, tp))
        _fill(eng, rows)
        eng.distill_label(teng)
        eng.distill_minibatch(idx, 257)
        eng.distill_minibatch(idx[:100], 100)                    # accumulates
        g = eng.get_grads()
        gn = eng.optimizer_step_eps(1e-3, INF, 1e-8, 1, want_norm=True)
        runs.append((g, eng.loss_log(), eng.get_params(), eng.distill_loss(eng), gn))
        eng.close(); teng.close()
    a, b = runs
    assert np.linalg.norm(a[0]) > 0 and abs(a[4] - np.linalg.norm(a[0].astype(np.float64))) < 1e-5 * a[4]
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and a[4] == b[4]


def test_optimizer_step_eps_is_optimizer_step_at_its_eps():
    """eps = 1e-5 and the same clip: the bits of mi_optimizer_step (same kernel, same scalars); eps = 1e-8 moves the parameters elsewhere;
    max_grad_norm = inf leaves the gradient unscaled (against a clip far above the norm)."""
    from mi355 import layout
    shapes, sp = _mlp_params(seed=31)
    rows = np.random.default_rng(32).standard_normal((16, 9)).astype(np.float32)
    out = []
    for how in ("plain", "eps5", "eps8", "inf", "huge"):
        eng = _mlp(2, 8, 2, 16)
        eng.set_params(layout.flatten(shapes, sp))
        _fill(eng, rows)
        eng.distill_label(eng)
        eng.set_params(layout.flatten(shapes, _mlp_params(seed=33)[1]))      # (the labels are the first parameters': the loss is not zero)
        eng.distill_minibatch(np.arange(16), 16)
        if how == "plain":
            eng.optimizer_step(1e-3, 0.01, 1)
        else:
            eng.optimizer_step_eps(1e-3, dict(eps5=0.01, eps8=0.01, inf=INF, huge=1e30)[how], 1e-5 if how == "eps5" else 1e-8, 1)
        out.append(eng.get_params())
        eng.close()
    assert np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2]) and np.array_equal(out[3], out[4])


def test_engine_refusals_name_the_entry_and_change_nothing():
    from mi355 import layout
    from mi355.engine import Engine, EngineError
    shapes, sp = _mlp_params(seed=41)
    rows = np.random.default_rng(42).standard_normal((16, 9)).astype(np.float32)
    idx = np.arange(8)
    eng = _mlp(2, 8, 2, 8)
    eng.set_params(layout.flatten(shapes, sp))
    _fill(eng, rows)
    with pytest.raises(EngineError, match="mi_distill_minibatch: no mi_distill_label"):
        eng.distill_minibatch(idx, 8)
    with pytest.raises(EngineError, match="mi_distill_loss: no mi_distill_label"):
        eng.distill_loss(eng)
    with pytest.raises(EngineError, match="mi_distill_targets: no mi_distill_label"):
        eng.distill_targets()
    eng.distill_label(eng)
    eng.distill_minibatch(idx, 8)
    state = lambda: (eng.get_grads(), eng.loss_log(reset=False))
    g0, log0 = state()

    def unchanged():
        g, log = state()
        assert np.array_equal(g, g0) and np.array_equal(log, log0)
    with pytest.raises(EngineError, match="mi_distill_minibatch: n > max_batch"):
        eng.distill_minibatch(np.arange(9), 9)
    with pytest.raises(EngineError, match="mi_distill_minibatch: minibatch index out of range"):
        eng.distill_minibatch(np.array([0, 16]), 2)
    eng.set_multirank(1)
    for call, name in ((lambda: eng.distill_minibatch(idx, 8), "mi_distill_minibatch"), (lambda: eng.distill_label(eng), "mi_distill_label"),
                       (lambda: eng.distill_loss(eng), "mi_distill_loss")):
        with pytest.raises(EngineError, match=name + ": multirank mode must be 0"):
            call()
    eng.set_multirank(0)
    unchanged()
    for other, word in ((_mlp(2, 8, 3, 8), "n_actions"), (_mlp(2, 8, 2, 8, obs_dim=5), "obs_dim"), (Engine("impala", 1, 2, 2, 2), "another kind of observation")):
        with pytest.raises(EngineError, match="mi_distill_label: .*" + word):
            eng.distill_label(other)
        other.close()
    lse = _mlp(2, 8, 2, 8, value_from_logits=True)
    lse.set_params(layout.flatten(shapes, sp))
    _fill(lse, rows)
    lse.distill_label(eng)                                     # (a teacher, or a data ring, may use it ...)
    eng.distill_label(lse)
    with pytest.raises(EngineError, match="mi_distill_minibatch: value_from_logits on the student"):
        lse.distill_minibatch(idx, 8)                            # ... a student may not
    with pytest.raises(EngineError, match="mi_distill_loss: value_from_logits on the student"):
        lse.distill_loss(eng)
    lse.close()
    unchanged()
    # the same minibatch again adds the same gradient a second time (up to the accumulating GEMMs' rounding) and one record: the refused
    # calls left the index ring and the log where they were
    eng.distill_label(eng)
    eng.distill_minibatch(idx, 8)
    log = eng.loss_log(reset=False)
    assert np.allclose(eng.get_grads(), 2 * g0, rtol=1e-5, atol=1e-9) and len(log) == 2 and log[1].tobytes() == log[0].tobytes()
    H = 64
    eng.set_gru(np.zeros((3 * H, H), np.float32), np.zeros((3 * H, H), np.float32), np.zeros(3 * H, np.float32), np.zeros(3 * H, np.float32))
    plain = _mlp(2, 8, 2, 8)
    for call, name in ((lambda: eng.distill_minibatch(idx, 8), "mi_distill_minibatch"), (lambda: eng.distill_label(plain), "mi_distill_label"),
                       (lambda: plain.distill_label(eng), "mi_distill_label"), (lambda: eng.distill_loss(eng), "mi_distill_loss")):
        with pytest.raises(EngineError, match=name + ": a recurrent context"):
            call()
    plain.close(); eng.close()


# ------------------------------------------------------------------------------------------------ 7: distill.py end to end
def _teacher_checkpoint(path):
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(77)
    pol = CategoricalPolicy(MLPModel(9, 4, 256, 64), False, 2)      # the cartpole set's shape
    with torch.no_grad():
        pol.fc_policy.weight.mul_(50.0)                             # (the 0.01-gain initialisation leaves the softmax uniform)
    torch.save({"model_state_dict": pol.state_dict()}, path)


def _run(tmp_path, monkeypatch, ck, check_row0=False):
    import distill
    from common.model import as_device_obs
    tmp_path.mkdir(exist_ok=True)
    monkeypatch.chdir(tmp_path)
    args = distill.parse_args(["--env_name", "cartpole", "--param_name", "cartpole", "--model_file", str(ck), "--n_envs", "8", "--explore_size", "64",
                               "--batch_size", "32", "--nb_epoch", "2", "--n_explore", "3", "--num_checkpoints", "1", "--seed", "3", "--lr", "1e-3"])
    d = distill.Distiller(args)
    try:
        assert (d.student.engine.T, d.student.engine.E, d.teacher.engine.T, d.student.engine.max_batch) == (8, 8, 1, 32)
        for n in range(3):
            perf = d.explore(n)
            if n == 0 and check_row0:
                # the validation loss of the student as it stands now, in float64 on the host from Engine.forward's log-probabilities
                eng, teng = d.student.engine, d.teacher.engine
                y = teng.distill_targets()
                lp = np.concatenate([eng.forward(teng.get_obs(t))[0] for t in range(teng.T)])
                ref = float(np.mean((lp.astype(np.float64) - y) ** 2))
                h = np.concatenate([lp, np.zeros((len(lp), 1), np.float32)], axis=1)      # (normalised rows: normalising again is the identity)
                _, _, terms = DI.mse(h, y)
                _, _, t32 = DI.mse(h, y, dtype=torch.float32)
                bound = DI.loss_bound(ref, terms, float(np.sqrt(np.mean((t32 - terms) ** 2))), y.size)
                print(f"row 0 Valid_Loss {perf['Valid_Loss']:.8g} host float64 {ref:.8g} bound {bound:.3g}")
                assert abs(perf["Valid_Loss"] - ref) <= bound and ref > 1e-4
        d.finish()
        return d.logdir, d.student.engine.get_params()
    finally:
        d.close()


def test_distill_end_to_end(tmp_path, monkeypatch):
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    ck = tmp_path / "teacher.pth"
    _teacher_checkpoint(ck)
    logdir, params = _run(tmp_path / "a", monkeypatch, ck, check_row0=True)
    with open(os.path.join(logdir, "log-append.csv")) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Exploration", "Epoch", "Loss", "Valid_Loss", "Mean_Reward"] and len(rows) == 4
    assert [r[0] for r in rows[1:]] == ["0", "1", "2"] and all(r[1] == "1" for r in rows[1:])
    assert all(np.isfinite(float(r[2])) and np.isfinite(float(r[3])) for r in rows[1:])
    cks = sorted(f for f in os.listdir(logdir) if f.startswith("model_"))
    assert cks == ["model_3.pth"], cks                              # (n > (0 + 1) * (3 // 1) never holds for n in 0..2: the final one only)
    sd = torch.load(os.path.join(logdir, cks[0]), map_location="cpu", weights_only=True)
    pol = CategoricalPolicy(MLPModel(9, 4, 256, 64), False, 2)
    pol.load_state_dict(sd["model_state_dict"])
    names = [n for n, _ in pol.named_parameters()]
    opt = sd["optimizer_state_dict"]
    with_state = sorted(opt["state"])
    assert [names[j] for j in with_state] == [n for n in names if not n.startswith("fc_value")]
    assert all(float(opt["state"][j]["step"]) == 3 * 2 * 2 for j in with_state) and opt["param_groups"][0]["eps"] == 1e-8
    logdir_b, params_b = _run(tmp_path / "b", monkeypatch, ck)
    assert params.tobytes() == params_b.tobytes()
    with open(os.path.join(logdir_b, "log-append.csv")) as f:
        assert list(csv.reader(f)) == rows
