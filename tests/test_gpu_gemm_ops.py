"""The generic GEMM (csrc/gemm.hip: gemm_kernel, gemm_splitk_reduce, launch_gemm's plan) one call at a time through mi_op_linear, against
the float64 reference of tests/gemm_inputs.py: linear_fwd / linear_dgrad / linear_wgrad as production calls them, and launch_gemm itself
with the SAE's strides, ldc > N, a null workspace and a capped one.

Every case is run in two layers -- small integers, where the result must EQUAL the reference whatever the summation order, and
standard-normal values under the derived per-element bound with nothing left out -- and on two contexts (an MLP and an IMPALA one: the
hook does not depend on the context).  The plan the hook reports must be the one the case is meant for, so a case that stops splitting
fails.  Each line printed is a row of profiles/gemm_ops_bounds.md."""
import numpy as np
import pytest

import gemm_inputs as GI
import policy_inputs as PI

pytestmark = pytest.mark.gpu

POISON = 0xFFFFFFFF


@pytest.fixture(scope="module")
def engines():
    from mi355.engine import Engine
    e = {"mlp": Engine("mlp", 2, 2, 2, 8, obs_dim=4, mlp_depth=2, mlp_width=8, out_dim=8), "impala": Engine("impala", 2, 2, 15, 4)}
    yield e
    for v in e.values():
        v.close()


def _run(eng, p, r, what):
    """one hook call -> (err / bound, relative L2, its ratio to torch's) with the plan, the padding and every element checked"""
    out, plan = eng.op_linear(**GI.hook_args(p))
    assert plan == p.c["plan"], f"{what}: ran the plan {plan}, the case is meant for {p.c['plan']}"
    got, gb = out if p.c["form"] == 2 else (out, None)
    if p.c["form"] == 3:
        assert got.shape == (p.M, p.ldc)
        pad = got[:, p.N:].view(np.uint32)
        assert (pad == POISON).all(), f"{what}: {int((pad != POISON).sum())} padding elements of C (columns {p.N} .. {p.ldc - 1}) were written"
        got = np.ascontiguousarray(got[:, :p.N])
    worst = GI.check(p, r, got, gb, what=what)
    if p.layer == "exact":
        return worst, 0.0, 0.0
    terr = GI.torch_error(p, r)
    err, _ = PI.check_measured(got, r.want, terr, what=what)
    return worst, err, (err / terr if terr > 0 else 0.0)


@pytest.mark.parametrize("name", sorted(GI.CASES))
def test_named_case(engines, name):
    """one case of gemm_inputs.CASES: the production forms, the split plan's edges, every epilogue option in one launch and through the reduce"""
    c = GI.CASES[name]
    for layer in GI.LAYERS:
        p, r = GI.named(name, layer)
        for ctx, eng in engines.items():
            worst, err, ratio = _run(eng, p, r, f"{name} {layer} on {ctx}")
            if layer == "real" and ctx == "mlp":
                M, N, K = GI.mnk(c)
                print(f"gemm_op | {name} | {c['form']} | {M} x {N} x {K} | {c['plan'][0]} x {c['plan'][1]} | {worst:.3f} | {err:.2e} | {ratio:.2f} |")


@pytest.mark.parametrize("a_kc,b_kc", GI.STRIDES)
def test_tile_and_stride_edges(engines, a_kc, b_kc):
    """M, N in {1, 3, 9, 16, 63, 64, 65, 129} x K in {1, 31, 32, 33, 300} under one of the four (sak == 1, sbk == 1) combinations, the
    epilogue options and ldc = N + 3 cycling: ragged last tiles in both directions, a single row or column, K below, at and past the K tile"""
    top = [0.0, 0.0, 0.0]
    for name, c in GI.edge_cases(a_kc, b_kc).items():
        for layer in GI.LAYERS:
            p = GI.build(c, layer)
            r = GI.reference(p, 1)
            for ctx, eng in engines.items():
                got = _run(eng, p, r, f"{name} {layer} on {ctx}")
                top = [max(a, b) for a, b in zip(top, got)]
    print(f"gemm_op | 64 edge cases, a_kc = {int(a_kc)}, b_kc = {int(b_kc)} (largest of each figure) | 3 | 1 .. 129 x 1 .. 129 x 1 .. 300 | 1 x 32 .. 320 | "
          f"{top[0]:.3f} | {top[1]:.2e} | {top[2]:.2f} |")


def test_padding_stays_poisoned_and_in_out_targets_start_from_the_caller(engines):
    """ldc > N on both paths: the hook hands back C whole, its padding is the poison, and with accumulate the kept part started from C0"""
    for name in ("direct_ldc_mask_acc", "split_ldc_acc", "split_ldc_mask"):
        p, r = GI.named(name, "exact")
        out, plan = engines["mlp"].op_linear(**GI.hook_args(p))
        assert out.shape == (p.M, p.ldc) and p.ldc > p.N and plan == p.c["plan"]
        assert (out[:, p.N:].view(np.uint32) == POISON).all() and np.array_equal(out[:, :p.N], r.want)
        if p.C0 is not None:
            kw = GI.hook_args(p)
            kw["C0"] = p.C0 + 1
            assert np.array_equal(engines["mlp"].op_linear(**kw)[0][:, :p.N], r.want + 1)


def test_refusals(engines):
    from mi355.engine import EngineError
    eng = engines["impala"]
    p = GI.build(GI.CASES["ws_cap"], "exact")
    kw = GI.hook_args(p)
    for dims in ((0, 64, 1024), (64, 0, 1024), (64, 64, 0), (-1, 64, 1024)):          # nothing to write: refused by name, not launched
        with pytest.raises(EngineError, match="sizes must be positive"):
            eng.op_linear(**dict(kw, dims=dims))
    with pytest.raises(EngineError, match="ws_floats above the context's"):
        eng.op_linear(**dict(kw, ws_floats=GI.WS_FLOATS + 1))
    with pytest.raises(EngineError, match="at most 65536"):
        eng.op_linear(**dict(kw, dims=(65537, 64, 1024)))
    with pytest.raises(EngineError, match="2\\^26 elements"):
        eng.op_linear(**dict(kw, dims=(65536, 2048, 8)))
    with pytest.raises(EngineError, match="ldc >= N"):
        eng.op_linear(**dict(kw, strides=kw["strides"][:4] + (63,)))
    with pytest.raises(EngineError, match="sizes must be positive"):
        eng.op_linear(0, np.zeros((0, 9), np.float32), np.zeros((4, 9), np.float32))
    with pytest.raises(EngineError, match="form 0 has no mask"):
        eng.op_linear(0, np.zeros((2, 9), np.float32), np.zeros((4, 9), np.float32), mask=np.ones((2, 4), np.float32))
    out, plan = eng.op_linear(**dict(kw, ws_floats=GI.WS_FLOATS))          # the context's own size is the largest override
    assert plan == (8, 128) and np.array_equal(out, GI.reference(p, 8).want)
