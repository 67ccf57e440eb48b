"""The cases and the checker of the op-level GEMM tests (tests/gemm_inputs.py) on the host: every case names the plan launch_gemm's rule
gives it, every exact case meets its exactness precondition, torch's float32 CPU result passes the per-element bound with nothing left
out, and the checker rejects four planted errors -- with the bound shown to be smaller than a single dropped term."""
import os

import numpy as np
import pytest

import gemm_inputs as GI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {"named": GI.CASES}
GROUPS.update({f"edge_{int(a)}{int(b)}": GI.edge_cases(a, b) for a, b in GI.STRIDES})


def _all_cases():
    return [(n, c) for g in GROUPS.values() for n, c in g.items()]


def test_plan_table():
    """The split plan at its edges, by hand from launch_gemm: split = min(512 / tiles, K / 128) from K = 512 on below 192 tiles, k_chunk =
    ceil(K / split) rounded up to 32, split = ceil(K / k_chunk)."""
    assert GI.rule(64, 64, 511) == (1, 512)
    assert GI.rule(64, 64, 512) == (4, 128)
    assert GI.rule(64, 64, 513) == (4, 160)                 # 160 + 160 + 160 + 33
    assert GI.rule(64, 64, 1030) == (7, 160)                # planned 8 -> ceil(1030 / 8) = 129 -> 160 -> 7 slabs
    assert GI.rule(64, 64, 2432) == (19, 128)
    assert GI.rule(640, 640, 2048) == (5, 416)              # 100 tiles: 512 / 100 = 5
    assert GI.rule(769, 1024, 512) == (1, 512)              # 13 x 16 = 208 tiles
    assert GI.rule(768, 1024, 512) == (1, 512)              # 192 tiles: gated as well
    assert GI.rule(704, 1024, 512) == (2, 256)              # 176 tiles: 512 / 176 = 2
    assert GI.rule(64, 64, 1024, ws_floats=3 * 4096 + 100) == (3, 352)      # the workspace cap: 8 -> 3
    assert GI.rule(64, 64, 1024, ws_floats=4095) == (1, 1024)
    assert GI.rule(65, 129, 2048, use_ws=False) == (1, 2048)


def test_every_case_names_its_plan():
    seen = set()
    for name, c in _all_cases():
        M, N, K = GI.mnk(c)
        ws = GI.WS_FLOATS if c["ws_floats"] < 0 else c["ws_floats"]
        assert c["plan"] == GI.rule(M, N, K, c["use_ws"], ws), name
        seen.add(c["plan"])
    assert {(1, 512), (4, 128), (4, 160), (7, 160), (19, 128), (5, 416), (3, 352), (1, 2048)} <= seen


def test_sizes_and_strides_are_covered():
    for a_kc, b_kc in GI.STRIDES:
        cs = GI.edge_cases(a_kc, b_kc).values()
        assert {(GI.mnk(c)[0], GI.mnk(c)[1]) for c in cs} == {(m, n) for m in GI.EDGE_MN for n in GI.EDGE_MN}
        assert {GI.mnk(c)[2] for c in cs} == set(GI.EDGE_K)
    for M in GI.EDGE_MN:
        for N in GI.EDGE_MN:
            ks = {GI.mnk(c)[2] for g in GROUPS.values() for c in g.values() if GI.mnk(c)[:2] == (M, N) and c["form"] == 3 and c["plan"][0] == 1}
            assert len(ks & set(GI.EDGE_K)) >= 4, (M, N, ks)


def test_every_option_runs_direct_and_split():
    """each epilogue option, and the ReLU on an fp32 and on a bf16 operand, at least once in one launch and once through the reduce"""
    opts = {
        "bias": lambda c: c["bias"], "relu_out after bias": lambda c: c["bias"] and c["relu_out"],
        "mask fp32": lambda c: c["mask"] and not GI.c_bf16(c), "mask bf16": lambda c: c["mask"] and GI.c_bf16(c),
        "accumulate": lambda c: c["acc"], "bf16 output": GI.c_bf16, "ldc > N with a mask": lambda c: c["mask"] and (c["ldc"] or 0) > GI.mnk(c)[1],
        "relu_a fp32": lambda c: c["form"] == 0 and c["relu_x"] and not c["x_bf16"], "relu_a bf16": lambda c: c["form"] == 0 and c["relu_x"] and c["x_bf16"],
        "relu_b fp32": lambda c: c["form"] == 2 and c["relu_x"] and not c["x_bf16"], "relu_b bf16": lambda c: c["form"] == 2 and c["relu_x"] and c["x_bf16"],
    }
    for what, f in opts.items():
        paths = {c["plan"][0] > 1 for c in GI.CASES.values() if f(c)}
        assert paths == {False, True}, what
    assert {c["form"] for c in GI.CASES.values()} == {0, 1, 2, 3}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_exact_cases_are_exact(group):
    """S < 2^24 (2^8 for a bf16 output): every partial sum of every order is an integer the output type holds; the float32 CPU result
    equals the float64 one"""
    for name, c in GROUPS[group].items():
        p = GI.build(c, "exact")
        r = GI.reference(p, c["plan"][0])
        s, lim = GI.exact_margin(p, r)
        assert s < lim, (name, s, lim)
        assert np.array_equal(r.want, np.round(r.want))
        got, gb = GI.cpu_result(p)
        GI.check(p, r, got, gb, what=name)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_torch_float32_is_inside_the_bound(group):
    top = 0.0
    for name, c in GROUPS[group].items():
        p = GI.build(c, "real")
        r = GI.reference(p, c["plan"][0])
        got, gb = GI.cpu_result(p)
        top = max(top, GI.check(p, r, got, gb, what=name))
    print(f"{group}: worst err / bound of torch's float32 result = {top:.3g}")
    assert top <= 1.0


@pytest.mark.parametrize("fault", GI.FAULTS)
@pytest.mark.parametrize("layer", GI.LAYERS)
def test_planted_errors_are_rejected(layer, fault):
    """one k dropped from one output tile, the bias one column on, the mask read with stride N under ldc > N, one slab added twice"""
    n = 0
    for name, c in _all_cases():
        if not GI.fault_applies(c, fault):
            continue
        p = GI.build(c, layer)
        if np.array_equal(GI.cpu_result(p, fault, np.float64)[0], GI.cpu_result(p, None, np.float64)[0]):
            continue          # (every element the error touches is masked or clamped, or a few small integers repeat: nothing to see)
        r = GI.reference(p, c["plan"][0])
        got, gb = GI.cpu_result(p, fault)
        with pytest.raises(AssertionError):
            GI.check(p, r, got, gb, what=f"{name} {fault}")
        n += 1
    assert n >= {"drop_k": 200, "bias_shift": 100, "mask_stride": 30, "slab_twice": 12}[fault], n


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_the_bound_bites(group):
    """Drop ONE term a(m, k) b(k, n) from the elements of one output tile, in float64: where that changes the result at all, the bound is
    smaller than the change in most of those elements of every case, and over all cases in more than nine of ten.  (Not in all: a product
    of two standard-normal values is below t with probability about t (1 + ln(1 / t)), and the bound of the longest sum here, K = 2432,
    is 0.23.)"""
    hit = tot = 0
    for name, c in GROUPS[group].items():
        p = GI.build(c, "real")
        r = GI.reference(p, c["plan"][0])
        change = np.abs(GI.cpu_result(p, "drop_k", np.float64)[0] - GI.cpu_result(p, None, np.float64)[0])
        touched = change > 0
        if not touched.any():
            continue
        assert not touched[64:].any() and not touched[:, 64:].any()
        over = change[touched] > r.bound[touched]
        assert over.mean() > 0.5, (name, float(over.mean()))
        hit, tot = hit + int(over.sum()), tot + int(touched.sum())
    print(f"{group}: the bound is below a dropped term in {hit} of {tot} touched elements")
    assert hit > 0.9 * tot


def test_checker_sees_poison_and_masked_leaks():
    p, r = GI.named("direct_ldc_mask_acc", "real")
    got, _ = GI.cpu_result(p)
    bad = got.copy()
    bad[3, 2] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        GI.check(p, r, bad)
    m, n = np.argwhere(~r.kept)[0]
    bad = got.copy()
    bad[m, n] = np.nextafter(bad[m, n], np.float32(np.inf))
    with pytest.raises(AssertionError, match="masked"):
        GI.check(p, r, bad)


def test_hook_is_declared():
    from mi355 import engine
    text = open(os.path.join(ROOT, "include", "mi355ppo.h")).read()
    assert "int mi_op_linear(" in text and "mi_op_linear" in engine.EXPORTS and callable(engine.Engine.op_linear)
