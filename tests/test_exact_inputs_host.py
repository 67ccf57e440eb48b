"""The dyadic-grid method of tests/exact_inputs.py, proved on the CPU: for every case tests/test_gpu_bf16_exact.py runs, the float32
torch evaluation of the reference (which sums in another order than float64's) equals the float64 one bit for bit and every
accumulation stays below 2^24 units; the inputs exercise the rounding rule (ties, rounded outputs, both ReLU branches, pool ties); and
the exact comparison rejects the mutations that the 1e-2 criterion of tests/test_gpu_bf16.py accepts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E


def _id(c):
    return c[0] + "-" + "-".join(map(str, c[1]))


def relerr(a, b):
    """Today's criterion in tests/test_gpu_bf16.py: max |out - ref| / max |ref|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.mark.parametrize("case", E.cases(False), ids=_id)
def test_float32_equals_float64_and_inputs_are_not_degenerate(case):
    c = E.FAMILIES[case[0]][0](*case[1])
    ref64, _, tally = E.evaluate(c, torch.float64)          # (every accumulation's assert_exact runs in here)
    ref32, _, _ = E.evaluate(c, torch.float32)
    assert set(ref64) == set(ref32) and len(ref64) > 0
    for k in ref64:
        assert np.isfinite(ref64[k]).all() and np.abs(ref64[k]).max() > 0, k
        assert np.array_equal(ref64[k], ref32[k]), (c.what, k)
    assert tally.log2 < 24
    if c.strict:
        tally.assert_not_degenerate(c.relu, c.pool)
    else:                   # mode 2 stores no bf16 value; its ReLU and the proofs are still checked
        print(tally.line())
        assert tally.stored == 0 and (tally.relu_pos > 0 and tally.relu_neg > 0) == c.relu


@pytest.mark.parametrize("case", [c for c in E.cases(True) if c[1][-1] == 2051 and c[0] != "pair" and c[0] != "conv_pool"], ids=_id)
def test_update_sized_weight_gradient_sums_stay_below_2_24(case):
    """n = 2051, the largest launch: the bounds of the weight- and bias-gradient sums alone, on float32 operands (the gathered sum or
    the bf16 da they multiply is the only part of the reference that is run)."""
    c = E.FAMILIES[case[0]][0](*case[1])
    tally = E.Tally(c.what)
    c.bounds(tally)
    print(tally.line())
    assert float("-inf") < tally.log2 < 24


def test_bounds_evaluated_in_float32_are_the_float64_bounds():
    g = torch.Generator().manual_seed(9)
    x, (w, b) = E.grid((6, 32, 16, 16), g, E.FINE_STEP, E.X_LIM), E.filters(32, 32, g)
    assert torch.equal(E.conv(x.abs().float(), w.abs().float(), b.abs().float()).double(), E.conv(x.abs(), w.abs(), b.abs()))
    d = E.grid((6, 32, 16, 16), g, E.G_STEP, E.G_LIM)
    for a32, a64 in zip(E.wgrad(x.abs().float(), d.abs().float()), E.wgrad(x.abs(), d.abs())):
        assert torch.equal(a32.double(), a64)


def test_assert_exact_rejects_a_sum_that_does_not_fit():
    E.assert_exact(torch.tensor([2.0 ** 24 - 1]), 1.0, "fits")
    with pytest.raises(AssertionError):
        E.assert_exact(torch.tensor([2.0 ** 24]), 1.0, "does not fit")
    with pytest.raises(AssertionError):          # the pair on filters in multiples of 1/8: one more bit per conv than 24 bits hold
        g = torch.Generator().manual_seed(532)
        W = [E.grid((32, 32, 3, 3), g, 1 / 8, 0.5, 0.5) for _ in range(4)]
        B = [E.grid((32,), g, E.B_STEP, E.B_LIM) for _ in range(4)]
        step, E.W_STEP = E.W_STEP, 1 / 8
        try:
            E.ref_pair(E.grid((6, 32, 16, 16), g, E.X_STEP, E.X_LIM), W, B, E.X_STEP, E.Tally("pair, filters in eighths"))
        finally:
            E.W_STEP = step


def test_exact_levels_come_from_the_table():
    assert list(E.exact_levels(2)) == [0, 191, 255]
    l5, l6 = E.exact_levels(5), E.exact_levels(6)
    assert len(l5) == 17 and list(l5[:3]) == [0, 135, 143] and l5[-1] == 255
    assert len(l6) == 33 and list(l6[:3]) == [0, 131, 135] and set(l5) <= set(l6)
    t = E.bf16_table()
    assert all(float(t[k]) * 32 == round(float(t[k]) * 32) for k in l5) and len(E.exact_levels(8)) > len(l6)


def test_grid_stays_on_its_grid():
    t = E.grid((4000,), torch.Generator().manual_seed(1), 1 / 8, 2.0, 0.5)
    assert t.dtype == torch.float64 and float(t.abs().max()) == 2.0 and torch.equal(t * 8, (t * 8).round())
    assert 0.45 < float((t == 0).double().mean()) < 0.6 and torch.equal(E.r16(t), t)


# ------------------------------------------------------------------ sensitivity: the mutations of a kernel that today's 1e-2 accepts

def _drop_corner_tap_at_last_column(v, xin, w):
    """The conv output v with tap (0, 0) of every filter left out at the last output column."""
    w0 = torch.zeros_like(w)
    w0[:, :, 0, 0] = w[:, :, 0, 0]
    v = v.clone()
    v[..., -1] -= E.conv(xin, w0)[..., -1]
    return v


def test_forward_mutations_are_rejected_by_the_exact_comparison_and_accepted_at_1e_2():
    cin, cout, hw, n = 32, 32, 16, 1
    case = E.case_conv_forward(cin, cout, hw, n)
    ref = torch.from_numpy(E.evaluate(case)[0]["out"]).permute(0, 3, 1, 2).double()
    w, b, _, x, _ = E.conv_inputs(cin, cout, hw, n, 1, E.FINE_STEP, bits=E.FRAME_BITS_FINE)          # the case's own inputs
    res = E.grid((n, cout, hw, hw), torch.Generator().manual_seed(2), E.FINE_STEP, E.X_LIM)
    xin, bb = F.relu(x), b.view(1, -1, 1, 1)
    v = E.conv(xin, w)
    assert torch.equal(E.r16(v + bb + res), ref)
    mutants = {"truncation": E.trunc16(v + bb + res),
               "conv + bias rounded before the residual": E.r16(E.r16(v + bb) + res),
               "bias added after the rounding": E.r16(E.r16(v + res) + bb),
               "a corner tap dropped at one border column": E.r16(_drop_corner_tap_at_last_column(v, xin, w) + bb + res)}
    for k, m in mutants.items():
        diff = float((m != ref).double().mean())
        print(f"forward, {k}: {100 * diff:.2f} % of the outputs differ, max |d| / max |ref| = {relerr(m, ref):.2e}")
        assert not torch.equal(m, ref), k
        if not k.startswith("a corner"):
            assert relerr(m, ref) < 1e-2, k              # why this file exists: today's criterion lets the mutant through


def test_backward_mutations_are_rejected_by_the_exact_comparison_and_accepted_at_1e_2():
    ch, hw, n = 32, 16, 1
    case = E.case_resblock_backward(ch, hw, n)
    out = E.evaluate(case)[0]
    ref_da, ref_dx = (torch.from_numpy(out[k]).permute(0, 3, 1, 2).double() for k in ("da", "dx"))
    g = torch.Generator().manual_seed(200 + ch + hw)                                                # the case's own inputs
    W, _ = E._res_filters(ch, g, 2)
    x, a = E.grid((n, ch, hw, hw), g, E.X_STEP, E.X_LIM), E.grid((n, ch, hw, hw), g, E.X_STEP, E.X_LIM)
    dy = E.grid((n, ch, hw, hw), g, E.RES_STEP, E.X_LIM)

    def chain(rnd, early=False, drop=False):
        da = rnd(E.convT(dy, W[1]) * (a > 0))
        v = E.convT(da, W[0])
        if drop:
            v = _drop_corner_tap_at_last_column(v, da, W[0].transpose(0, 1).flip(2, 3))
        v = v * (x > 0)
        return da, rnd(rnd(v) + dy) if early else rnd(v + dy)
    da, dx = chain(E.r16)
    assert torch.equal(da, ref_da) and torch.equal(dx, ref_dx)
    mutants = {"truncation": chain(E.trunc16), "conv rounded before the skip is added": chain(E.r16, early=True),
               "a corner tap dropped at one border column": chain(E.r16, drop=True)}
    for k, (mda, mdx) in mutants.items():
        print(f"backward, {k}: {100 * float((mdx != ref_dx).double().mean()):.2f} % of dx differ, max |d| / max |ref| = {relerr(mdx, ref_dx):.2e}")
        assert not torch.equal(mdx, ref_dx), k
        if not k.startswith("a corner"):
            assert relerr(mdx, ref_dx) < 1e-2 and relerr(mda, ref_da) < 1e-2, k


def _gather_rounding_each_contribution(dq, idx, shape):
    """A pool backward that keeps its running sum in bf16: the windows of one (row, column) parity never share an element, so four
    collision-free scatters, each rounded, visit every element's contributions one at a time."""
    dc = torch.zeros(shape, dtype=dq.dtype).flatten(2)
    for py in (0, 1):
        for px in (0, 1):
            m = torch.zeros_like(dq)
            m[:, :, py::2, px::2] = 1
            dc = E.r16(dc.scatter_add(2, idx.flatten(2), (dq * m).flatten(2)))
    return dc.reshape(shape)


@pytest.mark.parametrize("hw,c", E.MAXPOOL_SHAPES)
def test_pool_backward_rounding_each_contribution_is_rejected(hw, c):
    case = E.case_maxpool(hw, c)
    ref = case.ref(torch.float64, E.Tally(case.what))["dx"]
    mut = case.ref(torch.float64, E.Tally(case.what), mutant=_gather_rounding_each_contribution)["dx"]
    trunc = case.ref(torch.float64, E.Tally(case.what), rnd=E.trunc16)["dx"]
    print(f"pool backward {c}@{hw}: {int((mut != ref).sum())} elements differ when each contribution is rounded, {int((trunc != ref).sum())} when the sum is truncated")
    assert not torch.equal(mut, ref) and not torch.equal(trunc, ref)
    assert torch.equal(mut != 0, ref != 0)                  # (the same routes: only the rounding differs)


@pytest.mark.parametrize("cin,cout,hw", E.POOL_SHAPES)
def test_weight_gradient_from_a_pooled_gradient_sees_the_gather_rounding_point(cin, cout, hw):
    """Modes 4 and 6 at n = 1: dW moves when the gathered sum is truncated, rounded per contribution, left unrounded where block2 / block3
    round it, or rounded where block1's one-hot form does not."""
    case = E.case_conv_pool_wgrad(cin, cout, hw, 1)
    ref = case.ref(torch.float64, E.Tally(case.what))["dW"]
    plain = lambda dq, idx, shape: E.pool_scatter(dq, idx, shape)
    mutants = {"the sum truncated": lambda *a: E.trunc16(plain(*a)), "each contribution rounded": _gather_rounding_each_contribution,
               "the sum rounded" if cin == 3 else "the sum left unrounded": (lambda *a: E.r16(plain(*a))) if cin == 3 else plain}
    for k, m in mutants.items():
        mut = case.ref(torch.float64, E.Tally(case.what), mutant=m)["dW"]
        print(f"dW from the pooled gradient ({cin},{cout},{hw}), {k}: {int((mut != ref).sum())} of {ref.numel()} elements differ")
        assert not torch.equal(mut, ref), k
