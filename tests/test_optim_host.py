"""CPU checks of tests/optim_inputs.py, the references and checkers behind tests/test_gpu_optim_ops.py: the float64 Adam reference against
torch's own float64 Adam, the size of the documented constant deviation of adam_kernel, the clip cases, the headroom of the exact
reduction inputs, the claim that one missing term exceeds every rounding bound -- and that each reduction checker rejects a result
computed with one defect."""
import numpy as np
import pytest
import torch

import optim_inputs as OI


# ------------------------------------------------------------------------------------------------ Adam reference
@pytest.mark.parametrize("name", list(OI.ADAM_CASES))
def test_reference_with_torch_constants_is_torch_float64_adam(name):
    """The injected state (step, exp_avg, exp_avg_sq) and the clip reproduce in plain numpy what torch computes"""
    variant, inputs, step, max_norm = OI.adam_case(name)
    (r,), norm = OI.torch_adam([inputs], OI.LR, max_norm, step, torch.float64)
    p, m, v, ref_norm, _ = OI.adam_reference(*inputs, OI.LR, max_norm, step, OI.TORCH)
    assert abs(norm - ref_norm) <= (inputs[0].size + 2) * 2.0 ** -53 * ref_norm          # (torch adds the n squares in float64, the reference without error)
    for got, want in ((r[0], p), (r[1], m), (r[2], v)):
        assert OI.rel_l2(got, want) <= 1e-14


def test_two_parameter_clip_is_one_norm():
    """Variant 1's reference: two tensors in one optimizer are clipped with the norm of both, as one concatenated vector is"""
    a, b = OI.adam_inputs(300, 2, "big", False, seed=1), OI.adam_inputs(77, 2, "big", False, seed=2)
    (ra, rb), norm = OI.torch_adam([a, b], OI.LR, 0.5, 2, torch.float64)
    p, m, v, ref_norm, coef = OI.adam_reference(*[np.concatenate(q) for q in zip(a, b)], OI.LR, 0.5, 2, OI.TORCH)
    assert coef < 1 and abs(norm - ref_norm) <= 1e-14 * ref_norm
    assert OI.rel_l2(np.concatenate([ra[0], rb[0]]), p) <= 1e-14 and OI.rel_l2(np.concatenate([ra[2], rb[2]]), v) <= 1e-14


def test_documented_constant_deviation():
    """adam_kernel's fp32 1 - beta2 = 0.000999987 against torch's 0.001 (csrc/sae.hip, above sae_adam_kernel): at step 1 exp_avg_sq
    differs by at most 1.4e-5 relative and the step by 7e-6 (measured 1.29e-5 and 6.7e-6) -- and by no less than 1e-5 / 5e-6, so a
    test with the wrong constants cannot hide inside the Adam bounds of the GPU tests."""
    inputs = OI.adam_inputs(4097, 1, "big", True)
    pk, mk, vk, _, _ = OI.adam_reference(*inputs, OI.LR, 0.5, 1, OI.KERNEL)
    pt, mt, vt, _, _ = OI.adam_reference(*inputs, OI.LR, 0.5, 1, OI.TORCH)
    dv, dp = np.abs(vk / vt - 1).max(), np.abs(pk / pt - 1).max()
    print(f"v' deviation {dv:.3e}  step deviation {dp:.3e}")
    assert 1e-5 < dv <= 1.4e-5 and 5e-6 < dp <= 7e-6
    assert OI.KERNEL.w1 == float(np.float32(1) - np.float32(0.9)) and OI.KERNEL.w2 == float(np.float32(1) - np.float32(0.999))
    assert OI.KERNEL.w2 != float(np.float32(0.001))


@pytest.mark.parametrize("name", list(OI.ADAM_CASES))
def test_clip_cases_clip_as_named(name):
    variant, n, step, grad, max_norm, p_zero = OI.ADAM_CASES[name]
    _, inputs, _, _ = OI.adam_case(name)
    p, g, m, v = inputs
    _, _, _, norm, coef = OI.adam_reference(*inputs, OI.LR, max_norm, step, OI.KERNEL)
    assert ("big" in name) == (grad == "big") and ("small" in name) == (grad == "small") and ("zero" in name) == (grad == "zero")
    assert ("-p0" in name) == p_zero == (not p.any())
    if OI.clips(name):
        assert norm > 3 * max_norm and coef < 1 / 3
    else:
        assert coef == 1.0 and (grad != "small" or norm < max_norm / 100) and (grad != "zero" or norm == 0.0)
    assert (step == 1) == (not m.any() and not v.any())
    assert (v >= 0).all() and (step == 1 or (v > 0).all())
    if grad == "zero":
        assert step > 1 and m.any()          # only the momentum moves the parameters


def test_adam_cases_cover_the_issue():
    cases = list(OI.ADAM_CASES.values())
    assert {c[1] for c in cases} == {1, 255, 256, 257, 4097, 131200} and {c[2] for c in cases} == {1, 2, 1000, 30000}
    assert {c[0] for c in cases} == {0, 1, 2} and {c[3] for c in cases} == {"big", "small", "zero"} and any(c[4] == 1e9 for c in cases)
    assert sum(c[5] for c in cases) >= 2 and len(cases) <= 16


# ------------------------------------------------------------------------------------------------ reductions: inputs
def test_exact_inputs_keep_every_partial_sum_below_2_to_24():
    """|x| <= 8 and at most 1024 slabs / 5889 rows plus the starting value: analytically 8 * 5890 < 2^24; measured on the largest inputs"""
    assert 8 * (max(OI.SLAB_NSLAB) + 1) < 2 ** 24 and 8 * (max(OI.ALL_NSLAB) + 1) < 2 ** 24 and 8 * (max(c[0] for c in OI.COLSUM_CASES) + 1) < 2 ** 24
    for ns, sl, nw, nb in ((1024, 448, 432, 16), (512, 33, 20, 13)):
        part, w0, b0 = OI.slab_case(ns, sl, nw, nb, True)
        assert np.abs(part).max() <= 8 and np.array_equal(part, np.rint(part))
        w, b = OI.slab_reference(part, w0, b0)
        assert max(OI.exact_headroom(w), OI.exact_headroom(b)) < 2 ** 24
    ws, desc, g0, layers = OI.all_slabs_case(0, True)
    assert OI.exact_headroom(OI.all_slabs_reference(ws, layers, g0)) < 2 ** 24
    dY, db0 = OI.colsum_case(4096 + 1793, 256, 256, True)
    assert OI.exact_headroom(OI.colsum_reference(dY, db0)) < 2 ** 24


def test_one_missing_term_exceeds_every_rounding_bound():
    """|x| >= 0.5, so a missing term moves a sum by at least 0.5: above the bound's largest possible value at every listed shape"""
    for ns in OI.SLAB_NSLAB + OI.ALL_NSLAB:
        assert 0.5 > OI.worst_bound(OI.slab_depth(ns), ns), ns
    for M, N, ld in OI.COLSUM_CASES:
        assert 0.5 > OI.worst_bound(OI.colsum_depth(M, N), M), (M, N)
    assert OI.slab_depth(1) == 33 and OI.slab_depth(33) == 34 and OI.slab_depth(1024) == 64
    assert OI.colsum_groups(4095, 1024) == 64 and OI.colsum_groups(4096, 1024) == 256 and OI.colsum_groups(4097, 1025) == 64
    assert OI.colsum_depth(5889, 256) == 24 + 8 + 32 and OI.colsum_depth(300, 4096) == 5 + 2 + 32
    # and on real inputs: the bound per element stays below the analytic maximum, the inputs at or above 0.5
    part, w0, b0 = OI.slab_case(1024, 100, 60, 30, False)
    w, b = OI.slab_reference(part, w0, b0)
    assert np.abs(part).min() >= 0.5 and np.abs(w0).min() >= 0.5
    assert OI.bound(w.depth, w.sum_abs, w.want).max() <= OI.worst_bound(64, 1024) < 0.5


def test_cases_are_the_listed_ones():
    assert len(OI.SLAB_CASES) == 48 and (33, 100, 60, 30) in OI.SLAB_CASES and (1024, 4112, 4096, 16) in OI.SLAB_CASES
    for case in OI.ALL_SLAB_CASES:
        ws, desc, g0, layers = OI.all_slabs_case(case, True)
        assert {l[4] for l in layers} == {448, 2320, 4640, 9248} and {l[3] for l in layers} == set(OI.ALL_NSLAB)
        assert not (desc[:, [0, 1, 2, 4, 5]] % 4).any()
        # the regions do not overlap and leave gaps: every gradient element belongs to at most one layer
        owner = np.zeros(g0.size, np.int32)
        for so, wo, bo, ns, sl, nw in layers:
            owner[wo:wo + nw] += 1; owner[bo:bo + sl - nw] += 1
            assert np.isfinite(ws[so:so + ns * sl]).all() and np.isnan(ws[so - 1]) and (so + ns * sl == ws.size or np.isnan(ws[so + ns * sl]))
        assert owner.max() == 1 and (owner == 0).sum() >= 4 * 20
    assert {(a, b) for case in OI.ALL_SLAB_CASES for a, b in [(l[4], l[3]) for l in OI.all_slabs_case(case, True)[3]]} >= {(9248, 1), (9248, 224), (2320, 1024), (4640, 1024)}


# ------------------------------------------------------------------------------------------------ reductions: the checkers have teeth
def _f32(r):
    return r.want.astype(np.float32)


@pytest.mark.parametrize("exact", (True, False))
def test_slab_checker_rejects_each_defect(exact):
    check = OI.check_exact if exact else OI.check_rounding
    for ns, sl, nw, nb in ((33, 33, 20, 13), (1024, 100, 60, 30), (2, 448, 432, 16)):
        part, w0, b0 = OI.slab_case(ns, sl, nw, nb, exact)
        w, b = OI.slab_reference(part, w0, b0)
        check(_f32(w), w); check(_f32(b), b)          # the float64 sum rounded once passes
        for defect in (dict(drop_slab=ns // 2), dict(drop_tail=True), dict(shift_boundary=True)):
            ww, wb = OI.slab_reference(part, w0, b0, **defect)
            with pytest.raises(AssertionError):
                check(_f32(ww), w); check(_f32(wb), b)
    # one slab dropped shows in EVERY element of a rounding case, and in most of an exact one
    part, w0, b0 = OI.slab_case(65, 448, 432, 16, exact)
    w, _ = OI.slab_reference(part, w0, b0)
    ww, _ = OI.slab_reference(part, w0, b0, drop_slab=64)
    wrong = np.abs(_f32(ww) - w.want) > (0 if exact else OI.bound(w.depth, w.sum_abs, w.want))
    assert wrong.all() if not exact else wrong.mean() > 0.9


@pytest.mark.parametrize("exact", (True, False))
def test_all_slabs_checker_rejects_each_defect(exact):
    check = OI.check_exact if exact else OI.check_rounding
    ws, desc, g0, layers = OI.all_slabs_case(3, exact)
    r = OI.all_slabs_reference(ws, layers, g0)
    check(_f32(r), r)
    for defect in (dict(drop_slab=(3, 128)), dict(drop_slab=(7, 0)), dict(write_past=True)):
        with pytest.raises(AssertionError):
            check(_f32(OI.all_slabs_reference(ws, layers, g0, **defect)), r)
    moved = _f32(r)
    moved[layers[2][1] - 1] += 1.0          # a gap element in front of a weight region
    with pytest.raises(AssertionError):
        check(moved, r)


@pytest.mark.parametrize("exact", (True, False))
def test_colsum_checker_rejects_a_dropped_row(exact):
    check = OI.check_exact if exact else OI.check_rounding
    for M, N, ld in ((65, 16, 17), (513, 65, 65), (4097, 1025, 1025)):
        dY, db0 = OI.colsum_case(M, N, ld, exact)
        r = OI.colsum_reference(dY, db0)
        check(_f32(r), r)
        for row in (0, M - 1):
            with pytest.raises(AssertionError):
                check(_f32(OI.colsum_reference(dY, db0, drop_row=row)), r)
        if ld > N:          # the column past N summed into the last one
            wrong = _f32(r); wrong[N - 1] += dY[:, N].sum()
            if dY[:, N].sum() != 0:
                with pytest.raises(AssertionError):
                    check(wrong, r)


# ------------------------------------------------------------------------------------------------ norm, advantage statistics
def test_norm_reference_and_split():
    for n in OI.NORM_N:
        if n >= 5:
            n1, off = OI.split_in_two(n)
            assert 1 <= n1 < n and off[0] == 0 and off[4] == n - n1 and (np.diff(off) > 0).all()
    g = OI.norm_case(32773, True)
    assert OI.norm_reference(g) == np.float32(np.sqrt(np.float64((g.astype(np.int64) ** 2).sum())))
    chunks = {n: -(-n // 128) for n in OI.NORM_N}
    assert chunks[1] == 1 and chunks[129] == 2 and chunks[32773] == 257 and chunks[131072] == 1024 and chunks[131200] == 1025
    assert 129 - 64 * 2 == 1          # n = 129: 64 whole chunks of 2, one element in workgroup 64, workgroups 65 .. 127 empty


def test_adv_references():
    from mi355.dist import merge_adv_stats
    for dist in OI.ADV_DISTS:
        x = OI.adv_case(66, 130, dist)
        s = OI.adv_stats_reference(x)
        x64 = x.astype(np.float64)
        assert s[0] == x.size and abs(s[1] - x64.mean()) < 1e-9 and abs(s[2] - x64.var() * x.size) < 1e-9 * s[2]
        OI.check_adv_stats(s, x)
        with pytest.raises(AssertionError):          # one value left out
            OI.check_adv_stats(OI.adv_stats_reference(x.ravel()[:-1]) + np.array([1.0, 0, 0]), x)
        for R in OI.MERGE_R:
            parts = OI.merge_parts(x, R)
            counts = [p.size for p in parts]
            assert len(parts) == R and sum(counts) == x.size and np.array_equal(np.concatenate(parts), x.ravel())
            zeros = {1: 0, 2: 0, 3: 1, 8: 2}[R]
            assert counts.count(0) == zeros and len(set(c for c in counts if c)) == R - zeros >= min(R, 2)          # unequal counts, two or more ranks with data
            merged = merge_adv_stats([OI.adv_stats_reference(p) for p in parts])
            OI.check_adv_stats(merged, x)
        out, b = OI.adv_apply_reference(x, s)
        assert abs(out.mean()) < 1e-6 and abs(out.std(ddof=1) - 1) < 2e-6          # (sd + 1e-8 with sd = 0.01)
        if dist == "normal":
            assert b.max() < 2e-6          # below the suite's existing tolerance for the normalised advantages


def test_mlp_wider_than_the_column_sum_workspace_is_refused_at_creation():
    """mi_create checks the widths before it looks for a device: an MLP whose bias gradients would overflow the column-sum workspace
    (launch_colsum_acc, 64 x 4096 partial sums) cannot be created"""
    from mi355.engine import Engine, EngineError
    for kw in (dict(mlp_width=4097, out_dim=8), dict(mlp_width=8, out_dim=4097)):
        with pytest.raises(EngineError, match="at most 4096"):
            Engine("mlp", 2, 2, 2, 8, obs_dim=4, mlp_depth=2, **kw)
