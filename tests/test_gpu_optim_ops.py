"""The last links of every gradient's way to a parameter, one launch sequence at a time on caller data: the fixed-order slab and column
sums (csrc/reduce.hip) through mi_op_reduce, the gradient norm and Adam (csrc/optim.hip, sae_adam_kernel of csrc/sae.hip) through
mi_op_adam, the advantage statistics, their cross-rank merge (mi_op_adv_merge) and the GAE scan (csrc/estimates.hip).  Inputs, the
float64 / integer references and every bound's derivation are in tests/optim_inputs.py; tests/test_optim_host.py checks those on the CPU.

Every hook call goes through the production launchers into poisoned outputs followed by canary bands: a write past the end of a target
(the elements past n_w + n_b, an Adam element past n) fails the call itself."""
import numpy as np
import pytest
import torch

import optim_inputs as OI

pytestmark = pytest.mark.gpu


def _small_engine(T=2, E=2):
    from mi355.engine import Engine
    return Engine("mlp", T, E, 2, max(E, 8), obs_dim=4, mlp_depth=2, mlp_width=8, out_dim=8)


@pytest.fixture(scope="module")
def hook_engine():
    eng = _small_engine()          # the hooks are independent of the context's sizes
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------------ reductions
def _check_pair(check, got, refs, what):
    worst = 0.0
    for g, r, name in zip(got, refs, ("dst_w", "dst_b")):
        assert (g is None) == (r is None)
        if r is not None:
            worst = max(worst, check(g, r, f"{what} {name}") or 0.0)
    return worst


@pytest.mark.parametrize("nslab,slab_len,n_w,n_b", OI.SLAB_CASES)
def test_reduce_slabs_exact(hook_engine, nslab, slab_len, n_w, n_b):
    """reduce_slabs_kernel on integers: the result is the int64 sum whatever the order; the starting values are not zero"""
    part, w0, b0 = OI.slab_case(nslab, slab_len, n_w, n_b, True)
    got = hook_engine.op_reduce_slabs(part, w0, b0)
    _check_pair(OI.check_exact, got, OI.slab_reference(part, w0, b0), f"reduce_slabs {nslab}x{slab_len}")


@pytest.mark.parametrize("nslab,slab_len,n_w,n_b", OI.SLAB_CASES)
def test_reduce_slabs_rounding_and_determinism(hook_engine, nslab, slab_len, n_w, n_b):
    """reduce_slabs_kernel on |x| in [0.5, 2] against the float64 sum, bound with d = ceil(nslab / 32) + 32; twice the same bits"""
    part, w0, b0 = OI.slab_case(nslab, slab_len, n_w, n_b, False)
    got = hook_engine.op_reduce_slabs(part, w0, b0)
    worst = _check_pair(OI.check_rounding, got, OI.slab_reference(part, w0, b0), f"reduce_slabs {nslab}x{slab_len}")
    print(f"reduce_slabs nslab={nslab} slab_len={slab_len}: worst err/bound {worst:.3f}")
    again = hook_engine.op_reduce_slabs(part, w0, b0)
    assert got[0].tobytes() == again[0].tobytes() and (got[1] is None or got[1].tobytes() == again[1].tobytes())


@pytest.mark.parametrize("case", OI.ALL_SLAB_CASES)
@pytest.mark.parametrize("exact", (True, False), ids=("exact", "rounding"))
def test_reduce_all_slabs(hook_engine, case, exact):
    """reduce_all_slabs_kernel, ten layers in one launch: the four conv slab lengths, slab counts on the boundaries of the 4-in-flight
    loop, workgroups past a short layer's end, weights and biases scattered over one flat vector whose gaps must keep their values
    (the reference holds the starting values there, with a bound of 3 * 2^-24 |value| that only the unchanged value meets)."""
    ws, desc, g0, layers = OI.all_slabs_case(case, exact)
    got = hook_engine.op_reduce_all_slabs(ws, desc, g0)
    r = OI.all_slabs_reference(ws, layers, g0)
    if exact:
        OI.check_exact(got, r, f"reduce_all_slabs case {case}")
    else:
        worst = OI.check_rounding(got, r, f"reduce_all_slabs case {case}")
        print(f"reduce_all_slabs case {case}: worst err/bound {worst:.3f}")
        assert got.tobytes() == hook_engine.op_reduce_all_slabs(ws, desc, g0).tobytes()
    owned = np.zeros(g0.size, bool)
    for so, wo, bo, ns, sl, nw in layers:
        owned[wo:wo + nw] = True; owned[bo:bo + sl - nw] = True
    assert np.array_equal(got[~owned], g0[~owned])


@pytest.mark.parametrize("M,N,ld", OI.COLSUM_CASES)
def test_colsum_exact(hook_engine, M, N, ld):
    """colsum_partial_kernel + reduce_slabs_kernel through launch_colsum_acc on integers, the workspace exactly 64 x 4096 floats"""
    dY, db0 = OI.colsum_case(M, N, ld, True)
    OI.check_exact(hook_engine.op_colsum(dY, N, db0), OI.colsum_reference(dY, db0), f"colsum {M}x{N} ld {ld}")


@pytest.mark.parametrize("M,N,ld", OI.COLSUM_CASES)
def test_colsum_rounding_and_determinism(hook_engine, M, N, ld):
    """launch_colsum_acc against the float64 sum, d = ceil(M / groups) + ceil(groups / 32) + 32 with groups = 256 for M >= 4096 and
    N <= 1024, else 64; twice the same bits"""
    dY, db0 = OI.colsum_case(M, N, ld, False)
    got = hook_engine.op_colsum(dY, N, db0)
    worst = OI.check_rounding(got, OI.colsum_reference(dY, db0), f"colsum {M}x{N} ld {ld}")
    print(f"colsum M={M} N={N} ld={ld}: worst err/bound {worst:.3f}")
    assert got.tobytes() == hook_engine.op_colsum(dY, N, db0).tobytes()


def test_widths_above_4096_are_refused(hook_engine):
    """The column sum's workspace holds 64 x 4096 partial sums: the launcher refuses a wider N before it launches anything, and mi_create
    refuses an MLP whose bias gradients would need one.  A refusal test only: the overflowing launch never runs."""
    from mi355.engine import Engine, EngineError
    dY, db0 = np.ones((1, 4097), np.float32), np.zeros(4097, np.float32)
    with pytest.raises(EngineError, match="at most 4096"):
        hook_engine.op_colsum(dY, 4097, db0)
    OI.check_exact(hook_engine.op_colsum(dY[:, :4096], 4096, db0[:4096]), OI.colsum_reference(dY[:, :4096], db0[:4096]))      # the context still works
    with pytest.raises(EngineError, match="at most 4096"):
        Engine("mlp", 2, 2, 2, 8, obs_dim=4, mlp_depth=2, mlp_width=4097, out_dim=8)
    with pytest.raises(EngineError, match="at most 4096"):
        Engine("mlp", 2, 2, 2, 8, obs_dim=4, mlp_depth=2, mlp_width=8, out_dim=4097)


# ------------------------------------------------------------------------------------------------ gradient norm
def _norm(eng, g, variant1=False):
    """the norm mi_op_adam reports for gradient g (max_norm = 1e9: nothing clips); Variant 1 takes g as two vectors"""
    z = np.zeros_like(g)
    if not variant1:
        out = eng.op_adam(0, z, g, z, z, OI.LR, 1e9, 1)
        assert not out[1].any()
        return out[4]
    n1, off = OI.split_in_two(g.size)
    out = eng.op_adam(1, z[:n1], g[:n1], z[:n1], z[:n1], OI.LR, 1e9, 1, second=(z[n1:], g[n1:], z[n1:], z[n1:]), offsets=off)
    return out[4]


@pytest.mark.parametrize("n", OI.NORM_N)
def test_gradient_norm(hook_engine, n):
    """sumsq_partial_kernel's 128 chunks (of 1, 2, 257, 1024, 1025 ... elements, ragged unrolled tails, empty workgroups) + the sum in
    adam_kernel: exactly float32(sqrt(sum g^2)) on integers, within one float32 ulp of it on real gradients; the same from Variant 1's
    256 partial sums over the vector split in two (n >= 5: its second vector has four non-empty pieces); twice the same bits."""
    g = OI.norm_case(n, True)
    want = OI.norm_reference(g)
    got = _norm(hook_engine, g)
    assert got == want, (got, want)
    if n >= 5:
        assert _norm(hook_engine, g, variant1=True) == want
    g = OI.norm_case(n, False)
    want = OI.norm_reference(g)
    got = _norm(hook_engine, g)
    print(f"norm n={n}: {got!r} vs {want!r}")
    assert abs(np.float64(got) - np.float64(want)) <= np.spacing(want), (got, want)
    assert _norm(hook_engine, g).tobytes() == got.tobytes()
    if n >= 5:
        assert _norm(hook_engine, g, variant1=True) == got


# ------------------------------------------------------------------------------------------------ Adam
_BOUNDS = {}


def _torch_errors(name):
    """torch's own fp32 error on this case's inputs (n < 256: on the n = 4097 inputs of the same distribution), computed once"""
    if name not in _BOUNDS:
        variant, n, step, grad, max_norm, p_zero = OI.ADAM_CASES[name]
        _BOUNDS[name] = OI.torch_fp32_errors(OI.adam_bound_inputs(name), step, max_norm)
    return _BOUNDS[name]


@pytest.mark.parametrize("name", list(OI.ADAM_CASES))
def test_adam(hook_engine, name):
    """sumsq_partial_kernel + adam_kernel / sae_adam_kernel with the host scalars of mi_optimizer_step against float64 clip_grad_norm_ +
    Adam(eps=1e-5) (Variants 0 and 1: with the constants adam_kernel documents; Variant 2: torch's own).  Per quantity m', v', p' over
    the whole vector: error <= 8 x the error of torch's fp32 Adam against torch's float64 Adam.  g comes back zero, the norm is the
    unclipped one, and Variant 1's four pieces give the bits of one launch over the whole second vector."""
    variant, (p, g, m, v), step, max_norm = OI.adam_case(name)
    n = p.size
    consts = OI.TORCH if variant == 2 else OI.KERNEL
    rp, rm, rv, rnorm, coef = OI.adam_reference(p, g, m, v, OI.LR, max_norm, step, consts)
    assert (coef < 1) == OI.clips(name)
    if variant == 1:
        n1, off = OI.split_in_two(n)
        first, second = [a[:n1] for a in (p, g, m, v)], [a[n1:] for a in (p, g, m, v)]
        out = hook_engine.op_adam(1, *first, OI.LR, max_norm, step, second=second, offsets=off)
        gp, gg, gm, gv = (np.concatenate([out[k], out[5][k]]) for k in range(4))
        # the second vector in one launch (as the first of a Variant 1 call) gives the same bits as in four pieces
        whole = hook_engine.op_adam(1, *second, OI.LR, max_norm, step, second=first, offsets=np.array([0, 1, 2, 3, n1], dtype=np.int64))
        assert whole[4].tobytes() == out[4].tobytes(), "the two orders of the 256 partial sums round to different norms"
        for k in range(4):
            assert whole[k].tobytes() == out[5][k].tobytes(), ("p", "g", "m", "v")[k]
            assert whole[5][k].tobytes() == out[k].tobytes(), ("p", "g", "m", "v")[k]
    else:
        gp, gg, gm, gv, _ = out = hook_engine.op_adam(variant, p, g, m, v, OI.LR, max_norm, step)
    norm = out[4]
    assert not gg.any(), "the gradient must come back zeroed"
    assert abs(np.float64(norm) - rnorm) <= np.spacing(np.float32(rnorm)), (norm, rnorm)          # the unclipped norm
    assert np.isfinite(gp).all() and np.isfinite(gm).all() and np.isfinite(gv).all()
    bad = []
    for label, got, ref, terr in zip(("m'", "v'", "p'"), (gm, gv, gp), (rm, rv, rp), _torch_errors(name)):
        err = OI.rel_l2(got, ref)
        print(f"adam {name} {label}: kernel {err:.3e}  torch fp32 {terr:.3e}  bound {8 * terr:.3e}")
        if not err <= 8 * terr:
            bad.append((label, err, terr))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ advantage statistics
@pytest.fixture(scope="module", params=OI.ADV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def adv_engine(request):
    T, E = request.param
    eng = _small_engine(T, E)
    yield eng
    eng.close()


@pytest.mark.parametrize("dist", OI.ADV_DISTS)
def test_adv_stats_and_apply(adv_engine, dist):
    """advnorm_stats_kernel against math.fsum in float64, advnorm_apply_kernel against the float64 formula with the bound from its three
    float32 roundings"""
    from mi355 import engine as M
    eng = adv_engine
    x = OI.adv_case(eng.T, eng.E, dist)
    eng.write_field(M.F_ADV, x)
    got = eng.adv_stats()
    r_mean, r_m2 = OI.check_adv_stats(got, x, f"adv_stats {x.size} {dist}")
    assert got.tobytes() == eng.adv_stats().tobytes()
    ref = OI.adv_stats_reference(x)
    eng.adv_apply(ref)
    out, b = OI.adv_apply_reference(x, ref)
    err = np.abs(eng.read_field(M.F_ADV).astype(np.float64) - out)
    print(f"adv n={x.size} {dist}: mean err/bound {r_mean:.3f}  M2 err/bound {r_m2:.3f}  apply worst err/bound {(err / b).max():.3f}  largest bound {b.max():.2e}")
    assert (err <= b).all(), (err.max(), b[np.argmax(err - b)])
    if dist == "normal":
        assert b.max() < 2e-6


@pytest.mark.parametrize("dist", OI.ADV_DISTS)
@pytest.mark.parametrize("R", OI.MERGE_R)
@pytest.mark.parametrize("shape", ((1, 1025), (66, 130)), ids=("1025", "8580"))
def test_adv_merge(hook_engine, shape, R, dist):
    """advnorm_merge_kernel on R ranks' triples (unequal counts, ranks with nothing): mi355.dist.merge_adv_stats to 1e-15, and the
    statistics of the concatenated data within the bound of the direct statistics (n * 2^-53 * sum|x - mean|^2 + one ulp for M2).

    [1025-8-offset] (1025 values of mean 1000, sd 0.01 on six ranks of 28 .. 313 values and two empty ones) is the case that found the
    pairwise recurrence too coarse: it gave M2 2.27e-14 off, the bound is 1.12e-14, while the exact rational merge of the same eight
    float64 triples is 3.1e-15 off.  The kernel and the host function now merge in two passes around a pivot (csrc/estimates.hip)."""
    from mi355.dist import merge_adv_stats
    x = OI.adv_case(*shape, dist)
    triples = [OI.adv_stats_reference(p) for p in OI.merge_parts(x, R)]
    got = hook_engine.op_adv_merge(triples)
    host = merge_adv_stats(triples)
    ref, (b_mean, b_m2) = OI.adv_stats_reference(x), OI.adv_stats_bounds(x)
    print(f"merge n={x.size} R={R} {dist}: mean err {abs(got[1] - ref[1]):.3e} bound {b_mean:.3e}  M2 err {abs(got[2] - ref[2]):.3e} bound {b_m2:.3e}"
          f"  against the host merge: {np.abs(got[1:] / host[1:] - 1).max():.1e}")
    assert got[0] == host[0] and np.all(np.abs(got[1:] - host[1:]) <= 1e-15 * np.abs(host[1:])), (got, host)
    OI.check_adv_stats(got, x, f"merge R={R} {dist}")


# ------------------------------------------------------------------------------------------------ GAE
@pytest.mark.parametrize("T,E", OI.GAE_SHAPES)
def test_gae_bit_exact(T, E):
    """gae_kernel against the oracle bit for bit: one env, a partial wave (63), a partial wave in the second and third workgroup (65,
    130); four (gamma, lambda); dones at t = 0 and t = T - 1, an always-done and a never-done column; with and without GAE"""
    from mi355 import engine as M
    from oracle import ppo_oracle as O
    eng = _small_engine(T, E)
    try:
        for k in range(2 if E == 1 else 1):
            rew, done, val = OI.gae_case(T, E, k)
            if E > 3:
                assert done[:, 0].all() and not done[:, 1].any() and done[0, 2] == 1 and done[T - 1, 3] == 1
            eng.write_field(M.F_REW, rew); eng.write_field(M.F_DONE, done); eng.write_field(M.F_VALUE, val)
            for gamma, lmbda in OI.GAE_PARAMS:
                for use_gae in (True, False):
                    eng.compute_estimates(gamma, lmbda, use_gae, False)
                    adv, ret = O.compute_estimates(torch.from_numpy(rew), torch.from_numpy(done), torch.from_numpy(val), gamma, lmbda, use_gae, False)
                    assert np.array_equal(eng.read_field(M.F_ADV), adv.numpy()), (gamma, lmbda, use_gae, k)
                    assert np.array_equal(eng.read_field(M.F_RET), ret.numpy()), (gamma, lmbda, use_gae, k)
                    assert use_gae or not eng.read_field(M.F_ADV).any()
    finally:
        eng.close()
