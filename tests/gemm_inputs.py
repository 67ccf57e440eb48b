"""Cases, float64 reference and per-element checker of the generic GEMM (csrc/gemm.hip: gemm_kernel, gemm_splitk_reduce, launch_gemm) at
op level, through mi_op_linear / Engine.op_linear.  Host only: numpy (and torch's float32 CPU product for the measured figure).

The operation.  With A(m, k) and B(k, n) read through strides (bf16 or fp32 in memory, ReLU on load), fp32 MFMA accumulation:
    v = sum_k A(m, k) B(k, n);  v += bias[n];  v = max(v, 0) (relu_out);  v = mask[m][n] > 0 ? v : 0;  C = bf16(v)  or  C (+)= v
The epilogue is written twice, at the end of gemm_kernel (one launch) and in gemm_splitk_reduce (split K): every case has ONE reference,
so the two copies are compared with each other through it.

Forms (Engine.op_linear): 0 linear_fwd (M, N, K) = (n, out, in); 1 linear_dgrad (n, in, out); 2 linear_wgrad (out, in, n), which also
returns gb += colsum(dY); 3 launch_gemm itself with explicit strides, ldc, workspace on / off and a workspace-size override.

The plan.  rule() restates launch_gemm's documented split rule; every case carries the (split, k_chunk) it is MEANT to run, the host test
checks it against rule(), the GPU test against what the hook reports.  A case that quietly stops splitting fails.

Two layers per case.
  exact  Operands, bias and C0 are integers in [-8, 8] ({-1, 0, 1}, a quarter non-zero, where the output is bf16), so every product and
         every partial sum is exact in the output type as long as  S = sum_k |a b| + |bias| + |C0| < 2^24  (2^8 for a bf16 output; the
         host test asserts it per case).  In any summation order the result must EQUAL the float64 reference: np.array_equal, no tolerance.
         A dropped, doubled or misplaced term cannot hide.
  real   Standard-normal values; bf16-typed operands hold bf16-representable values; mask entries and ReLU'd operands are at least 2^-9 from
         zero.  Per element |got - ref| <= (K + split + 4) 2^-24 S  (+ 2^-8 |ref| for a bf16 output): a once-rounded fma chain of K terms
         errs by at most K u S, the split - 1 slab adds, the bias and the accumulate are one rounding each of at most u S (u = 2^-24).
         ReLU is 1-Lipschitz and the mask either keeps or zeroes, so neither needs an exclusion: no element is left out.  Masked elements
         must be exactly 0 (or exactly C0).  Also measured: relative L2 against float64 <= 8 x torch's own float32 CPU error on the same
         inputs (policy_inputs.check_measured); below 256 output elements torch's error is taken on a 64 x 64 case of the same K, options
         and distribution.
"""
import functools

import numpy as np

U = 2.0 ** -24
AWAY = 2.0 ** -9
WS_FLOATS = 8 << 20          # the context's split workspace (mi_create)
LAYERS = ("exact", "real")


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even) as float32: the rounding of host_to_bf16 and of the kernels' store."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def rule(M, N, K, use_ws=True, ws_floats=WS_FLOATS):
    """launch_gemm's plan as documented in csrc/gemm.hip -> (split, k_chunk)."""
    tiles = -(-M // 64) * -(-N // 64)
    split = 1
    if K >= 512 and tiles < 192 and use_ws:
        split = max(1, min(512 // tiles, K // 128))
        while split > 1 and split * M * N > ws_floats:
            split -= 1
    k_chunk = -(-(-(-K // split)) // 32) * 32
    if split > 1:
        split = -(-K // k_chunk)
    return split, k_chunk


# ------------------------------------------------------------------------------------------------ cases
def _c(form, d, plan, **o):
    """d = (n, in, out) for forms 0 .. 2, (M, N, K) for form 3; o: relu_x, relu_out, x_bf16, bias, mask, acc, a_kc, b_kc, ldc, use_ws, ws_floats"""
    c = dict(form=form, d=tuple(d), plan=tuple(plan), relu_x=False, relu_out=False, x_bf16=False, bias=False, mask=False, acc=form == 2,
             a_kc=True, b_kc=True, ldc=None, use_ws=True, ws_floats=-1)
    assert set(o) <= set(c), o
    c.update(o)
    return c


CASES = {
    # ---- linear_fwd: (n, in, out).  The 9- and 5-wide observation layers as K, the heads' A + 1 as N
    "fwd_obs9": _c(0, (65, 9, 64), (1, 32), bias=True, relu_out=True),
    "fwd_obs5": _c(0, (1, 5, 63), (1, 32), bias=True),
    "fwd_heads": _c(0, (129, 64, 3), (1, 64), bias=True),
    "fwd_relu_x": _c(0, (16, 300, 65), (1, 320), bias=True, relu_x=True, relu_out=True),
    "fwd_bf16_relu_x": _c(0, (63, 33, 16), (1, 64), x_bf16=True, relu_x=True),
    "fwd_k511": _c(0, (3, 511, 9), (1, 512), bias=True),                                   # one tile, K = 511: no split
    "fwd_k512": _c(0, (3, 512, 9), (4, 128), bias=True, relu_out=True),                    # K = 512: split 4, chunk 128
    "fwd_k513_relu_x": _c(0, (9, 513, 3), (4, 160), bias=True, relu_x=True),               # ragged last slab: 160 + 160 + 160 + 33
    "fwd_k1030_bf16_relu_x": _c(0, (64, 1030, 63), (7, 160), x_bf16=True, relu_x=True, bias=True, relu_out=True),   # planned 8, runs 7
    # ---- linear_dgrad: (n, in, out), K = out.  The observation layers as N / ldc
    "dgrad_obs9": _c(1, (65, 9, 64), (1, 64)),
    "dgrad_mask": _c(1, (63, 65, 31), (1, 32), mask=True),
    "dgrad_bf16_mask": _c(1, (129, 64, 33), (1, 64), x_bf16=True, mask=True),
    "dgrad_bf16": _c(1, (3, 16, 32), (1, 32), x_bf16=True),
    "dgrad_k2432_mask": _c(1, (16, 63, 2432), (19, 128), mask=True),                       # 19 slabs: the reduce's 8 + 8 + 3
    "dgrad_k512_bf16_mask": _c(1, (64, 65, 512), (4, 128), x_bf16=True, mask=True),        # two tiles
    "dgrad_k513_bf16": _c(1, (9, 5, 513), (4, 160), x_bf16=True),
    "fc_dgrad_bf16_mask": _c(1, (65, 2048, 64), (1, 64), x_bf16=True, mask=True),          # backward_impala_bf16's embedder.fc dgrad, n < 1024
    # ---- linear_wgrad: (n, in, out), (M, N, K) = (out, in, n), accumulates
    "wgrad_obs9": _c(2, (300, 9, 64), (1, 320)),
    "wgrad_heads": _c(2, (33, 64, 3), (1, 64)),
    "wgrad_relu_x": _c(2, (31, 65, 16), (1, 32), relu_x=True),
    "wgrad_one": _c(2, (1, 129, 1), (1, 32)),
    "wgrad_k513_relu_x": _c(2, (513, 63, 9), (4, 160), relu_x=True),
    "fc_wgrad_bf16_relu_x": _c(2, (65, 2048, 64), (1, 96), x_bf16=True, relu_x=True),      # backward_impala_bf16's embedder.fc wgrad, n < 1024
    "fc_wgrad_bf16_relu_x_split": _c(2, (600, 2048, 64), (4, 160), x_bf16=True, relu_x=True),   # 32 tiles, K = n = 600
    # ---- launch_gemm itself: (M, N, K)
    "sae_encode": _c(3, (65, 129, 2048), (1, 2048), bias=True, relu_out=True, use_ws=False),       # null workspace: the SAE never splits
    "sae_denc_mask": _c(3, (16, 65, 33), (1, 64), b_kc=False, mask=True, use_ws=False),
    "sae_probe_acc": _c(3, (3, 129, 65), (1, 96), a_kc=False, b_kc=False, acc=True),               # sam = 1, sak = A + 1
    "sae_probe_acc_split": _c(3, (3, 129, 1030), (7, 160), a_kc=False, b_kc=False, acc=True),      # three tiles: planned 8, runs 7
    "ws_cap": _c(3, (64, 64, 1024), (3, 352), a_kc=False, ws_floats=3 * 4096 + 100),               # planned 8; the cap loop stops at 3
    "tiles100": _c(3, (640, 640, 2048), (5, 416), bias=True),                                      # split capped by 512 / tiles = 5
    "tile_gate": _c(3, (769, 1024, 512), (1, 512)),                                                # 208 tiles: no split by the tile gate
    "split_ldc_mask": _c(3, (9, 5, 512), (4, 128), b_kc=False, bias=True, relu_out=True, mask=True, ldc=8),
    "split_ldc_acc": _c(3, (63, 65, 513), (4, 160), acc=True, ldc=67),
    "direct_ldc_mask_acc": _c(3, (65, 9, 31), (1, 32), bias=True, mask=True, acc=True, ldc=12),
}

EDGE_MN = (1, 3, 9, 16, 63, 64, 65, 129)
EDGE_K = (1, 31, 32, 33, 300)
STRIDES = ((True, True), (True, False), (False, True), (False, False))       # (a_kc, b_kc)


def edge_cases(a_kc, b_kc):
    """The 64 (M, N) pairs of EDGE_MN under one stride combination, as form 3 on the direct path; K and the epilogue options cycle, so
    over the four combinations every (M, N) meets four of the five K."""
    s = STRIDES.index((a_kc, b_kc))
    out = {}
    for i, M in enumerate(EDGE_MN):
        for j, N in enumerate(EDGE_MN):
            K = EDGE_K[(i + j + s) % 5]
            t = (3 * i + j + s) % 6
            o = dict(bias=t in (1, 2, 5), relu_out=t in (2, 5), mask=t in (3, 5), acc=t in (4, 5), ldc=N + 3 if (i + j) % 2 else None)
            out[f"edge_{int(a_kc)}{int(b_kc)}_{M}x{N}x{K}"] = _c(3, (M, N, K), (1, -(-K // 32) * 32), a_kc=a_kc, b_kc=b_kc, **o)
    return out


def mnk(c):
    a, b, d = c["d"]
    return {0: (a, d, b), 1: (a, b, d), 2: (d, b, a), 3: (a, b, d)}[c["form"]]


def c_bf16(c):
    return c["form"] == 1 and c["x_bf16"]


# ------------------------------------------------------------------------------------------------ inputs
class Inputs:
    """Aop (M, K), Bop (K, N): the operands as stored (float32; bf16-typed ones hold bf16 values), before the ReLU on load.
    bias (N), mask (M, ldc), C0 (M, ldc), dY / gb0 (form 2) or None."""
    __slots__ = ("c", "layer", "M", "N", "K", "ldc", "Aop", "Bop", "bias", "mask", "C0", "gb0")


def _draw(rng, shape, layer, typed=False, sparse=False, away=False):
    if layer == "exact":
        if sparse:
            return (rng.integers(-1, 2, shape) * (rng.random(shape) < 0.375)).astype(np.float32)
        return rng.integers(-8, 9, shape).astype(np.float32)
    v = rng.standard_normal(shape)
    if away:
        v += np.copysign(AWAY, v)
    v = v.astype(np.float32)
    return bf16_round(v) if typed else v


def build(c, layer, seed=0):
    M, N, K = mnk(c)
    rng = np.random.default_rng([71, c["form"], M, N, K, LAYERS.index(layer), seed])
    p = Inputs()
    p.c, p.layer, p.M, p.N, p.K, p.ldc = c, layer, M, N, K, (c["ldc"] or N)
    f, bf, sparse = c["form"], c["x_bf16"], c_bf16(c)
    p.Aop = _draw(rng, (M, K), layer, typed=bf and f == 0, sparse=sparse, away=c["relu_x"] and f == 0)
    p.Bop = _draw(rng, (K, N), layer, typed=bf and f == 2, sparse=sparse, away=c["relu_x"] and f == 2)
    p.bias = _draw(rng, (N,), layer) if c["bias"] else None
    p.mask = None
    if c["mask"]:
        if layer == "exact":
            p.mask = rng.choice(np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], np.float32), (M, p.ldc))
        else:
            p.mask = _draw(rng, (M, p.ldc), layer, typed=bf and f == 1, away=True)
    p.C0 = _draw(rng, (M, p.ldc), layer) if c["acc"] else None
    p.gb0 = _draw(rng, (M,), layer) if f == 2 else None
    return p


def hook_args(p):
    """The keyword arguments of Engine.op_linear for p."""
    c, f = p.c, p.c["form"]
    kw = dict(form=f, relu_x=c["relu_x"], relu_out=c["relu_out"], x_bf16=c["x_bf16"], bias=p.bias)
    if f == 0:
        kw.update(A=p.Aop, B=np.ascontiguousarray(p.Bop.T))
    elif f == 1:
        kw.update(A=p.Aop, B=p.Bop, mask=p.mask)
    elif f == 2:
        kw.update(A=np.ascontiguousarray(p.Aop.T), B=p.Bop, C0=p.C0, gb0=p.gb0)
    else:
        A = p.Aop if c["a_kc"] else np.ascontiguousarray(p.Aop.T)            # [M][K] (sam = K, sak = 1) or [K][M] (sam = 1, sak = M)
        B = np.ascontiguousarray(p.Bop.T) if c["b_kc"] else p.Bop            # [N][K] (sbk = 1, sbn = K) or [K][N] (sbk = N, sbn = 1)
        st = ((p.K, 1) if c["a_kc"] else (1, p.M)) + ((1, p.K) if c["b_kc"] else (p.N, 1)) + (p.ldc,)
        kw.update(A=A.reshape(-1), B=B.reshape(-1), mask=p.mask, C0=p.C0, dims=(p.M, p.N, p.K), strides=st, use_ws=c["use_ws"], ws_floats=c["ws_floats"])
    return kw


# ------------------------------------------------------------------------------------------------ reference, checker
def _operands(p, dtype):
    A, B = p.Aop.astype(dtype), p.Bop.astype(dtype)
    if p.c["relu_x"]:
        if p.c["form"] == 0:
            A = np.maximum(A, 0)
        else:
            B = np.maximum(B, 0)
    return A, B


def _epilogue(p, pre, dtype, bias=None, mask=None):
    """the epilogue of gemm.hip on pre (M, N) in dtype; bias / mask override what the case has (the planted errors)"""
    N = p.N
    v = pre
    bias = p.bias if bias is None else bias
    if bias is not None:
        v = v + bias.astype(dtype)
    if p.c["relu_out"]:
        v = np.maximum(v, 0)
    if p.mask is not None:
        v = np.where((p.mask[:, :N] if mask is None else mask) > 0, v, 0).astype(dtype)
    if c_bf16(p.c):          # the one final rounding is the kernel's: the float64 reference keeps the unrounded value, the bound allows for it
        return bf16_round(v) if dtype == np.float32 else v
    if p.C0 is not None:
        v = v + p.C0[:, :N].astype(dtype)
    return v


class Ref:
    __slots__ = ("want", "S", "bound", "kept", "gb", "gb_bound")


def reference(p, split):
    """float64: the result, S = sum |a b| + |bias| + |C0| and the bound of the real layer for a run of `split` slabs."""
    A, B = _operands(p, np.float64)
    r = Ref()
    r.want = _epilogue(p, A @ B, np.float64)
    r.S = np.abs(A) @ np.abs(B)
    if p.bias is not None:
        r.S = r.S + np.abs(p.bias.astype(np.float64))
    if p.C0 is not None:
        r.S = r.S + np.abs(p.C0[:, :p.N].astype(np.float64))
    r.bound = (p.K + split + 4) * U * r.S
    if c_bf16(p.c):
        r.bound = r.bound + 2.0 ** -8 * np.abs(r.want)
    r.kept = None if p.mask is None else p.mask[:, :p.N] > 0
    r.gb = r.gb_bound = None
    if p.c["form"] == 2:          # gb += colsum(dY), dY = Aop^T: pinned by optim_inputs; here it has to be right
        a = p.Aop.astype(np.float64)
        r.gb = p.gb0.astype(np.float64) + a.sum(1)
        r.gb_bound = (p.K + 4) * U * (np.abs(p.gb0.astype(np.float64)) + np.abs(a).sum(1))
    return r


def exact_margin(p, r):
    """(largest S, the limit below which every partial sum is exact in the output type)"""
    s = float(r.S.max())
    if p.c["form"] == 2:
        s = max(s, float((np.abs(p.gb0) + np.abs(p.Aop).sum(1)).max()))
    return s, (2.0 ** 8 if c_bf16(p.c) else 2.0 ** 24)


def rel_l2(a, ref):
    den = np.sqrt((ref ** 2).sum())
    return float(np.sqrt(((np.asarray(a, np.float64) - ref) ** 2).sum()) / den) if den > 0 else float(np.abs(a).max())


def check(p, r, got, gb=None, what=""):
    """Assert got (M, N) (and gb) against r -> the largest error / bound of the real layer (0.0 for the exact layer)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == r.want.shape, (what, got.dtype, got.shape, r.want.shape)
    bad = ~np.isfinite(got)
    assert not bad.any(), f"{what}: {int(bad.sum())} non-finite elements (skipped by the kernel?), first at {tuple(np.argwhere(bad)[0])}"
    pairs = [("C", got.astype(np.float64), r.want, r.bound)]
    if r.gb is not None:
        gb = np.asarray(gb)
        assert gb.dtype == np.float32 and gb.shape == r.gb.shape and np.isfinite(gb).all(), (what, "gb")
        pairs.append(("gb", gb.astype(np.float64), r.gb, r.gb_bound))
    if r.kept is not None:
        zero = 0.0 if p.C0 is None or c_bf16(p.c) else p.C0[:, :p.N].astype(np.float64)
        leak = ~r.kept & (pairs[0][1] != zero)
        assert not leak.any(), f"{what}: {int(leak.sum())} masked elements are not exactly 0 (or C0), first at {tuple(np.argwhere(leak)[0])}"
    worst = 0.0
    for name, g, want, bound in pairs:
        if p.layer == "exact":
            ne = g != want
            assert not ne.any(), (f"{what} {name}: {int(ne.sum())} elements differ from the exact result, first at {tuple(np.argwhere(ne)[0])}: "
                                  f"{g[tuple(np.argwhere(ne)[0])]!r} != {want[tuple(np.argwhere(ne)[0])]!r}")
            continue
        err = np.abs(g - want)
        k = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        assert err[k] <= bound[k], (f"{what} {name}: element {tuple(int(v) for v in k)} = {g[k]!r}, reference {want[k]!r}: error {err[k]:.3e} > bound "
                                    f"{bound[k]:.3e}; {int((err > bound).sum())} elements out of bound")
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.where(bound > 0, err / bound, 0.0).max()))
    return worst


# ------------------------------------------------------------------------------------------------ float32 on the CPU, planted errors
FAULTS = ("drop_k", "bias_shift", "mask_stride", "slab_twice")


def fault_applies(c, fault):
    M, N, K = mnk(c)
    return {"drop_k": True, "bias_shift": c["bias"] and N >= 2, "mask_stride": c["mask"] and (c["ldc"] or N) > N and M >= 2,
            "slab_twice": c["plan"][0] > 1}[fault]


def planted_k(p):
    """the k whose term is dropped from output tile (0, 0): the one with the largest single product there"""
    A, B = _operands(p, np.float64)
    return int(np.argmax(np.abs(A[:64]).max(0) * np.abs(B[:, :64]).max(1)))


def cpu_result(p, fault=None, dtype=np.float32):
    """The case in torch's float32 on the CPU (dtype float64: the same expression exactly) -> (C, gb or None).  fault: one of FAULTS --
    one k dropped from one output tile, the bias read one column on, the mask read with stride N instead of ldc, slab 0 added twice."""
    import torch
    A, B = _operands(p, dtype)
    pre = (torch.from_numpy(A) @ torch.from_numpy(B)).numpy()
    bias = mask = None
    if fault == "drop_k":
        k = planted_k(p)
        pre = pre.copy()
        pre[:64, :64] -= np.outer(A[:64, k], B[k, :64])
    elif fault == "bias_shift":
        bias = np.roll(p.bias, -1)
    elif fault == "mask_stride":
        mask = p.mask.reshape(-1)[:p.M * p.N].reshape(p.M, p.N)
    elif fault == "slab_twice":
        kc = p.c["plan"][1]
        pre = pre + (torch.from_numpy(np.ascontiguousarray(A[:, :kc])) @ torch.from_numpy(np.ascontiguousarray(B[:kc]))).numpy()
    else:
        assert fault is None, fault
    gb = None
    if p.c["form"] == 2:
        gb = (p.gb0.astype(dtype) + p.Aop.astype(dtype).sum(1, dtype=dtype)).astype(dtype)
    return _epilogue(p, pre, dtype, bias=bias, mask=mask).astype(dtype), gb


POOL = 64
SMALL = 256


@functools.lru_cache(maxsize=None)
def _pooled_error(form, K, opts):
    c = dict(opts)
    c["d"] = {0: (POOL, K, POOL), 1: (POOL, POOL, K), 2: (K, POOL, POOL), 3: (POOL, POOL, K)}[form]
    c["ldc"] = None
    p = build(c, "real", seed=1)
    return rel_l2(cpu_result(p)[0], reference(p, 1).want)


def torch_error(p, r):
    """torch's float32 CPU error (relative L2 against float64) of p's C: measured on p itself from 256 output elements on, else on a
    64 x 64 case of the same K, options and distribution (a few numbers do not estimate an error)."""
    if p.M * p.N >= SMALL:
        return rel_l2(cpu_result(p)[0], r.want)
    return _pooled_error(p.c["form"], p.K, tuple(sorted((k, v) for k, v in p.c.items() if k not in ("d", "ldc", "plan"))))


@functools.lru_cache(maxsize=4)
def named(name, layer):
    """(inputs, reference) of one named case; treat both as read-only"""
    c = CASES[name]
    p = build(c, layer)
    return p, reference(p, c["plan"][0])
