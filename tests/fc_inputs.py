"""Inputs, float64 reference and per-element checker of the bf16 embedder.fc kernels (csrc/fc_bf16.hip) at op level.  Host only: numpy.

The kernels compute, on operands rounded to bf16 (x on the host, W by launch_fc_pack, dy while a kernel stages it), with fp32 accumulation:
  mode 0 / 1   y  = max(relu(x) W^T + b, 0)                      [n][D]      K' = 2048 + 1 addends per element (the bias counts)
  mode 2       dx = (dy W) * (x > 0), stored as bf16             [n][2048]   K' = D
  mode 3       gW = gW0 + dy^T relu(x)                           [D][2048]   K' = n + 1 (the initial gradient counts)
               gb = gb0 + colsum(dy), dy NOT rounded             [D]         K' = n + 1
The reference evaluates the same expressions in float64 on the same rounded operands, so what is left is accumulation error alone.

Bound, per element.  bf16 x bf16 products are exact in fp32, so any order of fp32 round-to-nearest accumulation of K' addends whose
absolute values sum to S errs by at most K' u S, u = 2^-24.  check() allows c K' 2^-24 S + 1e-30 with c = 2 (a matrix core that truncates
instead of rounding doubles u); mode 2 adds 2^-8 |ref| for the bf16 store (half an ulp of an 8-bit significand is between 2^-9 and 2^-8
of the value; the rounding of an accumulator that is itself off by the first term is covered by that term's factor c).
That term is TIGHT, not slack: just above a power of two a correctly rounded store alone uses all of 2^-8 |ref|, and the first term is the
only cushion (the float32 evaluation on the host reaches 0.991 of the mode-2 bound, the MI355X 0.99).  A correct kernel can therefore come
within a percent of the bound; a failure there is to be understood element by element, not met by a wider bound.
Exact: every masked dx element is 0.0, every value is finite (the hook poisons its outputs: a skipped element is NaN).

Rows: x has per-row scales (1e-3, 1e3, 1) cycling, dy the inverse ones, so neighbouring rows differ by 1e3 or 1e6 in both -- a value that
leaks from one row into another breaks the per-element bound by orders of magnitude -- while the products dy x of mode 3 stay O(1) in
every row, so each row of the batch weighs the same in gW.  About half of x is negative, 1 % each is exactly +0.0 / -0.0 (both "not > 0"),
and row n // 2 is negative throughout (n >= 2; a single row keeps its signs, or nothing of it would reach gW or dx): its y is relu(b), its
dx row zero, its share of gW nothing.
"""
import functools

import numpy as np

K = 2048
WIDTHS = (64, 128, 192, 256, 320, 384, 448, 512)
U = 2.0 ** -24
C_DEFAULT = 2.0

# (mode, what) -> batch sizes; tests/test_gpu_fc_ops.py says which launch path each reaches
FWD_DEDICATED_N = (64, 576)
FWD_NT_N = (1, 65, 200)
SMALL_N = (1, 16, 17, 250)
DGRAD_GUARDED_N = (1, 127, 129, 1088)            # D != 256
DGRAD256_DEDICATED_N = (128, 1152)
DGRAD256_NT64_N = (1, 200, 1088)
DGRAD256_NT128_N = (2056,)
WGRAD_N = (1, 128, 129, 1024, 1088)
WGRAD_LONG = (64, 4100)                          # (D, n)


def cases(mode):
    """Every (D, n) the GPU tests run in this mode."""
    if mode == 0:
        return [(D, n) for D in WIDTHS for n in FWD_DEDICATED_N + FWD_NT_N]
    if mode == 1:
        return [(D, n) for D in WIDTHS for n in SMALL_N]
    if mode == 2:
        return [(D, n) for D in WIDTHS for n in (DGRAD256_DEDICATED_N + DGRAD256_NT64_N + DGRAD256_NT128_N if D == 256 else DGRAD_GUARDED_N)]
    return [(D, n) for D in WIDTHS for n in WGRAD_N] + [WGRAD_LONG]


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even) as float32: the rounding of host_to_bf16, v_cvt_pk_bf16_f32 and torch's .bfloat16()."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def row_scales(n):
    return np.array([1e-3, 1e3, 1.0])[np.arange(n) % 3]


def negative_row(n):
    return n // 2 if n >= 2 else None


class Inputs:
    __slots__ = ("mode", "D", "n", "x", "W", "b", "dy", "gW0", "gb0")


def make_inputs(mode, D, n):
    rng = np.random.default_rng([mode, D, n])
    s = row_scales(n)[:, None]
    p = Inputs()
    p.mode, p.D, p.n = mode, D, n
    x = rng.standard_normal((n, K)) * s
    z = rng.random((n, K))
    x[z < 0.01] = 0.0
    x[(z >= 0.01) & (z < 0.02)] = -0.0
    r = negative_row(n)
    if r is not None:
        x[r] = -(np.abs(rng.standard_normal(K)) + 0.01) * s[r]
    p.x = x.astype(np.float32)
    p.W = (0.05 * rng.standard_normal((D, K))).astype(np.float32)
    b = 0.1 * rng.standard_normal(D)
    p.b = (b + np.copysign(0.01, b)).astype(np.float32)
    p.dy = (rng.standard_normal((n, D)) / s).astype(np.float32)
    g = rng.standard_normal((D, K))
    p.gW0 = (g + np.copysign(0.01, g)).astype(np.float32)
    g = rng.standard_normal(D)
    p.gb0 = (g + np.copysign(0.01, g)).astype(np.float32)
    return p


def operands(p):
    """The operands as the kernels see them, float64: x, relu(x), W, dy rounded to bf16; the mask x > 0."""
    xb = bf16_round(p.x).astype(np.float64)
    return dict(xb=xb, xr=np.maximum(xb, 0.0), Wb=bf16_round(p.W).astype(np.float64), dyb=bf16_round(p.dy).astype(np.float64), mask=xb > 0)


def reference(p):
    """[(name, ref, S, K')] in float64: the outputs of p.mode, the sum of the absolute values of each element's addends, their number."""
    o = operands(p)
    if p.mode in (0, 1):
        pre = o["xr"] @ o["Wb"].T + p.b.astype(np.float64)
        S = o["xr"] @ np.abs(o["Wb"]).T + np.abs(p.b.astype(np.float64))
        return [("y", np.maximum(pre, 0.0), S, K + 1)]
    if p.mode == 2:
        return [("dx", (o["dyb"] @ o["Wb"]) * o["mask"], np.abs(o["dyb"]) @ np.abs(o["Wb"]), p.D)]
    dy = p.dy.astype(np.float64)
    gW = p.gW0.astype(np.float64) + o["dyb"].T @ o["xr"]
    SW = np.abs(p.gW0.astype(np.float64)) + np.abs(o["dyb"]).T @ o["xr"]
    return [("gW", gW, SW, p.n + 1), ("gb", p.gb0.astype(np.float64) + dy.sum(0), np.abs(p.gb0.astype(np.float64)) + np.abs(dy).sum(0), p.n + 1)]


@functools.lru_cache(maxsize=2)
def case(mode, D, n):
    """(inputs, reference) of one case; the last two stay cached (treat both as read-only)."""
    p = make_inputs(mode, D, n)
    return p, reference(p)


def check(p, got, ref=None, c=C_DEFAULT):
    """Assert `got` (the mode's output; mode 3: (gW, gb)) against the float64 reference.  Returns {name: (worst err / bound, worst
    accumulation error in units of K' 2^-24 S)} -- the second figure is what a measured c would be set from."""
    ref = reference(p) if ref is None else ref
    got = got if isinstance(got, (tuple, list)) else (got,)
    assert len(got) == len(ref)
    worst = {}
    for g, (name, r, S, kp) in zip(got, ref):
        tag = f"fc mode {p.mode} D={p.D} n={p.n} {name}"
        g = np.asarray(g)
        assert g.shape == r.shape, f"{tag}: shape {g.shape}, expected {r.shape}"
        bad = ~np.isfinite(g)
        assert not bad.any(), f"{tag}: {int(bad.sum())} non-finite elements (skipped by the kernel?), first at {tuple(np.argwhere(bad)[0])}"
        g = g.astype(np.float64)
        if p.mode == 2:
            leak = ~(bf16_round(p.x) > 0) & (g != 0)
            assert not leak.any(), f"{tag}: {int(leak.sum())} masked elements are not 0.0, first at {tuple(np.argwhere(leak)[0])}"
        unit = kp * U * S
        store = 2.0 ** -8 * np.abs(r) if p.mode == 2 else 0.0
        bound = c * unit + store + 1e-30
        err = np.abs(g - r)
        ratio = err / bound
        acc = np.maximum(err - store, 0.0) / (unit + 1e-30)
        worst[name] = (float(ratio.max()), float(acc.max()))
        k = np.unravel_index(int(ratio.argmax()), ratio.shape)
        assert ratio[k] <= 1.0, (f"{tag}: element {tuple(int(v) for v in k)} = {g[k]!r}, reference {r[k]!r}: error {err[k]:.3e} is {ratio[k]:.3g} x the bound "
                                 f"{bound[k]:.3e} (c = {c}, K' = {kp}, S = {S[k]:.3e}); {int((ratio > 1).sum())} elements out of bound")
    return worst


def _blocked(A, B, tile=128):
    """fp32 A @ B with the K dimension summed in tiles of 128, the kernels' order."""
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k0 in range(0, A.shape[1], tile):
        acc += A[:, k0:k0 + tile] @ B[k0:k0 + tile]
    return acc


def emulate_f32(p):
    """The mode's output evaluated in numpy float32 on the rounded operands: what a correct kernel may return."""
    xb, Wb, dyb = bf16_round(p.x), bf16_round(p.W), bf16_round(p.dy)
    xr = np.maximum(xb, np.float32(0))
    if p.mode in (0, 1):
        return np.maximum(_blocked(xr, np.ascontiguousarray(Wb.T)) + p.b, np.float32(0))
    if p.mode == 2:
        return bf16_round(_blocked(dyb, Wb) * (xb > 0))
    return p.gW0 + _blocked(np.ascontiguousarray(dyb.T), xr), p.gb0 + p.dy.sum(0, dtype=np.float32)
