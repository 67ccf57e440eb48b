"""Inputs, float64 / integer references and checkers for the op-level tests of the optimizer tail and the fixed-order reductions
(tests/test_gpu_optim_ops.py on the GPU, tests/test_optim_host.py on the CPU).  Nothing here touches a GPU.

Reductions.  Two kinds of input per shape:
  exact     integers in [-8, 8] stored as float32, starting values included.  Every fp32 partial sum is an integer of magnitude at most
            8 * (terms + 1) < 2^24, so it is exact in ANY summation order and the result must equal the int64 sum: one dropped, doubled
            or misplaced term fails.
  rounding  |x| uniform in [0.5, 2] with a random sign, against the float64 sum with the derived bound
                |got - ref| <= (d + 2) * 2^-24 * sum|x| + 2^-24 * |ref|
            (sum|x| per output element, starting value included), where d is the longest chain of additions a term passes through:
              reduce_slabs_kernel, reduce_all_slabs_kernel   d = ceil(nslab / 32) + 32
                  a thread adds every 32nd slab (ceil(nslab / 32) additions), then one thread adds the 32 group sums
              colsum_partial_kernel + reduce_slabs_kernel    d = ceil(M / groups) + ceil(groups / 32) + 32
                  groups = 256 row groups when M >= 4096 and N <= 1024, else 64; a thread adds every groups-th row, the slab sum over
                  the `groups` partial rows follows
            and the + 2 covers the addition into the target and the first addition to zero.  With |x| >= 0.5 one missing term moves
            the result by at least 0.5, more than the bound at every listed shape (test_optim_host.py checks that).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of float32

# ------------------------------------------------------------------------------------------------ slab sums
SLAB_NSLAB = (1, 2, 31, 32, 33, 65, 512, 1024)
# (slab_len, n_w, n_b): (4112, 4096, 16) the heads at A = 15, H = 256; (100, 60, 30): ten trailing elements that are dropped
SLAB_SHAPES = ((1, 1, 0), (31, 31, 0), (33, 20, 13), (4112, 4096, 16), (448, 432, 16), (100, 60, 30))
SLAB_CASES = tuple((ns,) + sh for sh in SLAB_SHAPES for ns in SLAB_NSLAB)

# reduce_all_slabs: the four conv slab lengths (weights + biases of block1.conv, the 16-channel, 16 -> 32 and 32-channel convs) and the
# slab counts around the 4-in-flight loop's boundaries (b + 96 < nslab for slab groups b = 0 and b = 31)
CONV_SLABS = ((448, 432), (2320, 2304), (4640, 4608), (9248, 9216))          # (slab_len, n_w)
ALL_NSLAB = (1, 32, 96, 97, 127, 128, 129, 224, 225, 1024)
ALL_SLAB_CASES = (0, 3)          # layer k of a case: conv slab k % 4 with ALL_NSLAB[(k + case) % 10], ten layers per launch

# (M, N, ld)
COLSUM_CASES = ((1, 1, 1), (63, 15, 16), (65, 16, 17), (449, 64, 64), (513, 65, 65), (4095, 1024, 1024), (4096, 1024, 1024),
                (4097, 1025, 1025), (4096 + 1793, 256, 256), (300, 4096, 4096))


def _values(rng, shape, exact):
    if exact:
        return rng.integers(-8, 9, size=shape).astype(np.float32)
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice((-1.0, 1.0), size=shape)).astype(np.float32)


def slab_depth(nslab):
    return -(-nslab // 32) + 32


def colsum_groups(M, N):
    return 256 if (M >= 4096 and N <= 1024) else 64


def colsum_depth(M, N):
    g = colsum_groups(M, N)
    return -(-M // g) + -(-g // 32) + 32


def bound(depth, sum_abs, ref):
    return (depth + 2) * U * sum_abs + U * np.abs(ref)


def worst_bound(depth, terms):
    """The bound's largest possible value for `terms` summed inputs and one starting value, all of magnitude at most 2."""
    s = 2.0 * (terms + 1)
    return (depth + 2) * U * s + U * s


class Reduced:
    """want: the float64 result (exactly the integer sum for exact inputs); sum_abs: sum |x| per element; depth: d above."""
    def __init__(self, want, sum_abs, depth):
        self.want, self.sum_abs, self.depth = want, sum_abs, depth


def slab_case(nslab, slab_len, n_w, n_b, exact):
    rng = np.random.default_rng([7, nslab, slab_len, int(exact)])
    return _values(rng, (nslab, slab_len), exact), _values(rng, n_w, exact), (_values(rng, n_b, exact) if n_b else None)


def slab_reference(partial, w0, b0, drop_slab=None, drop_tail=False, shift_boundary=False):
    """-> (Reduced for dst_w, Reduced for dst_b or None).  The three switches build a WRONG result, for the checkers' own test: one slab
    left out, the last summed element left out, the weight / bias boundary one element early."""
    n_w, n_b = w0.size, 0 if b0 is None else b0.size
    p = partial.astype(np.float64)
    if drop_slab is not None:
        p = np.delete(p, drop_slab, axis=0)
    s, a = p.sum(0), np.abs(p).sum(0)
    if drop_tail:
        s[n_w + n_b - 1] = 0.0
    if shift_boundary:          # element n_w - 1 lands in dst_b[0], and every bias one place further
        b_s = s[n_w - 1:n_w - 1 + n_b].copy()
        s[n_w - 1] = 0.0
        s[n_w:n_w + n_b] = b_s
    d = slab_depth(partial.shape[0])
    w = Reduced(w0.astype(np.float64) + s[:n_w], np.abs(w0).astype(np.float64) + a[:n_w], d)
    b = None if b0 is None else Reduced(b0.astype(np.float64) + s[n_w:n_w + n_b], np.abs(b0).astype(np.float64) + a[n_w:n_w + n_b], d)
    return w, b


def all_slabs_case(case, exact):
    """-> (ws, desc (10, 6) int64, grads0, layers).  The slab regions lie in ws with gaps of NaN between them (a read outside a region
    poisons the sum); in the flat gradient vector the bias regions come first, in reverse layer order, then the weight regions, with
    gaps of 4 to 40 starting values between all of them.  layers: (src_off, w_off, b_off, nslab, slab_len, n_w) per layer."""
    rng = np.random.default_rng([11, case, int(exact)])
    layers, src_off = [], 8
    for k in range(10):
        slab_len, n_w = CONV_SLABS[k % 4]
        nslab = ALL_NSLAB[(k + case) % 10]
        layers.append([src_off, 0, 0, nslab, slab_len, n_w])
        src_off += nslab * slab_len + 4 * (1 + k % 3)
    ws = np.full(src_off, np.nan, np.float32)
    off = 4
    for k in reversed(range(10)):
        layers[k][2] = off
        off += (layers[k][4] - layers[k][5]) + 4 * (1 + k)
    for k in range(10):
        layers[k][1] = off
        off += layers[k][5] + 4 * (10 - k)
    for so, _, _, nslab, slab_len, _ in layers:
        ws[so:so + nslab * slab_len] = _values(rng, nslab * slab_len, exact)
    return ws, np.array(layers, dtype=np.int64), _values(rng, off, exact), [tuple(l) for l in layers]


def all_slabs_reference(ws, layers, grads0, drop_slab=None, write_past=False):
    """-> Reduced over the whole flat vector: the gaps keep their starting values (sum_abs = |start| there, so any change fails both
    checkers).  drop_slab = (layer, slab) and write_past (one gap element behind layer 0's biases receives a sum) build wrong results."""
    want, sabs = grads0.astype(np.float64), np.abs(grads0).astype(np.float64)
    depth = np.zeros(grads0.size)
    for k, (so, wo, bo, nslab, slab_len, n_w) in enumerate(layers):
        p = ws[so:so + nslab * slab_len].astype(np.float64).reshape(nslab, slab_len)
        if drop_slab is not None and drop_slab[0] == k:
            p = np.delete(p, drop_slab[1], axis=0)
        s, a = p.sum(0), np.abs(p).sum(0)
        want[wo:wo + n_w] += s[:n_w]; sabs[wo:wo + n_w] += a[:n_w]; depth[wo:wo + n_w] = slab_depth(nslab)
        want[bo:bo + slab_len - n_w] += s[n_w:]; sabs[bo:bo + slab_len - n_w] += a[n_w:]; depth[bo:bo + slab_len - n_w] = slab_depth(nslab)
        if write_past and k == 0:
            want[bo + slab_len - n_w] += s[0]
    return Reduced(want, sabs, depth)


def colsum_case(M, N, ld, exact):
    rng = np.random.default_rng([13, M, N, ld, int(exact)])
    return _values(rng, (M, ld), exact), _values(rng, N, exact)          # (the columns past N hold values too: they must not be summed)


def colsum_reference(dY, db0, drop_row=None):
    N = db0.size
    y = dY[:, :N].astype(np.float64)
    if drop_row is not None:
        y = np.delete(y, drop_row, axis=0)
    return Reduced(db0.astype(np.float64) + y.sum(0), np.abs(db0).astype(np.float64) + np.abs(y).sum(0), colsum_depth(dY.shape[0], N))


def exact_headroom(r):
    """Largest possible magnitude of any partial sum of an exact case: must stay below 2^24."""
    return float(np.max(r.sum_abs))


def check_exact(got, r, what=""):
    assert got.dtype == np.float32 and got.shape == r.want.shape, (what, got.dtype, got.shape)
    want = np.rint(r.want).astype(np.int64)
    assert np.array_equal(r.want, want), "the reference of an exact case must be integers"
    bad = np.flatnonzero(got.astype(np.float64) != want)
    assert bad.size == 0, f"{what}: {bad.size} elements differ from the integer sum, first at {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


def check_rounding(got, r, what=""):
    """-> the largest error / bound ratio."""
    assert got.dtype == np.float32 and got.shape == r.want.shape, (what, got.dtype, got.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite sums"
    err, b = np.abs(got.astype(np.float64) - r.want), bound(r.depth, r.sum_abs, r.want)
    k = int(np.argmax(err - b))
    assert err[k] <= b[k], f"{what}: element {k} is {err[k]:.3e} from the float64 sum, bound {b[k]:.3e}"
    return float(np.max(err / b))


# ------------------------------------------------------------------------------------------------ gradient norm
NORM_N = (1, 127, 128, 129, 257, 32773, 131072, 131200, 300001, 1000003)


def norm_case(n, exact):
    rng = np.random.default_rng([17, n, int(exact)])
    return rng.integers(-8, 9, size=n).astype(np.float32) if exact else rng.standard_normal(n).astype(np.float32)


def norm_reference(g):
    """float32(sqrt(float64(sum g^2))): each square is exact in float64; fsum adds them without error"""
    return np.float32(math.sqrt(math.fsum((g.astype(np.float64) ** 2).tolist())))


def split_in_two(n):
    """(n1, offsets of the second vector's four pieces) for a vector of n >= 5 elements handed to Variant 1 as two"""
    n2 = max(4, n // 3)
    q = n2 // 4
    return n - n2, np.array([0, q, 2 * q, 3 * q, n2], dtype=np.int64) if n2 > 4 else np.array([0, 1, 2, 3, 4], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ Adam
LR = 5e-4
BETA1, BETA2, EPS = 0.9, 0.999, 1e-5


class Consts:
    """Constants of the moment updates.  TORCH: what torch.optim.Adam computes in Python float64.  KERNEL: what adam_kernel documents --
    the betas as float32, 1 - beta subtracted in float32 (csrc/optim.hip; the comment above sae_adam_kernel in csrc/sae.hip).  The bias
    corrections are float64 powers of 0.9 and 0.999 in both, as in torch."""
    def __init__(self, beta1, beta2, w1, w2):
        self.beta1, self.beta2, self.w1, self.w2 = float(beta1), float(beta2), float(w1), float(w2)


TORCH = Consts(BETA1, BETA2, 1 - BETA1, 1 - BETA2)
KERNEL = Consts(np.float32(BETA1), np.float32(BETA2), np.float32(1) - np.float32(BETA1), np.float32(1) - np.float32(BETA2))


def adam_reference(p, g, m, v, lr, max_norm, step, consts):
    """clip_grad_norm_ + Adam(eps=1e-5).step() in float64 on one flat vector -> (p', m', v', norm, coef)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    norm = math.sqrt(math.fsum((g * g).tolist()))
    coef = min(1.0, max_norm / (norm + 1e-6))
    g = g * coef
    m2 = m + consts.w1 * (g - m)
    v2 = v * consts.beta2 + consts.w2 * g * g
    bc1, bc2 = 1 - BETA1 ** step, 1 - BETA2 ** step
    denom = np.sqrt(v2) / math.sqrt(bc2) + EPS
    return p - (lr / bc1) * (m2 / denom), m2, v2, norm, coef


def torch_adam(vectors, lr, max_norm, step, dtype):
    """torch's own clip_grad_norm_ + optim.Adam(eps=1e-5) on a list of (p, g, m, v), the state injected -> ([(p', m', v')], norm)"""
    params = []
    for p, g, _, _ in vectors:
        q = torch.nn.Parameter(torch.tensor(np.asarray(p), dtype=dtype))
        q.grad = torch.tensor(np.asarray(g), dtype=dtype)
        params.append(q)
    opt = torch.optim.Adam(params, lr=lr, betas=(BETA1, BETA2), eps=EPS)
    for q, (_, _, m, v) in zip(params, vectors):
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.tensor(np.asarray(m), dtype=dtype),
                        "exp_avg_sq": torch.tensor(np.asarray(v), dtype=dtype)}
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    out = [(q.detach().numpy(), opt.state[q]["exp_avg"].numpy(), opt.state[q]["exp_avg_sq"].numpy()) for q in params]
    assert all(int(opt.state[q]["step"]) == step for q in params)
    return out, float(norm)


def rel_l2(a, ref):
    a, ref = np.asarray(a, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    den = math.sqrt(float((ref * ref).sum()))
    return math.sqrt(float(((a - ref) ** 2).sum())) / den if den > 0 else math.sqrt(float(((a - ref) ** 2).sum()))


# name: (variant, n, step, grad, max_norm, p_zero, moments).  grad: "big" (norm far above max_norm: coefficient < 1), "small" (far below:
# coefficient exactly 1), "zero" (only the momentum moves p).  moments: zero at step 1, non-zero afterwards.
# clips(name) tells whether the case must clip; with p = 0 the new p is the step itself.
ADAM_CASES = {
    "v0-n1-step1-big-p0":             (0, 1, 1, "big", 0.5, True),
    "v0-n255-step2-small":            (0, 255, 2, "small", 0.5, False),
    "v0-n256-step1000-big":           (0, 256, 1000, "big", 0.5, False),
    "v0-n257-step30000-big-nomax-p0": (0, 257, 30000, "big", 1e9, True),
    "v0-n4097-step1-big-p0":          (0, 4097, 1, "big", 0.5, True),
    "v0-n4097-step1000-zero-p0":      (0, 4097, 1000, "zero", 0.5, True),
    "v0-n131200-step2-small":         (0, 131200, 2, "small", 0.5, False),
    "v1-n257-step1-big-p0":           (1, 257, 1, "big", 0.5, True),
    "v1-n4097-step2-big":             (1, 4097, 2, "big", 0.5, False),
    "v1-n131200-step30000-small-p0":  (1, 131200, 30000, "small", 0.5, True),
    "v2-n1-step30000-zero":           (2, 1, 30000, "zero", 0.5, False),
    "v2-n255-step2-big-nomax":        (2, 255, 2, "big", 1e9, False),
    "v2-n4097-step1-big-p0":          (2, 4097, 1, "big", 0.5, True),
    "v2-n131200-step1000-small-p0":   (2, 131200, 1000, "small", 0.5, True),
}


def clips(name):
    _, _, _, grad, max_norm, _ = ADAM_CASES[name]
    return grad == "big" and max_norm < 1e8


def adam_inputs(n, step, grad, p_zero, seed=0):
    """(p, g, m, v) float32.  |g| is about 3 ("big": the norm of even one element is six times max_norm = 0.5), about 1e-5 ("small": the norm of
    131200 elements is 4e-3) or 0; the moments are those of a run at this gradient scale, v > 0."""
    rng = np.random.default_rng([19, n, step, seed, {"big": 0, "small": 1, "zero": 2}[grad]])
    scale = {"big": 3.0, "small": 1e-5, "zero": 1e-3}[grad]
    g = (rng.uniform(0.5, 1.5, n) * rng.choice((-1.0, 1.0), n) * scale).astype(np.float32) if grad != "zero" else np.zeros(n, np.float32)
    p = np.zeros(n, np.float32) if p_zero else (0.1 * rng.standard_normal(n)).astype(np.float32)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        c = min(1.0, 0.5 / (scale * math.sqrt(n))) * scale if grad == "big" else scale          # the clipped scale
        m = (c * 0.3 * rng.standard_normal(n)).astype(np.float32)
        v = (c * c * rng.uniform(0.2, 1.0, n)).astype(np.float32)
    return p, g, m, v


def adam_case(name):
    variant, n, step, grad, max_norm, p_zero = ADAM_CASES[name]
    return variant, adam_inputs(n, step, grad, p_zero), step, max_norm


def torch_fp32_errors(inputs, step, max_norm):
    """(error of m', v', p') of torch's float32 Adam against torch's float64 Adam on the same float32 inputs, relative L2"""
    (r64,), _ = torch_adam([inputs], LR, max_norm, step, torch.float64)
    (r32,), _ = torch_adam([inputs], LR, max_norm, step, torch.float32)
    return rel_l2(r32[1], r64[1]), rel_l2(r32[2], r64[2]), rel_l2(r32[0], r64[0])


def adam_bound_inputs(name):
    """The inputs torch's own fp32 error is measured on: the case's, or for n < 256 the n = 4097 inputs of the same distribution (a few
    numbers do not estimate an error)."""
    variant, n, step, grad, max_norm, p_zero = ADAM_CASES[name]
    return adam_inputs(4097 if n < 256 else n, step, grad, p_zero)


# ------------------------------------------------------------------------------------------------ advantage statistics
ADV_SHAPES = ((1, 2), (1, 3), (1, 1023), (1, 1025), (66, 130))          # (T, E): T * E in {2, 3, 1023, 1025, 66 * 130}
ADV_DISTS = ("normal", "offset")


def adv_case(T, E, dist):
    rng = np.random.default_rng([23, T, E, ADV_DISTS.index(dist)])
    x = rng.standard_normal((T, E))
    return (x if dist == "normal" else 1000.0 + 0.01 * x).astype(np.float32)


def adv_stats_reference(x):
    """{count, mean, M2} of float32 values in float64 with math.fsum"""
    x = np.asarray(x, dtype=np.float64).ravel()
    if x.size == 0:
        return np.zeros(3)
    mean = math.fsum(x.tolist()) / x.size
    return np.array([x.size, mean, math.fsum(((x - mean) ** 2).tolist())])


def adv_stats_bounds(x):
    """(bound on mean, bound on M2): n * 2^-53 * sum|x| (sum|x - mean|^2 for M2), plus one float64 ulp of the value"""
    x = np.asarray(x, dtype=np.float64).ravel()
    s = adv_stats_reference(x)
    n = x.size
    return (n * 2.0 ** -53 * np.abs(x).sum() + np.spacing(abs(s[1])), n * 2.0 ** -53 * s[2] + np.spacing(s[2]))


def check_adv_stats(got, x, what=""):
    ref, (b_mean, b_m2) = adv_stats_reference(x), adv_stats_bounds(x)
    assert got[0] == ref[0], (what, "count", got[0], ref[0])
    assert abs(got[1] - ref[1]) <= b_mean, (what, "mean", got[1], ref[1], b_mean)
    assert abs(got[2] - ref[2]) <= b_m2, (what, "M2", got[2], ref[2], b_m2)
    return abs(got[1] - ref[1]) / b_mean, abs(got[2] - ref[2]) / b_m2


def adv_apply_reference(a, stats3):
    """(a - mean) / (sd + 1e-8) in float64 and the bound from the kernel's three float32 roundings (the difference, the sum sd + 1e-8,
    the quotient) and the float32 mean and sd it starts from: 2^-24 * (4 |out| + (|a| + |mean|) / sd)"""
    a = np.asarray(a, dtype=np.float64)
    mean, sd = stats3[1], math.sqrt(stats3[2] / (stats3[0] - 1.0))
    out = (a - mean) / (sd + 1e-8)
    return out, U * (4 * np.abs(out) + (np.abs(a) + abs(mean)) / sd)


MERGE_R = (1, 2, 3, 8)


def merge_parts(x, R):
    """x split into R ranks with unequal counts; from R = 3 on rank 1 holds nothing (count 0), at R = 8 the last rank as well"""
    x = np.asarray(x).ravel()
    empty = set() if R < 3 else {1} if R == 3 else {1, R - 1}
    live = [r for r in range(R) if r not in empty]
    w = np.array([1.0 + 2.0 * k for k in range(len(live))])
    cuts = np.round(np.cumsum(w) / w.sum() * x.size).astype(int)
    cuts[-1] = x.size
    parts, lo = [], 0
    it = iter(cuts)
    for r in range(R):
        if r in empty:
            parts.append(x[:0])
        else:
            hi = int(next(it))
            parts.append(x[lo:hi]); lo = hi
    return parts


# ------------------------------------------------------------------------------------------------ GAE
GAE_SHAPES = ((1, 1), (2, 63), (33, 65), (5, 130))
GAE_PARAMS = ((0.999, 0.95), (0.99, 0.9), (1.0, 1.0), (0.0, 0.0))


def gae_case(T, E, k):
    """rew, done, value; done is random (p = 0.2) with column 0 always done, column 1 never, column 2 done at t = 0 and column 3 done at
    t = T - 1.  With a single column, k picks the pattern: 0 never done, 1 always done (which is a done at t = 0 and at t = T - 1)."""
    rng = np.random.default_rng([29, T, E, k])
    rew = rng.standard_normal((T, E)).astype(np.float32)
    val = rng.standard_normal((T + 1, E)).astype(np.float32)
    done = (rng.random((T, E)) < 0.2).astype(np.float32)
    if E == 1:
        done[:] = float(k)
    else:
        done[:, 0] = 1.0; done[:, 1] = 0.0
        if E > 3:
            done[0, 2] = 1.0; done[T - 1, 3] = 1.0
    return rew, done, val
