"""Dyadic-grid inputs and exact float64 references for the bf16 conv, conv+pool, pool and residual-block kernels.

The method.  Every operand is a small multiple of a power of two, exactly representable in bf16.  Then every product of a contraction
is a multiple of one unit u (the product of the operands' steps), and if  sum |w||x| + |bias| + |residual| < 2^24 u  for an output
element, every partial sum of it -- in ANY order, on any accumulation tree -- is an integer multiple of u below 2^24 u, hence an fp32
number.  The kernel's fp32 accumulator then holds the mathematically exact value, which float64 torch computes as well, and the stored
output must equal bf16_rne(exact value) with zero tolerance.  A reordered sum can never break such a test; a change to what is computed
or to where it is rounded always does.

assert_exact() is the proof obligation: every reference builder below calls it for every accumulation it contains, with the bound built
by running the same contraction on absolute values.  In a chain the unit shrinks by the weight step at each conv; rounding a multiple of
u to bf16 leaves a multiple of u (a value that needs rounding has more than 8 significant bits above u).

The bounds are evaluated in fp32: a sum of non-negative multiples of u is exact in fp32 while it stays below 2^24 u, and rounding is
monotone, so the fp32 value is below 2^24 u if and only if the true bound is (tests/test_exact_inputs_host.py compares the two).

Rounding points: those of oracle/ppo_oracle_bf16.py, literally -- r16 on a filter bank (a no-op on the grid), a stored activation, a
stored or LDS-handed activation gradient, and the gathered pool-backward sum (not block1's, whose one-hot weight gradient never rounds
it).  Pool ties go to the first maximum (F.max_pool2d's return_indices), as in the oracle."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from update_inputs import DY_ZERO, FLAT_EVERY, SEAMS, UPDATE_N  # noqa: F401  (UPDATE_N re-exported for the tests)

SHAPES = [(3, 16, 64), (16, 16, 32), (16, 32, 32), (32, 32, 16), (32, 32, 8)]
POOL_SHAPES = [(3, 16, 64), (16, 32, 32), (32, 32, 16)]
RES_SHAPES = [(16, 32), (32, 16), (32, 8)]
MAXPOOL_SHAPES = [(64, 16), (32, 32), (16, 32)]         # (hw, channels) of test_maxpool_bf16

# the grids (step, lim): chosen so that the proven bound stays below 2^24 units through four chained convs at 32 channels
X_STEP, X_LIM = 1 / 8, 2.0            # activations
W_STEP, W_LIM, W_ZERO = 1 / 4, 0.5, 0.5         # filters {0, +-1/4, +-1/2}, half of them zero
B_STEP, B_LIM = 1 / 4, 1.0            # biases
FINE_STEP = 1 / 64                    # single convs and pooled gradients: 8 significant bits, so their sums need rounding
G_STEP, G_LIM, G_ZERO = 1 / 2, 1.0, 0.5         # operands of update-sized weight gradients: coarse, so that 2 M terms stay below 2^24
FRAME_BITS, FRAME_BITS_FINE = 5, 6    # block1's frames: the uint8 levels whose bf16(k / 255) is a multiple of 2^-5 (17 levels) / 2^-6 (33)


def r16(t):
    """Round to bf16 (nearest even), keeping the dtype.  Exact values are multiples of u below 2^24 u: float64 -> fp32 is lossless."""
    return t.float().bfloat16().to(t.dtype)


def trunc16(t):
    """Round to bf16 towards zero (a mutation the exact comparison must reject)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def grid(shape, gen, step, lim, p_zero=0.0):
    """float64 tensor of random multiples of `step` in [-lim, lim], a share p_zero of them zeroed."""
    k = int(round(lim / step))
    t = torch.randint(-k, k + 1, tuple(shape), generator=gen).double() * step
    if p_zero:
        t = t * (torch.rand(tuple(shape), generator=gen) >= p_zero)
    return t


def bf16_table():
    """The engine's uint8 -> bf16 table: (float)((double)k / 255.0) rounded to nearest even (engine.hip mi_create, lut16), as float64."""
    return torch.from_numpy((np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)).bfloat16().double()


def exact_levels(bits):
    """The uint8 levels k whose table value bf16(k / 255) is a multiple of 2^-bits."""
    v = bf16_table() * 2.0 ** bits
    return np.flatnonzero((v == v.round()).numpy()).astype(np.uint8)


def assert_exact(bound, unit, what):
    """bound: sum |operands| + |epilogue terms| per output element.  Asserts bound.max() / unit < 2^24 -- every partial sum, in any order,
    is then an fp32 number -- and prints log2 of the ratio, which it returns."""
    ratio = float(bound.max()) / unit
    lg = math.log2(ratio) if ratio > 0 else float("-inf")
    print(f"{what}: bound / unit = 2^{lg:.1f}")
    assert ratio < 2 ** 24, f"{what}: the bound is 2^{lg:.2f} units, not below 2^24: an fp32 partial sum may be inexact"
    return lg


class Tally:
    """What one reference proved and what its inputs exercised: the worst log2 bound / unit, and over every bf16-stored output the
    elements that need rounding at all and those that are exact half-ulp ties; ReLU inputs by branch; pool windows with a tied maximum."""

    def __init__(self, what):
        self.what, self.log2, self.stored, self.rounded, self.ties = what, float("-inf"), 0, 0, 0
        self.relu_pos, self.relu_neg, self.pool_windows, self.pool_ties, self.pool_sampled = 0, 0, 0, 0, False

    def exact(self, bound, unit, name):
        self.log2 = max(self.log2, assert_exact(bound, unit, f"{self.what} {name}"))

    def store(self, v, rnd=r16, where=None):
        """A bf16 store of the exact values v.  where: count only these elements (a pool backward's gathered sums: see gather)."""
        low = v.float().contiguous().view(torch.int32) & 0xFFFF
        if where is not None:
            low = low[where]
        self.stored += low.numel()
        self.rounded += int((low != 0).sum())
        self.ties += int((low == 0x8000).sum())
        return rnd(v)

    def relu(self, x):
        self.relu_pos += int((x > 0).sum())
        self.relu_neg += int((x <= 0).sum())
        return F.relu(x)

    def pool(self, c, sample=12):
        """MaxPool2d(3, 2, 1) with the first maximum's index; ties counted on the first `sample` images of c (a reference at
        update-sized n calls this once per chunk of 256 images: line() says when the figure is such a sample)."""
        q, idx = F.max_pool2d(c, kernel_size=3, stride=2, padding=1, return_indices=True)
        s = c[:sample]
        self.pool_sampled |= c.shape[0] > sample
        win = F.unfold(F.pad(s, (1, 1, 1, 1), value=float("-inf")).flatten(0, 1).unsqueeze(1), 3, stride=2)     # [n*c, 9, windows]
        self.pool_windows += win.shape[0] * win.shape[2]
        self.pool_ties += int(((win == win.max(1, keepdim=True)[0]).sum(1) > 1).sum())
        return q, idx

    def line(self):
        s = f"{self.what}: worst bound / unit 2^{self.log2:.1f}"
        if self.stored:
            s += f"; {self.stored} bf16 stores, {self.rounded} rounded ({100.0 * self.rounded / self.stored:.1f} %), {self.ties} ties ({100.0 * self.ties / self.stored:.1f} %)"
        if self.relu_pos + self.relu_neg:
            s += f"; ReLU inputs {self.relu_pos} > 0, {self.relu_neg} <= 0"
        if self.pool_windows:
            s += f"; {self.pool_ties} of {self.pool_windows} pool windows tied" + (" (sampled: the first 12 images of every 256)" if self.pool_sampled else "")
        return s

    def assert_not_degenerate(self, relu, pool):
        """>= 1 % of the counted bf16 stores are exact ties and >= 25 % need rounding; relu / pool: the case passes through a ReLU (or a
        ReLU mask) / a max pool, and then both ReLU branches / tied pool windows must have occurred."""
        print(self.line())
        assert self.stored and self.ties >= 0.01 * self.stored and self.rounded >= 0.25 * self.stored, self.line()
        assert (self.relu_pos > 0 and self.relu_neg > 0) if relu else (self.relu_pos + self.relu_neg == 0), self.line()
        assert (self.pool_ties > 0) if pool else (self.pool_windows == 0), self.line()


# ------------------------------------------------------------------ contractions (3x3, pad 1) and their bounds

def conv(x, w, b=None):
    return F.conv2d(x, w, b, padding=1)


def convT(d, w):
    """Data gradient of conv: the transposed 3x3 conv."""
    return F.conv2d(d, w.transpose(0, 1).flip(2, 3), padding=1)


def _b32(*ts):
    return [t.abs().float() for t in ts]


def wgrad(x, dy, chunk=64):
    """Weight and bias gradient of a 3x3 / pad 1 conv in x's dtype: sum over images and pixels of dy x unfold(x), in chunks."""
    n, cin = x.shape[:2]
    cout = dy.shape[1]
    acc = torch.zeros(cout, cin * 9, dtype=x.dtype)
    for k in range(0, n, chunk):
        u = F.unfold(x[k:k + chunk], 3, padding=1)
        acc += torch.einsum("nop,nkp->ok", dy[k:k + chunk].flatten(2), u)
    return acc.view(cout, cin, 3, 3), dy.sum(dim=(0, 2, 3))


def wgrad_bounds(x, dy, unit_x, unit_dy, tally, name):
    """The proof for both sums of a weight / bias gradient."""
    bw, bb = wgrad(*_b32(x, dy))
    tally.exact(bw.double(), unit_x * unit_dy, f"{name} weight gradient")
    tally.exact(bb.double(), unit_dy, f"{name} bias gradient")


def wgrad_exact(x, dy, unit_x, unit_dy, tally, name):
    """(dW, db) of a conv from its input x and output gradient dy, with the proof for both sums."""
    wgrad_bounds(x, dy, unit_x, unit_dy, tally, name)
    return wgrad(x, dy.to(x.dtype))


def pool_scatter(dy, idx, shape):
    """MaxPool2d backward: every pooled gradient to its window's arg-max, contributions summed."""
    dc = torch.zeros(shape[0], shape[1], shape[2] * shape[3], dtype=dy.dtype)
    dc.scatter_add_(2, idx.flatten(2), dy.flatten(2))
    return dc.reshape(shape)


def gather(dq, idx, shape, unit_d, tally, dt=torch.float64, rnd=r16, mutant=None):
    """MaxPool2d backward as the kernels stage it (PoolStage::gather in conv_bf16.hip, maxpool_bwd_bf16 in pool.hip): the <= 4 pooled
    gradients that reach an element are summed in fp32 and the SUM is rounded once (rnd=None: block1's one-hot weight gradient, which
    never rounds it).  An element that a single gradient reaches holds a bf16 number already, so the rounded and tie shares are counted
    over the elements where two or more gradients meet: only there can the rounding point show.  mutant: a wrong gather (host test)."""
    if mutant is not None:
        return mutant(dq.to(dt), idx, shape)
    tally.exact(pool_scatter(dq.abs().float(), idx, shape).double(), unit_d, "pool-backward gather")
    meet = pool_scatter(torch.ones_like(dq, dtype=torch.float32), idx, shape) >= 2
    return tally.store(pool_scatter(dq.to(dt), idx, shape), rnd if rnd is not None else (lambda v: v), where=meet)


def pooled_gradient(shape, gen):
    """A pooled gradient on the fine grid whose sums need rounding: magnitudes 128 .. 255 units of 1/64 (every 8-bit significand with
    the top bit set) and one sign per (image, channel), so that two gradients that meet always leave the 8 bits of a bf16 number."""
    mag = torch.randint(128, 256, tuple(shape), generator=gen).double() * FINE_STEP
    return mag * (torch.randint(0, 2, tuple(shape[:2]) + (1, 1), generator=gen) * 2 - 1).double()


# ------------------------------------------------------------------ references.  Inputs: float64 tensors on the grids (NCHW); dt: the dtype
# the contractions run in (float64 for the reference; float32 in the host test that proves fp32 == float64)

def ref_conv_forward(x, w, b, res, relu, unit_x, tally, dt=torch.float64, rnd=r16):
    """op_conv3x3 mode 0: out = r16(conv(relu?(x), r16(w)) + b + res): bias, ReLU and residual in fp32, one rounding at the store."""
    x, w, b = x.to(dt), r16(w.to(dt)), b.to(dt)
    xin = tally.relu(x) if relu else x
    v = conv(xin, w, b)
    bound = conv(*_b32(xin, w), b.abs().float())
    if res is not None:
        v = v + res.to(dt)
        bound = bound + res.abs().float()
    tally.exact(bound.double(), unit_x * W_STEP, "conv + bias + residual")
    return tally.store(v, rnd)


def ref_conv_dgrad(dout, w, mask, skip, unit_d, tally, dt=torch.float64, rnd=r16):
    """op_conv3x3 mode 1: din = r16(convT(dout, r16(w)) * (mask > 0) + skip)."""
    dout, w = dout.to(dt), r16(w.to(dt))
    tally.relu(mask)
    tally.exact((convT(*_b32(dout, w)) + skip.abs().float()).double(), unit_d * W_STEP, "transposed conv + skip")
    return tally.store(convT(dout, w) * (mask.to(dt) > 0) + skip.to(dt), rnd)


def ref_conv_wgrad(x, dout, relu, unit_x, unit_d, tally, dt=torch.float64):
    """op_conv3x3 mode 2: (dW, db) in fp32, never rounded to bf16."""
    x = x.to(dt)
    return wgrad_exact(tally.relu(x) if relu else x, dout.to(dt), unit_x, unit_d, tally, "conv")


def ref_conv_pool(x, w, b, unit_x, tally, dt=torch.float64, rnd=r16, count=True):
    """op_conv3x3 mode 3: c = r16(conv(x, r16(w)) + b), rounded BEFORE the pool; q = MaxPool2d(3, 2, 1)(c).  -> (q, idx, c.shape)
    count=False: c is not an output of the case (the weight-gradient modes re-run the forward for its arg-max only)."""
    x, w, b = x.to(dt), r16(w.to(dt)), b.to(dt)
    tally.exact(conv(*_b32(x, w), b.abs().float()).double(), unit_x * W_STEP, "conv + bias")
    c = tally.store(conv(x, w, b), rnd) if count else rnd(conv(x, w, b))
    q, idx = tally.pool(c)
    return q, idx, c.shape


def ref_maxpool(x, dq, unit_d, tally, dt=torch.float64, rnd=r16, mutant=None):
    """op_maxpool: mode 0 q = MaxPool2d(3, 2, 1)(x); mode 1 dx = r16(the scatter sum of dq)."""
    x = x.to(dt)
    q, idx = tally.pool(x)
    return q, gather(dq, idx, x.shape, unit_d, tally, dt, rnd, mutant)


def ref_resblock_forward(x, w1, b1, w2, b2, unit_x, tally, dt=torch.float64, rnd=r16):
    """op_resblock mode 0: a = r16(conv1(relu(x)) + b1), y = r16(conv2(relu(a)) + b2 + x)."""
    a = ref_conv_forward(x, w1, b1, None, True, unit_x, tally, dt, rnd)
    y = ref_conv_forward(a, w2, b2, x, True, unit_x * W_STEP, tally, dt, rnd)
    return a, y


def ref_resblock_backward(dy, w1, w2, a, x, unit_d, tally, dt=torch.float64, rnd=r16):
    """op_resblock mode 1: da = r16(convT2(dy) * (a > 0)) (handed on through LDS as bf16), dx = r16(convT1(da) * (x > 0) + dy)."""
    da = ref_conv_dgrad(dy, w2, a, torch.zeros_like(a), unit_d, tally, dt, rnd)
    dx = ref_conv_dgrad(da, w1, x, dy, unit_d * W_STEP, tally, dt, rnd)
    return da, dx


def ref_pair(x, W, B, unit_x, tally, dt=torch.float64, rnd=r16):
    """op_resblock mode 4: res1 + res2 with four distinct convs; A1, P1, A2, P2 each rounded once at its store."""
    a1, p1 = ref_resblock_forward(x, W[0], B[0], W[1], B[1], unit_x, tally, dt, rnd)
    a2, p2 = ref_resblock_forward(p1, W[2], B[2], W[3], B[3], unit_x * W_STEP ** 2, tally, dt, rnd)
    return a1, p1, a2, p2


def chunked(fn, n, chunk=256):
    """fn(lo, hi) -> tuple of per-image tensors; concatenated over chunks of images (the float64 references at update-sized n)."""
    parts = [fn(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(len(parts[0])))


# ------------------------------------------------------------------ inputs

def hard_grid_images(x, step, last=8):
    """hard_images of update_inputs.py, staying on the grid: images at SEAMS all negative, every FLAT_EVERY-th image with a flat band
    (pool ties, a carried row of equal keys), the last image scaled by 8 (`last`)."""
    x = x.clone()
    n, _, hw, _ = x.shape
    for j in SEAMS:
        if j < n - 1:
            x[j] = -x[j].abs() - step
    for j in range(1, n - 1, FLAT_EVERY):
        x[j, :, hw // 4 - 2:hw // 2 + 3, :] = x[j, :, :1, :1]
    if n >= 1024:
        x[-1] *= last
    return x


def hard_grid_frames(x_u8, levels):
    """hard_frames on the exact levels: black frames at SEAMS, a flat band every FLAT_EVERY-th frame, the last frame saturated."""
    x_u8 = x_u8.copy()
    n = x_u8.shape[0]
    for j in SEAMS:
        if j < n - 1:
            x_u8[j] = 0
    for j in range(1, n - 1, FLAT_EVERY):
        x_u8[j, 14:35] = levels[len(levels) // 2]
    if n >= 1024:
        x_u8[-1] = 255
    return x_u8


def hard_grid_dy(dy):
    dy = dy.clone()
    if dy.shape[0] > DY_ZERO:
        dy[DY_ZERO] = 0
    return dy


def filters(cout, cin, gen, lim=W_LIM, p_zero=W_ZERO):
    return grid((cout, cin, 3, 3), gen, W_STEP, lim, p_zero), grid((cout,), gen, B_STEP, B_LIM)


def conv_inputs(cin, cout, hw, n, seed, step=X_STEP, lim=X_LIM, bits=FRAME_BITS):
    # (block1's 27-tap sums on the fine frames get dense filters up to +-1: a quarter of its outputs need rounding only then)
    """-> (w, b, what the engine takes (uint8 NHWC frames for block1, else fp32 NHWC), x as float64 NCHW, x's unit)."""
    g = torch.Generator().manual_seed(seed)
    w, b = filters(cout, cin, g, *((1.0, 0.0) if cin == 3 and bits == FRAME_BITS_FINE else ()))
    if cin == 3:
        lv = exact_levels(bits)
        x_u8 = lv[torch.randint(0, len(lv), (n, hw, hw, 3), generator=g).numpy()]
        if n >= 1024:
            x_u8 = hard_grid_frames(x_u8, lv)
        x = bf16_table()[torch.from_numpy(x_u8.astype(np.int64))].permute(0, 3, 1, 2).contiguous()
        return w, b, x_u8, x, 2.0 ** -bits
    x = grid((n, cin, hw, hw), g, step, lim)
    if n >= 1024:
        x = hard_grid_images(x, step)
    return w, b, nhwc(x), x, step


def nhwc(t):
    """NCHW -> the engine's NHWC fp32 array.  Everything that goes to the engine is a bf16 number, so that no upload rounds."""
    assert torch.equal(r16(t), t), "an input off the bf16 grid"
    return _nhwc(t)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().numpy()


def w32(t):
    assert torch.equal(r16(t), t), "a filter or bias off the bf16 grid"
    return t.float().numpy()


def describe_mismatch(out, ref_exact, ref, what):
    """out, ref: NHWC arrays (kernel, r16 of the exact value); ref_exact: the exact values (or None for fp32 outputs).  The message the
    GPU tests fail with: the first differing element, the share of differing elements, and whether the kernel's value is the other bf16
    neighbour of the exact value (a rounding-rule problem) or further away (an arithmetic problem)."""
    out, ref = np.asarray(out), np.asarray(ref)
    bad = np.argwhere(out != ref)
    if len(bad) == 0:
        return f"{what}: equal"
    i = tuple(bad[0])
    msg = f"{what}: {len(bad)} of {out.size} elements differ ({100.0 * len(bad) / out.size:.3f} %); first at index {i}"
    msg += " (image, y, x, channel)" if out.ndim == 4 else ""
    msg += f": kernel {float(out[i])!r}, reference {float(ref[i])!r}"
    if ref_exact is not None:
        e = float(np.asarray(ref_exact)[i])
        lo, hi = float(trunc16(torch.tensor([e]))[0]), None
        ulp = 2.0 ** (math.floor(math.log2(abs(e))) - 7) if e else 0.0
        hi = lo + math.copysign(ulp, e)
        kind = "the other bf16 neighbour of the exact value: a rounding-rule problem" if float(out[i]) in (lo, hi) else "further away than the bf16 neighbours: an arithmetic problem"
        msg += f", exact {e!r} -- {kind}"
    return msg


# ------------------------------------------------------------------ the cases: one object per (kernel family, shape, n), shared by
# tests/test_exact_inputs_host.py (fp32 == float64, the proofs, non-degenerate inputs) and tests/test_gpu_bf16_exact.py (the kernels)

class Recorder:
    """A rounding function that keeps the exact value of every bf16 store, in store order (for the mismatch report)."""

    def __init__(self):
        self.v = []

    def __call__(self, v):
        self.v.append(v.float())
        return r16(v)


class Case:
    """what: the printed name.  ref(dt, tally, rnd) -> {output name: tensor} (activations NCHW, gradients in the reference layout);
    run(eng) -> {output name: array as the engine returns it}; stores: the names of ref's bf16 stores per chunk of images, in order;
    relu / pool: the case passes through a ReLU / a max pool; strict: the inputs must meet Tally.assert_not_degenerate (exempt: mode 2,
    which stores no bf16 value, and the update-sized weight-gradient cases, whose coarse grid a 2 M-term sum dictates -- the same
    launchers' roundings are exercised at n <= 12); bounds(tally): the weight-gradient proofs alone, in float32 (update-sized cases)."""

    def __init__(self, what, ref, run, stores, relu, pool, strict=True, bounds=None):
        self.what, self.ref, self.run, self.stores, self.relu, self.pool, self.strict, self.bounds = what, ref, run, stores, relu, pool, strict, bounds


def _g(seed):
    return torch.Generator().manual_seed(seed)


def case_conv_forward(cin, cout, hw, n):
    """Mode 0 with ReLU in, bias and residual (block1.conv: uint8 frames, no ReLU, no residual)."""
    w, b, x_dev, x, ux = conv_inputs(cin, cout, hw, n, 1, FINE_STEP, bits=FRAME_BITS_FINE)
    relu = cin != 3
    res = grid((n, cout, hw, hw), _g(2), FINE_STEP, X_LIM) if relu else None
    ref = lambda dt=torch.float64, tally=None, rnd=r16: {"out": ref_conv_forward(x, w, b, res, relu, ux, tally, dt, rnd)}
    run = lambda eng: {"out": eng.op_conv3x3(0, cin, cout, hw, w32(w), inp=x_dev, relu_in=relu, bias=w32(b), res=nhwc(res) if relu else None)}
    return Case(f"conv forward ({cin},{cout},{hw}) n={n}", ref, run, ["out"], relu=relu, pool=False)


def case_conv_dgrad(cin, cout, hw, n):
    """Mode 1 with mask and skip."""
    w, _, _, x, _ = conv_inputs(cin, cout, hw, n, 3)
    g = _g(4)
    dout, skip = grid((n, cout, hw, hw), g, FINE_STEP, X_LIM), grid((n, cin, hw, hw), g, FINE_STEP, X_LIM)
    ref = lambda dt=torch.float64, tally=None, rnd=r16: {"din": ref_conv_dgrad(dout, w, x, skip, FINE_STEP, tally, dt, rnd)}
    run = lambda eng: {"din": eng.op_conv3x3(1, cin, cout, hw, w32(w), dout=nhwc(dout), mask=nhwc(x), res=nhwc(skip))}
    return Case(f"conv data gradient ({cin},{cout},{hw}) n={n}", ref, run, ["din"], relu=True, pool=False)


def case_conv_wgrad(cin, cout, hw, n):
    """Mode 2: fp32 outputs, no bf16 store."""
    w, _, x_dev, x, ux = conv_inputs(cin, cout, hw, n, 5)
    relu = cin != 3
    dout = grid((n, cout, hw, hw), _g(6), G_STEP, G_LIM, G_ZERO)

    def ref(dt=torch.float64, tally=None, rnd=r16):
        dw, db = ref_conv_wgrad(x, dout, relu, ux, G_STEP, tally, dt)
        return {"dW": dw, "db": db}

    def run(eng):
        dw, db = eng.op_conv3x3(2, cin, cout, hw, w32(w), inp=x_dev, relu_in=relu, dout=nhwc(dout))
        return {"dW": dw, "db": db}
    return Case(f"conv weight gradient ({cin},{cout},{hw}) n={n}", ref, run, [], relu=relu, pool=False, strict=False)


def case_conv_pool(cin, cout, hw, n):
    """Mode 3 (the pooled map) and the data gradient from a pooled gradient (modes 5 and 7) on fine grids, where conv outputs, gathered
    sums and data gradients need rounding."""
    w, b, x_dev, x, ux = conv_inputs(cin, cout, hw, n, 21, FINE_STEP, bits=FRAME_BITS_FINE)
    dq = hard_grid_dy(pooled_gradient((n, cout, hw // 2, hw // 2), _g(22)))
    block1 = cin == 3

    def part(lo, hi, dt, tally, rnd):
        q, idx, cs = ref_conv_pool(x[lo:hi], w, b, ux, tally, dt, rnd)
        if block1:
            return (q,)
        dc = gather(dq[lo:hi], idx, cs, FINE_STEP, tally, dt, rnd)
        tally.exact(convT(*_b32(dc, w)).double(), FINE_STEP * W_STEP, "transposed conv")
        return q, tally.store(convT(dc, r16(w.to(dt))), rnd)

    def ref(dt=torch.float64, tally=None, rnd=r16):
        out = chunked(lambda lo, hi: part(lo, hi, dt, tally, rnd), n)
        return {"pooled": out[0]} if block1 else {"pooled": out[0], "dx": out[1], "dx fused": out[1]}

    def run(eng):
        out = {"pooled": eng.op_conv3x3(3, cin, cout, hw, w32(w), inp=x_dev, bias=w32(b))}
        if not block1:
            for m, k in ((5, "dx"), (7, "dx fused")):
                out[k] = eng.op_conv3x3(m, cin, cout, hw, w32(w), inp=x_dev, bias=w32(b), dout=nhwc(dq))
        return out
    return Case(f"conv + pool ({cin},{cout},{hw}) n={n}", ref, run, ["c"] if block1 else ["c", "dc", "dx"], relu=False, pool=True)


def case_conv_pool_wgrad(cin, cout, hw, n):
    """Modes 4 and 6: dW and db from a pooled gradient; block1's one-hot form never rounds the gathered sum, block2 / block3 round it
    once.  x in multiples of 1/2 ({0, 191, 255} frames for block1).  n <= 12: the pooled gradient on the fine grid, so that the gathered
    sums leave bf16 and the rounding point (or, for block1, its absence) decides bits of dW; the case is strict on those sums.
    n >= 1024: the pooled gradient in multiples of 1/2 as well -- 2051 * hw^2 terms per element have to stay below 2^24 units."""
    g = _g(23)
    w, b = filters(cout, cin, g)
    block1, big = cin == 3, n >= 1024
    if block1:
        lv = exact_levels(2)
        x_dev = lv[torch.randint(0, len(lv), (n, hw, hw, 3), generator=g).numpy()]
        if big:
            x_dev = hard_grid_frames(x_dev, lv)
        x, ux = bf16_table()[torch.from_numpy(x_dev.astype(np.int64))].permute(0, 3, 1, 2).contiguous(), 0.25
    else:
        x, ux = grid((n, cin, hw, hw), g, G_STEP, G_LIM), G_STEP
        if big:
            x = hard_grid_images(x, G_STEP)
        x_dev = nhwc(x)
    ud = G_STEP if big else FINE_STEP
    dq = hard_grid_dy(grid((n, cout, hw // 2, hw // 2), g, G_STEP, G_LIM, G_ZERO)) if big else pooled_gradient((n, cout, hw // 2, hw // 2), g)

    def gathered(dt, tally, rnd, mutant=None):
        def part(lo, hi):
            _, idx, cs = ref_conv_pool(x[lo:hi], w, b, ux, tally, dt, rnd, count=False)
            return (gather(dq[lo:hi], idx, cs, ud, tally, dt, None if block1 else rnd, mutant),)
        return chunked(part, n)[0]

    def ref(dt=torch.float64, tally=None, rnd=r16, mutant=None):
        dw, db = wgrad_exact(x.to(dt), gathered(dt, tally, rnd, mutant), ux, ud, tally, "conv from the pooled gradient")
        return {"dW": dw, "db": db} if block1 else {"dW": dw, "db": db, "dW fused": dw, "db fused": db}

    def bounds(tally):
        wgrad_bounds(x, gathered(torch.float32, tally, r16), ux, ud, tally, "conv from the pooled gradient")

    def run(eng):
        out = {}
        for m, k in ((4, ""),) + (() if block1 else ((6, " fused"),)):
            out["dW" + k], out["db" + k] = eng.op_conv3x3(m, cin, cout, hw, w32(w), inp=x_dev, bias=w32(b), dout=nhwc(dq))
        return out
    return Case(f"conv + pool weight gradient ({cin},{cout},{hw}) n={n}", ref, run, ["c"] if block1 else ["c", "dc"], relu=False, pool=True,
                strict=not big, bounds=bounds)


def case_maxpool(hw, c):
    """op_maxpool modes 0 and 1 on test_maxpool_bf16's three images: random, integers (ties), half of the image flat.  The random image
    is raised into (2, 4) at odd rows and columns, the elements that four windows share: their maxima collect up to four gradients,
    and a sum of 8-bit gradients needs rounding."""
    g = _g(hw)
    x = grid((3, c, hw, hw), g, FINE_STEP, X_LIM)
    x[0, :, 1::2, 1::2] = 3 + grid((c, hw // 2, hw // 2), g, FINE_STEP, 63 / 64)
    x[1] = torch.round(x[1])
    x[2, :, : hw // 2] = 0.25
    dq = pooled_gradient((3, c, hw // 2, hw // 2), g)

    def ref(dt=torch.float64, tally=None, rnd=r16, mutant=None):
        q, dx = ref_maxpool(x, dq, FINE_STEP, tally, dt, rnd, mutant)
        return {"pooled": q, "dx": dx}
    run = lambda eng: {"pooled": eng.op_maxpool(0, nhwc(x)), "dx": eng.op_maxpool(1, nhwc(x), dout=nhwc(dq))}
    return Case(f"max pool {c}@{hw}", ref, run, ["dx"], relu=False, pool=True)


RES_STEP = 1 / 32           # single residual block, forward and data gradients: fine enough that conv1's output needs rounding too


def _res_filters(ch, g, k):
    fb = [filters(ch, ch, g) for _ in range(k)]
    return [w for w, _ in fb], [b for _, b in fb]


def case_resblock_forward(ch, hw, n):
    g = _g(100 + ch + hw)
    W, B = _res_filters(ch, g, 2)
    x = grid((n, ch, hw, hw), g, RES_STEP, X_LIM)

    def ref(dt=torch.float64, tally=None, rnd=r16):
        a, y = ref_resblock_forward(x, W[0], B[0], W[1], B[1], RES_STEP, tally, dt, rnd)
        return {"a": a, "y": y}

    def run(eng):
        a, y = eng.op_resblock(0, nhwc(x), w32(W[0]), w32(W[1]), b1=w32(B[0]), b2=w32(B[1]))
        return {"a": a, "y": y}
    return Case(f"residual block {ch}@{hw} n={n} forward", ref, run, ["a", "y"], relu=True, pool=False)


def case_resblock_backward(ch, hw, n):
    g = _g(200 + ch + hw)
    W, _ = _res_filters(ch, g, 2)
    x, a = grid((n, ch, hw, hw), g, X_STEP, X_LIM), grid((n, ch, hw, hw), g, X_STEP, X_LIM)
    dy = grid((n, ch, hw, hw), g, RES_STEP, X_LIM)

    def ref(dt=torch.float64, tally=None, rnd=r16):
        da, dx = ref_resblock_backward(dy, W[0], W[1], a, x, RES_STEP, tally, dt, rnd)
        return {"da": da, "dx": dx}

    def run(eng):
        da, dx = eng.op_resblock(1, nhwc(dy), w32(W[0]), w32(W[1]), a_fwd=nhwc(a), x_fwd=nhwc(x))
        return {"da": da, "dx": dx}
    return Case(f"residual block {ch}@{hw} n={n} data gradients", ref, run, ["da", "dx"], relu=True, pool=False)


def case_resblock_whole_backward(ch, hw, n):
    """Mode 2: dx and both weight / bias gradients from one launch.  n <= 7: dy on the fine grid; update-sized n: every operand on the
    coarse grid, so that conv1's weight gradient -- 2051 * hw^2 products of relu(x) with the bf16 da -- stays below 2^24 units."""
    g = _g(77)
    W, _ = _res_filters(ch, g, 2)
    big = n >= 1024
    sx, sd = (G_STEP, G_STEP) if big else (X_STEP, RES_STEP)
    lim = G_LIM if big else X_LIM
    x, a = grid((n, ch, hw, hw), g, sx, lim), grid((n, ch, hw, hw), g, sx, lim)
    dy = grid((n, ch, hw, hw), g, sd, lim, G_ZERO if big else 0.0)
    if big:
        x, a, dy = hard_grid_images(x, sx), hard_grid_images(a, sx), hard_grid_dy(dy)

    def ref(dt=torch.float64, tally=None, rnd=r16):
        da, dx = chunked(lambda lo, hi: ref_resblock_backward(dy[lo:hi], W[0], W[1], a[lo:hi], x[lo:hi], sd, tally, dt, rnd), n)
        dw2, db2 = wgrad_exact(F.relu(a.to(dt)), dy.to(dt), sx, sd, tally, "conv2")
        dw1, db1 = wgrad_exact(F.relu(x.to(dt)), da, sx, sd * W_STEP, tally, "conv1")
        return {"dx": dx, "dW1": dw1, "db1": db1, "dW2": dw2, "db2": db2}

    def bounds(tally):
        f32 = torch.float32
        da, = chunked(lambda lo, hi: (ref_conv_dgrad(dy[lo:hi], W[1], a[lo:hi], torch.zeros_like(a[lo:hi]), sd, tally, f32),), n)
        wgrad_bounds(F.relu(a), dy, sx, sd, tally, "conv2")
        wgrad_bounds(F.relu(x), da, sx, sd * W_STEP, tally, "conv1")

    def run(eng):
        flat, dx = eng.op_resblock(2, nhwc(dy), w32(W[0]), w32(W[1]), a_fwd=nhwc(a), x_fwd=nhwc(x))
        flat, wl = flat.ravel(), ch * ch * 9
        return {"dx": dx, "dW1": flat[:wl].reshape(ch, ch, 3, 3), "db1": flat[wl:wl + ch],
                "dW2": flat[wl + ch:2 * wl + ch].reshape(ch, ch, 3, 3), "db2": flat[2 * wl + ch:2 * wl + 2 * ch]}
    return Case(f"residual block {ch}@{hw} n={n} whole backward", ref, run, ["da", "dx"], relu=True, pool=False, strict=not big, bounds=bounds)


def case_pair(ch, hw, n):
    """Mode 4: four distinct convs, A1, P1, A2 and P2 stored.  Update-sized n: the last image is scaled by 4, not 8 -- the chain's bound
    is 2^21 units at 32@16 on the plain grid, and three more bits do not fit below 2^24."""
    g = _g(500 + ch + hw)
    W, B = _res_filters(ch, g, 4)
    x = grid((n, ch, hw, hw), g, X_STEP, X_LIM)
    if n >= 1024:
        x = hard_grid_images(x, X_STEP, last=4)

    def ref(dt=torch.float64, tally=None, rnd=r16):
        a1, p1, a2, p2 = chunked(lambda lo, hi: ref_pair(x[lo:hi], W, B, X_STEP, tally, dt, rnd), n)
        return {"A1": a1, "P1": p1, "A2": a2, "P2": p2}

    def run(eng):
        oa, oy = eng.op_resblock(4, nhwc(x), torch.stack(W[:2]).float().numpy(), torch.stack(W[2:]).float().numpy(),
                                 b1=torch.cat(B[:2]).float().numpy(), b2=torch.cat(B[2:]).float().numpy())
        return {"A1": oa[0], "P1": oy[0], "A2": oa[1], "P2": oy[1]}
    return Case(f"residual pair {ch}@{hw} n={n}", ref, run, ["A1", "P1", "A2", "P2"], relu=True, pool=False)


def evaluate(case, dt=torch.float64):
    """-> ({name: array in the engine's layout}, {name: exact values of the bf16 outputs, same layout}, tally)"""
    tally, rec = Tally(case.what), Recorder()
    ref = case.ref(dt, tally, rec)
    k = len(case.stores)
    exact = {}
    for i, name in enumerate(case.stores):
        if name in ref:
            exact[name] = _nhwc(torch.cat(rec.v[i::k]))
    for name in list(exact):
        if name + " fused" in ref:
            exact[name + " fused"] = exact[name]
    out = {name: (_nhwc(t) if t.ndim == 4 and t.shape[2:] != (3, 3) else t.float().numpy()) for name, t in ref.items()}
    return out, exact, tally


def check_case(case, eng):
    """The GPU comparison: every output of the kernels equal to the float64 reference on all elements."""
    ref, exact, tally = evaluate(case)
    out = case.run(eng)
    print(tally.line())
    assert set(out) == set(ref)
    bad = []
    for name in ref:
        assert out[name].shape == ref[name].shape, (case.what, name, out[name].shape, ref[name].shape)
        if not np.array_equal(out[name], ref[name]):
            bad.append(describe_mismatch(out[name], exact.get(name), ref[name], f"{case.what}: {name}"))
            print(bad[-1])
    assert not bad, "\n".join(bad)


# every case of tests/test_gpu_bf16_exact.py: family -> (builder, [arguments]).  Small n is {1, 5}, 6 for the pair, 12 for conv + pool;
# update-sized n only where the launcher changes kernel or runs several items per workgroup
FAMILIES = {
    "conv_forward": (case_conv_forward, [s + (n,) for s in SHAPES for n in (1, 5)]),
    "conv_dgrad": (case_conv_dgrad, [s + (n,) for s in SHAPES[1:] for n in (1, 5)]),
    "conv_wgrad": (case_conv_wgrad, [s + (n,) for s in SHAPES for n in (1, 37)]),
    "conv_pool": (case_conv_pool, [s + (n,) for s in POOL_SHAPES for n in [1, 12] + UPDATE_N]),
    "conv_pool_wgrad": (case_conv_pool_wgrad, [s + (n,) for s in POOL_SHAPES for n in [1, 12] + UPDATE_N]),
    "maxpool": (case_maxpool, list(MAXPOOL_SHAPES)),
    "resblock_forward": (case_resblock_forward, [s + (n,) for s in RES_SHAPES for n in (1, 5)]),
    "resblock_backward": (case_resblock_backward, [s + (n,) for s in RES_SHAPES for n in (1, 5)]),
    "resblock_whole_backward": (case_resblock_whole_backward, [s + (n,) for s in RES_SHAPES for n in [1, 7] + UPDATE_N]),
    "pair": (case_pair, [s + (n,) for s in RES_SHAPES for n in [1, 6] + UPDATE_N]),
}


def cases(update_sized):
    """[(family, arguments)] of the small cases (update_sized False) or of the update-sized ones."""
    return [(f, a) for f, (_, args) in FAMILIES.items() for a in args if (f != "maxpool" and a[-1] >= 1024) == update_sized]
