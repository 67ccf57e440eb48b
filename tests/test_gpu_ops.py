"""Kernel-level parity (MI355X): each HIP op through the C ABI against plain PyTorch-CPU fp32.
Tolerances: the MFMA path is an exact-fp32 fmaf chain; only the summation order differs from
torch's CPU kernels, so 1e-4 relative to the tensor's scale is generous."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from update_inputs import batches, check_per_image, check_wgrad, frames_to_nchw, hard_dy, hard_frames, hard_images, wgrad64

pytestmark = pytest.mark.gpu

SHAPES = [(3, 16, 64), (16, 16, 32), (16, 32, 32), (32, 32, 16), (32, 32, 8)]


@pytest.fixture(scope="module")
def eng():
    from mi355.engine import Engine
    e = Engine("impala", n_steps=4, n_envs=4, n_actions=15, max_batch=16)
    yield e
    e.close()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def relerr(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def test_mfma_operand_maps(eng):
    assert eng.selftest_mfma() == 0.0


@pytest.mark.parametrize("M,N,K,ta,tb", [(70, 50, 33, False, False), (128, 256, 2048, False, True),
                                         (16, 256, 4096, True, False), (256, 9, 300, True, False), (5, 3, 2, False, True)])
def test_gemm(eng, M, N, K, ta, tb):
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
    B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    ref = (A.T if ta else A).astype(np.float64) @ (B.T if tb else B).astype(np.float64)
    out = eng.op_gemm(A, B, ta, tb)
    assert relerr(out, ref) < 1e-5


def _n(n, hw):
    """Update-sized launches (n = 2051) run >= 2 work items on every workgroup of the fp32 kernels, except at 32 channels @8x8,
    whose items are 2 images: 1026 items on up to 1024 workgroups.  There 4099 images (>= 2050 items) are used instead."""
    return 4099 if n == 2051 and hw == 8 else n


def _conv_inputs(cin, cout, hw, n, seed):
    """Update-sized n (>= 1024) get the hard images of update_inputs.py."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    if cin == 3:
        x_u8 = torch.randint(0, 256, (n, hw, hw, 3), generator=g, dtype=torch.uint8).numpy()
        if n >= 1024:
            x_u8 = hard_frames(x_u8)
        return w, b, x_u8, frames_to_nchw(x_u8)
    x = torch.randn(n, cin, hw, hw, generator=g)
    if n >= 1024:
        x = hard_images(x, bf16=False)
    return w, b, nhwc(x), x


@pytest.mark.parametrize("cin,cout,hw", SHAPES)
@pytest.mark.parametrize("n", [1, 5, 2051])
def test_conv_forward(eng, cin, cout, hw, n):
    n = _n(n, hw)
    w, b, x_dev, x = _conv_inputs(cin, cout, hw, n, 1)
    relu = cin != 3
    res = torch.randn(n, cout, hw, hw, generator=torch.Generator().manual_seed(2))
    ref = F.conv2d(F.relu(x) if relu else x, w, b, padding=1) + res
    out = eng.op_conv3x3(0, cin, cout, hw, w.numpy(), inp=x_dev, relu_in=relu, bias=b.numpy(), res=nhwc(res))
    assert relerr(out, nhwc(ref)) < 1e-5
    check_per_image(out, nhwc(ref), f"fp32 conv ({cin},{cout},{hw}) n={n} forward", 1e-4)
    out2 = eng.op_conv3x3(0, cin, cout, hw, w.numpy(), inp=x_dev, relu_in=False, bias=None)
    ref2 = nhwc(F.conv2d(x, w, None, padding=1))
    assert relerr(out2, ref2) < 1e-5
    check_per_image(out2, ref2, f"fp32 conv ({cin},{cout},{hw}) n={n} forward without ReLU / bias / residual", 1e-4)


@pytest.mark.parametrize("cin,cout,hw", SHAPES[1:])
@pytest.mark.parametrize("n", [1, 5, 2051])
def test_conv_dgrad(eng, cin, cout, hw, n):
    n = _n(n, hw)
    w, _, _, x = _conv_inputs(cin, cout, hw, n, 3)
    g = torch.Generator().manual_seed(4)
    dout = torch.randn(n, cout, hw, hw, generator=g)
    skip = torch.randn(n, cin, hw, hw, generator=g)
    if n >= 1024:
        dout = hard_dy(dout)
    din = torch.nn.grad.conv2d_input(x.shape, w, dout, padding=1)
    ref = din * (x > 0) + skip
    out = eng.op_conv3x3(1, cin, cout, hw, w.numpy(), dout=nhwc(dout), mask=nhwc(x), res=nhwc(skip))
    assert relerr(out, nhwc(ref)) < 1e-5
    check_per_image(out, nhwc(ref), f"fp32 conv ({cin},{cout},{hw}) n={n} data gradient, masked + skip", 1e-4)
    out2 = eng.op_conv3x3(1, cin, cout, hw, w.numpy(), dout=nhwc(dout))
    assert relerr(out2, nhwc(din)) < 1e-5
    check_per_image(out2, nhwc(din), f"fp32 conv ({cin},{cout},{hw}) n={n} data gradient", 1e-4)


@pytest.mark.parametrize("cin,cout,hw", SHAPES)
@pytest.mark.parametrize("n", [1, 5, 37, 2051])
def test_conv_wgrad(eng, cin, cout, hw, n):
    """Against float64 sums.  n = 2051 (4099 @8x8): several images per workgroup, accumulators carried across them."""
    n = _n(n, hw)
    w, _, x_dev, x = _conv_inputs(cin, cout, hw, n, 5)
    relu = cin != 3
    dout = torch.randn(n, cout, hw, hw, generator=torch.Generator().manual_seed(6))
    if n >= 1024:
        dout = hard_dy(dout)
    xin = F.relu(x) if relu else x
    ref_w, ref_b = wgrad64(xin, dout)
    gw, gb = eng.op_conv3x3(2, cin, cout, hw, w.numpy(), inp=x_dev, relu_in=relu, dout=nhwc(dout))
    check_wgrad(gw, gb, ref_w, ref_b, f"fp32 conv ({cin},{cout},{hw}) n={n} weight gradient", 2e-5)


@pytest.mark.parametrize("mode,cin,cout,hw", [(0,) + s for s in SHAPES] + [(1,) + s for s in SHAPES[1:]])
def test_update_sized_launch_equals_launches_of_12(eng, mode, cin, cout, hw):
    """Batch invariance of the fp32 conv forward (mode 0: ReLU in, bias, residual) and data gradient (mode 1: ReLU mask, skip; block1.conv
    has none): every image of a 2051-image launch (4099 @8x8, whose items are image pairs) equals, bit for bit, the same image launched
    in batches of <= 12, where every workgroup runs one item."""
    n = _n(2051, hw)
    w, b, x_dev, x = _conv_inputs(cin, cout, hw, n, 7)
    g = torch.Generator().manual_seed(8)
    if mode == 0:
        res = nhwc(torch.randn(n, cout, hw, hw, generator=g))
        launch = lambda lo, hi: eng.op_conv3x3(0, cin, cout, hw, w.numpy(), inp=x_dev[lo:hi], relu_in=cin != 3, bias=b.numpy(), res=res[lo:hi])
    else:
        dout = nhwc(hard_dy(torch.randn(n, cout, hw, hw, generator=g)))
        skip, mask = nhwc(torch.randn(n, cin, hw, hw, generator=g)), nhwc(x)
        launch = lambda lo, hi: eng.op_conv3x3(1, cin, cout, hw, w.numpy(), dout=dout[lo:hi], mask=mask[lo:hi], res=skip[lo:hi])
    whole = launch(0, n)
    assert np.isfinite(whole).all() and np.abs(whole).max() > 0
    for lo, hi in batches(n):
        assert np.array_equal(launch(lo, hi), whole[lo:hi]), (lo, hi)


@pytest.mark.parametrize("hw,c", [(64, 16), (32, 32), (16, 32)])
def test_maxpool_with_ties(eng, hw, c):
    g = torch.Generator().manual_seed(hw)
    x = torch.randn(3, c, hw, hw, generator=g)
    x[1] = torch.round(x[1])                 # many exact ties
    x[2, :, : hw // 2] = 0.25                # flat region (Procgen frames have these)
    x.requires_grad_(True)
    y = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    out = eng.op_maxpool(0, nhwc(x.detach()))
    assert np.array_equal(out, nhwc(y.detach()))
    dx = eng.op_maxpool(1, nhwc(x.detach()), dout=nhwc(dy))
    np.testing.assert_allclose(dx, nhwc(x.grad), rtol=0, atol=1e-6)
