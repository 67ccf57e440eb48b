"""Inputs and references for the op-level tests at update-sized launches (n >= 1024 images).

The conv and residual kernels of the update phase run persistent grids: each workgroup walks items work, work + gridDim.x, ...
At n <= 37 every workgroup runs one item, so these inputs are aimed at what only larger launches exercise: accumulators carried
across items, the uneven tail, the phantom image slots of the multi-image kernels and the n = 1024 kernel switches."""
import numpy as np
import torch
import torch.nn.functional as F

UPDATE_N = [1024, 1025, 2051]       # both sides of every n = 1024 switch; 2051: odd, = 3 (mod 4), >= 2 items per workgroup
# where a workgroup's second item starts, for the items (1/8, 1/2, 1, 2, 4 images) and grid caps (256 .. 1024) of the kernels
SEAMS = (128, 256, 512, 768, 1024)
FLAT_EVERY = 97                     # every 97th image carries a flat band (max-pool ties) over quantised values
DY_ZERO = 300                       # the image whose output gradient is zero


def r16(t):
    return t.bfloat16().float()


def hard_images(x, bf16=True):
    """x: NCHW float.  Images at SEAMS all negative (a dead ReLU where a workgroup's second item starts); every FLAT_EVERY-th image
    quantised to halves with a flat band across rows hw/4-2 .. hw/2+2 (pooling ties at the rolling kernel's carried row and at the
    4-pooled-row item seams); the last image scaled x8 (a phantom slot that copies it shows in the weight gradients).  bf16: rounded
    to bf16 values (the bf16 mode's inputs); otherwise the other images keep their full fp32 mantissas."""
    x = x.clone()
    n, _, hw, _ = x.shape
    for j in SEAMS:
        if j < n - 1:
            x[j] = -x[j].abs() - 0.125
    for j in range(1, n - 1, FLAT_EVERY):
        x[j] = torch.round(x[j] * 2) / 2
        x[j, :, hw // 4 - 2:hw // 2 + 3, :] = x[j, :, :1, :1]
    x[-1] *= 8
    return r16(x) if bf16 else x


def hard_frames(x_u8):
    """uint8 NHWC frames: black frames at SEAMS, flat bands every FLAT_EVERY-th frame, the last frame saturated."""
    x_u8 = x_u8.copy()
    n = x_u8.shape[0]
    for j in SEAMS:
        if j < n - 1:
            x_u8[j] = 0
    for j in range(1, n - 1, FLAT_EVERY):
        x_u8[j, 14:35] = 128
    x_u8[-1] = 255
    return x_u8


def frames_to_nchw(x_u8):
    """block1.conv in bf16 mode stages a frame as bf16(k / 255) (uint8 -> bf16 table); fp32 mode as k / 255."""
    return torch.from_numpy((x_u8.transpose(0, 3, 1, 2) / 255.0).astype(np.float32))


def hard_dy(dy):
    """An output gradient with image DY_ZERO zeroed."""
    dy = dy.clone()
    if dy.shape[0] > DY_ZERO:
        dy[DY_ZERO] = 0
    return dy


def check_per_image(out, ref, what, tol):
    """Every output finite; for every image i, max|out_i - ref_i| / max|ref_i| < tol.  Returns the worst value."""
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.isfinite(out).all(), f"{what}: {int((~np.isfinite(out)).sum())} non-finite outputs"
    n = out.shape[0]
    o, r = out.reshape(n, -1), ref.reshape(n, -1)
    e = np.abs(o - r).max(1) / (np.abs(r).max(1) + 1e-12)
    i = int(e.argmax())
    print(f"{what}: worst per-image error {e[i]:.2e} (image {i} of {n})")
    assert e[i] < tol, (what, i, float(e[i]))
    return float(e[i])


def wgrad64(x, dy, chunk=64):
    """Float64 weight and bias gradients of a 3x3 / pad 1 conv: sum over images and pixels of dy x unfold(x), in chunks."""
    n, cin = x.shape[:2]
    cout = dy.shape[1]
    acc = torch.zeros(cout, cin * 9, dtype=torch.float64)
    for k in range(0, n, chunk):
        u = F.unfold(x[k:k + chunk].double(), 3, padding=1)
        acc += torch.bmm(dy[k:k + chunk].double().flatten(2), u.transpose(1, 2)).sum(0)
    return acc.view(cout, cin, 3, 3).numpy(), dy.double().sum(dim=(0, 2, 3)).numpy()


def check_wgrad(gw, gb, ref_w, ref_b, what, tol):
    """Weight and bias gradient within tol of the float64 reference's max; prints the measured values."""
    ew = float(np.abs(gw - ref_w).max() / (np.abs(ref_w).max() + 1e-30))
    eb = float(np.abs(gb - ref_b).max() / (np.abs(ref_b).max() + 1e-30))
    print(f"{what}: weight gradient {ew:.2e}, bias gradient {eb:.2e} of the float64 reference's max")
    assert ew < tol and eb < tol, (what, ew, eb)
    return ew, eb


def batches(n, size=12):
    return [(k, min(n, k + size)) for k in range(0, n, size)]
