"""Cases and hashing for tests/test_gpu_resblock_pins.py: SHA-256 of every output tensor of the residual-block bf16 kernels.

Engine.op_resblock mode 2 (whole backward: full16d / full32s / full32q at update sizes) and modes 3 and 4 (pair forward), at 16@32, 32@16
and 32@8, n = 6 and the UPDATE_N sizes, with the seeded inputs of test_residual_block_whole_backward_bf16 and
test_residual_pair_with_distinct_weights (hard_images / hard_dy of update_inputs.py at n >= 1024).  The kernels reduce in a fixed
order (no float atomics), so their outputs are reproducible bit for bit; scratch/gen_resblock_pins.py records the hashes."""
import hashlib
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from update_inputs import UPDATE_N, hard_dy, hard_images, r16

PIN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pins", "resblock_bf16_sha256.json")
SHAPES = [(16, 32), (32, 16), (32, 8)]
SIZES = [6] + UPDATE_N
MODES = [2, 3, 4]
CASES = [(mode, ch, hw, n) for mode in MODES for ch, hw in SHAPES for n in SIZES]


def case_id(mode, ch, hw, n):
    return f"mode{mode}-{ch}@{hw}-n{n}"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def run_case(eng, mode, ch, hw, n):
    """{output name: sha256 of its float32 bytes} for one launch."""
    if mode == 2:
        g = torch.Generator().manual_seed(77)
        w1, w2 = torch.randn(ch, ch, 3, 3, generator=g) * 0.15, torch.randn(ch, ch, 3, 3, generator=g) * 0.15
        x = r16(torch.randn(n, ch, hw, hw, generator=g))
        if n >= 1024:
            x = hard_images(x)
        a = r16(F.conv2d(F.relu(x), r16(w1), torch.randn(ch, generator=g), padding=1))
        dy = r16(torch.randn(n, ch, hw, hw, generator=g))
        if n >= 1024:
            dy = hard_dy(dy)
        flat, gx = eng.op_resblock(2, nhwc(dy), w1.numpy(), w2.numpy(), a_fwd=nhwc(a), x_fwd=nhwc(x))
        return {"wgrads": sha(flat.ravel()[:2 * (ch * ch * 9 + ch)]), "dx": sha(gx)}
    g = torch.Generator().manual_seed(500 + ch + hw)
    W = [torch.randn(ch, ch, 3, 3, generator=g) * 0.1 for _ in range(4)]
    Bs = [torch.randn(ch, generator=g) * 0.5 for _ in range(4)]
    x = r16(torch.randn(n, ch, hw, hw, generator=g))
    if n >= 1024:
        x = hard_images(x)
    if mode == 3:
        oa, oy = eng.op_resblock(3, nhwc(x), W[0].numpy(), W[1].numpy(), b1=Bs[0].numpy(), b2=Bs[1].numpy())
        return {"A2": sha(oa), "P2": sha(oy)}
    oa, oy = eng.op_resblock(4, nhwc(x), torch.stack(W[:2]).numpy(), torch.stack(W[2:]).numpy(), b1=torch.cat(Bs[:2]).numpy(), b2=torch.cat(Bs[2:]).numpy())
    return {"A1": sha(oa[0]), "A2": sha(oa[1]), "P1": sha(oy[0]), "P2": sha(oy[1])}


def load_pins():
    with open(PIN_FILE) as f:
        return json.load(f)
