"""The checker of the op-level embedder.fc tests (tests/fc_inputs.py) on the host: its bf16 rounding is torch's, a correct float32
evaluation passes the derived bound (c = 2) at every case the GPU tests run, and each way a kernel is likely to be wrong fails it."""
import numpy as np
import pytest
import torch

import fc_inputs as FI


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def test_bf16_rounding_is_torch_bfloat16():
    p = FI.make_inputs(3, 192, 129)
    u = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x00008000, 0x00018000,
                  0x80018000, 0x7F7F8000, 0x7F7F7FFF, 0x3EFFFFFF, 0x00000001], dtype=np.uint32)      # ties to even / odd, +-0, denormals, overflow
    for a in (p.x, p.W, p.dy, u.view(np.float32)):
        want = torch.from_numpy(np.ascontiguousarray(a)).bfloat16().float().numpy()
        assert np.array_equal(FI.bf16_round(a).view(np.uint32), want.view(np.uint32))
    x = FI.bf16_round(p.x)
    assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()          # both zeros survive, with their signs
    assert (x[FI.negative_row(129)] < 0).all() and 0.4 < (x < 0).mean() < 0.6


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_float32_evaluation_passes_everywhere(mode):
    """Rounded operands, np.float32 products summed over K in tiles of 128: inside the bound with c = 2 at every (D, n) of the GPU tests."""
    top = 0.0
    for D, n in FI.cases(mode):
        p = FI.make_inputs(mode, D, n)
        w = FI.check(p, FI.emulate_f32(p))
        top = max(top, max(v[0] for v in w.values()))
    print(f"mode {mode}: worst err / bound of the float32 evaluation = {top:.3g}")
    assert top <= 1.0


def test_every_width_runs_in_every_mode():
    for mode in range(4):
        assert {D for D, _ in FI.cases(mode)} == set(FI.WIDTHS)


# ---------------------------------------------------------------------------------------------- mutations of a correct result
def _fails(p, ref, got, match=None):
    with pytest.raises(AssertionError, match=match):
        FI.check(p, got, ref=ref)


def _correct(mode, D, n):
    p, ref = FI.case(mode, D, n)
    good = FI.emulate_f32(p)
    FI.check(p, good, ref=ref)
    return p, ref, good, FI.operands(p)


def _with(good, k, new):
    """mode 3: (gW, gb) with one of the two replaced"""
    out = list(good)
    out[k] = new
    return tuple(out)


@pytest.mark.parametrize("mode,D,n", [(0, 192, 65), (1, 64, 17), (2, 448, 129), (2, 256, 200)])
def test_swapped_neighbouring_rows_fail(mode, D, n):
    p, ref, good, _ = _correct(mode, D, n)
    for r in (0, n - 2):
        bad = good.copy()
        bad[[r, r + 1]] = bad[[r + 1, r]]
        _fails(p, ref, bad)


def test_swapped_gradient_rows_fail():
    p, ref, good, _ = _correct(3, 128, 129)
    bad = good[0].copy()
    bad[[63, 64]] = bad[[64, 63]]
    _fails(p, ref, _with(good, 0, bad))
    _fails(p, ref, _with(good, 1, good[1][::-1].copy()))


def test_missing_k_tile_fails():
    """One 128-deep K tile left out of one output block of each kernel family."""
    p, ref, good, o = _correct(0, 128, 200)                  # forward: k in [128, 256) missing from rows 64.., columns 64..
    bad = good.copy()
    pre = o["xr"] @ o["Wb"].T + p.b - o["xr"][:, 128:256] @ o["Wb"][:, 128:256].T
    bad[64:128, 64:128] = _f32(np.maximum(pre, 0))[64:128, 64:128]
    _fails(p, ref, bad)
    p, ref, good, o = _correct(2, 256, 200)                  # data gradient: k in [128, 256) missing from one 128 x 64 block
    bad = good.copy()
    part = (o["dyb"][:, :128] @ o["Wb"][:128]) * o["mask"]
    bad[128:200, 64:128] = FI.bf16_round(_f32(part))[128:200, 64:128]
    _fails(p, ref, bad)
    p, ref, good, o = _correct(3, 64, 1088)                  # weight gradient: batch rows [128, 256) missing from one 64 x 128 block
    bad = good[0].copy()
    bad[:, 128:256] = _f32(ref[0][1] - o["dyb"][128:256].T @ o["xr"][128:256])[:, 128:256]
    _fails(p, ref, _with(good, 0, bad))


def test_clamped_last_rows_fail():
    """The last n % 128 rows replaced by the clamped row n - 1: as outputs (forward, data gradient) and as operands (weight gradient)."""
    for mode, D, n in ((0, 64, 200), (2, 192, 1088)):
        p, ref, good, _ = _correct(mode, D, n)
        bad = good.copy()
        bad[n - n % 128:] = bad[n - 1]
        _fails(p, ref, bad)
    p, ref, good, o = _correct(3, 64, 1088)
    dyb, xr = o["dyb"].copy(), o["xr"].copy()
    dyb[1024:], xr[1024:] = dyb[1087], xr[1087]
    _fails(p, ref, _with(good, 0, _f32(p.gW0 + dyb.T @ xr)))
    dy = p.dy.astype(np.float64)
    dy[1024:] = dy[1087]
    _fails(p, ref, _with(good, 1, _f32(p.gb0 + dy.sum(0))))


@pytest.mark.parametrize("mode,D,n", [(0, 128, 64), (2, 64, 127), (3, 64, 128)])
def test_shifted_columns_fail(mode, D, n):
    """The columns of one 64-column step shifted by 4 (a lane's four consecutive columns)."""
    p, ref, good, _ = _correct(mode, D, n)
    out = (good[0] if mode == 3 else good).copy()
    out[:, 64:128] = np.roll(out[:, 64:128], 4, axis=1)
    _fails(p, ref, _with(good, 0, out) if mode == 3 else out)


def test_unmasked_element_fails():
    p, ref, good, o = _correct(2, 320, 127)
    full = FI.bf16_round(_f32(o["dyb"] @ o["Wb"]))
    for r, c in (np.argwhere(~o["mask"] & (full != 0))[k] for k in (0, -1)):
        bad = good.copy()
        bad[r, c] = full[r, c]
        _fails(p, ref, bad, match="masked elements are not 0.0")
    r, c = np.argwhere(FI.bf16_round(p.x) == 0)[0]            # x == +-0.0 is masked too
    assert good[r, c] == 0
    bad = good.copy()
    bad[r, c] = np.float32(1e-30)
    _fails(p, ref, bad, match="masked elements are not 0.0")


def test_skipped_element_fails():
    p, ref, good, _ = _correct(1, 64, 17)
    bad = good.copy()
    bad[16, 63] = np.nan                                      # what the hook's poison reads back as
    _fails(p, ref, bad, match="non-finite")


def test_skipped_input_relu_fails():
    p, ref, good, o = _correct(0, 64, 65)                     # forward: one row multiplied without relu(x)
    bad = good.copy()
    bad[64] = _f32(np.maximum(o["xb"][64] @ o["Wb"].T + p.b, 0))
    _fails(p, ref, bad)
    p, ref, good, o = _correct(3, 64, 129)                    # weight gradient: one batch row enters without relu(x)
    bad = _f32(ref[0][1] + np.outer(o["dyb"][128], np.minimum(o["xb"][128], 0)))
    _fails(p, ref, _with(good, 0, bad))
    r = FI.negative_row(129)                                  # the all-negative row must add nothing
    bad = _f32(ref[0][1] + np.outer(o["dyb"][r], o["xb"][r]))
    _fails(p, ref, _with(good, 0, bad))


def test_lost_initial_gradient_fails():
    p, ref, good, o = _correct(3, 64, 128)
    _fails(p, ref, _with(good, 0, _f32(o["dyb"].T @ o["xr"])))
    _fails(p, ref, _with(good, 1, _f32(p.dy.astype(np.float64).sum(0))))


def test_dropped_second_k_chunk_fails():
    """D = 320 walks K in two chunks of 160: the second one (k >= D / 2) dropped."""
    p, ref, good, o = _correct(2, 320, 129)
    bad = FI.bf16_round(_f32((o["dyb"][:, :160] @ o["Wb"][:160]) * o["mask"]))
    _fails(p, ref, bad)
    bad2 = good.copy()
    bad2[128] = bad[128]                                      # ... in the partial last row block alone
    _fails(p, ref, bad2)
