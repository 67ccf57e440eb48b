"""The bf16 embedder.fc kernels (csrc/fc_bf16.hip) one launch at a time through mi_op_fc_bf16, element by element against the float64
reference of tests/fc_inputs.py, at all eight widths D = 64 .. 512 and at the batch sizes that reach every path of the launchers.

Every case is one hook call (production launcher, production arguments, poisoned outputs, canary bands) and one float64 product; the
bound per element is derived in fc_inputs.py (c = 2), masked dx elements must be exactly 0.0 and nothing may be NaN.  Each docstring
names the path by the launcher's own condition, so a changed dispatch threshold shows which case moves.

Left out: the forward's tiled kernel fc_nt_kernel<false, 128>.  launch_fc_nt takes 128-row tiles only from 512 workgroups on, which at
D = 512 (8 column tiles) needs n >= 8065 with n % 64 != 0; the float64 reference of such a case does not fit a test of a few seconds.
Its A_F32 = true sibling, the same code but for the operand conversion, runs in test_dgrad_256_tiled_128_rows."""
import time

import numpy as np
import pytest

import fc_inputs as FI

pytestmark = pytest.mark.gpu

NOT_256 = tuple(D for D in FI.WIDTHS if D != 256)


@pytest.fixture(scope="module")
def hook_engine():
    from mi355.engine import Engine
    eng = Engine("mlp", 2, 2, 2, 8, obs_dim=4, mlp_depth=2, mlp_width=8, out_dim=8)      # mi_op_fc_bf16 is independent of the context's sizes and precision
    yield eng
    eng.close()


def _run(eng, mode, D, n):
    p, ref = FI.case(mode, D, n)
    t0 = time.perf_counter()
    if mode <= 1:
        got = eng.op_fc_bf16(mode, D, x=p.x, W=p.W, b=p.b)
    elif mode == 2:
        got = eng.op_fc_bf16(2, D, x=p.x, W=p.W, dy=p.dy)
    else:
        got = eng.op_fc_bf16(3, D, x=p.x, dy=p.dy, gW0=p.gW0, gb0=p.gb0)
    dt = time.perf_counter() - t0
    try:
        worst = FI.check(p, got, ref=ref)
    except AssertionError:
        print(f"fc_op mode={mode} D={D} n={n} hook_s={dt:.3f} FAILED")
        raise
    print(f"fc_op mode={mode} D={D} n={n} hook_s={dt:.3f} " + " ".join(f"{k}: err/bound={a:.4g} acc/(K'uS)={b:.4g}" for k, (a, b) in worst.items()))
    r = FI.negative_row(n)
    if r is not None:          # the all-negative row of x, exactly
        if mode <= 1:
            assert np.array_equal(got[r], np.maximum(p.b, 0))
        elif mode == 2:
            assert not got[r].any()


@pytest.mark.parametrize("n", FI.FWD_DEDICATED_N)
@pytest.mark.parametrize("D", FI.WIDTHS)
def test_fwd_dedicated(hook_engine, D, n):
    """launch_fc_fwd_bf16, n % 64 == 0 -> fc_fwd_bf16_kernel<D>.  576 rows are nine row blocks: fc_block_map deals eight of them XCD-wise
    and the ninth through its branch for the last, partial group."""
    _run(hook_engine, 0, D, n)


@pytest.mark.parametrize("n", FI.FWD_NT_N)
@pytest.mark.parametrize("D", FI.WIDTHS)
def test_fwd_tiled(hook_engine, D, n):
    """launch_fc_fwd_bf16, n % 64 != 0 -> launch_fc_nt, (D / 64) * ceil(n / 128) < 512 workgroups -> fc_nt_kernel<false, 64>: a single row,
    one row past a tile, a partial last tile."""
    _run(hook_engine, 0, D, n)


@pytest.mark.parametrize("n", FI.SMALL_N)
@pytest.mark.parametrize("D", FI.WIDTHS)
def test_fwd_small(hook_engine, D, n):
    """launch_fc_fwd_small_bf16 -> fc_small_bf16_kernel<D>, 16 x 16 output tiles: rows past n are loaded from the clamped row n - 1 and not
    stored (1, 17 and 250 rows leave a partial tile)."""
    _run(hook_engine, 1, D, n)


@pytest.mark.parametrize("n", FI.DGRAD_GUARDED_N)
@pytest.mark.parametrize("D", NOT_256)
def test_dgrad_guarded(hook_engine, D, n):
    """launch_fc_dgrad_bf16, D != 256 -> fc_dgrad_bf16_kernel<D> with GUARD for any n (rows past n clamped on load, not stored); D > 256
    walks K in NKC = 2 chunks of D / 2.  1088 rows are nine 128-row blocks (fc_block_map's partial group) with 64 rows in the last."""
    _run(hook_engine, 2, D, n)


@pytest.mark.parametrize("n", FI.DGRAD256_DEDICATED_N)
def test_dgrad_256_dedicated(hook_engine, n):
    """launch_fc_dgrad_bf16, D == 256 and n % 128 == 0 -> fc_dgrad_bf16_kernel<256> without the row guard: one and nine row blocks."""
    _run(hook_engine, 2, 256, n)


@pytest.mark.parametrize("n", FI.DGRAD256_NT64_N)
def test_dgrad_256_tiled_64_rows(hook_engine, n):
    """launch_fc_dgrad_bf16, D == 256 and n % 128 != 0 -> launch_fc_nt, 32 * ceil(n / 128) < 512 workgroups -> fc_nt_kernel<true, 64>."""
    _run(hook_engine, 2, 256, n)


@pytest.mark.parametrize("n", FI.DGRAD256_NT128_N)
def test_dgrad_256_tiled_128_rows(hook_engine, n):
    """launch_fc_dgrad_bf16, D == 256 and n % 128 != 0 -> launch_fc_nt, 32 * ceil(2056 / 128) = 544 >= 512 workgroups -> fc_nt_kernel<true, 128>,
    8 rows in the last tile."""
    _run(hook_engine, 2, 256, n)


@pytest.mark.parametrize("n", FI.WGRAD_N)
@pytest.mark.parametrize("D", FI.WIDTHS)
def test_wgrad(hook_engine, D, n):
    """launch_fc_tn with the engine's 8 M-float workspace + launch_colsum_acc (16 row-group blocks: n < 4096).  (split, k_chunk) by
    launch_fc_tn's rule: n = 1 -> (1, 128), one row in a zeroed tile; 128 -> (1, 128); 129 -> (1, 256), one row in the second tile;
    1024 -> (8, 128); 1088 -> (5, 256), the last slab has 64 rows."""
    _run(hook_engine, 3, D, n)


def test_wgrad_long(hook_engine):
    """launch_fc_tn at D = 64, n = 4100: split 8 -> k_chunk 640 -> 7 slabs, the last of 260 rows (two whole tiles and 4 rows of a third);
    launch_colsum_acc's 64-block branch (M >= 4096)."""
    _run(hook_engine, 3, *FI.WGRAD_LONG)


def test_refusals(hook_engine):
    from mi355.engine import EngineError
    p = FI.make_inputs(2, 64, 3)
    with pytest.raises(EngineError, match="multiple of 64"):
        hook_engine.op_fc_bf16(0, 96, x=p.x, W=np.zeros((96, FI.K), np.float32), b=np.zeros(96, np.float32))
    with pytest.raises(EngineError, match="multiple of 64"):
        hook_engine.op_fc_bf16(0, 576, x=p.x, W=np.zeros((576, FI.K), np.float32), b=np.zeros(576, np.float32))
    with pytest.raises(EngineError, match=r"n must be in \[1, 65536\]"):
        hook_engine.op_fc_bf16(0, 64, x=p.x[:0], W=p.W, b=p.b)
    with pytest.raises(EngineError, match="mode 2 needs the mask source"):
        hook_engine.op_fc_bf16(2, 64, W=p.W, dy=p.dy)
