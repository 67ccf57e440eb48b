"""The bf16 conv, conv + pool, pool and residual-block kernels against float64, bit for bit.

Inputs sit on dyadic grids (tests/exact_inputs.py): every product is a multiple of one unit and every sum stays below 2^24 units, so
every fp32 partial sum -- in any order, on any matrix-core accumulation tree -- is exact, and each kernel output must EQUAL the bf16
round-to-nearest-even of the float64 value at the rounding points of oracle/ppo_oracle_bf16.py.  Every comparison is np.array_equal on
all elements: no tolerance, no exempt element.  A rewrite that reorders a sum cannot break these tests; one that truncates, rounds twice,
adds the bias after the rounding, loses a tap at a border, counts a phantom image slot or drops a tail item always does.  Each test
prints its case's proven bound / unit and its rounding and tie counts; a mismatch is reported with its first element (image, y, x,
channel), the share of differing elements and whether the kernel's value is the other bf16 neighbour of the exact value."""
import pytest

import exact_inputs as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from mi355.engine import Engine
    e = Engine("impala", n_steps=4, n_envs=4, n_actions=15, max_batch=16, precision="bf16")
    yield e
    e.close()


def _params(family):
    return pytest.mark.parametrize("args", E.FAMILIES[family][1], ids=lambda a: "-".join(map(str, a)))


def _check(family, args, eng):
    E.check_case(E.FAMILIES[family][0](*args), eng)


@_params("conv_forward")
def test_conv_forward_exact(eng, args):
    """op_conv3x3 mode 0, ReLU in + bias + residual in fp32 and ONE rounding at the store; block1.conv from uint8 frames on the levels
    whose bf16(k / 255) is a multiple of 2^-6."""
    _check("conv_forward", args, eng)


@_params("conv_dgrad")
def test_conv_dgrad_exact(eng, args):
    """Mode 1 with mask and skip: r16(convT(dout) * (mask > 0) + skip)."""
    _check("conv_dgrad", args, eng)


@_params("conv_wgrad")
def test_conv_wgrad_exact(eng, args):
    """Mode 2: the fp32 weight and bias gradients equal the float64 sums."""
    _check("conv_wgrad", args, eng)


@_params("conv_pool")
def test_conv_pool_exact(eng, args):
    """Mode 3's pooled map (the conv output rounded BEFORE the pool) and, for block2 / block3, the data gradient from a pooled gradient
    (modes 5 and 7): the gathered sum rounded once, then the transposed conv's output.  The arg-max routes -- first maximum among tied
    bf16 keys -- are checked through these gradients.  n >= 1024: the rolling-rows forward, several items per workgroup."""
    _check("conv_pool", args, eng)


@_params("conv_pool_wgrad")
def test_conv_pool_wgrad_exact(eng, args):
    """Modes 4 and 6: dW and db from a pooled gradient, block1's one-hot form included.  n <= 12: pooled gradients on the fine grid, so
    that more than half of the gathered sums leave bf16 -- a kernel that truncates the sum, rounds per contribution, feeds block2 / block3
    an unrounded sum or rounds block1's changes most elements of dW.  n >= 1024: coarse operands (the 2^24 condition on 2051 * hw^2
    terms); those launches check the grid walk and the tail."""
    _check("conv_pool_wgrad", args, eng)


@_params("maxpool")
def test_maxpool_exact(eng, args):
    """op_maxpool modes 0 and 1: dx = r16(the float64 scatter sum), ties to the first maximum."""
    _check("maxpool", args, eng)


@_params("resblock_forward")
def test_resblock_forward_exact(eng, args):
    """op_resblock mode 0: a and y."""
    _check("resblock_forward", args, eng)


@_params("resblock_backward")
def test_resblock_backward_exact(eng, args):
    """op_resblock mode 1: da (handed on through LDS as bf16) and dx."""
    _check("resblock_backward", args, eng)


@_params("resblock_whole_backward")
def test_resblock_whole_backward_exact(eng, args):
    """op_resblock mode 2: dx, dW1, db1, dW2 and db2 from one launch.  n >= 1024: full16d, full32s and full32q with their phantom slots --
    a slot counted twice or a dropped tail item changes low bits of the weight gradients that 1e-4 of the maximum cannot see."""
    _check("resblock_whole_backward", args, eng)


@_params("pair")
def test_residual_pair_exact(eng, args):
    """op_resblock mode 4: A1, P1, A2 and P2 of four distinct convs.  n >= 1024: pair32r, RB_32_8S and RB_32_8P."""
    _check("pair", args, eng)
