"""Bit-for-bit pins of the residual-block bf16 kernels (whole backward and pair forward).

tests/pins/resblock_bf16_sha256.json holds the SHA-256 of every output tensor of Engine.op_resblock modes 2, 3 and 4 at 16@32, 32@16
and 32@8, n = 6, 1024, 1025 and 2051, recorded by scratch/gen_resblock_pins.py on the commit named in the file's "commit" entry: the
parent of the change that cut the vector-instruction count of these kernels (role-specific item loops, affine LDS addresses, mask
tests on the bf16 bits).  Such a change leaves every multiply, add and rounding point alone, so every output must keep its bits.
A change that is MEANT to alter the arithmetic re-records the file with the generator and says so."""
import pytest

from resblock_pin_cases import CASES, case_id, load_pins, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from mi355.engine import Engine
    e = Engine("impala", n_steps=4, n_envs=4, n_actions=15, max_batch=16, precision="bf16")
    yield e
    e.close()


@pytest.fixture(scope="module")
def pins():
    return load_pins()


def test_pin_file_covers_every_case(pins):
    assert len(pins["commit"]) >= 7
    assert sorted(pins["sha256"]) == sorted(case_id(*c) for c in CASES)


@pytest.mark.parametrize("mode,ch,hw,n", CASES, ids=[case_id(*c) for c in CASES])
def test_resblock_outputs_keep_their_bits(eng, pins, mode, ch, hw, n):
    got = run_case(eng, mode, ch, hw, n)
    want = pins["sha256"][case_id(mode, ch, hw, n)]
    print(case_id(mode, ch, hw, n), {k: (got[k][:12], want.get(k, "")[:12]) for k in got})
    assert got == want
