"""Bit-for-bit pins of whole update-phase passes (mi_minibatch, _multi, _finish, _fused, _rec, mi_ipl_minibatch, mi_value_saliency).

tests/pins/update_pass_sha256.json holds the SHA-256 of the gradients after each of two passes in a row, the loss log, the parameters
after one optimizer step and each entry's own outputs, for the cases of tests/pass_pin_cases.py, recorded by scratch/gen_pass_pins.py on
the commit named in the file's "commit" entry: the parent of the change that gave net_backward an explicit option list (BwdOpts) and
the update entries one prologue.  Such a change moves host code between launches only -- no kernel, no launch and no launch order
changes -- so every pass must keep its bits.  A change that is MEANT to alter the arithmetic or the launch list of a pass re-records
the file with the generator and says so."""
import pytest

from pass_pin_cases import CASES, ENTRIES, load_pins, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pins():
    return load_pins()


def test_pin_file_covers_every_case(pins):
    assert len(pins["commit"]) >= 7
    assert sorted(pins["sha256"]) == sorted(CASES)
    assert {entry for entry, _ in CASES.values()} == set(ENTRIES)


@pytest.mark.parametrize("name", list(CASES))
def test_update_pass_keeps_its_bits(pins, name):
    got = run_case(name)
    want = pins["sha256"][name]
    print(name, {k: (got[k][:12], want.get(k, "")[:12]) for k in got})
    assert got == want
