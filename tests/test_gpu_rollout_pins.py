"""Bit-for-bit pins of whole small rollouts (mi_policy_step, mi_rollout_step, mi_rollout_groups / _submit / _wait, mi_predict_staged +
mi_commit_staged, mi_predict_greedy, mi_forward, mi_forward_rec, mi_set_gru / mi_rec_state / mi_rec_begin / mi_get_hidden_ring / mi_get_hidden).

tests/pins/rollout_sha256.json holds the SHA-256 of the rings, of every array the entries return and of the hidden ring and state of
the GRU cases, for the cases of tests/rollout_pin_cases.py, recorded by scratch/gen_rollout_pins.py on the commit named in the file's
"commit" entry: the parent of the change that moved the rollout's host code into csrc/rollout.hip, gave every env group one struct and
took the worker hand-off into csrc/group_worker.h.  Such a change moves host code between launches only -- no kernel, no launch and no
launch order changes -- so every rollout must keep its bits, whatever the grouping and the order the groups are served in.  A change
that is MEANT to alter the arithmetic or the launch list of a rollout step re-records the file with the generator and says so."""
import pytest

from rollout_pin_cases import CASES, KINDS, load_pins, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pins():
    return load_pins()


def test_pin_file_covers_every_case(pins):
    assert len(pins["commit"]) >= 7
    assert sorted(pins["sha256"]) == sorted(CASES)
    assert {kind for kind, _ in CASES.values()} == set(KINDS)


@pytest.mark.parametrize("name", list(CASES))
def test_rollout_keeps_its_bits(pins, name):
    got = run_case(name)
    want = pins["sha256"][name]
    print(name, {k: (got[k][:12], want.get(k, "")[:12]) for k in got})
    assert got == want
