"""make_env's env-group choice for recurrent policies (CPU): env groups only from an explicit --rollout_groups G >= 2; the automatic
setting keeps the single VecEnv (and with it the reference's exact reward-normalisation order); non-recurrent choices are unchanged."""
import argparse

import pytest


def _make(rec, groups, n_envs=16, valid=False, env_name="synthetic"):
    from common.env.vec_envs import EnvGroups
    from train import add_training_args, make_env
    argv = ["--env_name", env_name, "--rollout_groups", str(groups)] + ([] if valid else ["--no-use_valid_env"])
    args = add_training_args(argparse.ArgumentParser()).parse_args(argv)
    env = make_env(env_name, n_envs, 3, 15, args, {"recurrent": rec, "normalize_rew": True}, is_valid=valid)
    return len(env.env_groups) if isinstance(env, EnvGroups) else 1


@pytest.mark.parametrize("groups", [2, 4])
def test_recurrent_policy_gets_env_groups_when_asked(groups):
    assert _make(True, groups) == groups
    assert _make(True, groups, valid=True) == groups


@pytest.mark.parametrize("n_envs,valid", [(16, False), (256, False), (256, True)])
def test_recurrent_policy_auto_setting_keeps_one_env(n_envs, valid):
    assert _make(True, 0, n_envs=n_envs, valid=valid) == 1
    assert _make(True, 1, n_envs=n_envs, valid=valid) == 1


@pytest.mark.parametrize("n_envs,valid,groups,want", [(16, False, 0, 2), (256, False, 0, 4), (256, True, 0, 2), (16, False, 1, 1),
                                                      (16, False, 4, 4), (12, False, 4, 1), (16, False, 2, 2)])
def test_non_recurrent_choice_unchanged(n_envs, valid, groups, want):
    assert _make(False, groups, n_envs=n_envs, valid=valid) == want


def test_more_than_four_groups_refused_for_recurrent_too():
    with pytest.raises(ValueError, match="at most 4"):
        _make(True, 8)
