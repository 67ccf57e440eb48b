"""IMPALA embedder widths other than 256 (output_dim, --output_dim): host side, against the reference's G12 vectors
(tests/golden/make_golden_width.py).  CPU only."""
import argparse
import hashlib
import types

import numpy as np
import pytest
import torch

from conftest import load_npz, npz_json
from oracle import ppo_oracle as O
from width_inputs import frames_fwd, frames_rec, frames_rollout, grad_errors, sha

torch.set_num_threads(8)
SEED, A = 6033, 15


def _policy(D, recurrent=False):
    from common.model import ImpalaModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(SEED)
    return CategoricalPolicy(ImpalaModel(3, output_dim=D), recurrent, A)


def _sha(policy):
    flat = np.concatenate([x.detach().numpy().ravel() for x in policy.parameters()]).astype(np.float32)
    return hashlib.sha256(flat.tobytes()).hexdigest()


def _params(D):
    return {k: v.detach().numpy().copy() for k, v in _policy(D).state_dict().items()}


@pytest.mark.parametrize("D", [64, 128, 512])
def test_width_init_is_bit_identical_to_reference(D):
    z = load_npz("g12_impala_width.npz")
    p = _policy(D)
    assert _sha(p) == npz_json(z, "sha")[f"D{D}"]
    assert p.embedder.output_dim == D
    if D == 128:
        assert list(p.state_dict().keys()) == npz_json(z, "keys")
        assert {k: list(v.shape) for k, v in p.state_dict().items()} == npz_json(z, "shapes")


def test_width_recurrent_init_matches_reference():
    z = load_npz("g12_impala_width.npz")
    p = _policy(128, recurrent=True)
    assert _sha(p) == npz_json(z, "sha")["D128_rec"]
    assert tuple(p.state_dict()["gru.gru.weight_ih_l0"].shape) == (3 * 128, 128)


@pytest.mark.parametrize("D", [64, 128, 384, 512])
def test_width_param_shapes_match_module(D):
    from mi355 import layout
    shapes = layout.impala_param_shapes(A, output_dim=D)
    sd = _policy(D).state_dict()
    assert list(shapes) == list(sd.keys())
    assert all(tuple(shapes[k]) == tuple(v.shape) for k, v in sd.items())
    assert _policy(D).param_shapes() == shapes


def test_width_fixture_frames_are_rebuilt_exactly():
    """G12 stores the SHA-256 of its frames, not the frames: the seeded generators must give the same bytes."""
    ref = npz_json(load_npz("g12_impala_width.npz"), "frames_sha")
    assert (sha(frames_fwd()), sha(frames_rollout()), sha(frames_rec())) == (ref["fwd"], ref["rollout"], ref["rec"])


def test_width_oracle_forward_matches_reference():
    z = load_npz("g12_impala_width.npz")
    p = {k: torch.from_numpy(v) for k, v in _params(128).items()}
    with torch.no_grad():
        feat, _, _ = O.impala_embed(p, O.frames_to_obs(frames_fwd()))
        lp, v = O.heads(p, feat)
    tol = dict(rtol=0, atol=1e-6)
    np.testing.assert_allclose(feat.numpy(), z["fwd/feat"], **tol)
    np.testing.assert_allclose(lp.numpy(), z["fwd/logits"], **tol)
    np.testing.assert_allclose(v.numpy(), z["fwd/value"], **tol)


def test_width_oracle_losses_and_grads_match_reference():
    z = load_npz("g12_impala_width.npz")
    T, E = 4, 8
    fr = frames_rollout(T, E)
    obs = O.frames_to_obs(fr.reshape(-1, 64, 64, 3)).reshape(T + 1, E, 3, 64, 64)
    adv, ret = O.compute_estimates(torch.from_numpy(z["in/rew"]), torch.from_numpy(z["in/done"]), torch.from_numpy(z["in/val"]),
                                   0.999, 0.95, True, True)
    np.testing.assert_allclose(adv.numpy(), z["adv"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(ret.numpy(), z["ret"], rtol=0, atol=1e-6)
    ro = dict(obs=obs, act=z["in/act"].astype(np.float32), logp=z["in/logp"], val=z["in/val"], adv=adv.numpy(), ret=ret.numpy())
    ag = O.OraclePPO(_params(128), "impala", T, E, epoch=1, n_minibatch=1, mini_batch_size=T * E,
                     gamma=0.999, lmbda=0.95, learning_rate=5e-4, grad_clip_norm=1e9, x_entropy_coef=0.0)
    torch.manual_seed(5)
    summ = ag.optimize(ro)
    ref = npz_json(z, "raw/summary")
    for k in ("Loss/pi", "Loss/v", "Loss/entropy", "Loss/x_entropy", "Loss/total"):
        assert abs(summ[k] - ref[k]) < 2e-6, (k, summ[k], ref[k])
    g = {k: v.numpy() for k, v in ag.grad_log[0].items()}
    for k in z.files:
        if k.startswith("raw/g/"):
            np.testing.assert_allclose(g[k[len("raw/g/"):]], z[k], rtol=1e-4, atol=2e-6, err_msg=k)
    err = grad_errors(g, z)
    assert sorted(err) == sorted(g.keys())
    assert max(err.values()) < 1e-5, max((v, k) for k, v in err.items())


def test_width_oracle_recurrent_predict_matches_reference():
    z = load_npz("g12_impala_width.npz")
    policy = _policy(128, recurrent=True)
    p = {k: v.detach().clone() for k, v in policy.state_dict().items()}
    h = torch.zeros(8, 128)
    with torch.no_grad():
        for t in range(3):
            feat, _, _ = O.impala_embed(p, O.frames_to_obs(frames_rec()[t]))
            h = O.gru_cell(p, feat, h, torch.from_numpy(1.0 - z["rec/done"][t]))
            lp, v = O.heads(p, h)
            np.testing.assert_allclose(h.numpy(), z[f"rec/hx{t}"], rtol=0, atol=2e-6)
            np.testing.assert_allclose(lp.numpy(), z[f"rec/logits{t}"], rtol=0, atol=2e-6)
            np.testing.assert_allclose(v.numpy(), z[f"rec/value{t}"], rtol=0, atol=2e-6)


def test_train_output_dim_flag_builds_the_wider_model():
    import train
    args = train.add_training_args(argparse.ArgumentParser()).parse_args("--env_name coinrun --param_name hard-500 --output_dim 512".split())
    hp = train.merge_hyperparameters(train.get_hyperparams("hard-500"), args)
    assert hp["output_dim"] == 512
    env = types.SimpleNamespace(observation_space=types.SimpleNamespace(shape=(3, 64, 64)), action_space=types.SimpleNamespace(n=A))
    model, obs_shape, policy = train.initialize_model(torch.device("cpu"), env, hp)
    assert model.output_dim == 512 and obs_shape == (3, 64, 64)
    assert tuple(policy.state_dict()["embedder.fc.weight"].shape) == (512, 2048)
    assert tuple(policy.state_dict()["fc_policy.weight"].shape) == (A, 512)
    # a config-file value when the flag is not given on the command line
    model, _, _ = train.initialize_model(torch.device("cpu"), env, dict(hp, output_dim=128))
    assert model.output_dim == 128


@pytest.mark.parametrize("D", [100, 1024, 0, 32, 576])
def test_unsupported_width_is_refused_with_the_supported_set(D):
    from common.model import ImpalaModel
    with pytest.raises(NotImplementedError, match=r"output_dim=%d: .*\[64, 128, 192, 256, 320, 384, 448, 512\]" % D):
        ImpalaModel(3, output_dim=D)


def test_latent_dim_and_in_channels_keep_their_own_refusals():
    from common.model import ImpalaModel
    with pytest.raises(NotImplementedError, match="latent_dim=16"):
        ImpalaModel(3, output_dim=128, latent_dim=16)
    with pytest.raises(NotImplementedError, match="in_channels=4"):
        ImpalaModel(4, output_dim=128)


def test_checkpoint_of_another_width_is_refused():
    a, b = _policy(128), _policy(256)
    with pytest.raises(RuntimeError, match="size mismatch"):
        b.load_state_dict(a.state_dict())
