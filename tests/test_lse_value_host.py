"""CategoricalPolicy(logsumexp_logits_is_v=True) (reference: common/policy.py:77-78), host side: the torch restatement of
tests/lse_inputs.py against fixture G14 (tests/golden/make_golden_lse.py ran the reference), and the Python surface -- policy,
train.initialize_model, DeviceAdam's state layout, the config struct, PPOPure's refusal.  CPU only.

Bounds against the fixture are the oracle tests' (tests/test_oracle_golden.py, test_width_host.py): forward 2e-6, losses 2e-6,
stored gradient tensors rtol 1e-4 + 2e-6, sketched ones 1e-5 of their norm, the Adam step 2e-6 absolute."""
import ctypes
import types

import numpy as np
import pytest
import torch

import lse_inputs as LI
from conftest import npz_json
from width_inputs import grad_errors, sketch

torch.set_num_threads(8)
ARCHS = ("impala", "mlp")


def _policy(arch, recurrent=False, **kw):
    from common.model import ImpalaModel, MLPModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(6033)
    emb = ImpalaModel(3) if arch == "impala" else MLPModel(9, 4, 256, 64)
    return CategoricalPolicy(emb, recurrent, LI.ARCHS[arch]["A"], **kw)


@pytest.fixture(scope="module", params=ARCHS)
def case(request):
    return LI.case(request.param)


@pytest.fixture(scope="module")
def minibatch(case):
    """The restatement's fp32 losses and gradients of G14's one minibatch (all 32 samples, index order), raw and xent."""
    obs = LI.ref_obs(case["arch"], case["frames"][:LI.T])
    f = lambda a: np.asarray(a).reshape(-1)
    return {tag: LI.loss_and_grads(case["params"], case["arch"], obs, f(case["act"]), f(case["logp"]), f(case["val"][:LI.T]), f(case["ret"]),
                                   f(case["adv"]), x_entropy_coef=xc) for tag, xc in (("raw", 0.0), ("xent", 0.05))}


def test_fixture_inputs_meet_their_conditions(case):
    """G14's parameters are G3's / G7's with one tensor scaled; the logits spread; the value clip acts on some samples and not on others."""
    arch, z = case["arch"], case["z"]
    base = LI.base_params(arch)
    assert np.array_equal(case["params"]["fc_policy.weight"], (base["fc_policy.weight"] * z[f"{arch}/scale"]).astype(np.float32))
    assert all(np.array_equal(case["params"][k], base[k]) for k in base if k != "fc_policy.weight")
    noise = (np.random.default_rng(LI.NOISE_SEED).standard_normal((LI.T + 1, LI.E)) * LI.NOISE_STD).astype(np.float32)
    np.testing.assert_allclose(case["val"][:LI.T].reshape(-1) - noise[:LI.T].reshape(-1), z[f"{arch}/value"], rtol=0, atol=1e-6)
    v, oldv, ret = z[f"{arch}/value"].astype(np.float64), case["val"][:LI.T].reshape(-1).astype(np.float64), case["ret"].reshape(-1).astype(np.float64)
    outside = np.abs(v - oldv) > LI.HP["eps_clip"]
    vs1, vs2 = (v - ret) ** 2, (oldv + np.clip(v - oldv, -0.2, 0.2) - ret) ** 2
    assert outside.sum() >= 8 and (~outside).sum() >= 8
    assert (vs1 > vs2).any() and (vs2 > vs1).any()
    lp = z[f"{arch}/logits"]
    assert np.exp(lp).max(axis=1).mean() > 1.5 / lp.shape[1]          # far from the uniform softmax of the 0.01-gain initialisation


def test_restatement_forward_matches_g14(case):
    arch, z = case["arch"], case["z"]
    lp, v, _ = LI.forward(case["params"], arch, LI.ref_obs(arch, case["frames"][:LI.T]))
    np.testing.assert_allclose(lp, z[f"{arch}/logits"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(v, z[f"{arch}/value"], rtol=0, atol=2e-6)
    # the value is the logsumexp of the RAW logits: log-probs + value give them back, and fc_value plays no part
    p2 = dict(case["params"], **{"fc_value.weight": case["params"]["fc_value.weight"] * 3 + 1})
    assert np.array_equal(LI.forward(p2, arch, LI.ref_obs(arch, case["frames"][:LI.T]))[1], v)
    adv, ret = LI.O.compute_estimates(torch.from_numpy(case["rew"]), torch.from_numpy(case["done"]), torch.from_numpy(case["val"]), 0.999, 0.95)
    np.testing.assert_allclose(adv.numpy(), case["adv"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(ret.numpy(), case["ret"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("tag", ["raw", "xent"])
def test_restatement_losses_and_gradients_match_g14(case, minibatch, tag):
    arch, z = case["arch"], case["z"]
    L, g, none = minibatch[tag]
    ref = npz_json(z, f"{arch}/{tag}/summary")
    assert abs(-L["pi_loss"] - ref["Loss/pi"]) < 2e-6 and abs(-L["value_loss"] - ref["Loss/v"]) < 2e-6 * max(1, abs(ref["Loss/v"]))
    assert abs(L["entropy"] - ref["Loss/entropy"]) < 2e-6 and abs(L["x_ent"] - ref["Loss/x_entropy"]) < 2e-6
    assert abs(L["total"] - ref["Loss/total"]) < 2e-6 * max(1, abs(ref["Loss/total"]))
    assert none == npz_json(z, f"{arch}/{tag}/none") == list(LI.VALUE_KEYS)
    sub = LI.Sub(z, f"{arch}/{tag}/")
    for k in sub.files:
        if k.startswith("g/"):
            np.testing.assert_allclose(g[k[2:]], sub[k], rtol=1e-4, atol=2e-6, err_msg=k)
    err = grad_errors(g, sub, prefix="")
    assert sorted(err) == sorted(g) and len(g) == len(case["params"]) - 2
    assert max(err.values()) < 1e-5, max((v, k) for k, v in err.items())


def test_value_gradient_reaches_the_policy_head(case, minibatch):
    """d v / d logit_k = softmax(logits)_k: with the value loss switched off fc_policy's gradient is another one, by the amount the
    analytic expression gives."""
    arch = case["arch"]
    obs = LI.ref_obs(arch, case["frames"][:LI.T])
    f = lambda a: np.asarray(a).reshape(-1)
    hp = dict(LI.HP)
    try:
        LI.HP["value_coef"] = 0.0
        _, g0, _ = LI.loss_and_grads(case["params"], arch, obs, f(case["act"]), f(case["logp"]), f(case["val"][:LI.T]), f(case["ret"]), f(case["adv"]))
    finally:
        LI.HP.update(hp)
    g = minibatch["raw"][1]
    lp, v, feat = LI.forward(case["params"], arch, obs, torch.float64)
    raw = feat @ case["params"]["fc_policy.weight"].astype(np.float64).T + case["params"]["fc_policy.bias"]
    sm1 = np.exp(raw - v[:, None])
    oldv, ret = f(case["val"][:LI.T]).astype(np.float64), f(case["ret"]).astype(np.float64)
    vc = oldv + np.clip(v - oldv, -0.2, 0.2)
    inr = (np.abs(v - oldv) <= 0.2).astype(np.float64)
    gv = np.where((v - ret) ** 2 > (vc - ret) ** 2, 2 * (v - ret), 2 * (vc - ret) * inr)
    want = ((0.5 * 0.5 / 32) * gv[:, None] * sm1).T @ feat
    assert LI.rel_l2(g["fc_policy.weight"] - g0["fc_policy.weight"], want) < 1e-4
    assert np.linalg.norm(want) > 0.05 * np.linalg.norm(g["fc_policy.weight"])


def test_restatement_adam_step_matches_g14(case, minibatch):
    arch, z = case["arch"], case["z"]
    after, norm = LI.adam_first_step(case["params"], minibatch["raw"][1], 0.5, 5e-4)
    assert abs(norm - float(z[f"{arch}/step/norm"])) < 1e-5 * max(1.0, norm)
    sub = LI.Sub(z, f"{arch}/step/")
    for k in sub.files:
        if k.startswith("g/"):
            np.testing.assert_allclose(after[k[2:]], sub[k], rtol=0, atol=2e-6, err_msg=k)
        elif k.startswith("sketch/"):          # |s . (a - r)| <= ||a - r|| <= 2e-6 sqrt(n) for unit vectors s
            a = after[k[7:]]
            assert np.abs(sketch(a) - sub[k]).max() < 2e-6 * np.sqrt(a.size), k
    for k in LI.VALUE_KEYS:
        assert np.array_equal(after[k], case["params"][k]) and np.array_equal(sub["g/" + k], case["params"][k])


def test_restatement_saliency_matches_g14(case):
    arch, z = case["arch"], case["z"]
    v, grad, _ = LI.saliency(case["params"], arch, LI.ref_obs(arch, case["frames"][0]))
    ref = z[f"{arch}/sal"]
    assert grad.shape == ref.shape and np.abs(ref).max() > 0
    assert np.abs(grad - ref).max() < 1e-5 * np.abs(ref).max() + 1e-9
    np.testing.assert_allclose(v, z[f"{arch}/value"][:LI.E], rtol=0, atol=2e-6)


# ---------------------------------------------------------------------------------------------- Python surface
@pytest.mark.parametrize("arch", ARCHS)
def test_policy_accepts_the_flag_and_keeps_its_state_dict(arch):
    on, off = _policy(arch, logsumexp_logits_is_v=True), _policy(arch)
    assert on.logsumexp_logits_is_v is True and off.logsumexp_logits_is_v is False
    sd_on, sd_off = torch.nn.Module.state_dict(on), torch.nn.Module.state_dict(off)
    assert list(sd_on) == list(sd_off) and all(torch.equal(sd_on[k], sd_off[k]) for k in sd_on)
    assert [n for n, _ in on.named_parameters()] == [n for n, _ in off.named_parameters()]
    assert list(sd_on)[-2:] == list(LI.VALUE_KEYS)
    assert list(sd_on) == [m[0] for m in npz_json(LI.load("g14_lse_value.npz"), f"{arch}/step/opt")["model"]]


@pytest.mark.parametrize("kw", ["has_vq", "continuous_actions", "extra_params"])
def test_remaining_refusals_name_their_option(kw):
    with pytest.raises(NotImplementedError, match=kw + "=True"):
        _policy("mlp", **{kw: True})
    with pytest.raises(NotImplementedError, match=kw + "=True"):
        _policy("mlp", logsumexp_logits_is_v=True, **{kw: True})


def test_initialize_model_passes_the_hyperparameter():
    import train
    assert "logsumexp_logits_is_v" in train.OVERRIDE_FIRST
    env = types.SimpleNamespace(observation_space=types.SimpleNamespace(shape=(3, 64, 64)), action_space=types.SimpleNamespace(n=15))
    hp = train.get_hyperparams("hard-500")
    _, _, policy = train.initialize_model(torch.device("cpu"), env, dict(hp, logsumexp_logits_is_v=True))
    assert policy.logsumexp_logits_is_v is True
    _, _, policy = train.initialize_model(torch.device("cpu"), env, hp)
    assert policy.logsumexp_logits_is_v is False
    env = types.SimpleNamespace(observation_space=types.SimpleNamespace(shape=(9,)), action_space=types.SimpleNamespace(n=2))
    _, _, policy = train.initialize_model(torch.device("cpu"), env, dict(architecture="mlpmodel", logsumexp_logits_is_v=True))
    assert policy.logsumexp_logits_is_v is True and policy.arch == "mlp"
    # no command-line flag: the reference has none
    import argparse
    with pytest.raises(SystemExit):
        train.add_training_args(argparse.ArgumentParser()).parse_args(["--logsumexp_logits_is_v"])


class _StubEngine:
    """What DeviceAdam asks of an engine: flat moment vectors and a step."""

    def __init__(self, n):
        self.m, self.v, self.steps = np.zeros(n, np.float32), np.zeros(n, np.float32), 0

    def optimizer_step(self, lr, max_grad_norm, adam_step, want_norm=False):
        self.steps += 1
        self.m[:-65] += 0.25
        self.v[:-65] += 0.5
        return 1.0 if want_norm else None

    def get_adam_state(self):
        return self.m.copy(), self.v.copy()

    def set_adam_state(self, m, v):
        self.m, self.v = np.array(m, np.float32), np.array(v, np.float32)


def test_device_adam_leaves_fc_value_out_of_the_state():
    from mi355 import layout
    from mi355.optim import DeviceAdam
    ref = npz_json(LI.load("g14_lse_value.npz"), "mlp/step/opt")
    policy = _policy("mlp", logsumexp_logits_is_v=True)
    n = layout.flatten(policy.param_shapes(), policy._host_tensors()).size
    eng = _StubEngine(n)                                      # (fc_value = the last 64 + 1 entries of the flat vectors)
    opt = DeviceAdam(policy, eng, 5e-4)
    assert opt.state_dict()["state"] == {}
    opt.step(0.5)
    sd = opt.state_dict()
    P = ref["n_parameters"]
    assert len(list(policy.parameters())) == P and sorted(sd["state"]) == list(range(P - 2)) == [s[0] for s in ref["opt_state"]]
    assert sd["param_groups"][0]["params"] == list(range(P)) == ref["param_groups"][0]["params"]
    for (i, fields, step), (name, prm) in zip(ref["opt_state"], policy.named_parameters()):
        s = sd["state"][i]
        assert [[k, list(t.shape), str(t.dtype)] for k, t in s.items()] == fields, name
        assert float(s["step"]) == step == 1.0
    # a state without the two entries loads: zero moments for fc_value, the step count from the entries that exist
    eng2 = _StubEngine(n)
    opt2 = DeviceAdam(_policy("mlp", logsumexp_logits_is_v=True), eng2, 5e-4)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 1
    assert np.array_equal(eng2.m, eng.m) and np.array_equal(eng2.v, eng.v) and not eng2.m[-65:].any() and eng2.m[:-65].all()
    # flag off: every parameter has an entry, as before
    eng3 = _StubEngine(n)
    opt3 = DeviceAdam(_policy("mlp"), eng3, 5e-4)
    opt3.step(0.5)
    eng3.m[-65:] = 0.125; eng3.v[-65:] = 0.75                   # (the fc_value head is trained there: non-zero moments)
    sd_off = opt3.state_dict()
    assert sorted(sd_off["state"]) == list(range(P)) and sd_off["state"][P - 1]["exp_avg"].any()
    # such a checkpoint loaded with the flag on: fc_value's moments go up as zeros (they would move it under a zero gradient) and its
    # entries are dropped, so what is written next has this mode's layout
    eng4 = _StubEngine(n)
    opt4 = DeviceAdam(_policy("mlp", logsumexp_logits_is_v=True), eng4, 5e-4)
    opt4.load_state_dict(sd_off)
    assert opt4.step_count == 1 and not eng4.m[-65:].any() and not eng4.v[-65:].any()
    assert np.array_equal(eng4.m[:-65], eng3.m[:-65]) and np.array_equal(eng4.v[:-65], eng3.v[:-65])
    assert sorted(opt4.state_dict()["state"]) == list(range(P - 2))


def test_config_struct_keeps_its_size_and_offsets():
    from mi355.engine import _Config
    assert ctypes.sizeof(_Config) == 72
    assert _Config.value_from_logits.offset == 44 and _Config.reserved.offset == 48 and _Config.reserved.size == 16
    assert _Config.precision.offset == 40 and _Config.stream.offset == 64
    assert _Config().value_from_logits == 0


def test_recurrent_ppo_pure_with_the_flag_is_refused():
    from agents.ppo_pure import PPOPure
    policy = _policy("mlp", recurrent=True, logsumexp_logits_is_v=True)
    with pytest.raises(NotImplementedError, match="logsumexp_logits_is_v"):
        PPOPure(None, policy, None, None, torch.device("cpu"), 1, n_steps=8, n_envs=8, n_minibatch=2, mini_batch_size=32)
