"""The sparse-autoencoder agent (`algo: sae`; reference agents/sae.py), host side: the models' initialisation and state_dict against
fixture G15 (tests/golden/make_golden_sae.py ran the reference), the CLI / hyper-parameter surface, the refusals, the feature column
permutation, the torch restatement of tests/sae_inputs.py against G15, and SAE.train's control flow on a fake engine and env.  CPU only.

Bounds of the restatement against the fixture: it is the same arithmetic as the reference's methods (same torch ops in the same
order), so only the thread-dependent summation order of torch's CPU kernels may differ: losses 1e-5 relative, tensors 2e-4 of
their L2 norm (the Adam step divides by sqrt(v) + 1e-5 and so amplifies the last bits of small gradients)."""
import argparse
import hashlib
import os

import numpy as np
import pytest
import torch

import sae_inputs as SI
from conftest import load_npz, npz_json

torch.set_num_threads(8)


@pytest.fixture(scope="module")
def z():
    return load_npz("g15_sae.npz")


def _models(c):
    from common.model import LinearSAEProbe, SparseAutoencoder
    return SI.make_models(c, SparseAutoencoder, LinearSAEProbe)


def _sha(module):
    return hashlib.sha256(np.concatenate([p.detach().numpy().ravel() for p in module.parameters()]).astype(np.float32).tobytes()).hexdigest()


@pytest.mark.parametrize("name", list(SI.CASES))
def test_seeded_init_and_state_dict_match_the_reference(z, name):
    want = npz_json(z, f"init/{name}")
    for key, model in zip(("sae", "probe"), _models(SI.CASES[name])):
        assert _sha(model) == want[key]["sha256"], key
        assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == want[key]["keys"], key
    sae, probe = _models(SI.CASES[name])
    assert list(sae.state_dict()) == ["encoder.0.weight", "encoder.0.bias", "decoder.0.weight", "decoder.0.bias"]
    assert list(probe.state_dict()) == ["fc_policy.weight", "fc_policy.bias", "fc_value.weight", "fc_value.bias"]
    assert sae.rho == SI.RHO
    with pytest.raises(NotImplementedError, match="engine"):
        sae(torch.zeros(1, SI.D))


def test_cli_accepts_sae_and_still_refuses_espo():
    import train
    parse = train.add_training_args(argparse.ArgumentParser()).parse_args
    assert parse(["--algo", "sae", "--param_name", "sae"]).algo == "sae"
    with pytest.raises(SystemExit):
        parse(["--algo", "espo"])


def test_sae_hyperparameter_set_is_the_references():
    import train
    hp = train.get_hyperparams("sae")
    # the reference's `sae` set (hyperparams/procgen/config.yml), keys and values as there
    assert hp == dict(algo="sae", n_envs=256, n_steps=256, epoch=3, mini_batch_per_epoch=8, mini_batch_size=8192, gamma=0.999, lmbda=0.95,
                      learning_rate=0.0005, grad_clip_norm=0.5, eps_clip=0.2, value_coef=0.5, entropy_coef=0.01, normalize_adv=True,
                      normalize_rew=True, use_gae=True, architecture="impala", recurrent=False, sae_dim=1024, close_envs=True, anneal_lr=False)
    assert list(hp)[:2] == ["algo", "n_envs"]
    with pytest.raises(KeyError):
        train.get_hyperparams("hard-500-impalavq")
    assert train.get_hyperparams("hard-500")["algo"] == "ppo"


def _policy(arch="impala", recurrent=False, A=15):
    from common.model import ImpalaModel, MLPModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(1)
    emb = ImpalaModel(3) if arch == "impala" else MLPModel(9, 4, 64, 64)
    return CategoricalPolicy(emb, recurrent, A)


def test_refusals_name_their_option(monkeypatch):
    from agents.sae import check_supported
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    check_supported(_policy(), 8, None, 1024)
    with pytest.raises(NotImplementedError, match="mlpmodel"):
        check_supported(_policy("mlp", A=2), 8)
    with pytest.raises(NotImplementedError, match="recurrent"):
        check_supported(_policy(recurrent=True), 8)
    with pytest.raises(NotImplementedError, match="sae_dim=100"):
        check_supported(_policy(), 8, None, 100)
    groups = type("Env", (), {"env_groups": (1, 2)})()
    with pytest.raises(NotImplementedError, match="rollout_groups"):
        check_supported(_policy(), 8, groups)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        check_supported(_policy(), 8)
    from common.storage import SAEStorage
    with pytest.raises(NotImplementedError, match="mlpmodel"):
        SAEStorage((9,), 2048, 4, 4, None, act_shape=2)
    st = SAEStorage((3, 64, 64), 2048, 4, 4, None, act_shape=15)
    with pytest.raises(NotImplementedError, match="recurrent"):
        next(st.fetch_train_generator(4, recurrent=True))


def test_train_refuses_sae_without_a_model_file():
    import train
    args = train.add_training_args(argparse.ArgumentParser()).parse_args(["--algo", "sae", "--param_name", "sae", "--env_name", "synthetic"])
    with pytest.raises(ValueError, match="--model_file"):
        train.train_ppo(args)


def test_feature_column_permutation_round_trips():
    from mi355 import layout
    idx = layout.feature_device_index()
    assert sorted(idx.tolist()) == list(range(2048))
    # reference column ch*64 + p is the device's p*32 + ch: the Flatten() of NCHW against the engine's NHWC block output
    nchw = np.arange(2 * 32 * 8 * 8, dtype=np.float32).reshape(2, 32, 8, 8)
    ref, dev = nchw.reshape(2, -1), nchw.transpose(0, 2, 3, 1).reshape(2, -1)
    assert np.array_equal(layout.features_to_device(ref), dev)
    assert np.array_equal(layout.features_from_device(dev), ref)
    x = np.random.default_rng(0).standard_normal((3, 5, 2048)).astype(np.float32)
    assert np.array_equal(layout.features_from_device(layout.features_to_device(x)), x)


def test_index_stream_is_the_references_draw(z):
    """SAEStorage.fetch_train_generator yields the index vectors the reference's BatchSampler(SubsetRandomSampler) drew (fixture G2's rule)."""
    from common.storage import SAEStorage
    for name, c in SI.CASES.items():
        mbs, _ = SI.accumulation(c)
        st = SAEStorage((3, 64, 64), SI.D, c["T"], c["E"], None, act_shape=c["A"])
        for stage, off in (("sae", 100), ("probe", 200)):
            torch.manual_seed(c["seed"] + off)
            got = [idx for _ in range(c["epoch"]) for idx in st.fetch_train_generator(mbs, recurrent=False)]
            assert np.array_equal(np.stack(got), z[f"{name}/idx_{stage}"]), (name, stage)


@pytest.mark.parametrize("name", list(SI.CASES))
def test_restatement_matches_the_reference(z, name):
    """tests/sae_inputs.replay in float32 is the reference's optimize_sae / optimize_linear_model; in float64 the pairwise value loss
    differs from the per-sample one on these inputs, and every unit keeps 0 < rho_hat < 1."""
    c, roll, idx_sae, idx_probe = SI.load_case(z, name)
    init = {k: v.detach().numpy() for m in _models(c) for k, v in m.state_dict().items()}
    out = SI.replay(c, init, roll, idx_sae, idx_probe, torch.float32)
    for stage in ("sae", "probe"):
        pre = f"{name}/{stage}/"
        np.testing.assert_allclose(out[stage]["losses"], z[pre + "losses"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(out[stage]["losses"].mean(0)[[2, 0, 1]], z[pre + "summary"], rtol=1e-5, atol=1e-7)
        for kind, key in (("g0", "g0/"), ("params", "p/"), ("m", "m/"), ("v", "v/")):
            for n, a in out[stage][kind].items():
                err = SI.tensor_error(a, z, pre + key, n)
                assert err < 2e-4, (stage, kind, n, err)
    assert npz_json(z, f"{name}/sae/summary_keys") == ["Loss/total", "Loss/recon", "Loss/sparsity"]
    assert npz_json(z, f"{name}/probe/summary_keys") == ["Loss/total_linear", "Loss/value", "Loss/logit"]
    P = {k: torch.from_numpy(init[k]).double() for k in SI.SAE_KEYS}
    Q = {k: torch.from_numpy(init[k]).double() for k in SI.PROBE_KEYS}
    T, E = c["T"], c["E"]
    x = torch.from_numpy(roll["hidden"][:T].reshape(T * E, -1)).double()
    for idx in idx_sae[:c["mini_batch_per_epoch"]]:
        rho_hat = SI.sae_losses(P, x[idx])[2]
        assert (rho_hat > 0).all() and (rho_hat < 1).all()
    idx = torch.as_tensor(idx_probe[0])
    vl, _, per_sample = SI.probe_losses(P, Q, x[idx], torch.from_numpy(roll["logits"].reshape(T * E, -1)).double()[idx],
                                        torch.from_numpy(roll["value"][:T].reshape(-1)).double()[idx])
    assert abs(float(vl) - float(per_sample)) > 1e-2 * float(per_sample)      # (fp32 resolves 1e-6 of it)


# ------------------------------------------------------------------------------------------ SAE.train on a fake engine and env
class FakeEngine:
    """What agents.sae.SAE, SAEStorage and DeviceModelAdam call, recording the calls; no arithmetic."""
    SAE, PROBE = 0, 1
    SAE_DIMS = tuple(range(64, 4097, 64))

    def __init__(self, T, E, A):
        self.T, self.E, self.A = T, E, A
        self.steps, self.minibatches, self.opt_steps, self.params = [], [], [], {}

    def set_params(self, flat):
        self.policy_flat = np.array(flat)

    def pinned(self, shape, dtype):
        return np.zeros(shape, dtype)

    def sae_create(self, sae_dim, rho):
        self.sae_dim, self.rho = sae_dim, rho

    def sae_set_params(self, which, flat):
        self.params[which] = np.array(flat, np.float32)

    def sae_get_params(self, which):
        return self.params[which].copy()

    def sae_get_adam_state(self, which):
        n = self.params[which].size
        return np.full(n, 0.5, np.float32), np.full(n, 0.25, np.float32)

    def sae_set_adam_state(self, which, m, v):
        self.adam = getattr(self, "adam", {})
        self.adam[which] = (np.array(m, np.float32), np.array(v, np.float32))

    def sae_step(self, t, obs, act_from_probe=False, store=True, seed=0, u=None):
        self.steps.append((t, int(obs[0, 0, 0, 0]), bool(act_from_probe), bool(store)))
        return np.zeros(self.E, np.int64), np.zeros(self.E, np.float32)

    def put_step(self, t, rew, done):
        pass

    def sae_minibatch(self, idx, sparse_coef):
        self.minibatches.append(("sae", len(idx)))
        return np.array([1.0, 2.0, 3.0], np.float32)

    def sae_probe_minibatch(self, idx):
        self.minibatches.append(("probe", len(idx)))
        return np.array([4.0, 5.0, 9.0], np.float32)

    def sae_optimizer_step(self, which, lr, max_grad_norm, adam_step, want_norm=False):
        self.opt_steps.append((which, lr, adam_step))
        self.params[which] = self.params[which] + 1.0


class FakeEnv:
    """reset() hands out frames filled with 7; the k-th step's frames are filled with 10 + k."""

    def __init__(self, E):
        self.E, self.k, self.closed = E, 0, False

    def reset(self):
        return np.full((self.E, 64, 64, 3), 7, np.uint8)

    def step(self, act):
        self.k += 1
        return np.full((self.E, 64, 64, 3), 10 + self.k % 200, np.uint8), np.ones(self.E, np.float32), np.zeros(self.E, bool), [{}] * self.E

    def close(self):
        self.closed = True


def test_train_control_flow_on_a_fake_engine(tmp_path, monkeypatch):
    from agents.sae import SAE
    from common.logger import SimpleLogger
    from common.storage import SAEStorage
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    T, E, A, S, N = 2, 2, 15, 64, 8
    eng = FakeEngine(T, E, A)
    monkeypatch.setattr(SAE, "_make_engine", lambda self, policy, device, max_batch: eng)
    dumps = []

    class Rec(SimpleLogger):
        def dump(self, summary={}, lr=0.):
            dumps.append((dict(summary), lr, self.timesteps))
            super().dump(summary, lr)

    logger = Rec(E, str(tmp_path))
    env, env_v = FakeEnv(E), FakeEnv(E)
    mk = lambda: SAEStorage((3, 64, 64), 2048, T, E, None, act_shape=A)
    agent = SAE(env, _policy(A=A), logger, mk(), torch.device("cpu"), 2, env_valid=env_v, storage_valid=mk(), n_steps=T, n_envs=E, epoch=1,
                mini_batch_per_epoch=2, mini_batch_size=2, learning_rate=1e-3, sae_dim=S, anneal_lr=True)
    # reference defaults kept
    import inspect
    d = {k: v.default for k, v in inspect.signature(SAE.__init__).parameters.items()}
    assert (d["mini_batch_per_epoch"], d["sae_dim"], d["rho"], d["sparse_coef"], d["anneal_lr"], d["close_envs"]) == (8, 1024, 0.05, 1e-3, True, True)
    assert eng.params[0].size == 2 * S * 2048 + S + 2048 and eng.params[1].size == (A + 1) * S + A + 1
    agent.train(N)
    # self.t is shared: stage 1 runs to N, stage 2 from N to 2 N
    assert agent.t == 2 * N
    assert [d[2] for d in dumps] == [4, 8, 12, 16]
    assert [list(d[0]) for d in dumps] == [["Loss/total", "Loss/recon", "Loss/sparsity"]] * 2 + [["Loss/total_linear", "Loss/value", "Loss/logit"]] * 2
    assert dumps[0][0] == {"Loss/total": 3.0, "Loss/recon": 1.0, "Loss/sparsity": 2.0}
    assert dumps[2][0] == {"Loss/total_linear": 9.0, "Loss/value": 4.0, "Loss/logit": 5.0}
    # anneal_lr anneals the SAE's optimizer against the stage's horizon, also in stage 2 (agents/sae.py:257-258)
    assert [round(d[1], 9) for d in dumps] == [0.0005, 0.0, 0.00025, 0.0]
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".pth")) == ["linear_12.pth", "sae_8.pth"]
    sae_ck = torch.load(tmp_path / "sae_8.pth", weights_only=True)
    lin_ck = torch.load(tmp_path / "linear_12.pth", weights_only=True)
    assert list(sae_ck["model_state_dict"]) == list(SI.SAE_KEYS) and list(lin_ck["model_state_dict"]) == list(SI.PROBE_KEYS)
    from common.model import LinearSAEProbe, SparseAutoencoder
    ref_sae, ref_lin = SparseAutoencoder(2048, S, 0.05), LinearSAEProbe(S, A)
    ref_sae.load_state_dict(sae_ck["model_state_dict"]); ref_lin.load_state_dict(lin_ck["model_state_dict"])
    torch.optim.Adam(ref_sae.parameters(), lr=1e-3, eps=1e-5).load_state_dict(sae_ck["optimizer_state_dict"])
    torch.optim.Adam(ref_lin.parameters(), lr=1e-3, eps=1e-5).load_state_dict(lin_ck["optimizer_state_dict"])
    assert float(sae_ck["optimizer_state_dict"]["state"][0]["step"]) == 4.0 and float(lin_ck["optimizer_state_dict"]["state"][0]["step"]) == 2.0
    # the checkpoint holds the DEVICE's parameters (pulled before saving): the fake adds 1 per optimizer step
    assert torch.equal(sae_ck["model_state_dict"]["encoder.0.bias"], torch.full((S,), 4.0))
    # every rollout starts from the reset observation (7): collect_rollouts does not hand the last observation back; the training
    # rollout stores, the validation rollout does not; stage 2 acts from the probe
    per_iter = 2 * (T + 1)
    assert len(eng.steps) == 4 * per_iter
    for it in range(4):
        tr, va = eng.steps[it * per_iter:it * per_iter + T + 1], eng.steps[it * per_iter + T + 1:(it + 1) * per_iter]
        assert [s[0] for s in tr] == [0, 1, 2] and [s[0] for s in va] == [0, 1, 2]
        assert tr[0][1] == 7 and va[0][1] == 7 and tr[1][1] != 7
        assert all(s[3] for s in tr) and not any(s[3] for s in va)
        assert all(s[2] == (it >= 2) for s in tr + va)
    assert eng.minibatches == [("sae", 2)] * 4 + [("probe", 2)] * 4
    assert [s[0] for s in eng.opt_steps] == [0] * 4 + [1] * 4
    assert env.closed and env_v.closed
    for name in ("predict_for_logit_saliency", "predict_for_rew_saliency"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(agent, name)(None, None)


def test_device_adam_state_round_trips_through_torch_adam():
    """DeviceModelAdam.state_dict() is what a stock torch.optim.Adam over the same module loads, and load_state_dict() hands a stock
    optimizer's moments and step count to the engine, flat in parameters() order."""
    from common.model import LinearSAEProbe
    from mi355.optim import DeviceModelAdam
    torch.manual_seed(0)
    eng, model = FakeEngine(2, 2, 9), LinearSAEProbe(64, 9)
    stock = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-5)
    for p in model.parameters():
        p.grad = torch.randn_like(p)
    stock.step(); stock.step()
    opt = DeviceModelAdam(LinearSAEProbe(64, 9), eng, FakeEngine.PROBE, 1e-3)
    opt.load_state_dict(stock.state_dict())
    assert opt.step_count == 2
    st = stock.state_dict()["state"]
    m, v = eng.adam[FakeEngine.PROBE]
    assert np.array_equal(m, np.concatenate([st[i]["exp_avg"].numpy().ravel() for i in range(4)]))
    assert np.array_equal(v, np.concatenate([st[i]["exp_avg_sq"].numpy().ravel() for i in range(4)]))
    opt.push_params()
    back = opt.state_dict()                                   # (the fake engine answers 0.5 / 0.25 for the moments)
    assert float(back["state"][0]["step"]) == 2.0 and back["param_groups"][0]["eps"] == 1e-5
    torch.optim.Adam(LinearSAEProbe(64, 9).parameters(), lr=1e-3, eps=1e-5).load_state_dict(back)
