"""Policy distillation (distill.py, mi_distill_*), the parts that need no GPU: the five new names in the header, the library and the
binding; the script's flags; every Python-side refusal, by name and before an engine exists; fixture G19's own consistency and the
float64 restatement of tests/distill_inputs.py against it.  Every test here fails without the feature."""
import os
import re

import numpy as np
import pytest
import torch

import distill_inputs as DI
from conftest import ROOT, npz_json

torch.set_num_threads(8)
NAMES = ("mi_distill_label", "mi_distill_minibatch", "mi_distill_loss", "mi_optimizer_step_eps", "mi_op_distill_loss")


def test_header_library_and_binding_export_the_five_names():
    text = open(os.path.join(ROOT, "include", "mi355ppo.h")).read()
    for sig in (r"int mi_distill_label\(mi_ctx\* data, mi_ctx\* teacher\);",
                r"int mi_distill_minibatch\(mi_ctx\* student, const int64_t\* idx, int32_t n, int32_t n_global\);",
                r"int mi_distill_loss\(mi_ctx\* student, mi_ctx\* data, float\* loss_out\);",
                r"int mi_optimizer_step_eps\(mi_ctx\* ctx, float lr, float max_grad_norm, float eps, int32_t adam_step, float\* grad_norm_out\);",
                r"int mi_op_distill_loss\(mi_ctx\* ctx, int32_t n, int32_t A, const float\* hout, const float\* target, int32_t n_global, float\* rec8_out, float\* dY_out\);"):
        assert re.search(sig, text), sig
    from mi355 import engine
    lib = engine.load_library()
    for n in NAMES:
        assert n in engine.EXPORTS and hasattr(lib, n), n
    for m in ("distill_label", "distill_minibatch", "distill_loss", "optimizer_step_eps", "op_distill_loss"):
        assert callable(getattr(engine.Engine, m)), m


def test_parser_has_the_references_flags_and_defaults():
    import distill
    a = distill.parse_args([])
    want = dict(lr=1e-4, batch_size=8192, nb_epoch=10, explore_size=256 * 256, n_explore=300, num_checkpoints=1, start_level=0,
                num_levels=500, distribution_mode="easy", num_threads=8, use_wandb=False, wandb_tags=None, mirror_env=False, gpu_device=0)
    for k, v in want.items():
        assert getattr(a, k) == v, (k, getattr(a, k), v)
    assert isinstance(a.seed, int) and 0 <= a.seed <= 9999
    assert a.device == "gpu"                                   # (the reference's default is cpu, which has no meaning here: refused below)
    assert (a.env_name, a.param_name, a.model_file, a.teacher_param_name, a.precision) == ("coinrun", "hard-500", None, None, None)
    b = distill.parse_args(["--lr", "3e-4", "--batch_size", "32", "--nb_epoch", "2", "--explore_size", "64", "--n_explore", "3", "--seed", "5",
                            "--num_checkpoints", "2", "--start_level", "7", "--num_levels", "9", "--distribution_mode", "hard", "--num_threads", "2",
                            "--device", "gpu", "--use_wandb", "--wandb_tags", "a", "b", "--mirror_env", "--env_name", "cartpole",
                            "--param_name", "cartpole", "--model_file", "x.pth", "--teacher_param_name", "cartpole", "--precision", "bf16"])
    assert (b.lr, b.batch_size, b.nb_epoch, b.explore_size, b.n_explore, b.seed, b.wandb_tags, b.precision) == (3e-4, 32, 2, 64, 3, 5, ["a", "b"], "bf16")


class Reached(Exception):
    pass


def _ckpt(tmp_path, obs_dim=9, A=2, name="model_100.pth"):
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(1)
    path = tmp_path / name
    torch.save({"model_state_dict": CategoricalPolicy(MLPModel(obs_dim, 4, 256, 64), False, A).state_dict()}, path)
    return str(path)


def test_refusals_fire_by_name_before_an_env_or_an_engine_exists(monkeypatch, tmp_path):
    import agents.ppo as P
    import distill
    import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(tmp_path)
    ck = _ckpt(tmp_path)
    cp = ["--env_name", "cartpole", "--param_name", "cartpole", "--model_file", ck, "--n_envs", "8", "--explore_size", "64",
          "--batch_size", "32", "--nb_epoch", "2", "--n_explore", "3", "--seed", "3"]
    run = lambda extra=(), base=cp: distill.distill(distill.parse_args(list(base) + list(extra)))
    real_make_env = train.make_env

    def built(env_name, *a, **k):
        raise Reached(env_name)
    monkeypatch.setattr(train, "make_env", built)
    with pytest.raises(Reached, match="cartpole"):                                   # past every refusal, at the env's construction
        run()
    monkeypatch.setattr(train, "make_env", lambda *a, **k: pytest.fail("an env was built"))
    with pytest.raises(NotImplementedError, match="--device must be 'gpu', not cpu"):
        run(["--device", "cpu"])
    with pytest.raises(ValueError, match="--model_file is required"):
        run(base=[a for a in cp if a not in ("--model_file", ck)])
    with pytest.raises(FileNotFoundError, match="no such file"):
        run(["--model_file", str(tmp_path / "absent.pth")])
    base = train.get_hyperparams
    monkeypatch.setattr(train, "get_hyperparams", lambda name: dict(base(name), recurrent=True))
    with pytest.raises(NotImplementedError, match="recurrent: True on the student"):
        run()
    monkeypatch.setattr(train, "get_hyperparams", lambda name: dict(base(name), recurrent=name == "mountain_car"))
    with pytest.raises(NotImplementedError, match="recurrent: True on the teacher"):
        run(["--teacher_param_name", "mountain_car"])
    monkeypatch.setattr(train, "get_hyperparams", lambda name: dict(base(name), logsumexp_logits_is_v=True))
    with pytest.raises(NotImplementedError, match="logsumexp_logits_is_v on the student"):
        run()
    monkeypatch.setattr(train, "get_hyperparams", base)
    with pytest.raises(NotImplementedError, match="different observation shapes.*mlpmodel.*impala"):
        run(["--teacher_param_name", "hard-500"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="single GPU: WORLD_SIZE = 2"):
        run()
    monkeypatch.delenv("WORLD_SIZE")
    # the checkpoint against the env: the envs exist, an engine must not
    monkeypatch.setattr(train, "make_env", real_make_env)
    monkeypatch.setattr(P, "Engine", lambda *a, **k: pytest.fail("an engine was created"))
    with pytest.raises(NotImplementedError, match="different action counts.*has 2.*checkpoint 3"):
        run(["--model_file", _ckpt(tmp_path, 9, 3, "model_3.pth")])
    with pytest.raises(NotImplementedError, match="different observation shapes.*takes 5 inputs"):
        run(["--model_file", _ckpt(tmp_path, 5, 2, "model_5.pth")])

    def engine(*a, **k):
        raise Reached("engine")
    monkeypatch.setattr(P, "Engine", engine)
    with pytest.raises(Reached, match="engine"):                                     # a matching pair reaches the engines
        run()
    assert distill.newest_checkpoint(str(tmp_path)).endswith("model_100.pth")       # the reference's rule for a run directory


def test_g19_is_consistent():
    z = DI.load()
    names, state_names = npz_json(z, "tensor_names"), npz_json(z, "state_names")
    assert z["obs"].shape == (96, 9) and z["y_gold"].shape == (96, 2) and z["loss"].shape == (6,) and int(z["adam_step"]) == 6
    assert (int(z["batch"]), int(z["epochs"]), float(z["lr"])) == (32, 2, 1e-3)
    assert list(DI.fixture_params(z, "student/")) == names
    assert state_names == [n for n in names if not n.startswith("fc_value")] and len(names) == len(state_names) + 2
    assert np.abs(np.logaddexp.reduce(z["y_gold"].astype(np.float64), axis=1)).max() < 1e-6          # the targets are normalised log-probabilities
    assert z["step_norms"].shape == (6, 2, len(state_names)) and np.isfinite(z["step_norms"]).all() and (z["step_norms"][:, 1] > 0).all()
    for k in range(6):
        assert set(DI.fixture_params(z, f"g{k}/")) == set(state_names), k            # fc_value's gradient is None: absent
        assert list(DI.fixture_params(z, f"p{k}/")) == names
        for n in ("fc_value.weight", "fc_value.bias"):                               # ... and Adam never touches it
            assert np.array_equal(z[f"p{k}/{n}"], z["student/" + n])
        prev = DI.fixture_params(z, f"p{k - 1}/" if k else "student/")
        assert all(np.abs(z[f"p{k}/{n}"] - prev[n]).max() > 0 for n in state_names)
    # the teacher's logits are the teacher's: the float64 restatement on the stored teacher reproduces them
    lp, _ = DI.forward({k: torch.from_numpy(v.astype(np.float64)) for k, v in DI.fixture_params(z, "teacher/").items()}, "mlp",
                       torch.from_numpy(z["obs"].astype(np.float64)))
    assert np.abs(lp.numpy() - z["y_gold"]).max() < 2e-6


def test_float64_restatement_reproduces_g19_losses_and_gradients():
    """Every step from the fixture's own parameters (no Adam in between): the loss to 2e-6 relative -- float32's eps on a mean of 64
    terms, generously -- and every gradient to 1e-5 relative L2 (the reference's float32 autograd against float64: worst tensor measured 4.7e-7)."""
    z = DI.load()
    worst = 0.0
    for k, rows in DI.batches(z):
        params = DI.fixture_params(z, f"p{k - 1}/" if k else "student/")
        loss, grads = DI.minibatch(params, "mlp", z["obs"][rows], z["y_gold"][rows])
        assert abs(loss - float(z["loss"][k])) < 2e-6 * abs(loss), (k, loss, float(z["loss"][k]))
        assert set(grads) == set(DI.fixture_params(z, f"g{k}/")), k
        for n, g in grads.items():
            worst = max(worst, DI.rel_l2(z[f"g{k}/{n}"], g))
            assert DI.rel_l2(z[f"g{k}/{n}"], g) < 1e-5, (k, n)
    print("worst gradient error of the fixture against float64:", worst)


def test_loss_restatement_on_head_rows():
    """mse() is MSELoss(Categorical(logits=log_softmax(z)).logits, y) with its autograd gradient: against torch's own classes; the value
    column gets no gradient; the row that equals its target gets none either; n_global scales loss and gradient."""
    from torch.distributions import Categorical
    hout, y = DI.op_case(65, 9)
    loss, dY, terms = DI.mse(hout, y)
    h = torch.from_numpy(hout.astype(np.float64)).requires_grad_(True)
    ref = torch.nn.MSELoss()(Categorical(logits=torch.log_softmax(h[:, :9], dim=1)).logits, torch.from_numpy(y.astype(np.float64)))
    ref.backward()
    assert abs(loss - float(ref.detach())) < 1e-12 * abs(loss) and np.abs(dY - h.grad.numpy()).max() < 1e-15
    assert not dY[:, 9].any() and np.abs(dY[1]).max() < 1e-80 and terms[0] > 1e4 and abs(terms.sum() / (65 * 9) - loss) < 1e-12 * loss
    loss2, dY2, _ = DI.mse(hout, y, n_global=130)
    assert abs(loss2 - loss / 2) < 1e-15 and np.abs(dY2 - dY / 2).max() < 1e-18
    terr, rms_q = DI.torch_errors(65, 9)
    assert 0 < terr < 1e-5 and 0 < rms_q
