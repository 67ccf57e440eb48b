"""The one-launch evaluation of the device-resident envs (csrc/env_evaluate.hip, mi_env_evaluate, Engine.env_evaluate, PPO.evaluate,
evaluate.py) against the float64 CPU oracle of tests/evaluate_inputs.py, beside the merged resident rollout kernel, and through the agent
and the command line.

The oracle's cases are checked on the CPU in tests/test_evaluate_host.py: every env margin holds, no sampler uniform is within 1e-4 of a
float64 CDF edge, every greedy row's two largest log-probabilities are 1e-3 apart -- so the device's actions, and with them the lengths,
the termination flags and the constant-reward returns, are expected to BE the oracle's.  Dense returns: within ENV_MARGIN = 1e-9 per
episode (the device's cos / sin against numpy's in the last digit).  value0: relative L2 error against float64 <= 8 x the error of torch's
own float32 CPU evaluation of the same network (policy_inputs.check_measured: the bound of the resident-rollout test).  The measured
figures are printed and on record in profiles/env_evaluate.md."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import evaluate_inputs as EI
import policy_inputs as PI
import resident_inputs as RI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "train-procgen-pytorch_amd")
RECORDS = ("ret", "length", "terminated", "value0", "start")


def _engine(c, T=2, **kw):
    from mi355.engine import Engine
    E = c["E"]
    kw = dict(dict(mlp_depth=c["depth"], mlp_width=c["width"], out_dim=c["out"]), **kw)
    return Engine("mlp", T, E, RI.ACTIONS[c["kind"]], E, obs_dim=RI.WIDTH[c["kind"]], value_from_logits=bool(c["lse"]), **kw)


def _device_env(c, eng):
    from common.env.vec_envs import DeviceCartPole, DeviceCartPoleSwing, DeviceMountainCar
    cls = {"cartpole": DeviceCartPole, "cartpole_swing": DeviceCartPoleSwing, "mountain_car": DeviceMountainCar}[c["env"]]
    env = cls(eng.E, seed=c["env_seed"], **EI.env_kwargs(c))
    env.attach_engine(eng)
    return env


def _same_bytes(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in RECORDS)


# ------------------------------------------------------------------------------------------ 1: the records against the oracle
@pytest.mark.parametrize("name", list(EI.CASES))
def test_records_match_the_float64_oracle(name):
    o = EI.oracle(name)
    c, flat, want = o["c"], o["flat"], o["ev"]
    eng = _engine(c)
    eng.set_params(flat)
    _device_env(c, eng)
    got = eng.env_evaluate(c["K"], seed=c["seed"], greedy=c["greedy"], starts=o["starts"])
    eng.close()
    E, K = c["E"], c["K"]
    assert got["ret"].dtype == np.float64 and got["length"].dtype == np.int32 and got["terminated"].dtype == np.int32
    assert got["value0"].dtype == np.float32 and got["start"].dtype == np.float64 and got["ret"].shape == (E, K)
    assert got["start"].tobytes() == np.ascontiguousarray(want["start"]).tobytes()      # bit for bit: the planted row or the reset stream
    assert np.array_equal(got["length"], want["length"]), name
    assert np.array_equal(got["terminated"], want["terminated"]), name
    diff = np.abs(got["ret"] - want["ret"])
    if name in EI.DENSE:
        print(f"{name}: dense return, largest difference from the float64 replay per episode: {diff.max():.3e} (bound {EI.ENV_MARGIN:g})")
        assert (diff <= EI.ENV_MARGIN).all(), (name, diff.max())
    else:
        assert np.array_equal(got["ret"], want["ret"]) and np.array_equal(got["ret"], want["length"].astype(np.float64)), name
    terr_v, _ = RI.torch_errors(c, flat, want["obs"])
    ev, _ = PI.check_measured(got["value0"], want["value0"], terr_v, what=name + " value0")
    print(f"{name}: value0 error {ev:.3e} = {ev / terr_v:.2f} x torch float32's {terr_v:.3e} (bound: 8 x)")


# ------------------------------------------------------------------------------------------ 2: beside the resident rollout kernel
def test_the_episodes_of_the_rollout_kernel_are_the_evaluations():
    """From the evaluation's start states and episode counters, mi_env_rollout_resident with the same sampler seed on a context whose
    T = 15 covers the whole evaluation: the first K episodes of every env in its reward / done rings have the evaluation's lengths and
    returns, and their starts are the evaluation's start rows."""
    from mi355.engine import F_DONE, F_REW
    o = EI.oracle("cartpole_sampled")
    c, flat = o["c"], o["flat"]
    E, K, T = c["E"], c["K"], 15
    assert T == K * o["max_steps"]
    eng = _engine(c, T=T)
    eng.set_params(flat)
    _device_env(c, eng).reset()
    ev = eng.env_evaluate(K, seed=c["seed"])
    eng.env_set_state(ev["start"][:, 0], np.zeros(E, np.int32), np.full(E, EI.F_DEFAULT, np.int64))
    eng.env_rollout(c["seed"], resident=True)
    rew, done = eng.read_field(F_REW).astype(np.float64), eng.read_field(F_DONE) > 0
    obs = np.stack([eng.get_obs(t) for t in range(T + 1)])
    eng.close()
    for e in range(E):
        ends = np.nonzero(done[:, e])[0][:K]
        assert len(ends) == K
        first = np.concatenate([[0], ends[:-1] + 1])
        assert np.array_equal(ends + 1 - first, ev["length"][e]), e
        assert np.array_equal([rew[a:b + 1, e].sum() for a, b in zip(first, ends)], ev["ret"][e]), e
        assert np.array_equal(obs[first, e], ev["start"][e].astype(np.float32)), e


# ------------------------------------------------------------------------------------------ 3: purity
def test_an_evaluation_reads_and_writes_no_training_state():
    from mi355.engine import F_ACT, F_ADV, F_DONE, F_LOGP, F_RET, F_REW, F_VALUE
    o = EI.oracle("cartpole_sampled")
    c, flat = o["c"], o["flat"]
    K = c["K"]
    eng = _engine(c, T=4)
    eng.set_params(flat)
    _device_env(c, eng).reset()
    eng.env_rollout(3, resident=True)                        # rings and an env state in the middle of episodes

    def snapshot():
        return [a.tobytes() for a in eng.env_state()] + [eng.read_field(f).tobytes() for f in (F_ACT, F_LOGP, F_VALUE, F_REW, F_DONE, F_ADV, F_RET)] \
            + [eng.get_obs(t).tobytes() for t in range(eng.T + 1)]
    before = snapshot()
    a = eng.env_evaluate(K, seed=c["seed"])
    assert snapshot() == before
    eng.env_rollout(4, resident=True)                        # whatever the env does in between ...
    b = eng.env_evaluate(K, seed=c["seed"])
    assert _same_bytes(a, b)                                 # ... the same arguments give the same records
    other = eng.env_evaluate(K, seed=c["seed"], first_episode=EI.F_DEFAULT + K)
    assert not (other["start"][..., :4] == a["start"][..., :4]).any()      # (x, x_dot, theta, theta_dot: drawn from ranges of non-zero width)
    assert np.array_equal(eng.env_evaluate(2 * K, seed=c["seed"])["start"][:, K:], other["start"])      # (more episodes in one call; episode F + K + i)
    g = eng.env_evaluate(K, seed=1, greedy=True)
    assert _same_bytes(g, eng.env_evaluate(K, seed=2, greedy=True))      # greedy: the sampler's seed does not matter
    eng.close()


# ------------------------------------------------------------------------------------------ 4: refusals by name
def test_refusals_by_name_leave_the_records_alone():
    from mi355.engine import Engine, EngineError
    from common.env.vec_envs import DeviceCartPole
    E, K, W = 4, 2, 9
    rng = np.random.default_rng(9)
    mk = lambda **kw: Engine("mlp", 2, E, 2, E, obs_dim=W, **dict(dict(mlp_depth=4, mlp_width=64, out_dim=64), **kw))
    eng = mk()
    eng.set_params(0.2 * rng.standard_normal(eng.n_params).astype(np.float32))
    with pytest.raises(EngineError, match="no env"):
        eng.env_evaluate(K)
    DeviceCartPole(E, seed=1).attach_engine(eng)             # max_steps = 500
    # an accepted call straight through the C entry, then every refusal on the same output arrays: they stay as that call left them
    out = dict(ret=np.zeros((E, K)), length=np.zeros((E, K), np.int32), terminated=np.zeros((E, K), np.int32), value0=np.zeros((E, K), np.float32),
               start=np.zeros((E, K, W)))
    ptr = [out[k].ctypes.data_as(C.c_void_p) for k in RECORDS]

    def raw(episodes, first_episode=1 << 40, starts=None):
        s = None if starts is None else starts.ctypes.data_as(C.c_void_p)
        eng._chk(eng.lib.mi_env_evaluate(eng._ctx, C.c_int32(episodes), C.c_uint64(7), C.c_int32(0), C.c_int64(first_episode), s, *ptr))
    raw(K)
    assert (out["length"] >= 1).all() and np.array_equal(out["ret"], out["length"])
    kept = {k: out[k].copy() for k in RECORDS}
    nan = np.array(kept["start"])
    nan[E - 1, K - 1, W - 1] = np.nan
    for args, msg in (((0,), "mi_env_evaluate: episodes must be at least 1"),
                      ((-3,), "mi_env_evaluate: episodes must be at least 1"),
                      ((2098,), r"mi_env_evaluate: episodes \* max_steps must be at most 2\^20"),      # 2098 * 500 = 1 049 000 > 1 048 576
                      ((K, 0), "mi_env_evaluate: first_episode must be at least 1"),
                      ((K, 1 << 40, nan), "mi_env_evaluate: starts must not hold a NaN")):
        with pytest.raises(EngineError, match=msg):
            raw(*args)
        assert all(np.array_equal(out[k], kept[k]) for k in RECORDS), msg
    assert _same_bytes(eng.env_evaluate(K, seed=7), out)     # and the context still evaluates
    with pytest.raises(EngineError, match="starts must have 4 x 2 x 9 elements"):
        eng.env_evaluate(K, starts=np.zeros((E, K, W - 1)))
    # a context that got a GRU after its env
    H = 64
    eng.set_gru(*(0.1 * rng.standard_normal(n).astype(np.float32) for n in (3 * H * H, 3 * H * H, 3 * H, 3 * H)))
    with pytest.raises(EngineError, match="mi_env_evaluate: a recurrent context"):
        raw(K)
    assert all(np.array_equal(out[k], kept[k]) for k in RECORDS)
    eng.close()
    # a shape outside the 16-row tile's list
    eng = mk(mlp_width=72)
    DeviceCartPole(E, seed=1).attach_engine(eng)
    with pytest.raises(EngineError, match="mi_env_evaluate: mlp_width must be a multiple of 16 and at most 512"):
        eng.env_evaluate(K)
    eng.close()


# ------------------------------------------------------------------------------------------ 5: agent and command line
def test_ppo_evaluate_is_the_engines_evaluation():
    """PPO.evaluate(episodes=2) on a live agent between two training iterations: the records of Engine.env_evaluate with the same
    arguments plus their statistics, on either lane, and training goes on from the same env state."""
    from agents.ppo import PPO
    from common.env.vec_envs import DeviceCartPole
    from common.logger import EVALUATION_KEYS, Logger, evaluation_stats
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    T, E = 8, 8
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    kw = RI.ENV_KW["cartpole"]
    env, env_v = DeviceCartPole(E, seed=4, **kw), DeviceCartPole(E, seed=5, **kw)
    policy = CategoricalPolicy(MLPModel(9, 4, 64, 64), False, 2)
    agent = PPO(env, policy, Logger(E, None), Storage((9,), 64, T, E, dev), dev, 1, env_valid=env_v, storage_valid=Storage((9,), 64, T, E, dev),
                n_steps=T, n_envs=E, epoch=2, n_minibatch=2, mini_batch_size=32, gamma=0.99, lmbda=0.95, learning_rate=1e-3, entropy_coef=0.01,
                seed=0, detect_nan=True, resident_rollout=True)
    agent.train(T * E)
    state = [a.tobytes() for a in agent.engine.env_state()]
    for valid, eng in ((False, agent.engine), (True, agent.engine_valid)):
        out = agent.evaluate(episodes=2, valid=valid, seed=11)
        assert set(out) == set(RECORDS) | set(EVALUATION_KEYS)
        assert _same_bytes(out, eng.env_evaluate(2, seed=11))
        assert {k: out[k] for k in EVALUATION_KEYS} == evaluation_stats(out["ret"], out["length"], 5)
        assert out["ret"].shape == (E, 2) and (out["ret"] == out["length"]).all() and out["length"].max() <= 5
        assert _same_bytes(agent.evaluate(episodes=2, valid=valid), eng.env_evaluate(2, seed=agent.seed * 1000003 + agent._iter))
        g = agent.evaluate(episodes=2, valid=valid, greedy=True)
        assert _same_bytes(g, eng.env_evaluate(2, greedy=True))
    assert np.array_equal(agent.engine_valid.get_params(), agent.engine.get_params())      # the twin evaluated the current policy
    assert [a.tobytes() for a in agent.engine.env_state()] == state
    agent.engine.close(); agent.engine_valid.close()


def test_train_then_evaluate_py_on_both_ranges(tmp_path):
    """`python train.py --env_name cartpole --param_name cartpole --device_env --resident_rollout --fused_update` for one iteration with one
    checkpoint, then `python evaluate.py --model_file <it> --episodes 2 --both --n_envs 16`, each in a fresh child process."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    cmd = [sys.executable, os.path.join(PKG, "train.py"), "--exp_name", "dev", "--env_name", "cartpole", "--param_name", "cartpole",
           "--n_envs", "8", "--n_steps", "16", "--mini_batch_size", "32", "--seed", "3", "--detect_nan", "--num_timesteps", "120",
           "--num_checkpoints", "1", "--device_env", "--resident_rollout", "--fused_update"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    runs = os.listdir(tmp_path / "logs" / "train" / "cartpole" / "dev")
    assert len(runs) == 1
    rd = tmp_path / "logs" / "train" / "cartpole" / "dev" / runs[0]
    models = [f for f in os.listdir(rd) if f.startswith("model_") and f.endswith(".pth")]
    assert len(models) == 1, os.listdir(rd)
    cmd = [sys.executable, os.path.join(PKG, "evaluate.py"), "--model_file", str(rd / models[0]), "--env_name", "cartpole", "--param_name", "cartpole",
           "--episodes", "2", "--both", "--n_envs", "16", "--seed", "3"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "training ranges: 16 envs x 2 episodes, sampled actions" in r.stdout and "validation ranges: 16 envs x 2 episodes" in r.stdout
    assert "val_mean_episode_rewards" in r.stdout
    with np.load(rd / "evaluation.npz") as z:
        rec = {k: z[k] for k in z.files}
    assert set(rec) == set(RECORDS) | {"val_" + k for k in RECORDS}
    for p in ("", "val_"):
        assert rec[p + "ret"].shape == rec[p + "length"].shape == rec[p + "terminated"].shape == rec[p + "value0"].shape == (16, 2)
        assert rec[p + "start"].shape == (16, 2, 9)
        assert (rec[p + "length"] >= 1).all() and (rec[p + "length"] <= 500).all() and np.array_equal(rec[p + "ret"], rec[p + "length"])
        assert np.array_equal(rec[p + "terminated"] == 0, rec[p + "length"] == 500) and np.isfinite(rec[p + "value0"]).all()
    # the parameter columns an episode was drawn with lie in create_cartpole's ranges: the training set's and the validation set's
    from common.env.vec_envs import create_vector_env
    for p, is_valid in (("", False), ("val_", True)):
        host = create_vector_env("cartpole", {}, is_valid, seed=0, n_envs=16)      # (the set's own overrides, degrees_v / h_range_v, are thresholds, not ranges)
        s = rec[p + "start"]
        assert (s >= host.low).all() and (s <= host.high).all(), p
    assert (rec["val_start"][..., 4] >= 10.4).all() and (rec["start"][..., 4] <= 10.4).all()      # gravity: 9.8-10.4 against 10.4-24.8
    assert (rec["val_start"][..., 5] >= 1.0).all() and (rec["start"][..., 5] <= 1.0).all()        # pole length: 0.5-1 against 1-2
    rows = open(rd / "evaluation.csv").read().strip().splitlines()
    assert len(rows) == 2 and rows[0].startswith("model_file,env_name,param_name,n_envs,episodes,greedy,seed,max_episode_rewards")
    cells = dict(zip(rows[0].split(","), rows[1].split(",")))
    assert cells["model_file"] == models[0] and cells["episodes"] == "2" and cells["n_envs"] == "16"
    assert float(cells["mean_episode_len"]) == rec["length"].mean() and float(cells["val_mean_episode_len"]) == rec["val_length"].mean()
