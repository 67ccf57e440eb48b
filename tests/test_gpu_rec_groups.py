"""Recurrent (GRU) policies on the pipelined env-group rollout: the fused group-sized GRU step (mi_debug_gru_step) against float64, the
pipelined recurrent collector against the serial one, independence of the group count, the joint training + validation lanes with a
GRU, and `train.py --rollout_groups 2` for a recurrent parameter set."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, PKG, ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


class _Log:
    episode_reward_buffer = [0.0]
    logdir = "/tmp"


class _Streams:
    """A vector env whose every env draws from its own random stream (frames, rewards, dones): what an env shows does not depend on
    how the envs are split into groups.  Frames are handed out in two buffers of its own, in turn (as Procgen reuses its rgb buffer)."""

    def __init__(self, seeds, n_actions=15, p_done=0.15):
        from common.env.vec_envs import _Space
        self.n_envs = len(seeds)
        self.rngs = [np.random.default_rng(s) for s in seeds]
        self.observation_space, self.action_space = _Space(shape=(3, 64, 64)), _Space(n=n_actions)
        self.p_done = p_done
        self._bufs, self._k = [np.empty((self.n_envs, 64, 64, 3), np.uint8) for _ in range(2)], 0

    def _obs(self):
        self._k ^= 1
        buf = self._bufs[self._k]
        for i, r in enumerate(self.rngs):
            buf[i] = r.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
        return buf

    def reset(self):
        return self._obs()

    def step(self, act):
        from common.env.vec_envs import StepInfo
        rew = np.array([r.standard_normal() for r in self.rngs], np.float32)
        done = np.array([r.random() < self.p_done for r in self.rngs])
        return self._obs(), rew, done, StepInfo(self.n_envs, {"env_reward": rew, "prev_level_seed": np.zeros(self.n_envs, np.int64)})

    def close(self):
        pass


class _Serial:
    """The same env without the group attribute: forces the serial path."""

    def __init__(self, env):
        self._e = env
        self.observation_space, self.action_space = env.observation_space, env.action_space

    def reset(self):
        return self._e.reset()

    def step(self, a):
        return self._e.step(a)


def _groups(E, G, base):
    from common.env.vec_envs import EnvGroups
    ng = E // G
    return EnvGroups([_Streams([base + e for e in range(g * ng, (g + 1) * ng)]) for g in range(G)])


def _rec_agent(T, E, H=256, precision="fp32", valid=False, seed=6033):
    from agents.ppo import PPO
    from common.model import ImpalaModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(seed)
    policy = CategoricalPolicy(ImpalaModel(3, output_dim=H), True, 15)
    st = Storage((3, 64, 64), H, T, E, DEV)
    stv = Storage((3, 64, 64), H, T, E, DEV) if valid else None
    agent = PPO(None, policy, _Log(), st, DEV, 1, storage_valid=stv, n_steps=T, n_envs=E, epoch=1, n_minibatch=1, mini_batch_size=16,
                precision=precision)
    agent._iter = 1
    if valid:
        agent.engine_valid.copy_params_from(agent.engine)
    return agent, st, stv


def _carried_in(E, H, seed=7):
    rng = np.random.default_rng(seed)
    hid = (0.6 * np.tanh(rng.standard_normal((E, H)))).astype(np.float32)
    done = (np.arange(E) % 3 == 1).astype(np.float32)                   # some envs start a new episode at t = 0: their state is masked
    return hid, done


def _ring(eng, T):
    from mi355 import engine as M
    return dict(frames=np.stack([eng.get_obs(t) for t in range(T + 1)]), act=eng.read_field(M.F_ACT), rew=eng.read_field(M.F_REW),
                done=eng.read_field(M.F_DONE), logp=eng.read_field(M.F_LOGP), val=eng.read_field(M.F_VALUE))


EXACT = ("frames", "act", "rew", "done", "obs", "dn")
CLOSE = ("logp", "val", "hidden", "hid")


def _two_iterations(agent, st, env, T, E, H):
    hid, done = _carried_in(E, H)
    obs = env.reset()
    its = []
    for it in range(2):
        agent._iter = it + 1
        obs, hid, done = agent._collect(env, agent.engine, st, obs, hid, done)
        its.append(dict(_ring(agent.engine, T), hidden=st._hidden.copy(), hid=np.array(hid, np.float32), obs=np.array(obs),
                        dn=np.array(done, np.float32)))
    return its


# ---------------------------------------------------------------------------------------------------------------- 1. the fused kernel
@pytest.mark.parametrize("H", [64, 256, 512])
def test_fused_gru_step_against_float64_gru_cell(H):
    """h' = GRU(x, h (1 - done)) of the fused group step against torch.nn.GRUCell in float64 (same fp32 weights and inputs) for 1 .. 256
    rows, non-zero incoming states and masks mixing 0 and 1; the kernel's two copies of h' are equal; every row of a 256-row launch equals
    the same row computed in launches of 1 or 7 rows at other offsets, bit for bit."""
    from mi355.engine import Engine
    eng = Engine("impala", 2, 8, 15, 8)
    rng = np.random.default_rng(H)
    bound = 1.0 / np.sqrt(H)
    w_ih, w_hh = (rng.uniform(-bound, bound, (3 * H, H)).astype(np.float32) for _ in range(2))
    b_ih, b_hh = (rng.uniform(-bound, bound, 3 * H).astype(np.float32) for _ in range(2))
    cell = torch.nn.GRUCell(H, H, dtype=torch.float64)
    with torch.no_grad():
        for p, v in ((cell.weight_ih, w_ih), (cell.weight_hh, w_hh), (cell.bias_ih, b_ih), (cell.bias_hh, b_hh)):
            p.copy_(torch.from_numpy(v).double())
    N = 256
    x = (2.0 * np.maximum(rng.standard_normal((N, H)), 0)).astype(np.float32)            # the embedder's fc + ReLU output
    h = (0.8 * np.tanh(2.0 * rng.standard_normal((N, H)))).astype(np.float32)
    done = (rng.random(N) < 0.4).astype(np.float32)
    done[:2] = (0.0, 1.0)
    with torch.no_grad():
        ref = cell(torch.from_numpy(x).double(), torch.from_numpy(h).double() * (1.0 - torch.from_numpy(done).double())[:, None]).numpy()
    worst = 0.0
    full = None
    for ng in (1, 7, 64, 128, 256):
        out, cp = eng.debug_gru_step(x[:ng], h[:ng], done[:ng], w_ih, w_hh, b_ih, b_hh, with_copy=True)
        assert np.array_equal(out, cp), ng
        err = float(np.abs(out - ref[:ng]).max())
        worst = max(worst, err)
        assert err < 2e-6, (ng, err)
        full = out
    assert np.abs(full - ref).max() < 2e-6 and np.abs(ref).max() > 0.3 and worst > 0
    # the mask matters: rows that start an episode differ from the unmasked cell
    with torch.no_grad():
        unmasked = cell(torch.from_numpy(x).double(), torch.from_numpy(h).double()).numpy()
    assert np.abs(unmasked[done > 0] - full[done > 0]).max() > 1e-2
    for a, n in ((0, 1), (5, 1), (255, 1), (0, 7), (100, 7), (249, 7), (64, 7)):
        part = eng.debug_gru_step(x[a:a + n], h[a:a + n], done[a:a + n], w_ih, w_hh, b_ih, b_hh)
        assert np.array_equal(part, full[a:a + n]), (a, n)
    eng.close()


def test_fused_gru_step_refuses_unsupported_widths():
    from mi355.engine import Engine, EngineError
    eng = Engine("impala", 2, 8, 15, 8)
    for H in (32, 96, 576):
        z = np.zeros((2, H), np.float32)
        with pytest.raises(EngineError, match="multiple of 64"):
            eng.debug_gru_step(z, z, np.zeros(2), np.zeros((3 * H, H)), np.zeros((3 * H, H)), np.zeros(3 * H), np.zeros(3 * H))
    eng.close()


# ------------------------------------------------------------------------------------------- 2. pipelined recurrent collect vs serial
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("H,E,G", [(256, 16, 2), (256, 64, 4), (512, 16, 2)])
def test_pipelined_recurrent_collect_equals_serial_collect(precision, H, E, G):
    """PPO._collect of a GRU policy over an env with `.env_groups` (the cell inside every group step, mi_rec_begin, the hidden ring)
    against the serial loop over the same EnvGroups with the group attribute hidden, two consecutive iterations from a non-zero
    carried-in state with some done = 1 at t = 0: identical frames, actions, rewards and dones; log-probs, values, every stored hidden
    state and the returned state within 1e-5 (the GEMMs' summation order differs)."""
    T = 5
    res = []
    for pipelined in (False, True):
        agent, st, _ = _rec_agent(T, E, H, precision)
        env = _groups(E, G, base=100)
        res.append(_two_iterations(agent, st, env if pipelined else _Serial(env), T, E, H))
        assert getattr(agent.engine, "n_groups", 1) == (G if pipelined else 1)
    for it, (a, b) in enumerate(zip(*res)):
        for k in EXACT:
            assert np.array_equal(a[k], b[k]), (it, k)
        for k in CLOSE:
            np.testing.assert_allclose(b[k], a[k], rtol=0, atol=1e-5, err_msg=f"iteration {it}: {k}")
        assert np.abs(a["hid"]).max() > 1e-2 and a["done"].any() and len(np.unique(a["act"])) > 3
        np.testing.assert_array_equal(b["hidden"][0], res[1][it - 1]["hid"] if it else _carried_in(E, H)[0])   # slot 0: the carried-in state
        np.testing.assert_array_equal(b["hidden"][T], b["hid"])                                               # _hidden[T] = the returned state


# ------------------------------------------------------------------------------------------------------ 3. group-count independence
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_recurrent_rollout_does_not_depend_on_the_group_count(precision):
    """G = 2 and G = 4 over the same per-env frame streams: bit-identical ring, stored hidden states and returned hidden state (a row's
    GRU step is a fixed function of that row's inputs)."""
    T, E, H = 5, 16, 256
    res = []
    for G in (2, 4):
        agent, st, _ = _rec_agent(T, E, H, precision)
        res.append(_two_iterations(agent, st, _groups(E, G, base=300), T, E, H))
        assert agent.engine.n_groups == G
    for it, (a, b) in enumerate(zip(*res)):
        for k in EXACT + CLOSE:
            assert np.array_equal(a[k], b[k]), (it, k)


# ---------------------------------------------------------------------------------------------------------- 4. joint lanes with a GRU
def test_joint_training_and_validation_lanes_with_a_gru():
    """PPO._collect_lanes with a GRU policy: the training lane equals the solo pipelined collector bit for bit; the validation lane's
    stored log-probs and values are reproduced by replaying its frames serially through the twin (rec_state with the stored hidden state
    of each step + forward_rec), and so are its stored next-step states and returned state."""
    from mi355 import engine as M
    T, E, G, H = 5, 16, 2, 256
    hid0, done0 = _carried_in(E, H)
    hv0, dv0 = _carried_in(E, H, seed=8)
    a1, st1, stv1 = _rec_agent(T, E, H, "bf16", valid=True)
    env1, envv1 = _groups(E, G, base=0), _groups(E, G, base=500)
    (o, h, d), (ov, hv, dv) = a1._collect_lanes([(env1, a1.engine, st1, env1.reset(), hid0, done0),
                                                 (envv1, a1.engine_valid, stv1, envv1.reset(), hv0, dv0)])
    a2, st2, _ = _rec_agent(T, E, H, "bf16")
    env2 = _groups(E, G, base=0)
    o2, h2, d2 = a2._collect(env2, a2.engine, st2, env2.reset(), hid0, done0)
    r1, r2 = _ring(a1.engine, T), _ring(a2.engine, T)
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), k
    assert np.array_equal(st1._hidden, st2._hidden) and np.array_equal(h, h2) and np.array_equal(o, o2) and np.array_equal(d, d2)
    ev = a1.engine_valid
    rv = _ring(ev, T)
    assert not np.array_equal(rv["act"], r1["act"]) and len(np.unique(rv["act"])) > 3
    assert np.array_equal(stv1._hidden[0], hv0)
    h_prev = None
    for t in range(T + 1):
        ev.rec_state(stv1._hidden[t] if t < T else h_prev, dv0 if t == 0 else rv["done"][t - 1])
        lp_all, v, h_out = ev.forward_rec(rv["frames"][t])
        np.testing.assert_allclose(v, rv["val"][t], rtol=0, atol=1e-5)
        if t < T:
            np.testing.assert_allclose(lp_all[np.arange(E), rv["act"][t].astype(int)], rv["logp"][t], rtol=0, atol=1e-5)
        if t + 1 < T:
            np.testing.assert_allclose(h_out, stv1._hidden[t + 1], rtol=0, atol=1e-5)
        h_prev = h_out
    np.testing.assert_allclose(hv, h_prev, rtol=0, atol=1e-5)
    assert np.array_equal(stv1._hidden[T], hv) and np.array_equal(ev.get_obs(T), ov) and np.array_equal(stv1._done[T - 1], dv)
    assert np.array_equal(ev.read_field(M.F_DONE), rv["done"]) and rv["done"].any()


# ------------------------------------------------------------------------------------------------------------------------- 5. CLI
def test_train_cli_recurrent_with_env_groups_runs_and_resumes(tmp_path):
    """`train.py --rollout_groups 2` with a recurrent parameter set (hard-local-dev-rec, shrunk): pipelined training + validation lanes,
    finite losses, a checkpoint with the structure of the reference-written recurrent fixture G11, and `--model_file auto` resumes."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    base = [sys.executable, os.path.join(PKG, "train.py"), "--exp_name", "rec", "--env_name", "synthetic", "--param_name", "hard-local-dev-rec",
            "--n_envs", "8", "--n_steps", "16", "--mini_batch_size", "32", "--seed", "3", "--detect_nan", "--precision", "bf16",
            "--rollout_groups", "2", "--no-reduce_duplicate_actions"]
    r = subprocess.run(base + ["--num_timesteps", "250", "--num_checkpoints", "1"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "rollout: 2 pipelined env groups" in r.stdout
    rd = tmp_path / "logs" / "train" / "synthetic" / "rec"
    rd = rd / os.listdir(rd)[0]
    ck = torch.load(rd / "model_256.pth", map_location="cpu", weights_only=True)
    want = json.load(open(os.path.join(GOLD, "g11_checkpoint_structure.json")))["impala_rec"]
    desc = lambda v: [list(v.shape), str(v.dtype)]
    assert [[k, *desc(v)] for k, v in ck["model_state_dict"].items()] == want["model"]
    osd = ck["optimizer_state_dict"]
    assert list(osd.keys()) == want["opt_keys"]
    assert [[int(i), [[k, *desc(v)] for k, v in s_.items()]] for i, s_ in osd["state"].items()] == [s_[:2] for s_ in want["opt_state"]]
    assert osd["param_groups"][0]["params"] == want["param_groups"][0]["params"]
    assert list(osd["param_groups"][0].keys()) == list(want["param_groups"][0].keys())
    with open(rd / "log-append.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2
    for k in ("loss_pi", "loss_v", "loss_entropy", "loss_total"):
        assert all(np.isfinite(float(row[k])) for row in rows), k
    r = subprocess.run(base + ["--num_timesteps", "500", "--num_checkpoints", "1", "--model_file", "auto"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Loading agent from" in r.stdout and "model_256.pth" in r.stdout and "rollout: 2 pipelined env groups" in r.stdout
    ck2 = torch.load(rd / "model_512.pth", map_location="cpu", weights_only=True)
    assert ck2["t"] == 512 and set(ck2["model_state_dict"]) == set(ck["model_state_dict"])
    for k in ("gru.gru.weight_ih_l0", "gru.gru.bias_hh_l0"):                 # the GRU is never trained (agents/ppo.py:123-128)
        assert torch.equal(ck2["model_state_dict"][k], ck["model_state_dict"][k])
