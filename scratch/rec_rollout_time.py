"""Rollout time of a recurrent (GRU) policy at hard-rec's shape (E = 256, T = 256, H = 256, A = 15): ms per T = 256 rollout, serial
(PPO._collect's reference-shaped loop: rec_state / rollout_step / get_hidden per step), pipelined with G = 2 and G = 4 env groups (the
fused GRU step inside every group step), and training + validation as lanes of one host loop with 2 + 2 groups (the pair of rollouts);
the non-recurrent policy's G = 4 rollout on the same box for scale.
    python scratch/rec_rollout_time.py [precisions=bf16,fp32] [iterations=3] [modes=serial,g2,g4,lanes,flat4]"""
import os, sys, time, numpy as np
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
sys.path[:0] = [".", "train-procgen-pytorch_amd"]
import torch
from agents.ppo import PPO
from common.env.vec_envs import EnvGroups, SyntheticTape
from common.model import ImpalaModel
from common.policy import CategoricalPolicy
from common.storage import Storage

precisions = (sys.argv[1] if len(sys.argv) > 1 else "bf16,fp32").split(",")
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 3
modes = (sys.argv[3] if len(sys.argv) > 3 else "serial,g2,g4,lanes,flat4").split(",")
T, E, H, A = 256, 256, 256, 15
dev = torch.device("cuda", 0)


class L:
    episode_reward_buffer = [0.0]
    logdir = "/tmp"


def agent_for(rec, precision):
    torch.manual_seed(1)
    policy = CategoricalPolicy(ImpalaModel(3, output_dim=H), rec, A); policy.device = dev
    st, stv = Storage((3, 64, 64), H, T, E, dev), Storage((3, 64, 64), H, T, E, dev)
    return PPO(None, policy, L(), st, dev, 1, storage_valid=stv, precision=precision, n_steps=T, n_envs=E, epoch=1, n_minibatch=8,
               mini_batch_size=8192), st, stv


def groups(G, s):
    return EnvGroups([SyntheticTape(E // G, A, seed=s + g, length=T) for g in range(G)])


def start(env):
    return [env.reset(), np.zeros((E, H), np.float32), np.zeros(E, np.float32)]


for precision in precisions:
    agent, st, stv = agent_for(True, precision)
    for mode in modes:
        if mode == "flat4":
            agent, st, stv = agent_for(False, precision)
        env = SyntheticTape(E, A, seed=0, length=T) if mode == "serial" else groups(2 if mode in ("g2", "lanes") else 4, 0)
        envv = groups(2, 100) if mode == "lanes" else None
        r, rv = start(env), (start(envv) if envv is not None else None)
        for it in range(iters):
            agent._iter = it + 1
            agent.engine_valid.copy_params_from(agent.engine)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "lanes":
                ra, rb = agent._collect_lanes([(env, agent.engine, st, *r), (envv, agent.engine_valid, stv, *rv)])
                r, rv = list(ra), list(rb)
            else:
                r = list(agent._collect(env, agent.engine, st, *r))
            ms = 1e3 * (time.perf_counter() - t0)
            print(f'{{"precision": "{precision}", "mode": "{mode}", "iteration": {it}, "ms": {ms:.1f}, "queues": "{os.environ["GPU_MAX_HW_QUEUES"]}"}}', flush=True)
