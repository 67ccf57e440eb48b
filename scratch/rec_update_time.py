"""Update time of a recurrent (GRU) policy at hard-rec's shape (E = 256, T = 256, H = 256, A = 15, bf16; 3 epochs x 8 minibatches of
32 envs x 256 steps): ms per optimize() under algo ppo (the GRU frozen: the update bypasses it) and under ppo-pure (BPTT through the
GRU: mi_minibatch_rec, csrc/gru_seq.hip), on one synthetic rollout.
    python scratch/rec_update_time.py [algos=ppo,ppo-pure] [iterations=3] [precision=bf16]
The two sequence kernels per minibatch, from a kernel trace of one ppo-pure update:
    rocprofv3 --kernel-trace --stats -d /tmp/rec_update_trace -- python scratch/rec_update_time.py ppo-pure 1
    python scratch/rec_update_time.py --stats /tmp/rec_update_trace
The yardstick for the sequential part is the fused rollout cell stepped 256 times at 21 us per launch = 5.4 ms per minibatch and
direction."""
import csv, glob, json, os, sys, time
import numpy as np

if len(sys.argv) > 2 and sys.argv[1] == "--stats":
    files = glob.glob(os.path.join(sys.argv[2], "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_stats.csv under {sys.argv[2]}")
    for row in csv.DictReader(open(files[0])):
        if "gru_seq" in row["Name"]:
            print(json.dumps({"kernel": row["Name"].split("(")[0][:60], "calls": int(row["Calls"]),
                              "avg_ms": float(row["AverageNs"]) / 1e6, "min_ms": float(row["MinNs"]) / 1e6, "max_ms": float(row["MaxNs"]) / 1e6}))
    sys.exit(0)

sys.path[:0] = [".", "train-procgen-pytorch_amd"]
import torch
from agents.ppo import PPO
from agents.ppo_pure import PPOPure
from common.model import ImpalaModel
from common.policy import CategoricalPolicy
from common.storage import Storage
from mi355 import engine as M

algos = (sys.argv[1] if len(sys.argv) > 1 else "ppo,ppo-pure").split(",")
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 3
precision = sys.argv[3] if len(sys.argv) > 3 else "bf16"
T, E, H, A = 256, 256, 256, 15
dev = torch.device("cuda", 0)


class L:
    episode_reward_buffer = [0.0]
    logdir = "/tmp"


for algo in algos:
    torch.manual_seed(1)
    policy = CategoricalPolicy(ImpalaModel(3, output_dim=H), True, A); policy.device = dev
    st = Storage((3, 64, 64), H, T, E, dev)
    agent = (PPOPure if algo == "ppo-pure" else PPO)(None, policy, L(), st, dev, 1, precision=precision, n_steps=T, n_envs=E, epoch=3,
                                                      n_minibatch=8, mini_batch_size=8192, gamma=0.999, lmbda=0.95, learning_rate=5e-4)
    eng, rng = agent.engine, np.random.default_rng(0)
    frames = rng.integers(0, 256, size=(8, E, 64, 64, 3), dtype=np.uint8)
    for t in range(T + 1):
        eng.put_obs(t, frames[t % 8])
    eng.sync()
    eng.write_field(M.F_ACT, rng.integers(0, A, (T, E)).astype(np.float32)); eng.write_field(M.F_LOGP, np.full((T, E), np.log(1 / A), np.float32))
    eng.write_field(M.F_VALUE, (0.5 * rng.standard_normal((T + 1, E))).astype(np.float32)); eng.write_field(M.F_REW, rng.standard_normal((T, E)).astype(np.float32))
    eng.write_field(M.F_DONE, (rng.random((T, E)) < 0.01).astype(np.float32))
    st._hidden[:] = 0.1 * rng.standard_normal(st._hidden.shape).astype(np.float32)
    st.compute_estimates(0.999, 0.95, True, True)
    for it in range(iters + 1):                      # iteration 0 warms up (lazy allocations, function attributes)
        eng.sync()
        t0 = time.perf_counter()
        summary = agent.optimize()
        eng.sync()
        ms = 1e3 * (time.perf_counter() - t0)
        if it:
            print(json.dumps({"algo": algo, "precision": precision, "iteration": it, "update_ms": round(ms, 2), "minibatches": 24,
                              "loss_total": round(summary["Loss/total"], 5)}), flush=True)
    eng.close()
