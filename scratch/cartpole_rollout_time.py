"""Rollout and iteration time of the `cartpole` hyper-parameter set (E = T = 256, MLPModel(9, 4, 256, 64)) with the host env
(CartPoleVec, the serial collector: 257 policy steps with a host round trip each) and with the device-resident env (DeviceCartPole:
one mi_env_rollout), same process, same build.

    timeout -k 10 600 python scratch/cartpole_rollout_time.py [--runs 9] [--out profiles-or-other-dir/file.json]

Two PPO agents with the set's hyper-parameters and the same initial policy, no validation env.  After one warm-up rollout and one warm-up
iteration of each, `--runs` rollouts of each are timed ALTERNATING host / device (host clock around PPO._collect + a stream
synchronise: the rollout as the training loop sees it, the reward / done mirrors on the host included), then `--runs` full iterations
of each, alternating (rollout + compute_estimates + optimize + fetch_log_data, ending in a synchronise).  Prints medians and ranges as a
markdown table and one JSON line; needs the GPU (there is no CPU fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "train-procgen-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def build(device_env, hp, seed=0):
    from agents.ppo import PPO
    from common.env.vec_envs import create_cartpole
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    E, T = hp["n_envs"], hp["n_steps"]
    env = create_cartpole(hp, False, seed=seed, n_envs=E, device=device_env)
    model = MLPModel(9, hp["depth"], hp["mid_weight"], hp["latent_size"])
    policy = CategoricalPolicy(model, False, 2)
    storage = Storage((9,), model.output_dim, T, E, dev)
    agent = PPO(env, policy, Logger(E, None), storage, dev, 1, seed=seed, **hp)
    agent.total_timesteps = 10 ** 9
    return agent


class Run:
    def __init__(self, agent):
        self.a = agent
        self.state = (agent.env.reset(), np.zeros((agent.n_envs, agent.storage.hidden_state_size)), np.zeros(agent.n_envs))

    def rollout(self):
        a = self.a
        a._iter += 1
        a.engine.sync()
        t0 = time.perf_counter()
        self.state = a._collect(a.env, a.engine, a.storage, *self.state)
        a.engine.sync()
        return (time.perf_counter() - t0) * 1e3

    def iteration(self):
        a = self.a
        a.engine.sync()
        t0 = time.perf_counter()
        a._iter += 1
        self.state = a._collect(a.env, a.engine, a.storage, *self.state)
        a.storage.compute_estimates(a.gamma, a.lmbda, a.use_gae, a.normalize_adv, a.coll)
        a.optimize()
        a.storage.fetch_log_data()
        a.engine.sync()
        return (time.perf_counter() - t0) * 1e3


def stats(x):
    return {"median_ms": float(np.median(x)), "min_ms": float(np.min(x)), "max_ms": float(np.max(x)), "runs": len(x)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.runs < 5:
        sys.exit("--runs must be at least 5")
    import train
    hp = train.get_hyperparams("cartpole")
    runs = {"host": Run(build(False, hp)), "device": Run(build(True, hp))}
    for r in runs.values():                      # warm-up: every kernel of the rollout and of the update has run once
        r.rollout(); r.iteration()
    times = {k + "_" + what: [] for k in runs for what in ("rollout", "iteration")}
    for what in ("rollout", "iteration"):
        for _ in range(args.runs):
            for k, r in runs.items():            # alternating: a drift of the box hits both sides alike
                times[k + "_" + what].append(getattr(r, what)())
    out = {k: stats(v) for k, v in times.items()}
    out["shape"] = {"n_envs": hp["n_envs"], "n_steps": hp["n_steps"], "embedder": "MLPModel(9, %d, %d, %d)" % (hp["depth"], hp["mid_weight"], hp["latent_size"])}
    out["rollout_speedup_median"] = out["host_rollout"]["median_ms"] / out["device_rollout"]["median_ms"]
    out["iteration_speedup_median"] = out["host_iteration"]["median_ms"] / out["device_iteration"]["median_ms"]
    print("| what | env | median ms | min ms | max ms | runs |\n|---|---|---|---|---|---|")
    for what in ("rollout", "iteration"):
        for k in runs:
            s = out[k + "_" + what]
            print("| %s | %s | %.2f | %.2f | %.2f | %d |" % (what, "CartPoleVec (host)" if k == "host" else "DeviceCartPole", s["median_ms"], s["min_ms"], s["max_ms"], s["runs"]))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for r in runs.values():
        r.a.engine.close()


if __name__ == "__main__":
    main()
