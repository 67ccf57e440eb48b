"""Rollout and iteration time of the device-resident envs with the chain of launches (mi_env_rollout: T + 1 policy steps and T env steps,
about ten launches per step) and with the one-launch rollout (mi_env_rollout_resident, train.py --resident_rollout), same process, same build,
at the shapes of the `cartpole` set (E = T = 256, MLPModel(9, 4, 256, 64)) and of the `mountain_car` set (E = T = 16, MLPModel(5, 4, 256, 64)).

    timeout -k 10 600 python scratch/resident_rollout_time.py [--runs 11] [--out profiles-or-other-dir/file.json]

Per shape two PPO agents with the set's hyper-parameters and the same initial policy on the device env, no validation env; one has
resident_rollout=True.  After one warm-up rollout and one warm-up iteration of each, `--runs` rollouts of each are timed ALTERNATING
chain / resident (host clock around PPO._collect + a stream synchronise: the rollout as the training loop sees it, the reward / done
mirrors on the host included), then `--runs` full iterations of each, alternating.  Prints medians and ranges as a markdown table and one
JSON line; the yardstick of the resident rollout is the chain measured beside it (non-overlap: the resident median below the chain's
smallest run).  Needs the GPU (there is no CPU fallback)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "train-procgen-pytorch_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from cartpole_rollout_time import Run, stats      # the timed rollout / iteration of one agent


def build(name, resident, hp, seed=0):
    from agents.ppo import PPO
    from common.env.vec_envs import vector_env
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    E, T = hp["n_envs"], hp["n_steps"]
    env = vector_env(name).create(hp, False, seed=seed, n_envs=E, device=True)
    W, A = env.observation_space.shape[0], env.action_space.n
    model = MLPModel(W, hp["depth"], hp["mid_weight"], hp["latent_size"])
    agent = PPO(env, CategoricalPolicy(model, False, A), Logger(E, None), Storage((W,), model.output_dim, T, E, dev), dev, 1, seed=seed,
                resident_rollout=resident, **hp)
    agent.total_timesteps = 10 ** 9
    return agent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.runs < 5:
        sys.exit("--runs must be at least 5")
    import train
    out = {}
    print("| shape | what | rollout | median ms | min ms | max ms | runs |\n|---|---|---|---|---|---|---|")
    for name in ("cartpole", "mountain_car"):
        hp = train.get_hyperparams(name)
        runs = {"chain": Run(build(name, False, hp)), "resident": Run(build(name, True, hp))}
        for r in runs.values():                      # warm-up: every kernel of the rollout and of the update has run once
            r.rollout(); r.iteration()
        times = {k + "_" + what: [] for k in runs for what in ("rollout", "iteration")}
        for what in ("rollout", "iteration"):
            for _ in range(args.runs):
                for k, r in runs.items():            # alternating: a drift of the box hits both sides alike
                    times[k + "_" + what].append(getattr(r, what)())
        o = {k: stats(v) for k, v in times.items()}
        o["shape"] = {"n_envs": hp["n_envs"], "n_steps": hp["n_steps"], "embedder": "MLPModel(%d, %d, %d, %d)" % (
            runs["chain"].a.env.observation_space.shape[0], hp["depth"], hp["mid_weight"], hp["latent_size"])}
        for what in ("rollout", "iteration"):
            o[what + "_speedup_median"] = o["chain_" + what]["median_ms"] / o["resident_" + what]["median_ms"]
            o[what + "_resident_median_below_chain_min"] = o["resident_" + what]["median_ms"] < o["chain_" + what]["min_ms"]
            for k in runs:
                s = o[k + "_" + what]
                print("| %s E = T = %d | %s | %s | %.3f | %.3f | %.3f | %d |" % (name, hp["n_envs"], what, k, s["median_ms"], s["min_ms"], s["max_ms"], s["runs"]))
        out[name] = o
        for r in runs.values():
            r.a.engine.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
