"""Rollout and iteration time of the `mountain_car` hyper-parameter set (MLPModel(5, 4, 256, 64), 3 actions) with the host env
(MountainCarVec, the serial collector: T + 1 policy steps with a host round trip each) and with the device-resident env
(DeviceMountainCar: one mi_env_rollout), same process, same build, at the set's own shape (E = T = 16) and at E = T = 256.

    timeout -k 10 600 python scratch/mountain_car_rollout_time.py [--runs 11] [--out profiles-or-other-dir/file.json]

The method of scratch/cartpole_rollout_time.py (whose Run / stats it reuses): per shape two PPO agents with the set's hyper-parameters
and the same initial policy, no validation env; after one warm-up rollout and one warm-up iteration of each, `--runs` rollouts of each
are timed ALTERNATING host / device, then `--runs` full iterations of each, alternating.  Prints medians and ranges as a markdown table
and one JSON line; needs the GPU (there is no CPU fallback)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cartpole_rollout_time import Run, stats  # noqa: E402  (puts the repository and the package on the path)


def build(device_env, hp, seed=0):
    from agents.ppo import PPO
    from common.env.vec_envs import create_mountain_car
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    E, T = hp["n_envs"], hp["n_steps"]
    env = create_mountain_car(hp, False, seed=seed, n_envs=E, device=device_env)
    model = MLPModel(5, hp["depth"], hp["mid_weight"], hp["latent_size"])
    policy = CategoricalPolicy(model, False, 3)
    storage = Storage((5,), model.output_dim, T, E, dev)
    agent = PPO(env, policy, Logger(E, None), storage, dev, 1, seed=seed, **hp)
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
    print("| shape | what | env | median ms | min ms | max ms | runs |\n|---|---|---|---|---|---|---|")
    for size in (16, 256):
        hp = dict(train.get_hyperparams("mountain_car"), n_envs=size, n_steps=size)
        runs = {"host": Run(build(False, hp)), "device": Run(build(True, hp))}
        for r in runs.values():                      # warm-up: every kernel of the rollout and of the update has run once
            r.rollout(); r.iteration()
        times = {k + "_" + what: [] for k in runs for what in ("rollout", "iteration")}
        for what in ("rollout", "iteration"):
            for _ in range(args.runs):
                for k, r in runs.items():            # alternating: a drift of the box hits both sides alike
                    times[k + "_" + what].append(getattr(r, what)())
        res = {k: stats(v) for k, v in times.items()}
        res["shape"] = {"n_envs": size, "n_steps": size, "embedder": "MLPModel(5, %d, %d, %d)" % (hp["depth"], hp["mid_weight"], hp["latent_size"]),
                        "epoch": hp["epoch"], "n_minibatch": hp["n_minibatch"], "mini_batch_size": hp["mini_batch_size"]}
        res["rollout_speedup_median"] = res["host_rollout"]["median_ms"] / res["device_rollout"]["median_ms"]
        res["iteration_speedup_median"] = res["host_iteration"]["median_ms"] / res["device_iteration"]["median_ms"]
        for what in ("rollout", "iteration"):
            for k in runs:
                s = res[k + "_" + what]
                print("| E = T = %d | %s | %s | %.2f | %.2f | %.2f | %d |" % (size, what, "MountainCarVec (host)" if k == "host" else "DeviceMountainCar",
                                                                             s["median_ms"], s["min_ms"], s["max_ms"], s["runs"]), flush=True)
        out["E%d" % size] = res
        for r in runs.values():
            r.a.engine.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
