"""Rollout and iteration time of the swing-up cart-pole (`--env_name cartpole_swing --param_name mlpmodel`, MLPModel(9, 4, 256, 64)) on its
three paths -- the host env (CartPoleSwingVec, the serial collector: T + 1 policy steps with a host round trip each), the device chain
(DeviceCartPoleSwing: one mi_env_rollout) and the resident rollout (one mi_env_rollout_resident launch) -- with the balance cart-pole's
device paths (DeviceCartPole: the same dynamics without the reward's two cos and one divide) as the yardstick, same process, same build.

    timeout -k 10 900 python scratch/cartpole_swing_rollout_time.py [--runs 11] [--shapes 256x256 1024x256] [--out dir/file.json]

Per shape E x T: five PPO agents with the `mlpmodel` set's hyper-parameters and the same initial policy, no validation env.  After one
warm-up rollout and one warm-up iteration of each, `--runs` rollouts of each are timed INTERLEAVED in one fixed order (host clock around
PPO._collect + a stream synchronise: the rollout as the training loop sees it, the reward / done mirrors on the host included), then
`--runs` full iterations of each, interleaved (rollout + compute_estimates + optimize + fetch_log_data, ending in a synchronise).  Prints
medians and spans as a markdown table and one JSON line per shape; needs the GPU (there is no CPU fallback).  The swing-up runs with its
own max_steps (1000), the balance task with its own (500) and its angle threshold, so the balance task resets far more often."""
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
from cartpole_rollout_time import Run, stats      # noqa: E402

PATHS = (("swing_host", "cartpole_swing", False, False, "CartPoleSwingVec (host, serial collector)"),
         ("swing_chain", "cartpole_swing", True, False, "DeviceCartPoleSwing, chain"),
         ("swing_resident", "cartpole_swing", True, True, "DeviceCartPoleSwing, resident"),
         ("balance_chain", "cartpole", True, False, "DeviceCartPole, chain (yardstick)"),
         ("balance_resident", "cartpole", True, True, "DeviceCartPole, resident (yardstick)"))


def build(env_name, device_env, resident, hp, seed=0):
    from agents.ppo import PPO
    from common.env.vec_envs import create_vector_env
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    E, T = hp["n_envs"], hp["n_steps"]
    env = create_vector_env(env_name, hp, False, seed=seed, n_envs=E, device=device_env)
    model = MLPModel(9, hp["depth"], hp["mid_weight"], hp["latent_size"])
    policy = CategoricalPolicy(model, False, 2)
    storage = Storage((9,), model.output_dim, T, E, dev)
    agent = PPO(env, policy, Logger(E, None), storage, dev, 1, seed=seed, **dict(hp, resident_rollout=resident))
    agent.total_timesteps = 10 ** 9
    return agent


def measure(E, T, n_runs):
    import train
    hp = dict(train.get_hyperparams("mlpmodel"), n_envs=E, n_steps=T)
    runs = {k: Run(build(name, dev, res, hp)) for k, name, dev, res, _ in PATHS}
    for r in runs.values():                      # warm-up: every kernel of the rollout and of the update has run once
        r.rollout(); r.iteration()
    times = {k + "_" + what: [] for k in runs for what in ("rollout", "iteration")}
    for what in ("rollout", "iteration"):
        for _ in range(n_runs):
            for k, r in runs.items():            # interleaved: a drift of the box hits every path alike
                times[k + "_" + what].append(getattr(r, what)())
    out = {k: stats(v) for k, v in times.items()}
    out["shape"] = {"n_envs": E, "n_steps": T, "embedder": "MLPModel(9, %d, %d, %d)" % (hp["depth"], hp["mid_weight"], hp["latent_size"])}
    for path in ("chain", "resident"):           # the swing-up's median against the yardstick's span
        s, b = out["swing_%s_rollout" % path], out["balance_%s_rollout" % path]
        out["swing_%s_vs_balance" % path] = {"median_ratio": s["median_ms"] / b["median_ms"], "inside_balance_span": b["min_ms"] <= s["median_ms"] <= b["max_ms"],
                                             "beyond_span_ms": max(s["median_ms"] - b["max_ms"], b["min_ms"] - s["median_ms"], 0.0)}
    print("\nE = %d, T = %d\n| what | path | median ms | min ms | max ms | runs |\n|---|---|---|---|---|---|" % (E, T))
    for what in ("rollout", "iteration"):
        for k, _, _, _, label in PATHS:
            s = out[k + "_" + what]
            print("| %s | %s | %.3f | %.3f | %.3f | %d |" % (what, label, s["median_ms"], s["min_ms"], s["max_ms"], s["runs"]))
    print(json.dumps(out), flush=True)
    for r in runs.values():
        r.a.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--shapes", type=str, nargs="+", default=["256x256", "1024x256"])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.runs < 5:
        sys.exit("--runs must be at least 5")
    out = {s: measure(*(int(v) for v in s.split("x")), args.runs) for s in args.shapes}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
