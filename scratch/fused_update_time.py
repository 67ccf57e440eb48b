"""Update and iteration time of the MLP sets with the chain of launches per minibatch (mi_minibatch / mi_minibatch_multi: more than twenty
launches) and with the fused pass (mi_minibatch_fused, train.py --fused_update: two launches), same process, same build, at the shapes of
the `cartpole` set (E = T = 256), of the `mountain_car` set (E = T = 16) and of the `mlpmodel` set with cartpole_swing (E = 1024, T = 256:
the merged two-segment pass), all MLPModel(., 4, 256, 64), all with the device-resident env and the one-launch rollout
(--device_env --resident_rollout).

    timeout -k 10 900 python scratch/fused_update_time.py [--runs 11] [--shapes cartpole mountain_car mlpmodel] [--out dir/file.json]

Per shape two PPO agents with the set's hyper-parameters and the same initial policy, no validation env; one has fused_update=True.
After one warm-up iteration of each, `--runs` optimize() calls of each are timed ALTERNATING chain / fused (host clock around
PPO.optimize + a stream synchronise, behind an untimed rollout and compute_estimates), then `--runs` full iterations of each,
alternating; and, for the split of an iteration, the chain agent's compute_estimates and fetch_log_data on their own.  Prints medians and
ranges as a markdown table and one JSON line; the yardstick of the fused pass is the chain measured beside it (non-overlap: the fused
median below the chain's smallest run).  Needs the GPU (there is no CPU fallback)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "train-procgen-pytorch_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from cartpole_rollout_time import Run, stats      # the timed rollout / iteration of one agent

SHAPES = {"cartpole": ("cartpole", "cartpole"), "mountain_car": ("mountain_car", "mountain_car"), "mlpmodel": ("mlpmodel", "cartpole_swing")}


def build(env_name, fused, hp, seed=0):
    from agents.ppo import PPO
    from common.env.vec_envs import vector_env
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    E, T = hp["n_envs"], hp["n_steps"]
    env = vector_env(env_name).create(hp, False, seed=seed, n_envs=E, device=True)
    W, A = env.observation_space.shape[0], env.action_space.n
    model = MLPModel(W, hp["depth"], hp["mid_weight"], hp["latent_size"])
    agent = PPO(env, CategoricalPolicy(model, False, A), Logger(E, None), Storage((W,), model.output_dim, T, E, dev), dev, 1, seed=seed,
                resident_rollout=True, fused_update=fused, **hp)
    agent.total_timesteps = 10 ** 9
    return agent


class UpdateRun(Run):
    def _timed(self, f):
        self.a.engine.sync()
        t0 = time.perf_counter()
        f()
        self.a.engine.sync()
        return (time.perf_counter() - t0) * 1e3

    def parts(self):
        """-> (compute_estimates, optimize, fetch_log_data) in ms, behind an untimed rollout"""
        a = self.a
        self.rollout()
        return (self._timed(lambda: a.storage.compute_estimates(a.gamma, a.lmbda, a.use_gae, a.normalize_adv, a.coll)), self._timed(a.optimize),
                self._timed(a.storage.fetch_log_data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--shapes", type=str, nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.runs < 5:
        sys.exit("--runs must be at least 5")
    import train
    out = {}
    print("| shape | what | update | median ms | min ms | max ms | runs |\n|---|---|---|---|---|---|---|")
    for shape in args.shapes:
        set_name, env_name = SHAPES[shape]
        hp = train.get_hyperparams(set_name)
        runs = {"chain": UpdateRun(build(env_name, False, hp)), "fused": UpdateRun(build(env_name, True, hp))}
        for r in runs.values():                      # warm-up: every kernel of the rollout and of the update has run once
            r.iteration()
        times = {k + "_" + what: [] for k in runs for what in ("estimates", "optimize", "fetch_log", "iteration")}
        for _ in range(args.runs):
            for k, r in runs.items():                # alternating: a drift of the box hits both sides alike
                e, o, f = r.parts()
                times[k + "_estimates"].append(e); times[k + "_optimize"].append(o); times[k + "_fetch_log"].append(f)
        for _ in range(args.runs):
            for k, r in runs.items():
                times[k + "_iteration"].append(r.iteration())
        o = {k: stats(v) for k, v in times.items()}
        a = runs["chain"].a
        n_total = hp["n_envs"] * hp["n_steps"]
        o["shape"] = {"set": set_name, "env": env_name, "n_envs": hp["n_envs"], "n_steps": hp["n_steps"], "epoch": hp["epoch"], "n_minibatch": hp["n_minibatch"],
                      "mini_batch_size": min(hp["mini_batch_size"], n_total // hp["n_minibatch"]), "max_batch": a.engine.max_batch,
                      "embedder": "MLPModel(%d, %d, %d, %d)" % (a.env.observation_space.shape[0], hp["depth"], hp["mid_weight"], hp["latent_size"])}
        for what in ("optimize", "iteration"):
            o[what + "_speedup_median"] = o["chain_" + what]["median_ms"] / o["fused_" + what]["median_ms"]
            o[what + "_fused_median_below_chain_min"] = o["fused_" + what]["median_ms"] < o["chain_" + what]["min_ms"]
        for what in ("estimates", "optimize", "fetch_log", "iteration"):
            for k in runs:
                s = o[k + "_" + what]
                print("| %s E = %d T = %d | %s | %s | %.3f | %.3f | %.3f | %d |" % (shape, hp["n_envs"], hp["n_steps"], what, k, s["median_ms"], s["min_ms"], s["max_ms"], s["runs"]))
        out[shape] = o
        for r in runs.values():
            r.a.engine.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
