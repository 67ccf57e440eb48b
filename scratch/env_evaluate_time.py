"""Time of evaluating a policy for K = 10 whole episodes per env on a device-resident env: the route the project had before
mi_env_evaluate against ONE Engine.env_evaluate call, same process, same build, interleaved.

    timeout -k 10 900 python scratch/env_evaluate_time.py [--runs 11] [--episodes 10] [--out profiles-or-other-dir/file.json]

Shapes: the `cartpole` set (E = T = 256, MLPModel(9, 4, 256, 64), DeviceCartPole, max_steps 500) and the `mlpmodel` set with cartpole_swing
(E = 1024, T = 256, the same network, DeviceCartPoleSwing, max_steps 1000); a freshly initialised policy (torch seed 0).

host route: from a fixed env state (every env at the start of an episode), Engine.env_rollout(resident=True) again and again; after each
rollout the reward / done rings are read back and the episodes are closed on the host (one vector operation over the envs per ring step),
until every env has K complete episodes.  Rollouts end at ring boundaries, so the last one runs past what is needed, and every env steps
for as long as the slowest one needs.  Timed: the rollouts, the ring reads and the host accounting (not the restore of the start state).

one launch: Engine.env_evaluate(K, seed) -- the launch, the wait and the copy of the records to the host.

After one warm-up of each, `--runs` of each are timed ALTERNATING (host clock around the calls, a stream synchronise before and after).
Prints medians and ranges as a markdown table and one JSON line.  The two routes do not run the same episodes (the host route's episodes
follow each other in the env's own reset stream from episode 1, the evaluation's start at 2^40), so the env steps of each are reported
beside the times: `steps` = the loop iterations the slowest env needed (host route: ring steps run), `us/step` = time / steps, the figure
to put beside the resident rollout's 26.8 us per step (profiles/resident_rollout.md).  Needs the GPU (there is no CPU fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "train-procgen-pytorch_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from cartpole_rollout_time import stats


def build(env_name, hp, seed=0):
    """a PPO agent with the set's hyper-parameters on the device env of that name (create_vector_env: the exact name cartpole_swing builds the
    swing-up), resident rollouts, no validation env"""
    import torch
    from agents.ppo import PPO
    from common.env.vec_envs import create_vector_env
    from common.logger import Logger
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    from common.storage import Storage
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    E, T = hp["n_envs"], hp["n_steps"]
    env = create_vector_env(env_name, hp, False, seed=seed, n_envs=E, device=True)
    W, A = env.observation_space.shape[0], env.action_space.n
    model = MLPModel(W, hp["depth"], hp["mid_weight"], hp["latent_size"])
    return PPO(env, CategoricalPolicy(model, False, A), Logger(E, None), Storage((W,), model.output_dim, T, E, dev), dev, 1, seed=seed,
               resident_rollout=True, **hp)


def host_route(eng, K, seed):
    """-> (ret (E, K), length (E, K), ring steps run)"""
    from mi355.engine import F_DONE, F_REW
    E, T = eng.E, eng.T
    ret, length = np.zeros((E, K)), np.zeros((E, K), np.int32)
    count, acc, ln = np.zeros(E, np.int64), np.zeros(E), np.zeros(E, np.int32)
    rollouts = 0
    while count.min() < K:
        eng.env_rollout(seed + rollouts, resident=True)
        rollouts += 1
        rew, done = eng.read_field(F_REW), eng.read_field(F_DONE) > 0
        for t in range(T):
            acc += rew[t]
            ln += 1
            d = done[t]
            if d.any():
                keep = np.nonzero(d & (count < K))[0]
                ret[keep, count[keep]], length[keep, count[keep]] = acc[keep], ln[keep]
                count[d] += 1
                acc[d], ln[d] = 0.0, 0
    return ret, length, rollouts * T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.runs < 5:
        sys.exit("--runs must be at least 5")
    import train
    K, out = args.episodes, {}
    print("| shape | route | median ms | min ms | max ms | runs | steps | us/step | env steps in the K episodes |\n|---|---|---|---|---|---|---|---|---|")
    for label, param_name, env_name in (("cartpole", "cartpole", "cartpole"), ("mlpmodel + cartpole_swing", "mlpmodel", "cartpole_swing")):
        hp = train.get_hyperparams(param_name)
        agent = build(env_name, hp)
        eng = agent.engine
        agent.env.reset()
        state0 = eng.env_state()

        def host():
            eng.env_set_state(*state0)
            eng.sync()
            t0 = time.perf_counter()
            ret, length, steps = host_route(eng, K, 1)
            eng.sync()
            return (time.perf_counter() - t0) * 1e3, steps, int(length.sum())

        def one():
            eng.sync()
            t0 = time.perf_counter()
            r = eng.env_evaluate(K, seed=1)
            eng.sync()
            return (time.perf_counter() - t0) * 1e3, int(r["length"].sum(axis=1).max()), int(r["length"].sum())
        routes = {"host": host, "one_launch": one}
        for f in routes.values():                    # warm-up: every kernel has run once, the record buffers exist
            f()
        got = {k: [] for k in routes}
        for _ in range(args.runs):
            for k, f in routes.items():              # alternating: a drift of the box hits both sides alike
                got[k].append(f())
        o = {"shape": {"n_envs": hp["n_envs"], "n_steps": hp["n_steps"], "episodes": K, "env": type(agent.env).__name__, "max_steps": agent.env.max_steps,
                       "embedder": "MLPModel(%d, %d, %d, %d)" % (agent.env.observation_space.shape[0], hp["depth"], hp["mid_weight"], hp["latent_size"])}}
        for k, v in got.items():
            s = stats([x[0] for x in v])
            s["steps"], s["env_steps"] = v[0][1], v[0][2]
            assert all(x[1:] == v[0][1:] for x in v)      # every run of a route does the same work
            s["us_per_step"] = 1e3 * s["median_ms"] / s["steps"]
            o[k] = s
            print("| %s E = %d | %s | %.3f | %.3f | %.3f | %d | %d | %.1f | %d |" % (label, hp["n_envs"], k, s["median_ms"], s["min_ms"], s["max_ms"],
                                                                                 s["runs"], s["steps"], s["us_per_step"], s["env_steps"]))
        o["speedup_median"] = o["host"]["median_ms"] / o["one_launch"]["median_ms"]
        o["one_launch_median_below_host_min"] = o["one_launch"]["median_ms"] < o["host"]["min_ms"]
        out[label] = o
        eng.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
