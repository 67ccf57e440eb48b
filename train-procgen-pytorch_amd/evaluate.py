#!/usr/bin/env python3
"""Evaluate a trained policy on a device-resident env: whole episodes, one kernel launch per env range (PPO.evaluate, mi_env_evaluate).

    python evaluate.py --model_file logs/train/cartpole/x/<run>/model_200015872.pth --env_name cartpole --param_name cartpole --both

Every env runs --episodes whole episodes of the checkpoint's policy -- sampled actions, or arg-max actions with --greedy -- on the
training ranges of the env's physics parameters, on the validation ranges (--valid), or on both (--both): the generalisation study the
reference's cart-pole and mountain-car sets are made for.  The envs are built as train.py --device_env builds them (same factories, same
hyper-parameter sets, `<name>_v` overrides included) and the policy through train.py's own initialize_model; the evaluation's episodes
come from the device env's reset stream at episode counters from 2^40 on, disjoint from any training run's.

Prints the statistics (common.logger.evaluation_stats) and writes, into the checkpoint's directory, evaluation.npz -- the per-episode
records ret / length / terminated / value0 / start, (n_envs, episodes) each, with the prefix `val_` for the validation ranges -- and one
row of evaluation.csv.  Only envs with a device-resident form (the cart-pole names and mountain_car), non-recurrent MLP policies, one GPU."""
import argparse
import csv
import os

import numpy as np

RECORD_KEYS = ("ret", "length", "terminated", "value0", "start")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument('--model_file', type=str, default=None, help="checkpoint of train.py (model_<timesteps>.pth); required")
    p.add_argument('--env_name', type=str, default='cartpole')
    p.add_argument('--param_name', type=str, default='cartpole')
    p.add_argument('--n_envs', type=int, default=None, help="default: the hyper-parameter set's")
    p.add_argument('--seed', type=int, default=0, help="the envs' reset streams (training: seed, validation: seed + 1) and the sampler")
    p.add_argument('--episodes', type=int, default=10, help="whole episodes per env")
    p.add_argument('--greedy', action="store_true", help="arg-max actions instead of sampled ones")
    p.add_argument('--gpu_device', type=int, default=0)
    g = p.add_mutually_exclusive_group()
    g.add_argument('--valid', action="store_true", help="the validation ranges instead of the training ranges")
    g.add_argument('--both', action="store_true", help="the training ranges and the validation ranges")
    return p.parse_args(argv)


def check_args(args):
    """Everything that can be refused before a GPU is touched -> (hyper-parameters, env name)."""
    import train
    if not args.model_file:
        raise ValueError("--model_file is required: evaluate.py evaluates the policy of a checkpoint (model_<timesteps>.pth of train.py)")
    if not os.path.isfile(args.model_file):
        raise FileNotFoundError(f"--model_file {args.model_file}: no such file")
    hp = train.get_hyperparams(args.param_name)
    if args.n_envs is not None:
        hp["n_envs"] = args.n_envs
    env_name = hp.get("env_name", args.env_name)
    train.check_device_env(env_name, hp, hp.get("algo", "ppo"))      # refuses a name without a device-resident env
    return hp, env_name


def evaluate(args):
    hp, env_name = check_args(args)
    import torch
    import train
    from agents.ppo import PPO
    from common.env.vec_envs import create_vector_env
    from common.logger import EVALUATION_KEYS, Logger
    from common.storage import Storage
    train.set_global_seeds(args.seed)
    device = torch.device("cuda", args.gpu_device)
    n_envs, n_steps = hp.get("n_envs", 256), hp.get("n_steps", 256)
    want_train, want_valid = not args.valid, args.valid or args.both
    env = create_vector_env(env_name, hp, False, seed=args.seed, n_envs=n_envs, device=True)
    env_valid = create_vector_env(env_name, hp, True, seed=args.seed + 1, n_envs=n_envs, device=True) if want_valid else None
    model, obs_shape, policy = train.initialize_model(device, env, hp)
    make_storage = lambda: Storage(obs_shape, model.output_dim, n_steps, n_envs, device)
    agent = PPO(env, policy, Logger(n_envs, None), make_storage(), device, 0, env_valid=env_valid,
                storage_valid=make_storage() if want_valid else None, seed=args.seed, **hp)
    print("Loading agent from %s" % args.model_file)
    ck = torch.load(args.model_file, map_location="cpu", weights_only=True)
    agent.policy.load_state_dict(ck["model_state_dict"])
    records, row = {}, {}
    for valid, prefix, label in ((False, "", "training ranges"), (True, "val_", "validation ranges")):
        if not (want_valid if valid else want_train):
            row.update({prefix + k: float("nan") for k in EVALUATION_KEYS})
            continue
        out = agent.evaluate(episodes=args.episodes, greedy=args.greedy, valid=valid, seed=args.seed)
        records.update({prefix + k: out[k] for k in RECORD_KEYS})
        row.update({prefix + k: out[k] for k in EVALUATION_KEYS})
        print(f"{label}: {n_envs} envs x {args.episodes} episodes, {'greedy' if args.greedy else 'sampled'} actions, "
              f"{int(out['length'].sum())} env steps")
        for k in EVALUATION_KEYS:
            print(f"  {prefix + k}:\t{out[k]:.4g}")
    logdir = os.path.dirname(os.path.abspath(args.model_file))
    np.savez(os.path.join(logdir, "evaluation.npz"), **records)
    head = dict(model_file=os.path.basename(args.model_file), env_name=env_name, param_name=args.param_name, n_envs=n_envs,
                episodes=args.episodes, greedy=int(args.greedy), seed=args.seed)
    head.update(row)
    path = os.path.join(logdir, "evaluation.csv")
    new = not os.path.exists(path) or os.path.getsize(path) == 0
    with open(path, "a") as f:
        w = csv.writer(f)
        if new:
            w.writerow(head.keys())
        w.writerow(head.values())
    print(f"Wrote {os.path.join(logdir, 'evaluation.npz')} and a row of {path}")
    for eng in (agent.engine, agent.engine_valid):
        if eng is not None:
            eng.close()
    return records, row


if __name__ == '__main__':
    evaluate(parse_args())
