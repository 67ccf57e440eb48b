#!/usr/bin/env python3
"""Time the update phase of one `hard-500-ipl` iteration (IMPALA, T = E = 256, A = 15, 8192-row minibatches, 3 epochs x 8 minibatches =
24 mi_ipl_minibatch passes + 24 optimizer steps) in bf16 on the engine, next to the PPO update of the same shape (`hard-500`: 24
mi_minibatch passes + 24 steps) on the same build and GPU, the two interleaved repetition by repetition.  One IPL minibatch is three
forward and two backward passes where PPO's is one of each.  Prints one JSON line; profiles/ipl_bench.md records a run.

    python scratch/ipl_update_time.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "train-procgen-pytorch_amd")):
    sys.path.insert(0, p)

import numpy as np
import torch

T = E = 256
A, MB, EPOCH, PER_EPOCH, LR, CLIP = 15, 8192, 3, 8, 5e-4, 0.5


def make_engine(rng):
    from common.model import ImpalaModel
    from common.policy import CategoricalPolicy
    from mi355 import engine as M, layout
    from mi355.engine import Engine
    eng = Engine("impala", T, E, A, MB, precision="bf16")
    torch.manual_seed(0)
    pol = CategoricalPolicy(ImpalaModel(3), False, A)
    eng.set_params(layout.flatten(layout.impala_param_shapes(A), {k: v.detach().numpy() for k, v in pol.state_dict().items()}))
    for t in range(T + 1):
        eng.put_obs(t, rng.integers(0, 256, size=(E, 64, 64, 3), dtype=np.uint8))
    for t in range(T):
        eng.put_step(t, rng.standard_normal(E).astype(np.float32), (rng.random(E) < 0.02).astype(np.float32))
    eng.write_field(M.F_ACT, rng.integers(0, A, size=(T, E)).astype(np.float32))
    eng.write_field(M.F_LOGP, np.full((T, E), -np.log(A), np.float32))
    eng.write_field(M.F_VALUE, (0.1 * rng.standard_normal((T + 1, E))).astype(np.float32))
    eng.compute_estimates(0.999, 0.95, True, True)
    eng.sync()
    return eng


def update(eng, minibatch, step0):
    eng.sync()
    t0 = time.perf_counter()
    step = step0
    for _ in range(EPOCH):
        perm = torch.randperm(T * E).numpy()
        for k in range(PER_EPOCH):
            minibatch(perm[k * MB:(k + 1) * MB])
            step += 1
            eng.optimizer_step(LR, CLIP, step)
    eng.loss_log(reset=True)
    eng.sync()
    return (time.perf_counter() - t0) * 1e3, step


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    e_ppo, e_ipl = make_engine(rng), make_engine(rng)
    hp_ppo, hp_ipl = e_ppo.hparams(), e_ipl.ipl_hparams(0.999, 1.0, 0.0)
    ppo, ipl, s_ppo, s_ipl = [], [], 0, 0
    for r in range(a.reps + 1):                 # interleaved; the first repetition warms up
        t, s_ppo = update(e_ppo, lambda i: e_ppo.minibatch(i, MB, hp_ppo), s_ppo)
        ppo.append(t)
        t, s_ipl = update(e_ipl, lambda i: e_ipl.ipl_minibatch(i, MB, hp_ipl), s_ipl)
        ipl.append(t)
    e_ppo.close(); e_ipl.close()
    med = lambda x: float(np.median(x))
    print(json.dumps({"shape": dict(T=T, E=E, A=A, minibatch=MB, epochs=EPOCH, minibatches_per_epoch=PER_EPOCH, precision="bf16"),
                      "ppo_update_ms": ppo[1:], "ipl_update_ms": ipl[1:], "ppo_median_ms": med(ppo[1:]), "ipl_median_ms": med(ipl[1:]),
                      "ratio": med(ipl[1:]) / med(ppo[1:])}))
