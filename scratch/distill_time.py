#!/usr/bin/env python3
"""Time the distiller's device passes at the reference's default shapes (`hard-500` IMPALA, T = E = 256 = 65 536 ring rows, A = 15,
batches of 8192 rows, bf16), every comparison interleaved repetition by repetition on one GPU, the first repetition of each leg a
warm-up that is dropped:

  (a) one mi_distill_minibatch of 8192 rows against one mi_minibatch (PPO) of the same rows: the same network passes, a lighter loss;
  (b) one exploration's fit phase -- 10 epochs x 8 batches = 80 minibatches + 80 Adam steps -- on the engine against torch-ROCm (fp32,
      eager) running the reference's loop (zero_grad, forward, MSELoss on the normalised logits, backward, Adam.step, loss.item()) on the
      same shapes, the network being the CPU oracle's functional IMPALA (oracle/ppo_oracle.py) on cuda tensors;
  (c) mi_distill_label over the full ring, with a teacher max_batch of 8192 (8 chunks) and of 2048 (32 chunks: what distill.py's
      validation ring gives the teacher by default).

    python scratch/distill_time.py [--reps 11] [--torch_reps 11] [--out FILE]

Prints one JSON line per leg as it finishes and the whole record at the end (and to --out); profiles/distill_bench.md records a run."""
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
A, MB, EPOCHS, LR = 15, 8192, 10, 1e-4
INF = float("inf")


def policy_params(seed, scale):
    from common.model import ImpalaModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(seed)
    p = {k: v.detach().numpy().copy() for k, v in CategoricalPolicy(ImpalaModel(3), False, A).state_dict().items()}
    p["fc_policy.weight"] *= np.float32(scale)                 # (the 0.01-gain initialisation leaves the softmax uniform)
    return p


def make_engine(frames, params, max_batch=MB, ppo=False):
    from mi355 import engine as M, layout
    from mi355.engine import Engine
    eng = Engine("impala", T, E, A, max_batch, precision="bf16")
    eng.set_params(layout.flatten(layout.impala_param_shapes(A), params))
    for t in range(T + 1):
        eng.put_obs(t, frames[t % T])
    if ppo:
        rng = np.random.default_rng(1)
        for t in range(T):
            eng.put_step(t, rng.standard_normal(E).astype(np.float32), (rng.random(E) < 0.02).astype(np.float32))
        eng.write_field(M.F_ACT, rng.integers(0, A, size=(T, E)).astype(np.float32))
        eng.write_field(M.F_LOGP, np.full((T, E), -np.log(A), np.float32))
        eng.write_field(M.F_VALUE, (0.1 * rng.standard_normal((T + 1, E))).astype(np.float32))
        eng.compute_estimates(0.999, 0.95, True, True)
    eng.sync()
    return eng


def timed(eng, fn):
    eng.sync()
    t0 = time.perf_counter()
    fn()
    eng.sync()
    return (time.perf_counter() - t0) * 1e3


def stats(x):
    x = [float(v) for v in x]
    return dict(runs=[round(v, 3) for v in x], median=round(float(np.median(x)), 3), min=round(min(x), 3), max=round(max(x), 3))


def torch_fit(p, opt, obs, y, perm):
    """the reference's batch loop (distill.py:178-204) on cuda tensors"""
    from oracle import ppo_oracle as O
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    total = 0.0
    for _ in range(EPOCHS):
        for i in range(len(perm) // MB):
            rows = perm[i * MB:(i + 1) * MB]
            opt.zero_grad()
            lp, _ = O.heads(p, O.impala_embed(p, obs[rows].float().div_(255.0))[0])
            loss = torch.nn.functional.mse_loss(lp, y[rows])
            loss.backward()
            opt.step()
            total += loss.item()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--torch_reps", type=int, default=11)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, size=(T, E, 64, 64, 3), dtype=np.uint8)
    sp, tp = policy_params(0, 100.0), policy_params(1, 300.0)
    student, ppo, teacher = make_engine(frames, sp), make_engine(frames, sp, ppo=True), make_engine(frames, tp)
    small_teacher = make_engine(frames, tp, max_batch=2048)
    out = dict(shape=dict(T=T, E=E, A=A, batch=MB, epochs=EPOCHS, precision="bf16"))

    def emit(key, val):
        out[key] = val
        print(json.dumps({key: val}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    # (c) the labels (also what (a) and (b) fit to)
    lab, lab_small = [], []
    for r in range(a.reps + 1):
        lab.append(timed(student, lambda: student.distill_label(teacher)))
        lab_small.append(timed(student, lambda: student.distill_label(small_teacher)))
    student.distill_label(teacher)
    emit("c_label_full_ring_ms", dict(teacher_max_batch_8192=stats(lab[1:]), teacher_max_batch_2048=stats(lab_small[1:])))

    # (a) one minibatch pass, PPO and distillation taking turns on the same rows
    hp = ppo.hparams()
    idx = rng.permutation(T * E)[:MB]
    t_ppo, t_dst = [], []
    for r in range(a.reps + 1):
        t_ppo.append(timed(ppo, lambda: ppo.minibatch(idx, MB, hp)))
        t_dst.append(timed(student, lambda: student.distill_minibatch(idx, MB)))
        ppo.loss_log(reset=True); student.loss_log(reset=True)
    ppo.optimizer_step(LR, 0.5, 1); student.optimizer_step_eps(LR, INF, 1e-8, 1)          # (zeroes the accumulated gradients)
    emit("a_minibatch_ms", dict(ppo=stats(t_ppo[1:]), distill=stats(t_dst[1:])))

    # (b) the fit phase of one exploration: engine and torch-ROCm taking turns
    dev = torch.device("cuda", 0)
    obs = torch.from_numpy(frames.reshape(T * E, 64, 64, 3)).to(dev).permute(0, 3, 1, 2).contiguous()      # uint8 NCHW, 805 MB
    y = torch.from_numpy(student.distill_targets()).to(dev)
    p = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sp.items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR)
    step = [1]

    def engine_fit(perm):
        for _ in range(EPOCHS):
            for i in range(len(perm) // MB):
                student.distill_minibatch(perm[i * MB:(i + 1) * MB], MB)
                step[0] += 1
                student.optimizer_step_eps(LR, INF, 1e-8, step[0])
        student.loss_log(reset=True)

    t_eng, t_torch = [], []
    for r in range(max(a.reps, a.torch_reps) + 1):
        perm = rng.permutation(T * E)
        if r <= a.reps:
            t_eng.append(timed(student, lambda: engine_fit(perm)))
        if r <= a.torch_reps:
            t_torch.append(torch_fit(p, opt, obs, y, torch.from_numpy(perm).to(dev)))
            emit("b_fit_phase_ms_partial", dict(engine=stats(t_eng[1:]) if len(t_eng) > 1 else None, torch_rocm_fp32=stats(t_torch[1:]) if len(t_torch) > 1 else None))
    emit("b_fit_phase_ms", dict(engine=stats(t_eng[1:]), torch_rocm_fp32=stats(t_torch[1:])))
    for e in (student, ppo, teacher, small_teacher):
        e.close()
    print(json.dumps(out))
