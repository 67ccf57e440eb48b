#!/usr/bin/env python3
"""Time one optimize_sae and one optimize_linear_model of the SAE agent at the `sae` hyper-parameter set's shape (E = T = 256,
sae_dim 1024, 8192-row minibatches, 3 epochs x 8 minibatches = 24 minibatch passes + 24 optimizer steps each) on the engine, and the same
math in torch-ROCm (fp32, eager) on the same GPU next to it.  Prints one JSON line; profiles/sae_bench.md records a run.

    python scratch/sae_update_time.py [--reps 3]
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
S, A, MB, EPOCH, PER_EPOCH = 1024, 9, 8192, 3, 8
D, RHO, COEF, LR, CLIP, EPS = 2048, 0.05, 1e-3, 5e-4, 0.5, 1e-10


def engine_times(reps):
    from mi355.engine import Engine
    rng = np.random.default_rng(0)
    eng = Engine("impala", T, E, A, MB, precision="bf16")
    eng.sae_create(S, RHO)
    from common.model import LinearSAEProbe, SparseAutoencoder
    torch.manual_seed(0)
    sae, probe = SparseAutoencoder(D, S, RHO), LinearSAEProbe(S, A)
    flat = lambda m: np.concatenate([p.detach().numpy().ravel() for p in m.parameters()])
    eng.sae_set_params(eng.SAE, flat(sae))
    eng.sae_set_params(eng.PROBE, flat(probe))
    for t in range(T + 1):
        hid = np.maximum(rng.standard_normal((E, D)), 0).astype(np.float32) * np.float32(0.3)
        z = rng.standard_normal((E, A)).astype(np.float32)
        eng.sae_put_ring(t, hid, z - np.log(np.exp(z).sum(-1, keepdims=True)) if t < T else None)
        eng.put_policy_outputs(t, None, None, rng.standard_normal(E).astype(np.float32))
    out = {}
    for name, which, mb in (("optimize_sae", eng.SAE, lambda i: eng.sae_minibatch(i, COEF)), ("optimize_linear_model", eng.PROBE, eng.sae_probe_minibatch)):
        ts, step = [], 0
        for r in range(reps + 1):
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(EPOCH):
                perm = torch.randperm(T * E).numpy()
                for k in range(PER_EPOCH):
                    mb(perm[k * MB:(k + 1) * MB])
                    step += 1
                    eng.sae_optimizer_step(which, LR, CLIP, step)
            eng.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = ts[1:]                      # the first repetition warms up
    eng.close()
    return out


def torch_times(reps):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    x_all = (torch.randn(T * E, D, generator=g).clamp_(min=0) * 0.3).to(dev)
    l_all = torch.randn(T * E, A, generator=g).log_softmax(-1).to(dev)
    v_all = torch.randn(T * E, generator=g).to(dev)
    enc_m = torch.nn.Sequential(torch.nn.Linear(D, S), torch.nn.ReLU()).to(dev)
    dec_m = torch.nn.Linear(S, D).to(dev)
    pol, val = torch.nn.Linear(S, A).to(dev), torch.nn.Linear(S, 1).to(dev)
    kld = torch.nn.KLDivLoss(reduction="batchmean")

    def sae_mb(idx):
        x = x_all[idx]
        enc = enc_m(x)
        rec = dec_m(enc)
        rh = enc.mean(0)
        kl = torch.sum(RHO * torch.log((RHO + EPS) / (rh + EPS)) + (1 - RHO) * torch.log((1 - RHO + EPS) / (1 - rh + EPS)))
        loss = ((rec - x) ** 2).mean() + COEF * kl
        loss.backward()
        return loss

    def probe_mb(idx):
        with torch.no_grad():
            enc = enc_m(x_all[idx])
        vh = val(enc)[:, 0]
        v = v_all[idx]
        # the reference's (n,1) - (n,) broadcast is an (n,n) matrix: 268 MB at n = 8192; its O(n) closed form is timed instead
        vl = (vh ** 2).mean() - 2 * vh.mean() * v.mean() + (v ** 2).mean()
        loss = kld(pol(enc).log_softmax(-1), l_all[idx].softmax(-1)) + vl
        loss.backward()
        return loss

    out = {}
    for name, params, mb in (("optimize_sae", list(enc_m.parameters()) + list(dec_m.parameters()), sae_mb),
                             ("optimize_linear_model", list(pol.parameters()) + list(val.parameters()), probe_mb)):
        opt = torch.optim.Adam(params, lr=LR, eps=1e-5)
        ts = []
        for r in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(EPOCH):
                perm = torch.randperm(T * E).to(dev)
                for k in range(PER_EPOCH):
                    mb(perm[k * MB:(k + 1) * MB]).item()          # (the reference reads every loss back: .item() per minibatch)
                    torch.nn.utils.clip_grad_norm_(params, CLIP)
                    opt.step()
                    opt.zero_grad()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = ts[1:]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps({"shape": dict(T=T, E=E, sae_dim=S, A=A, minibatch=MB, epochs=EPOCH, minibatches_per_epoch=PER_EPOCH),
                      "engine_ms": engine_times(a.reps), "torch_rocm_fp32_ms": torch_times(a.reps)}))
