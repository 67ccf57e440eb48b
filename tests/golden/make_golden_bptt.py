#!/usr/bin/env python3
"""Generate G13 (tests/golden/g13_bptt.npz): the reference's algo ppo-pure with a RECURRENT policy -- PPOPure.optimize
(agents/ppo_pure.py:98-176) through the training branch of GRU.forward (common/model.py:226-277), gradients for all parameters, the
GRU's four tensors included.

Runs the reference like make_golden.py (whose import recipe and helpers it reuses; that file is not changed) plus
`from agents.ppo_pure import PPOPure`, in the build container only.

    python tests/golden/make_golden_bptt.py

Data only.  No weights: the port's policy initialises bit-identically from the seed, the fixture keeps the flat SHA-256 (GRU
included).  The inputs are rebuilt by tests/bptt_inputs.py from seeded generators; the fixture keeps them for case (a) (they are
small) and the frames' SHA-256 for case (b).  Large tensors are stored as L2 norm, sum and 16 fixed +-1 projections
(width_inputs.sketch), tensors of up to 4608 elements whole; case (a) stores everything whole.

Both cases: gamma 0.999, lambda 0.95, normalised advantages, lr 5e-4, torch.manual_seed(5) before optimize() (the env permutation).
  a/...  MLPModel(9, 4, 64, 64), A = 2, T = 8, E = 8, n_minibatch = 2: two minibatches of 4 envs, an optimizer step after each;
         non-zero hidden_states_batch[0]; done drawn at p = 0.25 with a 1 at t = 0, a 1 at t = T - 1 and one env with none.
  b/...  ImpalaModel(3, output_dim=128), A = 15, T = 4, E = 4, one minibatch.
Per case:
  sha, envs (the env permutation of the first epoch), adv, ret
  raw/   grad_clip_norm = 1e9: summary; g<k>/ the gradients handed to optimizer step k (un-clipped); total_norm<k>
  clip/  grad_clip_norm = 0.5, two Adam steps (case b: epoch = 2): norm<k> = the norm clip_grad_norm_ returned at step k,
         p<k>/ all parameters after step k
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))      # the repository root, for `oracle` (behind the reference on the path)
import make_golden as G  # noqa: E402  (imports the reference)
from agents.ppo_pure import PPOPure  # noqa: E402  (the reference's)
import bptt_inputs as BI  # noqa: E402
import width_inputs as WI  # noqa: E402

OUT = os.path.join(HERE, "g13_bptt.npz")


def build(case):
    torch.manual_seed(BI.SEED)
    if case == "a":
        c = BI.CASE_A
        emb = G.MLPModel(c["obs"], c["depth"], c["width"], c["H"])
    else:
        c = BI.CASE_B
        emb = G.ImpalaModel(in_channels=3, output_dim=c["H"])
    policy = G.CategoricalPolicy(emb, True, c["A"])
    policy.device = G.CPU
    return policy


def storage(case, r):
    c = BI.CASE_A if case == "a" else BI.CASE_B
    T, E = c["T"], c["E"]
    st = G.Storage((9,) if case == "a" else (3, 64, 64), c["H"], T, E, G.CPU)
    G.fill_storage(st, r, T, E, case == "b")
    st.hidden_states_batch[0] = torch.from_numpy(r["h0"])
    st.compute_estimates(0.999, 0.95, True, True)
    return st


def run(case, r, clip, epoch):
    c = BI.CASE_A if case == "a" else BI.CASE_B
    T, E = c["T"], c["E"]
    policy, st = build(case), storage(case, r)
    hp = dict(G.BASE_HP, epoch=epoch, n_minibatch=c["n_minibatch"], mini_batch_size=T * E // c["n_minibatch"], grad_clip_norm=clip,
              x_entropy_coef=0.0)
    agent = PPOPure(None, policy, G._NullLogger(), st, G.CPU, 1, n_steps=T, n_envs=E, **hp)
    names = [k for k, _ in policy.named_parameters()]
    cap = dict(grads=[], params=[], norms=[])
    orig_step, orig_clip = agent.optimizer.step, torch.nn.utils.clip_grad_norm_

    def step_hook(*a, **k):
        cap["grads"].append({n: p.grad.detach().numpy().copy() for n, p in zip(names, policy.parameters())})
        out = orig_step(*a, **k)
        cap["params"].append(G.sd_numpy(policy))
        return out

    def clip_hook(params, max_norm, *a, **k):
        n = orig_clip(params, max_norm, *a, **k)
        cap["norms"].append(float(n))
        return n

    agent.optimizer.step = step_hook
    torch.nn.utils.clip_grad_norm_ = clip_hook
    try:
        torch.manual_seed(5)
        summary = agent.optimize()
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    return st, {k: float(v) for k, v in summary.items()}, cap


def put(out, prefix, tensors, whole):
    for k, v in tensors.items():
        if whole or v.size <= WI.SMALL:
            out[f"{prefix}/g/{k}"] = v
        else:
            out[f"{prefix}/norm/{k}"] = np.float64(np.linalg.norm(v.astype(np.float64)))
            out[f"{prefix}/sum/{k}"] = np.float64(v.astype(np.float64).sum())
            out[f"{prefix}/sketch/{k}"] = WI.sketch(v)


def main():
    out = {}
    for case, r in (("a", BI.rollout_a()), ("b", BI.rollout_b())):
        c = BI.CASE_A if case == "a" else BI.CASE_B
        out[f"{case}/sha"] = np.frombuffer(G.flat_sha(build(case)).encode(), np.uint8)
        torch.manual_seed(5)
        out[f"{case}/envs"] = torch.randperm(c["E"]).numpy().astype(np.int64)
        if case == "a":
            for k, v in r.items():
                out[f"a/in/{k}"] = v
        else:
            out["b/frames_sha"] = np.frombuffer(BI.sha(r["frames"]).encode(), np.uint8)
        st, summary, cap = run(case, r, 1e9, 1)
        assert all(np.abs(g[k]).max() > 0 for g in cap["grads"] for k in BI.GRU_KEYS), "the GRU's four tensors receive gradients"
        out[f"{case}/adv"], out[f"{case}/ret"] = st.adv_batch.numpy().copy(), st.return_batch.numpy().copy()
        out[f"{case}/raw/summary"] = np.frombuffer(json.dumps(summary).encode(), np.uint8)
        for k, g in enumerate(cap["grads"], 1):
            put(out, f"{case}/raw/g{k}", g, case == "a")
            out[f"{case}/raw/total_norm{k}"] = np.float64(np.sqrt(sum((v.astype(np.float64) ** 2).sum() for v in g.values())))
        _, summary, cap = run(case, r, 0.5, 1 if case == "a" else 2)
        assert len(cap["params"]) == 2 and len(cap["norms"]) == 2
        out[f"{case}/clip/summary"] = np.frombuffer(json.dumps(summary).encode(), np.uint8)
        for k in (1, 2):
            out[f"{case}/clip/norm{k}"] = np.float64(cap["norms"][k - 1])
            put(out, f"{case}/clip/p{k}", cap["params"][k - 1], case == "a")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
