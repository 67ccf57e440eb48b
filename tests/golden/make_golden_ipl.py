#!/usr/bin/env python3
"""Generate G16 (tests/golden/g16_ipl.npz): the reference's IPL agent (agents/IPL.py, `algo: IPL`) -- IPL.optimize run by the
reference's own method on a reference IPLStorage (common/storage.py:279-361) filled through store / store_last, on the CPU.

Runs the reference like make_golden.py (whose import recipe it reuses; that file is not changed; `wandb`, which agents/IPL.py imports
and never calls here, is registered as an empty module the way that recipe registers `gym`), in the build container only.

    python tests/golden/make_golden_ipl.py

Data only.  Cases, inputs and parameters: tests/ipl_inputs.py (frames of G4, parameters of G3 / G7 with fc_policy.weight scaled).
lr 5e-4, grad_clip_norm 0.5, torch.manual_seed(seed + 100) in front of optimize().

Asserted here, so that the reference alone meets what the tests rely on: every minibatch has a done row, one of them at t = T - 1, and a
non-done row; pred and rew have non-zero variance in every minibatch; in case b the two largest logits of every row of every minibatch
differ by more than 1e-3.

Keys per case '<case>/': act, rew, done (T, E), value (T+1, E); idx (minibatches, n) the index vectors drawn; terms (minibatches, 8)
in the summary's order (column 5, Loss/alpha, is the mean of an empty list: nan); pred0 / rew0 of the first minibatch; g0/ gradients
after the first minibatch's backward; step_norms (optimizer steps, 3, tensors) L2 norms of every parameter / exp_avg / exp_avg_sq after
each optimizer step, names in tensor_names; p/ m/ v/ the heads' parameters and Adam moments after the update; g0/ by the rule of
sae_inputs.store_tensor (whole up to 4608 elements, else norm / sum / sketch / samples); summary (8,) the returned values, adam_step.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))      # the repository root, for `oracle` (behind the reference on the path)
sys.modules.setdefault("wandb", types.ModuleType("wandb"))
import make_golden as G  # noqa: E402  (imports the reference)
import ipl_inputs as II  # noqa: E402
import sae_inputs as SI  # noqa: E402
import agents.IPL as ref_ipl  # noqa: E402  (the reference's: make_golden put it first on the path)
import common.storage as ref_storage  # noqa: E402

OUT = os.path.join(HERE, "g16_ipl.npz")


def build_policy(c, params):
    if c["arch"] == "impala":
        policy = G.CategoricalPolicy(G.ImpalaModel(in_channels=3), False, c["A"])
    else:
        policy = G.CategoricalPolicy(G.MLPModel(9, 4, 256, 64), False, c["A"])
    policy.device = G.CPU
    policy.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    return policy


def run_case(name, c, out):
    T, E, A = c["T"], c["E"], c["A"]
    o = II.opts(c)
    params, roll = II.initial_params(c), II.rollout(c)
    policy = build_policy(c, params)
    obs_shape = (3, 64, 64) if c["arch"] == "impala" else (9,)
    storage = ref_storage.IPLStorage(obs_shape, T, E, G.CPU)
    obs = II.ref_obs(c, roll["frames"]).numpy().reshape(T + 1, E, *obs_shape)
    for t in range(T):
        storage.store(obs[t], roll["act"][t].astype(np.float32), roll["rew"][t], roll["done"][t], [{}] * E, roll["value"][t])
    storage.store_last(obs[T], roll["value"][T])
    agent = ref_ipl.IPL(None, policy, G._NullLogger(), storage, G.CPU, 1, n_steps=T, n_envs=E, epoch=c["epoch"],
                        n_minibatch=c["n_minibatch"], mini_batch_size=c["mini_batch_size"], gamma=c["gamma"], learning_rate=II.LR,
                        grad_clip_norm=II.CLIP, **o)
    for k in ("act", "rew", "done", "value"):
        out[f"{name}/{k}"] = roll[k]

    # what the method keeps to itself: the index vectors (the sampler), the per-minibatch terms (the lists np.mean is called on), pred /
    # rew of every minibatch (mse_loss's arguments), the first backward's gradients (parameter hooks), the state after every step
    idx_log, mean_log, pred_log, grad_log, step_log, logit_log = [], [], [], {}, [], []
    Sampler = ref_storage.BatchSampler

    class RecordingSampler(Sampler):
        def __iter__(self):
            for b in super().__iter__():
                idx_log.append(np.asarray(b, np.int64))
                yield b
    ref_storage.BatchSampler = RecordingSampler
    real_np = ref_ipl.np
    ref_ipl.np = types.SimpleNamespace(mean=lambda lst: (mean_log.append(np.asarray(lst, np.float64)), real_np.mean(lst))[1])
    xbe = ref_ipl.cross_batch_entropy
    ref_ipl.cross_batch_entropy = lambda dist: (logit_log.append(dist.logits.detach().numpy().copy()), xbe(dist))[1]
    mse = torch.nn.functional.mse_loss
    torch.nn.functional.mse_loss = lambda a, b: (pred_log.append((a.detach().numpy().copy(), b.detach().numpy().copy())), mse(a, b))[1]
    names = [n for n, _ in policy.named_parameters()]
    def keep_first(g, n):
        grad_log.setdefault(n, g.detach().clone().numpy())

    hooks = [p.register_hook(lambda g, n=n: keep_first(g, n)) for n, p in policy.named_parameters()]
    opt_step = agent.optimizer.step
    nrm = lambda a: float(np.linalg.norm(np.asarray(a, np.float64)))

    def step(*a, **k):
        r = opt_step(*a, **k)
        st = agent.optimizer.state_dict()["state"]
        step_log.append([[nrm(p.detach().numpy()) for p in policy.parameters()], [nrm(st[i]["exp_avg"].numpy()) for i in range(len(names))],
                         [nrm(st[i]["exp_avg_sq"].numpy()) for i in range(len(names))]])
        return r
    agent.optimizer.step = step
    try:
        torch.manual_seed(c["seed"] + 100)
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                summary = agent.optimize()
    finally:
        ref_storage.BatchSampler, ref_ipl.np, torch.nn.functional.mse_loss, ref_ipl.cross_batch_entropy = Sampler, real_np, mse, xbe
        for h in hooks:
            h.remove()

    assert list(summary) == list(II.SUMMARY_KEYS), list(summary)
    assert len(step_log) == len(II.step_schedule(c)), (len(step_log), II.step_schedule(c))
    idx = np.stack(idx_log)
    done_flat, rew_flat = roll["done"].reshape(-1), roll["rew"].reshape(-1)
    for k, ix in enumerate(idx):
        d = done_flat[ix] > 0
        assert d.any() and (~d).any() and (d & (ix // E == T - 1)).any(), (name, k, "done rows")
        pr, rw = pred_log[k]
        assert np.array_equal(rw, rew_flat[ix]) and pr.std() > 1e-3 and rw.std() > 1e-3, (name, k, "variance")
        if name == "b":         # the max term's arg-max is not tied
            top = np.sort(logit_log[k], axis=-1)
            assert (top[:, -1] - top[:, -2]).min() > 1e-3, (name, k, "logit gap", float((top[:, -1] - top[:, -2]).min()))
    out[f"{name}/idx"] = idx
    out[f"{name}/terms"] = np.stack([m if len(m) else np.full(len(idx), np.nan) for m in mean_log], axis=1)      # (minibatches, 8); Loss/alpha's list is empty
    out[f"{name}/pred0"], out[f"{name}/rew0"] = pred_log[0]
    out[f"{name}/pred_last"] = agent.last_predicted_reward
    out[f"{name}/summary"] = np.asarray(list(summary.values()), np.float64)
    out[f"{name}/step_norms"] = np.asarray(step_log, np.float64)
    out[f"{name}/tensor_names"] = np.frombuffer(json.dumps(names).encode(), dtype=np.uint8)
    st = agent.optimizer.state_dict()["state"]
    for i, (n, p) in enumerate(policy.named_parameters()):
        SI.store_tensor(out, f"{name}/g0/", n, grad_log[n])
        if n.startswith("fc_"):                                  # the heads whole; every tensor's norms after every step are in step_norms
            out[f"{name}/p/{n}"], out[f"{name}/m/{n}"], out[f"{name}/v/{n}"] = p.detach().numpy(), st[i]["exp_avg"].numpy(), st[i]["exp_avg_sq"].numpy()
    out[f"{name}/adam_step"] = np.int64(float(st[0]["step"]))
    print(name, "minibatches", len(idx), "steps", len(step_log), "terms[0]", out[f"{name}/terms"][0])


def main():
    out = {}
    for name, c in II.CASES.items():
        run_case(name, c, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
