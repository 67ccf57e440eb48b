#!/usr/bin/env python3
"""Generate G15 (tests/golden/g15_sae.npz): the reference's sparse-autoencoder agent (agents/sae.py, `algo: sae`) -- the seeded
initialisation of SparseAutoencoder / LinearSAEProbe (common/model.py:1623-1667) and two cases of SAE.optimize_sae followed by
SAE.optimize_linear_model (agents/sae.py:135-218), run by the reference's own SAE methods on a reference SAEStorage
(common/storage.py:513-569) filled through store / store_last with the arrays of tests/sae_inputs.make_rollout.

Runs the reference like make_golden.py (whose import recipe it reuses; that file is not changed), in the build container only.

    python tests/golden/make_golden_sae.py

Data only.  Cases (sae_inputs.CASES): a -- T 4, E 4, A 15, sae_dim 64, 2 epochs of 2 minibatches, one optimizer step each;
b -- T 4, E 8, A 9, sae_dim 192, 1 epoch, mini_batch_per_epoch 4 with mini_batch_size 4: two minibatches accumulate per step.
lr 5e-4, grad_clip_norm 0.5, rho 0.05.  The generator asserts that every unit has 0 < rho_hat < 1 (means taken in float64) in every
minibatch of optimize_sae.

Keys: 'init/<case>' (json: sha256 of the flat parameters of each model, state_dict keys and shapes); per case '<case>/':
  hidden (T+1, E, 2048) float16 (exact), logits (T, E, A), value (T+1, E), act (T, E)
  idx_sae, idx_probe          the index vectors of the minibatches the reference drew (torch.manual_seed(seed + 100 / + 200) before each update)
  sae/ probe/                 losses (per minibatch: recon, KL, total / value, logit, total), summary (the three means the method returns),
                              g0/ = gradients after the first minibatch's backward, p/ = parameters, m/ v/ = Adam moments after the update;
                              storage rule of sae_inputs.store_tensor (whole up to 4608 elements, else norm / sum / sketch / samples)
"""
import hashlib
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
import make_golden as G  # noqa: E402  (imports the reference)
import sae_inputs as SI  # noqa: E402
import agents.sae as ref_sae  # noqa: E402  (the reference's: make_golden put it first on the path)
from common.model import LinearSAEProbe, SparseAutoencoder  # noqa: E402
from common.storage import SAEStorage  # noqa: E402

OUT = os.path.join(HERE, "g15_sae.npz")


def flat_sha(module):
    return hashlib.sha256(np.concatenate([p.detach().numpy().ravel() for p in module.parameters()]).astype(np.float32).tobytes()).hexdigest()


def run_case(name, c, out):
    T, E, A, S = c["T"], c["E"], c["A"], c["S"]
    storage = SAEStorage((3, 64, 64), SI.D, T, E, G.CPU, act_shape=A)
    policy = types.SimpleNamespace(embedder=types.SimpleNamespace(encoded_dim=SI.D), action_size=A)
    torch.manual_seed(c["seed"])           # SAE.__init__ builds the autoencoder, then the probe (agents/sae.py:60-63)
    agent = ref_sae.SAE(None, policy, G._NullLogger(), storage, G.CPU, 1, n_steps=T, n_envs=E, epoch=c["epoch"],
                        mini_batch_per_epoch=c["mini_batch_per_epoch"], mini_batch_size=c["mini_batch_size"], learning_rate=SI.LR,
                        grad_clip_norm=SI.CLIP, sae_dim=S, rho=SI.RHO, sparse_coef=c["sparse_coef"])
    mine = SI.make_models(c, SparseAutoencoder, LinearSAEProbe)
    for a, b in zip((agent.sae, agent.linear_model), mine):
        assert flat_sha(a) == flat_sha(b)
    out[f"init/{name}"] = np.frombuffer(json.dumps({
        "sae": {"sha256": flat_sha(agent.sae), "keys": [[k, list(v.shape)] for k, v in agent.sae.state_dict().items()]},
        "probe": {"sha256": flat_sha(agent.linear_model), "keys": [[k, list(v.shape)] for k, v in agent.linear_model.state_dict().items()]},
    }).encode(), dtype=np.uint8)

    roll = SI.make_rollout(c, agent.sae.encoder[0].weight.detach().numpy())
    assert (roll["hidden"] >= 0).all() and 0.3 < (roll["hidden"] == 0).mean() < 0.7
    obs = np.zeros((E, 3, 64, 64), np.float32)
    zero = np.zeros(E, np.float32)
    for t in range(T):
        storage.store(obs, roll["hidden"][t], roll["act"][t].astype(np.float32), zero, zero, [{}] * E, roll["logits"][t], roll["value"][t])
    storage.store_last(obs, roll["hidden"][T], roll["value"][T])
    out[f"{name}/hidden"] = roll["hidden"].astype(np.float16)
    assert np.array_equal(out[f"{name}/hidden"].astype(np.float32), roll["hidden"])
    out[f"{name}/logits"], out[f"{name}/value"], out[f"{name}/act"] = roll["logits"], roll["value"], roll["act"]

    # what the methods keep to themselves: the index vectors (collate_data), the per-minibatch losses (the lists np.mean is called on,
    # in the order total, first term, second term), the first minibatch's gradients (parameter hooks), rho_hat (kl_divergence)
    idx_log, mean_log, grad_log = [], [], {}
    collate = storage.collate_data
    storage.collate_data = lambda indices: (idx_log.append(np.asarray(indices, np.int64)), collate(indices))[1]
    ref_sae.np = types.SimpleNamespace(mean=lambda lst: (mean_log.append(np.asarray(lst, np.float64)), np.mean(lst))[1])
    kl = agent.sae.kl_divergence

    def kl_checked(encoded):
        rh = encoded.detach().double().mean(dim=0)
        assert (rh > 0).all() and (rh < 1).all(), (name, float(rh.min()), float(rh.max()))
        kl_checked.range = (min(kl_checked.range[0], float(rh.min())), max(kl_checked.range[1], float(rh.max())))
        return kl(encoded)
    kl_checked.range = (1.0, 0.0)
    agent.sae.kl_divergence = kl_checked

    for stage, model, fn, opt, seed_off in (("sae", agent.sae, agent.optimize_sae, lambda: agent.optimizer, 100),
                                            ("probe", agent.linear_model, agent.optimize_linear_model, lambda: agent.l_optimizer, 200)):
        del idx_log[:], mean_log[:]
        grad_log.clear()
        def keep_first(g, n):
            grad_log.setdefault(n, g.detach().clone().numpy())

        hooks = [p.register_hook(lambda g, n=n: keep_first(g, n)) for n, p in model.named_parameters()]
        torch.manual_seed(c["seed"] + seed_off)
        summary = fn()
        for h in hooks:
            h.remove()
        pre = f"{name}/{stage}/"
        out[f"{name}/idx_{stage}"] = np.stack(idx_log)
        total, first, second = mean_log
        out[pre + "losses"] = np.stack([first, second, total], axis=1)
        out[pre + "summary"] = np.asarray(list(summary.values()), np.float64)
        out[pre + "summary_keys"] = np.frombuffer(json.dumps(list(summary)).encode(), dtype=np.uint8)
        st = opt().state_dict()["state"]
        for i, (n, p) in enumerate(model.named_parameters()):
            SI.store_tensor(out, pre + "g0/", n, grad_log[n])
            SI.store_tensor(out, pre + "p/", n, p.detach().numpy())
            SI.store_tensor(out, pre + "m/", n, st[i]["exp_avg"].numpy())
            SI.store_tensor(out, pre + "v/", n, st[i]["exp_avg_sq"].numpy())
        out[pre + "adam_step"] = np.int64(float(st[0]["step"]))
    print(name, "rho_hat range", kl_checked.range, "minibatches", len(out[f"{name}/idx_sae"]), len(out[f"{name}/idx_probe"]))


def main():
    out = {}
    for name, c in SI.CASES.items():
        run_case(name, c, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
