#!/usr/bin/env python3
"""Generate G19 (tests/golden/g19_distill.npz): the fit phase of the reference's distill.py (distill.py:164-204) -- MSELoss on
`policy(obs).logits`, torch.optim.Adam(new_policy.parameters(), lr=lr), zero_grad / backward / step over contiguous batches in the same
order every epoch -- run on the reference's OWN common/model.py MLPModel and common/policy.py CategoricalPolicy, on the CPU.

    python tests/golden/make_golden_distill.py <path of the reference checkout>

The reference is imported from the path on the command line; modules its common/ package imports that are not installed in the build
container (gym, gymnasium, vector_quantize_pytorch) are registered as stand-ins that are never called.  distill.py itself is not
imported: it pulls in the Procgen wrappers, pandas and wandb (a stand-in for pandas breaks torch's own optional-import probing), and
its statements here are the few torch calls named above.  Data only; no test runs this file.

Student CategoricalPolicy(MLPModel(9, 4, 64, 64), False, 2), teacher CategoricalPolicy(MLPModel(9, 2, 32, 64), False, 2); fc_policy.weight
of both is scaled after the 0.01-gain initialisation (student x 20, teacher x 60: unscaled, both softmaxes are uniform and the loss is
1e-6).  96 observation rows, batch 32, 2 epochs, lr 1e-3: six optimizer steps.

Keys: obs (96, 9); student/<tensor>, teacher/<tensor> the two state dicts; y_gold (96, 2) = teacher(obs).logits; loss (6,) float32 as
loss.item() gives it; per step k = 0..5: g<k>/<tensor> the gradients after backward (fc_value.weight / fc_value.bias have grad None and
are ABSENT), p<k>/<tensor> every parameter after the step; step_norms (6, 2, tensors with state) the L2 norms of exp_avg / exp_avg_sq
after each step; tensor_names (json) policy.named_parameters() order; state_names (json) the tensors the final optimizer.state_dict()
has state for; adam_step; lr, batch, epochs."""
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "g19_distill.npz")
N, BATCH, EPOCHS, LR = 96, 32, 2, 1e-3
STUDENT_SCALE, TEACHER_SCALE = 20.0, 60.0


def import_reference(path):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules.setdefault(name, m)
        return sys.modules[name]

    stub("gym").logger = types.SimpleNamespace(set_level=lambda lvl: None)
    sp = stub("gymnasium.spaces", Box=type("Box", (), {}), Discrete=type("Discrete", (), {}))
    stub("gymnasium").spaces = sp
    stub("vector_quantize_pytorch", VectorQuantize=type("VectorQuantize", (nn.Module,), {}), FSQ=type("FSQ", (nn.Module,), {}))
    sys.path.insert(0, path)
    from common.model import MLPModel
    from common.policy import CategoricalPolicy
    return MLPModel, CategoricalPolicy


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_golden_distill.py <path of the reference checkout>")
    MLPModel, CategoricalPolicy = import_reference(sys.argv[1])
    cpu = torch.device("cpu")
    torch.manual_seed(1900)
    new_policy = CategoricalPolicy(MLPModel(9, 4, 64, 64), False, 2)
    policy = CategoricalPolicy(MLPModel(9, 2, 32, 64), False, 2)
    for p, s in ((new_policy, STUDENT_SCALE), (policy, TEACHER_SCALE)):
        p.device = cpu
        with torch.no_grad():
            p.fc_policy.weight.mul_(s)
    rng = np.random.default_rng(1901)
    obs = rng.uniform(-1.5, 1.5, size=(N, 9)).astype(np.float32)
    hidden_state = np.zeros((N, 64), np.float32)
    out = dict(obs=obs, lr=np.float64(LR), batch=np.int64(BATCH), epochs=np.int64(EPOCHS))
    for k, v in new_policy.state_dict().items():
        out["student/" + k] = v.detach().numpy().copy()
    for k, v in policy.state_dict().items():
        out["teacher/" + k] = v.detach().numpy().copy()
    policy.eval()
    with torch.no_grad():
        dist, _, _ = policy(torch.Tensor(obs), hidden_state, hidden_state)
        Y_gold = dist.logits
    out["y_gold"] = Y_gold.numpy().copy()

    criterion = torch.nn.MSELoss()
    optimizer = torch.optim.Adam(new_policy.parameters(), lr=LR)
    new_policy.train()
    obs_tensor = torch.Tensor(obs)
    names = [n for n, _ in new_policy.named_parameters()]
    losses, norms, step = [], [], 0
    for epoch in range(EPOCHS):
        for i in range(N // BATCH):
            optimizer.zero_grad()
            obs_batch = obs_tensor[i * BATCH:(i + 1) * BATCH]
            Y_batch = Y_gold[i * BATCH:(i + 1) * BATCH]
            dist_batch, value_batch, _ = new_policy(obs_batch, hidden_state, hidden_state)
            Y_pred = dist_batch.logits
            loss = criterion(Y_pred.squeeze(), Y_batch.squeeze())
            loss.backward()
            for n, p in new_policy.named_parameters():
                if p.grad is not None:
                    out[f"g{step}/{n}"] = p.grad.detach().numpy().copy()
            optimizer.step()
            losses.append(np.float32(loss.item()))
            for n, p in new_policy.named_parameters():
                out[f"p{step}/{n}"] = p.detach().numpy().copy()
            st = optimizer.state_dict()["state"]
            nrm = lambda a: float(np.linalg.norm(a.numpy().astype(np.float64)))
            norms.append([[nrm(st[j]["exp_avg"]) for j in sorted(st)], [nrm(st[j]["exp_avg_sq"]) for j in sorted(st)]])
            step += 1
    st = optimizer.state_dict()["state"]
    state_names = [names[j] for j in sorted(st)]
    assert not any(n.startswith("fc_value") for n in state_names) and len(state_names) == len(names) - 2
    assert all(f"g0/{n}" in out for n in state_names) and "g0/fc_value.weight" not in out
    for n in ("fc_value.weight", "fc_value.bias"):
        assert np.array_equal(out[f"p{step - 1}/{n}"], out["student/" + n])
    out["loss"] = np.asarray(losses, np.float32)
    out["step_norms"] = np.asarray(norms, np.float64)
    out["tensor_names"] = np.frombuffer(json.dumps(names).encode(), dtype=np.uint8)
    out["state_names"] = np.frombuffer(json.dumps(state_names).encode(), dtype=np.uint8)
    out["adam_step"] = np.int64(float(st[sorted(st)[0]]["step"]))
    np.savez_compressed(OUT, **out)
    print("losses", out["loss"], "steps", step, "wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
