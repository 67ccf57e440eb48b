"""Plain-torch restatement of one recurrent minibatch of algo ppo-pure (reference: agents/ppo_pure.py:121-156 with
Storage.fetch_train_generator(recurrent=True), common/storage.py:93-110, and the training branch of GRU.forward,
common/model.py:226-277), and the inputs of fixture G13 (tests/golden/make_golden_bptt.py).

The GRU runs step by step as an nn.GRU on h * m[t], m[t] = 1 - done_batch[t]: the done stored WITH step t.  The reference's
segment loop over has_zeros is the same arithmetic (inside a segment every mask is 1).  The embedder, the heads and the loss are
the CPU oracle's (oracle/ppo_oracle.py), which the oracle tests pin to the reference.  Everything runs in the dtype of the tensors
it is given, so the GPU tests use it as a float64 twin."""
import hashlib
from collections import OrderedDict

import numpy as np
import torch

from oracle import ppo_oracle as O

GRU_KEYS = ("gru.gru.weight_ih_l0", "gru.gru.weight_hh_l0", "gru.gru.bias_ih_l0", "gru.gru.bias_hh_l0")
HP = dict(eps_clip=0.2, value_coef=0.5, entropy_coef=0.01, x_entropy_coef=0.0)


def gru_sequence(x, h0, mask, w_ih, w_hh, b_ih, b_hh):
    """x (T, n, H), h0 (n, H), mask (T, n) -> h (T, n, H): h_t = GRU(x_t, h_{t-1} * mask[t]), one nn.GRU call per step with the
    given tensors as its weights (they stay the autograd leaves)."""
    H = w_hh.shape[1]
    g = torch.nn.GRU(H, H).to(w_ih.dtype)
    w = dict(weight_ih_l0=w_ih, weight_hh_l0=w_hh, bias_ih_l0=b_ih, bias_hh_l0=b_hh)
    h, out = h0, []
    for t in range(x.shape[0]):
        _, hn = torch.func.functional_call(g, w, (x[t].unsqueeze(0), (h * mask[t].unsqueeze(1)).unsqueeze(0)))
        h = hn.squeeze(0)
        out.append(h)
    return torch.stack(out)


def rec_minibatch(params, arch, obs, h0, done, act, old_logp, old_value, ret, adv, hp=HP, dtype=torch.float64, x_override=None):
    """One recurrent ppo-pure minibatch of n envs x T steps.  params: state-dict name -> array (GRU under gru.gru.*); obs (T, n, ...)
    in the reference's layout; h0 (n, H); done / act / old_logp / old_value / ret / adv (T, n).  x_override (T, n, H): run from these
    embedder outputs instead of the embedder (teacher forcing; it becomes a leaf whose gradient is returned as grads['x']).
    -> (losses dict of floats, grads OrderedDict name -> tensor)."""
    p = OrderedDict((k, torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True)) for k, v in params.items())
    T, n = done.shape
    to = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    if x_override is not None:
        xl = to(x_override).clone().requires_grad_(True)
        x = xl
    else:
        o = to(obs).reshape(T * n, *np.asarray(obs).shape[2:])
        x = (O.impala_embed(p, o)[0] if arch == "impala" else O.mlp_embed(p, o)).reshape(T, n, -1)
    h = gru_sequence(x, to(h0), 1.0 - to(done), *(p[k] for k in GRU_KEYS))
    lp, value = O.heads(p, h.reshape(T * n, -1))
    f = lambda a: to(a).reshape(-1)
    L = O.ppo_loss(lp, value, torch.as_tensor(np.asarray(act)).reshape(-1), f(old_logp), f(old_value), f(ret), f(adv), hp["eps_clip"],
                   hp["value_coef"], hp["entropy_coef"], hp["x_entropy_coef"], 1.0)
    L["total"].backward()
    grads = OrderedDict((k, t.grad.detach().clone()) for k, t in p.items() if t.grad is not None)
    if x_override is not None:
        grads["x"] = xl.grad.detach().clone()
    return {k: float(v.detach()) for k, v in L.items()}, grads


def rel_l2(a, r):
    a, r = np.asarray(a, np.float64).ravel(), np.asarray(r, np.float64).ravel()
    return float(np.linalg.norm(a - r) / (np.linalg.norm(r) + 1e-30))


# ---------------------------------------------------------------------------------------------- fixture G13 inputs
SEED = 6033
CASE_A = dict(T=8, E=8, A=2, obs=9, depth=4, width=64, H=64, n_minibatch=2)          # MLPModel(9, 4, 64, 64)
CASE_B = dict(T=4, E=4, A=15, H=128, n_minibatch=1)                                  # ImpalaModel(3, output_dim=128)


def done_pattern(rng, T, E, p=0.25):
    """done (T, E) drawn at p, forced to hold a 1 at t = 0, a 1 at t = T - 1 and one env that never finishes."""
    done = (rng.random((T, E)) < p).astype(np.float32)
    done[0, 1] = 1.0
    done[T - 1, 2] = 1.0
    done[:, 0] = 0.0
    return done


def rollout_a():
    """Case (a): everything the recurrent minibatches read, from default_rng(41)."""
    c = CASE_A
    rng = np.random.default_rng(41)
    T, E, A = c["T"], c["E"], c["A"]
    return dict(frames=rng.standard_normal((T + 1, E, c["obs"])).astype(np.float32),
                act=rng.integers(0, A, size=(T, E)).astype(np.int64),
                rew=rng.standard_normal((T, E)).astype(np.float32),
                done=done_pattern(rng, T, E),
                logp=(np.log(1.0 / A) + 0.1 * rng.standard_normal((T, E))).astype(np.float32),
                val=(0.5 * rng.standard_normal((T + 1, E))).astype(np.float32),
                h0=(0.5 * rng.standard_normal((E, c["H"]))).astype(np.float32))


def rollout_b():
    """Case (b): frames from default_rng(43) first (the fixture keeps their SHA-256), then the scalars."""
    c = CASE_B
    rng = np.random.default_rng(43)
    T, E, A = c["T"], c["E"], c["A"]
    return dict(frames=rng.integers(0, 256, size=(T + 1, E, 64, 64, 3), dtype=np.uint8),
                act=rng.integers(0, A, size=(T, E)).astype(np.int64),
                rew=rng.standard_normal((T, E)).astype(np.float32),
                done=done_pattern(rng, T, E),
                logp=(np.log(1.0 / A) + 0.1 * rng.standard_normal((T, E))).astype(np.float32),
                val=(0.5 * rng.standard_normal((T + 1, E))).astype(np.float32),
                h0=(0.5 * rng.standard_normal((E, c["H"]))).astype(np.float32))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def flat_sha(module):
    """SHA-256 of the concatenated parameters in policy.parameters() order (the GRU's four tensors last), as make_golden.flat_sha."""
    flat = np.concatenate([q.detach().cpu().numpy().ravel() for q in module.parameters()]).astype(np.float32)
    return hashlib.sha256(flat.tobytes()).hexdigest()


def build_policy(case):
    """The port's policy of a G13 case, initialised from SEED (bit-identical to the reference's: the fixture's flat SHA checks it)."""
    from common.model import ImpalaModel, MLPModel
    from common.policy import CategoricalPolicy
    torch.manual_seed(SEED)
    if case == "a":
        c = CASE_A
        emb = MLPModel(c["obs"], c["depth"], c["width"], c["H"])
    else:
        c = CASE_B
        emb = ImpalaModel(3, output_dim=c["H"])
    return CategoricalPolicy(emb, True, c["A"])


def host_params(policy):
    """state-dict name -> numpy of the HOST tensors (no engine attached, or before any device update)."""
    return OrderedDict((k, v.detach().cpu().numpy().copy()) for k, v in torch.nn.Module.state_dict(policy).items())
