"""Plain-torch restatement of CategoricalPolicy(logsumexp_logits_is_v=True) (reference: common/policy.py:74-87 with :77-78,
v = logits.logsumexp(-1)) under the PPO loss, and the inputs of fixture G14 (tests/golden/make_golden_lse.py).

The embedders and the loss are the CPU oracle's (oracle/ppo_oracle.py, pinned to the reference by tests/test_oracle_golden.py); only the
heads differ: the value is the logsumexp of the RAW fc_policy outputs, fc_value is a parameter that nothing reads (so autograd leaves
its gradient None, clip_grad_norm_ skips it and Adam never creates state for it).  Everything runs in the dtype it is asked for, so
the GPU tests use it as a float64 twin."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ppo_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T, E = 4, 8
ARCHS = {"impala": dict(A=15, H=256, g4="g4_impala_lossgrad.npz", params="g3_impala_forward.npz"),
         "mlp": dict(A=2, H=64, g4="g4_mlp_lossgrad.npz", params="g7_mlp_forward.npz")}
HP = dict(eps_clip=0.2, value_coef=0.5, entropy_coef=0.01)
VALUE_KEYS = ("fc_value.weight", "fc_value.bias")
GRU_KEYS = ("gru.gru.weight_ih_l0", "gru.gru.weight_hh_l0", "gru.gru.bias_ih_l0", "gru.gru.bias_hh_l0")
NOISE_SEED, NOISE_STD = 29, 0.25          # old values = the reference's own logsumexp values + default_rng(29).standard_normal * 0.25


def heads(p, feat):
    """hidden_to_output + distribution with logsumexp_logits_is_v (policy.py:74-87) -> (logp_all as Categorical.logits, value)."""
    logits = F.linear(feat, p["fc_policy.weight"], p["fc_policy.bias"])
    lp = F.log_softmax(logits, dim=1)
    lp = lp - lp.logsumexp(dim=-1, keepdim=True)        # Categorical.__init__ normalises again
    return lp, logits.logsumexp(-1)


def embed(p, arch, obs):
    return O.impala_embed(p, obs)[0] if arch == "impala" else O.mlp_embed(p, obs)


def _leaves(params, dtype):
    return OrderedDict((k, torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True)) for k, v in params.items())


def forward(params, arch, obs, dtype=torch.float32):
    """-> (logp_all, value, feat) as numpy."""
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in params.items()}
    with torch.no_grad():
        feat = embed(p, arch, torch.as_tensor(np.asarray(obs)).to(dtype))
        lp, v = heads(p, feat)
    return lp.numpy(), v.numpy(), feat.numpy()


def loss_and_grads(params, arch, obs, act, old_logp, old_value, ret, adv, x_entropy_coef=0.0, dtype=torch.float32, feat=None):
    """One minibatch.  feat (n, H): run the heads and the loss from these features instead of the embedder (teacher forcing on the
    engine's own features); only the heads' tensors then receive gradients.
    -> (losses dict of floats, grads OrderedDict name -> numpy for every tensor whose grad is not None, [names whose grad is None])."""
    p = _leaves(params, dtype)
    to = lambda a: torch.as_tensor(np.asarray(a)).to(dtype).reshape(-1)
    h = embed(p, arch, torch.as_tensor(np.asarray(obs)).to(dtype)) if feat is None else torch.as_tensor(np.asarray(feat)).to(dtype)
    lp, v = heads(p, h)
    L = O.ppo_loss(lp, v, torch.as_tensor(np.asarray(act)).reshape(-1), to(old_logp), to(old_value), to(ret), to(adv), HP["eps_clip"],
                   HP["value_coef"], HP["entropy_coef"], x_entropy_coef, 1.0)
    L["total"].backward()
    grads = OrderedDict((k, t.grad.detach().numpy().copy()) for k, t in p.items() if t.grad is not None)
    return {k: float(x.detach()) for k, x in L.items()}, grads, [k for k, t in p.items() if t.grad is None]


def adam_first_step(params, grads, clip, lr):
    """clip_grad_norm_ + the first Adam(eps=1e-5) step over the tensors that have a gradient; the others are returned unchanged."""
    p = OrderedDict((k, torch.as_tensor(np.array(v, dtype=np.float32)).clone()) for k, v in params.items())
    g = OrderedDict((k, torch.as_tensor(np.array(v, dtype=np.float32)).clone()) for k, v in grads.items())
    norm, _ = O.clip_grad_norm(g, clip)
    sub = OrderedDict((k, p[k]) for k in g)
    O.adam_step(sub, g, OrderedDict((k, torch.zeros_like(v)) for k, v in sub.items()),
                OrderedDict((k, torch.zeros_like(v)) for k, v in sub.items()), 1, lr)
    return OrderedDict((k, v.numpy()) for k, v in p.items()), norm


def saliency(params, arch, obs, dtype=torch.float32, hidden=None, done=None):
    """d sum_e value_e / d obs (agents/ppo.py:83-94; each value depends on its own observation only).  hidden (n, H) / done (n): the
    policy is recurrent (params holds gru.gru.*), the heads sit on h' = GRU(embedder(obs), hidden (1 - done)).
    -> (value, gradient in obs's layout, h' or None) as numpy."""
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in params.items()}
    x = torch.as_tensor(np.asarray(obs)).to(dtype).clone().requires_grad_(True)
    h = embed(p, arch, x)
    if hidden is not None:
        h = O.gru_cell(p, h, torch.as_tensor(np.asarray(hidden)).to(dtype), 1.0 - torch.as_tensor(np.asarray(done)).to(dtype))
    _, v = heads(p, h)
    v.sum().backward()
    return v.detach().numpy(), x.grad.numpy(), (h.detach().numpy() if hidden is not None else None)


def rel_l2(a, r):
    a, r = np.asarray(a, np.float64).ravel(), np.asarray(r, np.float64).ravel()
    return float(np.linalg.norm(a - r) / (np.linalg.norm(r) + 1e-30))


# ---------------------------------------------------------------------------------------------- fixture G14 inputs
def load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def base_params(arch):
    """The parameters of G3 (IMPALA, A = 15) / G7 (MLP, A = 2) as they are."""
    z = load(ARCHS[arch]["params"])
    return OrderedDict((k[2:], z[k]) for k in z.files if k.startswith("p/"))


def ref_obs(arch, frames):
    """(..., 64, 64, 3) uint8 frames -> the reference's float NCHW observations (flattened over the leading axes); MLP rows as they are."""
    f = np.asarray(frames)
    return O.frames_to_obs(f.reshape(-1, 64, 64, 3)) if arch == "impala" else torch.from_numpy(f.reshape(-1, f.shape[-1]).astype(np.float32))


def case(arch):
    """Everything a G14 test needs for one architecture: G4's rollout (frames, rew, done, act, logp -- read from the G4 fixture, not
    copied), G3 / G7's parameters with G14's scaled fc_policy.weight, G14's old values, and the fixture itself (keys under '<arch>/')."""
    c = dict(ARCHS[arch])
    g4, z = load(c["g4"]), load("g14_lse_value.npz")
    params = base_params(arch)
    params["fc_policy.weight"] = z[f"{arch}/fc_policy.weight"]
    c.update(arch=arch, z=z, params=params, frames=g4["in/frames"], rew=g4["in/rew"], done=g4["in/done"], act=g4["in/act"],
             logp=g4["in/logp"], val=z[f"{arch}/val"], adv=z[f"{arch}/adv"], ret=z[f"{arch}/ret"])
    return c


class Sub:
    """View of an npz under a key prefix, with the npz's .files / [] protocol (width_inputs.grad_errors reads a fixture through it)."""

    def __init__(self, z, prefix):
        self.z, self.prefix = z, prefix
        self.files = [k[len(prefix):] for k in z.files if k.startswith(prefix)]

    def __getitem__(self, k):
        return self.z[self.prefix + k]
