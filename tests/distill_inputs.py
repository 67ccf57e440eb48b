"""Inputs, the torch restatement and the bounds of the distillation loss (reference: distill.py:164-204 -- MSELoss(student(obs).logits,
teacher(obs).logits), Adam), shared by tests/test_distill_host.py and tests/test_gpu_distill.py.  Test infrastructure only: nothing here
is imported by the package, and nothing here touches a GPU.

Fixture G19 (tests/golden/g19_distill.npz, written by tests/golden/make_golden_distill.py from the reference's own MLPModel /
CategoricalPolicy): 96 observation rows, both state dicts, the teacher's logits, and per optimizer step the loss, every gradient
(fc_value's is None there: absent) and every parameter after the step.

The restatement.  `mse` is the loss on head outputs -- lp = Categorical(logits=log_softmax(z)).logits, the twice-normalised
log-probabilities, mean over n_global * A elements -- with dY by autograd; `minibatch` the whole pass through the CPU oracle's embedders
(oracle/ppo_oracle.py, pinned to the reference by tests/test_oracle_golden.py).  Both run in the dtype they are asked for: float64 is the
yardstick of the GPU tests, float32 the measure of what float32 can be asked to meet.

Bounds (the standing rule of tests/policy_inputs.py).  dY rows are transcendental per-sample quantities with no derivable bound:
relative L2 over all rows <= 8 x the error of torch's own float32 evaluation of the same function against its float64.  The loss is a
fixed-order sum OF such terms (one sum_k d_k^2 per row), so both parts apply: with rms_q the root-mean-square error of torch's float32
row terms and m rows,  |loss - ref| <= ((d + 2) 2^-24 sum|terms| + 8 m rms_q) / (n_global A) + 2 * 2^-24 |ref|,  d = 6 + 4 + 2 (the wave's six
shuffle steps, up to 1039 / 64 / 256 < 1 strided adds per thread and the finaliser's tree: the sums are fp64, so this part is generous).
Torch's errors are measured on at least POOL_N rows: a case with fewer rows is measured on as many independent draws of the SAME case
(other seeds) as make up POOL_N rows, so the special rows keep their share."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ppo_oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
POOL_N = 1039
OP_N = (1, 63, 64, 65, 257, 1039)          # one row, the wave / block edges, several blocks with a ragged tail
OP_A = (2, 3, 9, 15)                       # 15: A + 1 = 16 = MAXA, the heads' widest row
SUM_DEPTH = 12


def load():
    return np.load(os.path.join(GOLD, "g19_distill.npz"), allow_pickle=False)


def fixture_params(z, prefix):
    """prefix 'student/', 'teacher/' or 'p<k>/' -> name -> float32 array, in state-dict order."""
    return OrderedDict((k[len(prefix):], z[k]) for k in z.files if k.startswith(prefix))


# ------------------------------------------------------------------------------------------ the loss on head outputs
def log_probs(z):
    lp = torch.log_softmax(z, dim=1)
    return lp - lp.logsumexp(dim=-1, keepdim=True)            # Categorical(logits=.) normalises again


def mse(hout, y, n_global=None, dtype=torch.float64):
    """hout (n, A + 1) raw logits then the value, y (n, A) -> (loss, dY (n, A + 1), row terms sum_k d_k^2 (n,)), numpy float64."""
    h = torch.as_tensor(np.asarray(hout)).to(dtype).clone().requires_grad_(True)
    yt = torch.as_tensor(np.asarray(y)).to(dtype)
    n, A = yt.shape
    d = log_probs(h[:, :A]) - yt
    terms = (d * d).sum(1)
    loss = terms.sum() / ((n if n_global is None else n_global) * A)
    loss.backward()
    return float(loss.detach()), h.grad.numpy().astype(np.float64), terms.detach().numpy().astype(np.float64)


def op_case(n, A, seed=0):
    """Random head rows and targets (log-softmax of independent logits, as a teacher's).  From two rows on: row 0 has logits +80 / -80
    (a saturated softmax: lp = 0 and about -160) and row 1 EQUALS its target bit for bit -- logits (0, -200, ..): exp(-200) is 0 in
    float32, so lp = (0, -200, ..) exactly, in the kernel and in float64 -- so its gradient is exactly zero."""
    rng = np.random.default_rng(7919 * n + 31 * A + seed)
    hout = (2.0 * rng.standard_normal((n, A + 1))).astype(np.float32)
    y = torch.log_softmax(torch.from_numpy((2.0 * rng.standard_normal((n, A))).astype(np.float32)), dim=1).numpy()
    if n >= 2:
        hout[0, 0], hout[0, 1] = 80.0, -80.0
        hout[1, :A] = -200.0
        hout[1, 0] = 0.0
        y[1] = hout[1, :A]
    return hout, np.ascontiguousarray(y, dtype=np.float32)


_TORCH_ERR = {}


def torch_errors(n, A):
    """(relative L2 error of torch's float32 dY, rms error of its float32 row terms) against its float64, on the case's pool."""
    if (n, A) not in _TORCH_ERR:
        draws = [op_case(n, A, s) for s in range(-(-POOL_N // n))] if n < 256 else [op_case(n, A)]
        hout, y = np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws])
        _, g64, t64 = mse(hout, y)
        _, g32, t32 = mse(hout, y, dtype=torch.float32)
        _TORCH_ERR[(n, A)] = (rel_l2(g32, g64), float(np.sqrt(np.mean((t32 - t64) ** 2))))
    return _TORCH_ERR[(n, A)]


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-300))


def loss_bound(ref_loss, terms, rms_q, count):
    """terms: the float64 row terms the loss sums; count = n_global * A."""
    terms = np.asarray(terms, np.float64)
    return ((SUM_DEPTH + 2) * U * np.abs(terms).sum() + 8 * terms.size * rms_q) / count + 2 * U * abs(ref_loss)


# ------------------------------------------------------------------------------------------ the whole pass
def _leaves(params, dtype):
    return OrderedDict((k, torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True)) for k, v in params.items())


def forward(p, arch, obs):
    feat = O.impala_embed(p, obs)[0] if arch == "impala" else O.mlp_embed(p, obs)
    return O.heads(p, feat)


def minibatch(params, arch, obs, y, n_global=None, dtype=torch.float64):
    """One distillation minibatch at `dtype`: obs as the reference's policy is fed (float rows / NCHW frames), y (n, A) -> (loss,
    grads name -> numpy; a tensor the loss does not reach -- fc_value -- is absent, as its .grad is None)."""
    p = _leaves(params, dtype)
    lp, _ = forward(p, arch, torch.as_tensor(np.asarray(obs)).to(dtype))
    yt = torch.as_tensor(np.asarray(y)).to(dtype)
    loss = ((lp - yt) ** 2).sum() / ((yt.shape[0] if n_global is None else n_global) * yt.shape[1])
    loss.backward()
    return float(loss.detach()), OrderedDict((k, t.grad.detach().numpy().copy()) for k, t in p.items() if t.grad is not None)


def minibatch_bf16(params, frames_u8, y, forward=None, dtype=torch.float32):
    """The same minibatch with the bf16 engine's rounding points (oracle/ppo_oracle_bf16.py; its loss_and_grads with the MSE in place of
    the PPO loss) -> (loss, grads name -> numpy; fc_value absent).  forward = (feat, cache) of OB.cache_from_engine: the backward pass
    teacher-forced on the engine's own forward tensors.  dtype float64: every contraction accumulates in fp64, same rounding points."""
    from oracle import ppo_oracle_bf16 as OB
    p = OrderedDict((k, torch.as_tensor(np.asarray(v, dtype=np.float32))) for k, v in params.items())
    with torch.no_grad():
        if forward is None:
            feat, cache, _ = OB.impala_forward(p, frames_u8, True, dtype)
            feat = feat.float()
        else:
            feat, cache = forward
    leaf = feat.clone().requires_grad_(True)
    hp = {k: p[k].clone().requires_grad_(True) for k in ("fc_policy.weight", "fc_policy.bias", "fc_value.weight", "fc_value.bias")}
    lp, _ = O.heads(hp, leaf)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float32))
    loss = ((lp - yt) ** 2).sum() / (yt.shape[0] * yt.shape[1])
    loss.backward()
    with torch.no_grad():
        g = OB.impala_backward(p, cache, leaf.grad, feat, True, dtype)
    out = OrderedDict((k, v.float().numpy()) for k, v in g.items())
    for k, t in hp.items():
        if t.grad is not None:
            out[k] = t.grad.detach().numpy()
    return float(loss.detach()), OrderedDict((k, out[k]) for k in p if k in out)


def batches(z):
    """The fixture's batch loop: (step k, rows of the batch) in the reference's order -- contiguous batches, the same every epoch."""
    n, b = z["obs"].shape[0], int(z["batch"])
    k = 0
    for _ in range(int(z["epochs"])):
        for i in range(n // b):
            yield k, np.arange(i * b, (i + 1) * b)
            k += 1
