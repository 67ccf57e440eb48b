"""Inputs and the torch restatement of the sparse-autoencoder agent's two updates (reference: agents/sae.py:135-218, models
common/model.py:1623-1667), shared by tests/golden/make_golden_sae.py (which runs the reference itself), tests/test_sae_host.py and
tests/test_gpu_sae.py.  Test infrastructure only: nothing here is imported by the package.

Fixture G15 (tests/golden/g15_sae.npz) holds, per case, the stored rollout arrays, the minibatch index vectors the reference drew, its
per-minibatch losses, the gradients of the first minibatch and the parameters / Adam moments after the update.  Tensors of up to
4608 elements are stored whole; larger ones as L2 norm, sum, 16 fixed +-1 projections (width_inputs.sketch) and 4096 strided samples.

`replay(case, dtype)` runs the same two updates in torch at a chosen precision: float32 restates the reference (tests/test_sae_host.py
pins it to the fixture), float64 is the yardstick the GPU tests measure both the engine and torch's own fp32 arithmetic against."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from width_inputs import sketch  # noqa: E402

D = 2048                                    # ImpalaModel.encoded_dim
WHOLE = 4608                                # tensors up to this many elements are stored whole
N_SAMPLE = 4096
# T, E, A, sae_dim, epoch, mini_batch_per_epoch, mini_batch_size: case a takes one optimizer step per minibatch (batch_size = T*E/2 = 8 <
# mini_batch_size); in case b batch_size = 8 and mini_batch_size = 4, so two minibatches accumulate per optimizer step
CASES = OrderedDict(
    a=dict(T=4, E=4, A=15, S=64, epoch=2, mini_batch_per_epoch=2, mini_batch_size=256, sparse_coef=1e-3, seed=6033),
    b=dict(T=4, E=8, A=9, S=192, epoch=1, mini_batch_per_epoch=4, mini_batch_size=4, sparse_coef=0.02, seed=6034))
LR, CLIP, RHO, EPS = 5e-4, 0.5, 0.05, 1e-10
SAE_KEYS = ("encoder.0.weight", "encoder.0.bias", "decoder.0.weight", "decoder.0.bias")
PROBE_KEYS = ("fc_policy.weight", "fc_policy.bias", "fc_value.weight", "fc_value.bias")


def shapes(c):
    S, A = c["S"], c["A"]
    return OrderedDict([("encoder.0.weight", (S, D)), ("encoder.0.bias", (S,)), ("decoder.0.weight", (D, S)), ("decoder.0.bias", (D,)),
                        ("fc_policy.weight", (A, S)), ("fc_policy.bias", (A,)), ("fc_value.weight", (1, S)), ("fc_value.bias", (1,))])


def accumulation(c):
    """agents/sae.py:137-140 -> (mini_batch_size used, optimizer step every k minibatches)."""
    batch_size = c["T"] * c["E"] // c["mini_batch_per_epoch"]
    mbs = min(c["mini_batch_size"], batch_size)
    return mbs, batch_size / mbs


def make_models(c, sae_cls, probe_cls):
    """The two models as SAE.__init__ builds them (agents/sae.py:60-63) from the case's seed: the autoencoder first, then the probe."""
    torch.manual_seed(c["seed"])
    return sae_cls(D, c["S"], RHO), probe_cls(c["S"], c["A"])


def make_rollout(c, w_enc):
    """Stored arrays of a case.  hidden (T+1, E, 2048): non-negative like real ReLU features, about half of the entries zero, and built
    from the seeded encoder weights so that the initial pre-activations W_e x are chosen numbers: 0.25 .. 0.6 (the unit is active),
    except -0.1 on the rows r with (r + j) % 8 == 0 of unit j (silent there) -- with minibatches of 4 rows a unit that is silent on
    all 4 gives rho_hat = 0, which random features do to some unit of 192 nearly always.  Each row starts as relu(W_e^T a + noise) and is
    corrected on its support by the least-norm solution of W_e x = target; rounded to float16 (the fixture stores them as such).
    logits: normalised log-probabilities with a spread; value: rows with distinct means, so that the reference's pairwise value loss
    differs from the per-sample one."""
    T, E, A, S = c["T"], c["E"], c["A"], c["S"]
    rng = np.random.default_rng(c["seed"])
    W = w_enc.astype(np.float64)
    R = (T + 1) * E
    target = rng.uniform(0.25, 0.6, size=(R, S))
    target[(np.arange(R)[:, None] + np.arange(S)[None, :]) % 8 == 0] = -0.1
    x = np.maximum(rng.uniform(0.5, 1.5, size=(R, S)) @ W * 0.1 + 0.01 * rng.standard_normal((R, D)), 0.0)
    for r in range(R):
        sup = x[r] > 0
        Ws = W[:, sup]
        x[r, sup] += Ws.T @ np.linalg.solve(Ws @ Ws.T, target[r] - W @ x[r])
    hidden = np.maximum(x, 0.0).reshape(T + 1, E, D).astype(np.float16).astype(np.float32)
    z = 1.5 * rng.standard_normal((T, E, A))
    logits = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    value = (rng.standard_normal((T + 1, E)) + 2.0 * rng.standard_normal((1, E)) + 1.0).astype(np.float32)
    act = rng.integers(0, A, size=(T, E)).astype(np.int64)
    return dict(hidden=hidden, logits=logits, value=value, act=act)


def store_tensor(out, prefix, name, a):
    a = np.asarray(a)
    if a.size <= WHOLE:
        out[f"{prefix}g/{name}"] = a.astype(np.float32)
    else:
        a64 = a.astype(np.float64).ravel()
        out[f"{prefix}norm/{name}"] = np.float64(np.linalg.norm(a64))
        out[f"{prefix}sum/{name}"] = np.float64(a64.sum())
        out[f"{prefix}sketch/{name}"] = sketch(a64)
        out[f"{prefix}sample/{name}"] = a.ravel()[::max(1, a.size // N_SAMPLE)][:N_SAMPLE].astype(np.float32)


def tensor_error(a, z, prefix, name):
    """Error of tensor a against what the fixture holds for it, as a fraction of the reference tensor's L2 norm (whole tensors: the relative
    L2 error; sketched ones: the worst of norm, sum / sqrt(n), the projections and the strided samples' L2 error over the whole norm)."""
    a64 = np.asarray(a, np.float64).ravel()
    if f"{prefix}g/{name}" in z.files:
        r = z[f"{prefix}g/{name}"].astype(np.float64).ravel()
        return float(np.linalg.norm(a64 - r) / (np.linalg.norm(r) + 1e-300))
    nrm = float(z[f"{prefix}norm/{name}"])
    smp = z[f"{prefix}sample/{name}"].astype(np.float64)
    mine = a64[::max(1, a64.size // N_SAMPLE)][:N_SAMPLE]
    errs = [abs(np.linalg.norm(a64) - nrm), abs(a64.sum() - float(z[f"{prefix}sum/{name}"])) / np.sqrt(a64.size),
            float(np.abs(sketch(a64) - z[f"{prefix}sketch/{name}"]).max()), float(np.linalg.norm(mine - smp))]
    return max(errs) / (nrm + 1e-300)


def tensor_error_pair(a, r):
    """The same measure between two whole tensors (how far torch's own fp32 run is from the float64 one)."""
    a64, r64 = np.asarray(a, np.float64).ravel(), np.asarray(r, np.float64).ravel()
    if a64.size <= WHOLE:
        return float(np.linalg.norm(a64 - r64) / (np.linalg.norm(r64) + 1e-300))
    st = max(1, a64.size // N_SAMPLE)
    errs = [abs(np.linalg.norm(a64) - np.linalg.norm(r64)), abs(a64.sum() - r64.sum()) / np.sqrt(a64.size),
            float(np.abs(sketch(a64) - sketch(r64)).max()), float(np.linalg.norm(a64[::st][:N_SAMPLE] - r64[::st][:N_SAMPLE]))]
    return max(errs) / (np.linalg.norm(r64) + 1e-300)


# ------------------------------------------------------------------------------------------ the restatement
def sae_forward(P, x):
    enc = torch.relu(x @ P["encoder.0.weight"].T + P["encoder.0.bias"])
    return enc @ P["decoder.0.weight"].T + P["decoder.0.bias"], enc


def sae_losses(P, x, rho=RHO):
    """agents/sae.py:151-155 with SparseAutoencoder.kl_divergence (common/model.py:1645-1653) -> (recon, KL, rho_hat)."""
    rec, enc = sae_forward(P, x)
    recon = ((rec - x) ** 2).mean()
    rho_hat = enc.mean(dim=0)
    kl = torch.sum(rho * torch.log((rho + EPS) / (rho_hat + EPS)) + (1 - rho) * torch.log((1 - rho + EPS) / (1 - rho_hat + EPS)))
    return recon, kl, rho_hat


def probe_losses(P, Q, x, logit_batch, value_batch):
    """agents/sae.py:193-200 as written: value_hat is (n,1) and value_batch (n,), so the squared difference broadcasts to (n,n).
    -> (value_loss, logit_loss, the per-sample value loss the expression looks like)."""
    with torch.no_grad():
        _, enc = sae_forward(P, x)
    logit_hat = (enc @ Q["fc_policy.weight"].T + Q["fc_policy.bias"]).log_softmax(dim=-1)
    value_hat = enc @ Q["fc_value.weight"].T + Q["fc_value.bias"]
    value_loss = ((value_hat - value_batch) ** 2).mean()
    logit_loss = torch.nn.KLDivLoss(reduction='batchmean')(logit_hat, logit_batch.softmax(dim=-1))
    per_sample = ((value_hat[:, 0] - value_batch) ** 2).mean()
    return value_loss, logit_loss, per_sample


def _stage(params, loss_fn, idx_list, every, lr=LR, clip=CLIP):
    opt = torch.optim.Adam(list(params.values()), lr=lr, eps=1e-5)
    losses, g0 = [], None
    for k, idx in enumerate(idx_list):
        terms = loss_fn(idx)
        terms[-1].backward()
        losses.append([float(t.detach()) for t in terms])
        if k == 0:
            g0 = OrderedDict((n, p.grad.detach().clone().numpy()) for n, p in params.items())
        if (k + 1) % every == 0:
            torch.nn.utils.clip_grad_norm_(list(params.values()), clip)
            opt.step()
            opt.zero_grad()
    st = opt.state_dict()["state"]
    m = OrderedDict((n, st[i]["exp_avg"].numpy().copy()) for i, n in enumerate(params) if i in st)
    v = OrderedDict((n, st[i]["exp_avg_sq"].numpy().copy()) for i, n in enumerate(params) if i in st)
    return dict(losses=np.asarray(losses, np.float64), g0=g0, params=OrderedDict((n, p.detach().numpy().copy()) for n, p in params.items()), m=m, v=v)


def replay(c, init, roll, idx_sae, idx_probe, dtype):
    """optimize_sae then optimize_linear_model of case c in torch at `dtype`, on the minibatches idx_sae / idx_probe (lists of index
    vectors).  init: name -> initial fp32 array of all eight tensors.  -> {'sae': ..., 'probe': ...}, each with losses (rows
    (recon, KL, loss) / (value, logit, loss)), g0, params, m, v."""
    T, E = c["T"], c["E"]
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    x_all = t(roll["hidden"][:T].reshape(T * E, D))
    l_all, v_all = t(roll["logits"].reshape(T * E, -1)), t(roll["value"][:T].reshape(T * E))
    P = OrderedDict((n, t(init[n]).clone().requires_grad_(True)) for n in SAE_KEYS)
    Q = OrderedDict((n, t(init[n]).clone().requires_grad_(True)) for n in PROBE_KEYS)
    _, every = accumulation(c)

    def sae_fn(idx):
        recon, kl, _ = sae_losses(P, x_all[idx])
        return recon, kl, recon + c["sparse_coef"] * kl

    def probe_fn(idx):
        vl, ll, _ = probe_losses(P, Q, x_all[idx], l_all[idx], v_all[idx])
        return vl, ll, ll + vl

    out = {"sae": _stage(P, sae_fn, [torch.as_tensor(i) for i in idx_sae], every)}
    out["probe"] = _stage(Q, probe_fn, [torch.as_tensor(i) for i in idx_probe], every)
    return out


def load_case(z, name):
    """-> (case dict, rollout arrays, idx_sae, idx_probe) of fixture z."""
    c = CASES[name]
    roll = dict(hidden=z[f"{name}/hidden"].astype(np.float32), logits=z[f"{name}/logits"], value=z[f"{name}/value"], act=z[f"{name}/act"])
    return c, roll, list(z[f"{name}/idx_sae"]), list(z[f"{name}/idx_probe"])
