"""Inputs and the torch restatement of one IPL minibatch (reference: agents/IPL.py:125-192 with cross_batch_entropy,
common/misc_util.py:42-51), shared by tests/golden/make_golden_ipl.py (which runs the reference itself), tests/test_ipl_host.py and
tests/test_gpu_ipl.py.  Test infrastructure only: nothing here is imported by the package.

Fixture G16 (tests/golden/g16_ipl.npz) holds no observations and no initial parameters: the frames are those of G4 (IMPALA / MLP, T = 4,
E = 8), the parameters those of G3 / G7 with fc_policy.weight scaled by LOGIT_SCALE[arch] (the 0.01-gain initialisation leaves the softmax
uniform: the max term, the greedy action and the entropy gradient would see ties and zeros) -- case c takes the first four envs and
the first nine rows of fc_policy.  What it holds per case: act / rew / done / value as stored, the index vectors the reference drew, per
minibatch the eight summary terms, pred and rew of the first minibatch, the gradients after the first backward, parameter and Adam
moment norms after every optimizer step, parameters and moments after the update (rule of sae_inputs.store_tensor), the summary.

The embedders are the CPU oracle's (oracle/ppo_oracle.py, pinned to the reference by tests/test_oracle_golden.py); `ipl_terms` is the
loss itself on head outputs, `minibatch` the whole two-observation pass.  Both run in the dtype they are asked for: float64 is the
per-element yardstick of the GPU tests."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ppo_oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LR, CLIP = 5e-4, 0.5
LOGIT_SCALE = dict(impala=600.0, mlp=60.0)
TERMS = ("entropy", "mutual_info", "total", "rew_corr", "gamma", "alpha_loss", "alpha", "pred_reward")
SUMMARY_KEYS = ("Loss/entropy", "Loss/mutual_info", "Loss/total", "Loss/rew_corr", "Loss/gamma", "Loss/alpha", "alpha", "Loss/pred_reward")
DEFAULT_OPTS = dict(alpha=1, entropy_coef=0, entropy_modified=False, reward_incentive=False, adv_incentive=False, accumulate_all_grads=False)
# a: one minibatch of 32, one step.  b: batch_size = 32 / 2 = 16, mini_batch_size 8: two minibatches accumulate per step, 2 steps per
# epoch.  c: batch_size = 16 / 2 = 8 = mini_batch_size, accumulate_all_grads: the two minibatches of an epoch share ONE step.
CASES = OrderedDict(
    a=dict(arch="impala", T=4, E=8, A=15, epoch=1, n_minibatch=1, mini_batch_size=32, gamma=0.999, seed=7101, opts={}),
    b=dict(arch="mlp", T=4, E=8, A=2, epoch=2, n_minibatch=2, mini_batch_size=8, gamma=0.99, seed=7125,
           opts=dict(alpha=0.5, entropy_coef=0.01, entropy_modified=True, reward_incentive=True, adv_incentive=True)),
    c=dict(arch="impala", T=4, E=4, A=9, epoch=2, n_minibatch=2, mini_batch_size=8, gamma=0.999, seed=7103, opts=dict(accumulate_all_grads=True)))


def opts(c):
    return dict(DEFAULT_OPTS, **c["opts"])


def accumulation(c):
    """agents/IPL.py:113-116 -> (mini_batch_size used, batch_size / mini_batch_size)."""
    batch_size = c["T"] * c["E"] // c["n_minibatch"]
    mbs = min(c["mini_batch_size"], batch_size)
    return mbs, batch_size / mbs


def step_schedule(c):
    """Number of minibatches in front of each optimizer step of one optimize() (IPL.py:195-211)."""
    mbs, every = accumulation(c)
    per_epoch = c["T"] * c["E"] // mbs
    steps, cnt = [], 1
    for _ in range(c["epoch"]):
        for _ in range(per_epoch):
            if not opts(c)["accumulate_all_grads"] and cnt % every == 0:
                steps.append(cnt)
            cnt += 1
        if opts(c)["accumulate_all_grads"]:
            steps.append(cnt - 1)
    return steps


def _load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def initial_params(c):
    z = _load("g3_impala_forward.npz" if c["arch"] == "impala" else "g7_mlp_forward.npz")
    p = OrderedDict((k[2:], z[k].astype(np.float32)) for k in z.files if k.startswith("p/"))
    A = c["A"]
    p["fc_policy.weight"] = (p["fc_policy.weight"][:A] * np.float32(LOGIT_SCALE[c["arch"]])).astype(np.float32)
    p["fc_policy.bias"] = p["fc_policy.bias"][:A].copy()
    return p


def rollout(c):
    """frames (T+1, E, ...) of G4 (device layout: uint8 NHWC / fp32 rows) and seeded act / rew / done / value.  About a third of the rows
    are done, the last step's in every other env at least."""
    g4 = _load("g4_impala_lossgrad.npz" if c["arch"] == "impala" else "g4_mlp_lossgrad.npz")
    T, E, A = c["T"], c["E"], c["A"]
    rng = np.random.default_rng(c["seed"])
    done = (rng.random((T, E)) < 0.3).astype(np.float32)
    done[T - 1, ::2] = 1.0
    return dict(frames=g4["in/frames"][:, :E].copy(), act=rng.integers(0, A, size=(T, E)).astype(np.int64),
                rew=rng.standard_normal((T, E)).astype(np.float32), done=done,
                value=(0.5 * rng.standard_normal((T + 1, E))).astype(np.float32))


def ref_obs(c, frames):
    """device-layout observations -> what the reference's policy is fed (float NCHW frames / rows), flattened over the leading axes."""
    f = np.asarray(frames)
    if c["arch"] == "impala":
        return O.frames_to_obs(f.reshape(-1, 64, 64, 3))
    return torch.from_numpy(f.reshape(-1, f.shape[-1]).astype(np.float32))


# ------------------------------------------------------------------------------------------ the restatement
def ipl_terms(lp, v, nv_raw, act, rew, done, gamma, o):
    """IPL.py:129-188 from the head outputs: lp (n, A) normalised log-probs, v (n,), nv_raw (n,) = V(nobs) before the overwrite.
    -> (loss, pred, dict of the eight terms as tensors)."""
    nv = torch.where(done.bool(), rew, nv_raw)                # next_value_batch[done] = rew[done]: no gradient through those rows
    logp = lp.gather(1, act.reshape(-1, 1).long()).reshape(-1)
    modifier = o["alpha"] * (1 - logp.exp()) if o["entropy_modified"] else o["alpha"]
    pred = modifier * logp + v - gamma * nv
    loss = ((pred - rew) ** 2).mean()
    if o["reward_incentive"]:
        loss = loss - pred.mean()
    if o["adv_incentive"]:
        loss = loss - lp.max(dim=-1)[0].mean()
    corr = torch.corrcoef(torch.stack((pred, rew)))[0, 1] if len(pred) > 1 else torch.tensor(float("nan"))
    p = lp.exp()
    p = p / p.sum(-1, keepdim=True)                           # Categorical.probs = softmax(logits)
    entropy = -(p * lp).sum(-1).mean()
    action_p = p.mean(0)
    marg = -(action_p * torch.log(action_p)).sum()
    loss = loss + o["entropy_coef"] * entropy
    terms = dict(entropy=entropy, mutual_info=marg - entropy, total=loss, rew_corr=corr, pred_reward=pred.mean())
    return loss, pred, terms


def terms_row(terms, gamma, alpha):
    f = lambda k: float(terms[k].detach())
    return np.array([f("entropy"), f("mutual_info"), f("total"), f("rew_corr"), gamma, np.nan, alpha, f("pred_reward")], np.float64)


def _leaves(params, dtype):
    return OrderedDict((k, torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True)) for k, v in params.items())


def forward(p, arch, obs):
    feat = O.impala_embed(p, obs)[0] if arch == "impala" else O.mlp_embed(p, obs)
    return O.heads(p, feat)


def minibatch(c, params, roll, idx, dtype=torch.float64, o=None, next_only=False):
    """One IPL minibatch on rows idx of the rollout at `dtype` -> (terms row (8,), pred, grads name -> numpy).
    next_only: alpha = 0 and the obs-side value detached -- the gradient then reaches the network through obs[t + 1] alone."""
    o = dict(opts(c) if o is None else o)
    T, E = c["T"], c["E"]
    idx = np.asarray(idx, np.int64)
    p = _leaves(params, dtype)
    all_obs = ref_obs(c, roll["frames"]).to(dtype)
    obs, nobs = all_obs[:T * E][idx], all_obs[E:][idx]
    to = lambda a: torch.as_tensor(np.asarray(a)[:T].reshape(-1)[idx]).to(dtype)
    if next_only:           # (entropy and max terms reach the network through obs[t] only: off as well)
        o.update(alpha=0.0, entropy_coef=0.0, adv_incentive=False)
    lp, v = forward(p, c["arch"], obs)
    if next_only:
        v = v.detach()
    _, nv = forward(p, c["arch"], nobs)
    loss, pred, terms = ipl_terms(lp, v, nv, torch.as_tensor(roll["act"].reshape(-1)[idx]), to(roll["rew"]), to(roll["done"]), c["gamma"], o)
    loss.backward()
    grads = OrderedDict((k, t.grad.detach().numpy().copy()) for k, t in p.items() if t.grad is not None)
    return terms_row(terms, c["gamma"], o["alpha"]), pred.detach().numpy(), grads


def replay(c, params, roll, idx_list, dtype=torch.float64):
    """IPL.optimize of case c in torch at `dtype` on the given minibatches: clip_grad_norm_ + Adam(eps=1e-5) at the reference's step
    positions.  -> (terms (minibatches, 8), pred of the last minibatch)."""
    T, E = c["T"], c["E"]
    o = opts(c)
    p = _leaves(params, dtype)
    opt = torch.optim.Adam(list(p.values()), lr=LR, eps=1e-5)
    all_obs = ref_obs(c, roll["frames"]).to(dtype)
    steps, rows, pred = set(step_schedule(c)), [], None
    for k, idx in enumerate(idx_list):
        idx = np.asarray(idx, np.int64)
        to = lambda a: torch.as_tensor(np.asarray(a)[:T].reshape(-1)[idx]).to(dtype)
        lp, v = forward(p, c["arch"], all_obs[:T * E][idx])
        _, nv = forward(p, c["arch"], all_obs[E:][idx])
        loss, pred, terms = ipl_terms(lp, v, nv, torch.as_tensor(roll["act"].reshape(-1)[idx]), to(roll["rew"]), to(roll["done"]), c["gamma"], o)
        loss.backward()
        rows.append(terms_row(terms, c["gamma"], o["alpha"]))
        if k + 1 in steps:
            torch.nn.utils.clip_grad_norm_(list(p.values()), CLIP)
            opt.step()
            opt.zero_grad()
    return np.stack(rows), pred.detach().numpy()


# ------------------------------------------------------------------------------------------ fixture access
def load_case(z, name):
    """-> (case, rollout, params, list of index vectors) of fixture z; the rollout's scalars are the fixture's own copies."""
    c = CASES[name]
    roll = rollout(c)
    for k in ("act", "rew", "done", "value"):
        assert np.array_equal(roll[k], z[f"{name}/{k}"]), (name, k)
    return c, roll, initial_params(c), list(z[f"{name}/idx"])
