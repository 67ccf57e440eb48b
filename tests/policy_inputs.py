"""Inputs, float64 references, bounds and checkers for the op-level tests of the policy heads (csrc/heads.hip), the samplers and the PPO
loss (csrc/loss.hip, csrc/policy_math.h): tests/test_gpu_policy_ops.py on the GPU, tests/test_policy_host.py on the CPU.  Nothing here
touches a GPU.

References.  oracle.ppo_oracle.heads / ppo_loss / sample_actions restated in float64 torch (test_policy_host.py pins the restatement to the
oracle on the G4 / G14 inputs), per sample: the loss reference hands out dY = d total / d hout by autograd, every per-sample term, the
64-sample block sums and the per-segment records, with means taken as sum / n_global as the kernels do.  eps_clip and the coefficients are
the float32 values widened to double.

Bounds.  Two kinds, as in tests/optim_inputs.py:
  sums      a dot product or a fixed-order sum against the float64 sum,
                |got - ref| <= (d + 2) * 2^-24 * sum|terms| + 2^-24 * |ref|
            where d is the longest chain of additions in the kernel's documented order (stated next to each use):
              a logit (heads_fwd_kernel, heads_sample_kernel)   d = H       (64 steps of 4 products each for H = 256; H bounds every path)
              dfeat (heads_bwd_kernel)                          d = O       (one fmaf chain in output order)
              gW, gb (heads_bwd_kernel + reduce_slabs_kernel)   d = rows of a chunk + ceil(grid / 32) + 32
              a block partial of the loss                       d = 6       (wave_sum: six shuffle steps)
              a segment mean of the loss                        d = 6 + ceil(blocks / 8) + 8   (loss_finalize_body: 8 row groups, then the groups)
  measured  the transcendental per-sample quantities (log-probabilities, the logsumexp value, the entropy, dY rows) have no derivable
            bound: relative L2 over the rows that are not excluded <= 8 x the error of torch's own float32 evaluation of the same function
            on the same inputs against torch's float64 (the margin of the Adam tests).  For fewer than 256 rows torch's error is measured
            on the 1088-row inputs of the same distribution (a few numbers do not estimate an error).
A block partial or a segment mean is a fixed-order sum OF transcendental terms, so both parts apply: the additions get the derived bound
and each of the m terms its measured allowance, 8 x the root-mean-square error rms_q of torch's float32 terms of that kind,
                |got - ref| <= (d + 2) * 2^-24 * sum|terms| + 2 * 2^-24 * |ref| + 8 m rms_q.
(An absolute allowance per term, not one relative to the term: (v - ret)^2 and ratio * adv carry the cancellation error of v, old_v and the
log-probabilities they are made of, which does not shrink with the term -- a one-sample block holding a small term showed that.  A
dropped or doubled term moves a sum by the term itself, about 0.5: four orders of magnitude more.)
The derived records (marg, x_ent, total) carry the means' bounds through their formulas (record_bounds).

Decision margins.  A per-sample comparison leaves out the samples whose float64 decision could flip in float32: |ratio - (1 +- eps)|,
||v - old_v| - eps| or (clipped values) |vs1 - vs2| below 1e-4; sampler rows whose u is within 1e-5 of a float64 CDF edge.  Each exclusion
is capped at 1 % of a case's rows.  Exact ties stay in: v == old_v, and any ratio inside the clip (surr1 == surr2 bit for bit)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import optim_inputs as OI

U = OI.U
MARGIN, U_MARGIN, CAP = 1e-4, 1e-5, 0.01
HP = dict(eps_clip=0.2, value_coef=0.5, entropy_coef=0.01, x_entropy_coef=0.0, entropy_multiplier=0.75)


def hp64(hp):
    return {k: float(np.float32(v)) for k, v in hp.items()}


def rel_l2(a, ref):
    return OI.rel_l2(a, ref)


class Sum:
    """A sum's float64 value, sum|terms| per element and the chain length d (optim_inputs.Reduced's fields) + the terms' own allowance
    (8 m rms_q per element, or None for exact terms)."""
    def __init__(self, want, sum_abs, depth, terms=None):
        self.want, self.sum_abs, self.depth, self.terms = np.asarray(want, np.float64), np.asarray(sum_abs, np.float64), depth, terms

    def bound(self):
        if self.terms is None:
            return (self.depth + 2) * U * self.sum_abs + U * np.abs(self.want)
        return (self.depth + 2) * U * self.sum_abs + 2 * U * np.abs(self.want) + self.terms


def check_sum(got, r, what=""):
    """-> the largest error / bound ratio"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == r.want.shape, (what, got.dtype, got.shape, r.want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err, b = np.abs(got.astype(np.float64) - r.want), r.bound()
    k = int(np.argmax(err - b))
    assert err.flat[k] <= b.flat[k], f"{what}: element {k} is {err.flat[k]:.3e} from the float64 value, bound {b.flat[k]:.3e}"
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(b > 0, err / b, 0.0)
    return float(q.max()) if q.size else 0.0


def check_measured(got, ref, terr, keep=None, what=""):
    """Relative L2 of got against ref over the rows `keep` <= 8 x terr (torch's float32 error) -> (error, largest per-row error)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if keep is not None:
        got, ref = got[keep], ref[keep]
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = rel_l2(got, ref)
    row = np.abs(got - ref).reshape(got.shape[0], -1).max(axis=1) if got.size else np.zeros(1)
    assert err <= 8 * terr, f"{what}: relative L2 error {err:.3e} > 8 x torch's float32 error {terr:.3e}; worst row {int(row.argmax())}: {row.max():.3e}"
    return err, float(row.max())


def check_cap(excluded, what=""):
    share = float(np.mean(excluded)) if excluded.size else 0.0
    assert share <= CAP, f"{what}: {share:.2%} of the rows are excluded, the cap is {CAP:.0%}"
    return share


# ------------------------------------------------------------------------------------------------ heads forward / backward
FWD_O = (2, 3, 16)
FWD_N = (1, 15, 16, 17, 1024, 1039)
BWD_HO = ((256, 16), (256, 2), (64, 3), (30, 4), (1, 2))
BWD_N = (1, 7, 8, 9, 16, 17, 100, 8193, 8704)


def heads_case(n, H, O, seed=0):
    """feat (post-ReLU features: a quarter exact zeros, some of them negative zeros, and a few negative values for the mask), Wh, bh, dY,
    and non-zero starting gradients"""
    rng = np.random.default_rng([31, n, H, O, seed])
    feat = np.abs(rng.standard_normal((n, H))).astype(np.float32)
    r = rng.random((n, H))
    feat[r < 0.25] = 0.0
    feat[r < 0.08] = -0.0
    feat[(r > 0.25) & (r < 0.30)] *= -1.0
    Wh = (rng.standard_normal((O, H)) / math.sqrt(H)).astype(np.float32)
    bh = (0.1 * rng.standard_normal(O)).astype(np.float32)
    dY = (rng.standard_normal((n, O)) / n).astype(np.float32)
    return dict(feat=feat, Wh=Wh, bh=bh, dY=dY, gW0=(0.1 * rng.standard_normal((O, H))).astype(np.float32), gb0=(0.1 * rng.standard_normal(O)).astype(np.float32))


def heads_fwd_reference(feat, Wh, bh):
    """hout = feat Wh^T + bh; d = H"""
    f, w, b = (np.asarray(a, np.float64) for a in (feat, Wh, bh))
    return Sum(f @ w.T + b, np.abs(f) @ np.abs(w).T + np.abs(b), f.shape[1])


def heads_bwd_grid(n):
    return min(512, -(-n // 16))


def heads_bwd_reference(dY, feat, Wh, relu_mask, gW0, gb0):
    """-> (dfeat, gW, gb) as Sum.  dfeat: d = O.  gW / gb: a thread's fmaf chain over its chunk's rows, then the slab sum over the grid:
    d = ceil(n / grid) + ceil(grid / 32) + 32"""
    y, f, w = (np.asarray(a, np.float64) for a in (dY, feat, Wh))
    n, O = y.shape
    mask = (np.asarray(feat) > 0) if relu_mask else np.ones(f.shape, bool)
    grid = heads_bwd_grid(n)
    d = -(-n // grid) + OI.slab_depth(grid)
    g0, b0 = np.asarray(gW0, np.float64), np.asarray(gb0, np.float64)
    return (Sum(np.where(mask, y @ w, 0.0), np.where(mask, np.abs(y) @ np.abs(w), 0.0), O),
            Sum(g0 + y.T @ f, np.abs(g0) + np.abs(y).T @ np.abs(f), d), Sum(b0 + y.sum(0), np.abs(b0) + np.abs(y).sum(0), d))


# ------------------------------------------------------------------------------------------------ samplers
SAMPLE_A = (1, 2, 3, 15, 16)
SAMPLE_H = (256, 64, 30, 260, 512, 515)
SAMPLE_N = (1, 15, 16, 17, 20, 256)
SPREADS = (1.0, 4.0, 15.0)


def sample_case(n, H, A, spread, seed=0):
    """feat, Wh (A + 1, H) scaled to logits of the given spread, bh, u with the planted rows u = 0 (first) and u = 1 - 2^-24 (last).
    The planted rows' features are zeros (a row of dead ReLUs): their logits are bh, every probability is far above the edge margin and
    the rows stay in the comparison whatever the spread.  Below 256 rows one excluded row would be past the 1 % cap, so a uniform that
    falls within ten margins of a float64 CDF edge is drawn again (such a row would be left out of the comparison anyway)."""
    rng = np.random.default_rng([37, n, H, A, int(spread * 8), seed])
    feat = np.maximum(rng.standard_normal((n, H)), 0.0).astype(np.float32)
    feat[0] = 0.0; feat[-1] = 0.0
    Wh = (rng.standard_normal((A + 1, H)) * (spread / math.sqrt(0.34 * H))).astype(np.float32)
    bh = (0.3 * rng.standard_normal(A + 1)).astype(np.float32)
    u = rng.random(n).astype(np.float32)
    u[u >= 1.0] = np.float32(1 - 2.0 ** -24)
    if n < 256 and A > 1:
        z = feat.astype(np.float64) @ Wh[:A].astype(np.float64).T + bh[:A].astype(np.float64)
        p = np.exp(z - z.max(axis=1, keepdims=True))
        cdf = np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1)[:, :A - 1]
        for _ in range(64):
            near = (np.abs(cdf - u[:, None].astype(np.float64)) < 10 * U_MARGIN).any(axis=1)
            if not near.any():
                break
            u[near] = rng.random(int(near.sum())).astype(np.float32)
    u[0] = 0.0
    if n > 1:
        u[-1] = np.float32(1 - 2.0 ** -24)
    return dict(feat=feat, Wh=Wh, bh=bh, u=u)


def policy_terms(hout, lse):
    """(lp: the twice-normalised log-probabilities, value) of head rows hout (n, A + 1) in hout's dtype (heads of the oracle / lse_inputs)"""
    A = hout.shape[1] - 1
    z = hout[:, :A]
    lp = F.log_softmax(z, dim=1)
    lp = lp - lp.logsumexp(dim=-1, keepdim=True)
    return lp, (z.logsumexp(-1) if lse else hout[:, A])


def sample_reference(feat, Wh, bh, u, lse, dtype=torch.float64, off_by_one=False):
    """The heads + sample_actions of the oracle from the features, in dtype -> dict(hout (Sum for float64), lp, value, act, logp, edge: the
    rows whose u lies within U_MARGIN of a CDF edge that separates two actions).  off_by_one builds a WRONG act for the checker's test."""
    f, w, b = (torch.as_tensor(np.asarray(a)).to(dtype) for a in (feat, Wh, bh))
    hout = F.linear(f, w, b)
    lp, value = policy_terms(hout, lse)
    A = lp.shape[1]
    cdf = torch.cumsum(torch.exp(lp), dim=1)
    uu = torch.as_tensor(np.asarray(u)).to(dtype).reshape(-1, 1)
    act = (cdf <= uu).sum(dim=1).clamp(max=A - 1)
    edge = ((cdf[:, :A - 1] - uu).abs() < U_MARGIN).any(dim=1).numpy() if A > 1 else np.zeros(f.shape[0], bool)
    act = act.numpy()
    if off_by_one:
        k = int(np.flatnonzero(~edge)[0])
        act = act.copy(); act[k] = (act[k] + 1) % max(A, 2)
    logp = lp.gather(1, torch.as_tensor(act).clamp(max=A - 1).reshape(-1, 1)).reshape(-1)
    r = heads_fwd_reference(feat, Wh, bh) if dtype == torch.float64 else None
    return dict(hout=r, hout_t=hout.numpy(), lp=lp.numpy(), value=value.numpy(), act=act, logp=logp.numpy(), edge=edge)


def check_actions(got, ref, edge, A, what=""):
    got = np.asarray(got)
    assert ((got >= 0) & (got < A)).all(), f"{what}: an action outside [0, {A})"
    bad = np.flatnonzero((got != ref) & ~edge)
    assert bad.size == 0, f"{what}: {bad.size} actions differ from the float64 walk away from every CDF edge, first at row {bad[0]}: {got[bad[0]]} vs {ref[bad[0]]}"


# ------------------------------------------------------------------------------------------------ PPO loss
LOSS_A = (1, 2, 15, 16)
LOSS_N = (1, 63, 64, 65, 1088)
SEG_N = (0, 1, 63, 64, 65, 130, 0)
REGIMES = ("ratio<,adv>0", "ratio<,adv<0", "ratio in,adv>0", "ratio in,adv<0", "ratio>,adv>0", "ratio>,adv<0", "v in", "v out,vs1>vs2", "v out,vs2>vs1")
POOL_N = 1088          # the rows torch's float32 error is measured on when a case has fewer than 256


def logits_case(rng, n, A):
    """logits with a spread of about 3 and, from 16 rows on, a block of n / 8 rows with gaps up to 60 (no larger: past 103 a probability
    underflows in float32 and q log q is NaN in the reference project's arithmetic too)"""
    z = 1.5 * rng.standard_normal((n, A))
    if n >= 16:
        lo = n // 2
        z[lo:lo + n // 8] = rng.uniform(-30.0, 30.0, (n // 8, A))
    return z


def loss_case(n, A, lse, seed=0):
    """hout (n, A + 1) and the per-sample arrays of n + 37 rows behind idx (a permutation's first n entries, two of them repeated, from 8 rows on).  Sample s
    is built for ratio regime s % 3 (below / inside / above the clip), advantage sign (s // 3) % 2 and value regime (s // 6) % 3 (delta
    inside the clip / outside with vs1 larger / outside with vs2 larger), around the float64 log-prob and value of its own row; every 18th
    inside-the-clip row has old_v == v exactly (value head only).  Rows that idx never reaches hold other random values."""
    rng = np.random.default_rng([41, n, A, int(lse), seed])
    rows, eps = n + 37, float(np.float32(HP["eps_clip"]))
    hout = np.concatenate([logits_case(rng, n, A), rng.standard_normal((n, 1))], axis=1).astype(np.float32)
    idx = rng.permutation(rows)[:n].astype(np.int32)
    if n >= 8:          # (the repeated samples repeat the head row too: the stored values of a row are built around one head row)
        idx[3], idx[n - 1] = idx[1], idx[5]
        hout[3], hout[n - 1] = hout[1], hout[5]
    act = rng.integers(0, A, rows).astype(np.int32)
    old_logp, old_v, ret = (rng.standard_normal(rows).astype(np.float32) for _ in range(3))
    adv = (rng.uniform(0.3, 2.0, rows) * rng.choice((-1.0, 1.0), rows)).astype(np.float32)
    with torch.no_grad():
        lp, v = (t.numpy() for t in policy_terms(torch.as_tensor(hout).double(), lse))
    seen = set()
    for s in range(n):
        g = int(idx[s])
        if g in seen:
            continue
        seen.add(g)
        rr, sign, vr = s % 3, (1.0 if (s // 3) % 2 == 0 else -1.0), (s // 6) % 3
        target = (rng.uniform(0.5, 0.75), rng.uniform(0.85, 1.15), rng.uniform(1.3, 1.8))[rr]
        old_logp[g] = lp[s, act[g]] - math.log(target)
        adv[g] = sign * rng.uniform(0.3, 2.0)
        sd = rng.choice((-1.0, 1.0))
        if vr == 0:
            delta = sd * rng.uniform(0.0, 0.15)
            if not lse and s % 18 == 0:
                delta = 0.0
            old_v[g] = np.float32(v[s] - delta) if delta else hout[s, A]
            ret[g] = v[s] + rng.standard_normal()
        else:
            delta = sd * rng.uniform(0.3, 1.0)
            old_v[g] = v[s] - delta
            vclip = float(old_v[g]) + sd * eps
            ret[g] = (vclip - sd * rng.uniform(0.1, 1.0)) if vr == 1 else (v[s] + sd * rng.uniform(0.1, 1.0))
    return dict(hout=hout, idx=idx, act=act, old_logp=old_logp, old_value=old_v, ret=ret, adv=adv, n=n, A=A, lse=bool(lse))


def loss_reference(c, hp, n_global=None, seg_n=None, dtype=torch.float64, defect=None):
    """ppo_loss of the oracle per sample and per segment, means as sum / n_global, dY = d (sum of the segments' totals) / d hout by autograd.
    defect builds a WRONG gradient for the checkers' test: "clip_grad" passes the clip's gradient outside the range, "vswap" takes the
    value gradient from the smaller of vs1 / vs2.
    -> dict(dY, terms: pi / vm / H (n,) and p (n, A), ratio, v, old_v, vs1, vs2, clipped, records: per segment dict or None if empty)"""
    h = hp64(hp)
    eps, n, A, lse = h["eps_clip"], c["n"], c["A"], c["lse"]
    n_global = n if n_global is None else n_global
    hout = torch.as_tensor(c["hout"]).to(dtype).clone().requires_grad_(True)
    g = torch.as_tensor(c["idx"]).long()
    to = lambda k: torch.as_tensor(c[k]).to(dtype)[g]
    act, old_logp, old_v, ret, adv = torch.as_tensor(c["act"]).long()[g], to("old_logp"), to("old_value"), to("ret"), to("adv")
    lp, v = policy_terms(hout, lse)
    logp = lp.gather(1, act.reshape(-1, 1)).reshape(-1)
    ratio = torch.exp(logp - old_logp)
    surr1 = ratio * adv
    cl = torch.clamp(ratio, 1.0 - eps, 1.0 + eps)
    if defect == "clip_grad":
        cl = ratio + (cl - ratio).detach()
    surr2 = cl * adv
    pi_t = torch.min(surr1, surr2)
    clipped = old_v + (v - old_v).clamp(-eps, eps)
    vs1, vs2 = (v - ret).pow(2), (clipped - ret).pow(2)
    vm_t = torch.max(vs1, vs2)
    if defect == "vswap":
        other = torch.min(vs1, vs2)
        vm_t = other + (vm_t - other).detach()
    prob = torch.softmax(lp, dim=-1)
    H_t = -(prob * lp).sum(-1)
    seg = [n] if seg_n is None else list(seg_n)
    assert sum(seg) == n
    records, total_all, s0 = [], 0.0, 0
    for k in seg:
        sl = slice(s0, s0 + k); s0 += k
        if k == 0:
            records.append(None)
            continue
        pi_loss, value_loss, ent = -pi_t[sl].sum() / n_global, 0.5 * vm_t[sl].sum() / n_global, H_t[sl].sum() / n_global
        q = prob[sl].sum(0) / n_global
        marg = -(q * torch.log(q)).sum()
        x_ent = marg - ent
        total = pi_loss + h["value_coef"] * value_loss - h["entropy_coef"] * ent * h["entropy_multiplier"] - h["x_entropy_coef"] * x_ent
        total_all = total_all + total
        records.append(dict(pi_loss=pi_loss, value_loss=value_loss, entropy=ent, x_ent=x_ent, total=total, marg=marg, q=q))
    total_all.backward()
    d = lambda t: t.detach().numpy()
    return dict(dY=hout.grad.numpy(), pi=d(pi_t), vm=d(vm_t), H=d(H_t), p=d(prob), ratio=d(ratio), v=d(v), old_v=d(old_v), vs1=d(vs1), vs2=d(vs2),
                adv=d(adv), logp=d(logp), seg=seg, n_global=n_global,
                records=[None if r is None else {k: d(x) for k, x in r.items()} for r in records])


def loss_regimes(r, hp):
    """(9, n) bool: which of REGIMES each sample is in (float64 decisions)"""
    eps = hp64(hp)["eps_clip"]
    lo, hi, pos = r["ratio"] < 1 - eps, r["ratio"] > 1 + eps, r["adv"] > 0
    inside = np.abs(r["v"] - r["old_v"]) <= eps
    return np.stack([lo & pos, lo & ~pos, ~lo & ~hi & pos, ~lo & ~hi & ~pos, hi & pos, hi & ~pos, inside, ~inside & (r["vs1"] > r["vs2"]), ~inside & (r["vs2"] > r["vs1"])])


def loss_excluded(r, hp, margin=MARGIN):
    """rows whose float64 decision is within `margin` of flipping"""
    eps = hp64(hp)["eps_clip"]
    dv = np.abs(r["v"] - r["old_v"])
    near_ratio = (np.abs(r["ratio"] - (1 - eps)) < margin) | (np.abs(r["ratio"] - (1 + eps)) < margin)
    return near_ratio | (np.abs(dv - eps) < margin) | ((dv > eps) & (np.abs(r["vs1"] - r["vs2"]) < margin))


def term_errors(r32, r64):
    """rms_q: root-mean-square error of torch's float32 per-sample terms against float64, per kind"""
    return {k: float(np.sqrt(np.mean((r32[k].astype(np.float64) - r64[k]) ** 2))) for k in ("pi", "vm", "H", "p")}


def block_partials(r, A, eps_q):
    """[(row of the partial array, column, Sum)] is folded into three arrays: -> dict(pi, vm, H: Sum (blocks,), p: Sum (blocks, A)); blocks of
    64 samples per segment, no block straddling two segments.  d = 6 (wave_sum)"""
    out = {k: ([], [], []) for k in ("pi", "vm", "H", "p")}
    s0 = 0
    for k in r["seg"]:
        for b0 in range(s0, s0 + k, 64):
            sl = slice(b0, min(b0 + 64, s0 + k))
            for q in out:
                out[q][0].append(r[q][sl].sum(0)); out[q][1].append(np.abs(r[q][sl]).sum(0))
                out[q][2].append(np.full(np.shape(out[q][0][-1]), 8.0 * (sl.stop - sl.start) * eps_q[q]))
        s0 += k
    return {q: Sum(np.array(w), np.array(a), 6, np.array(t)) for q, (w, a, t) in out.items()}


def record_bounds(r, k, A, hp, eps_q):
    """Segment k's record as {name: (want, bound)}.  The means: d = 6 + ceil(blocks / 8) + 8, then one multiplication by 1 / n_global (the
    second 2^-24 |ref|).  marg = -sum q log q: each q_j's bound through |log q_j| + 1, logf to 2 ulp, the product, and A additions.
    x_ent = marg - ent and total = the weighted sum: the parts' bounds with their coefficients + one rounding per operation."""
    h, rec = hp64(hp), r["records"][k]
    s0 = sum(r["seg"][:k]); sl = slice(s0, s0 + r["seg"][k])
    d = 6 + -(-(-(-r["seg"][k] // 64)) // 8) + 8
    ng = r["n_global"]
    out = {}
    for name, q, scale in (("pi_loss", "pi", 1.0), ("value_loss", "vm", 0.5), ("entropy", "H", 1.0), ("q", "p", 1.0)):
        s = Sum(rec[name], scale * np.abs(r[q][sl]).sum(0) / ng, d, scale * 8.0 * r["seg"][k] * eps_q[q] / ng)
        out[name] = (s.want, s.bound())
    qv, bq = out["q"]
    qlq = np.abs(qv * np.log(qv))
    b_marg = float(((np.abs(np.log(qv)) + 1) * bq).sum() + (4 + A) * U * qlq.sum())
    out["marg"] = (rec["marg"], b_marg)
    b_x = b_marg + float(out["entropy"][1]) + U * (abs(float(rec["marg"])) + abs(float(rec["entropy"])))
    out["x_ent"] = (rec["x_ent"], b_x)
    parts = (abs(float(rec["pi_loss"])), h["value_coef"] * abs(float(rec["value_loss"])), h["entropy_coef"] * h["entropy_multiplier"] * abs(float(rec["entropy"])),
             abs(h["x_entropy_coef"] * float(rec["x_ent"])))
    b_t = (float(out["pi_loss"][1]) + h["value_coef"] * float(out["value_loss"][1]) + h["entropy_coef"] * h["entropy_multiplier"] * float(out["entropy"][1])
           + abs(h["x_entropy_coef"]) * b_x + 6 * U * sum(parts))
    out["total"] = (rec["total"], b_t)
    return out


def check_record(stats_row, log_row, r, k, A, hp, eps_q, what=""):
    """the finalised stats (0..6, 8..8+A) and the log record of segment k against record_bounds -> the largest error / bound ratio"""
    b = record_bounds(r, k, A, hp, eps_q)
    worst = 0.0
    for j, name in ((0, "pi_loss"), (1, "value_loss"), (2, "entropy"), (3, "x_ent"), (4, "total"), (6, "marg")):
        want, bound = float(b[name][0]), float(b[name][1])
        for src, row in (("stats", stats_row), ("log", log_row)):
            err = abs(float(row[j]) - want)
            assert np.isfinite(row[j]) and err <= bound, f"{what} segment {k} {src} {name}: {row[j]!r} vs {want!r}: error {err:.3e}, bound {bound:.3e}"
            worst = max(worst, err / bound if bound > 0 else 0.0)
    assert stats_row[5] == 0 and log_row[5] == 0 and log_row[7] == 0, f"{what} segment {k}: fs / pad are not zero"
    want, bound = b["q"]
    err = np.abs(stats_row[8:8 + A].astype(np.float64) - want)
    assert (err <= bound).all(), f"{what} segment {k} q: error {err.max():.3e}, bound {bound[np.argmax(err - bound)]:.3e}"
    return max(worst, float((err / bound).max()))
