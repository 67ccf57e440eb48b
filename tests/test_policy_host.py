"""CPU checks of tests/policy_inputs.py, the references and bounds behind tests/test_gpu_policy_ops.py: the float64 restatement agrees with
oracle.ppo_oracle (and the logsumexp heads of tests/lse_inputs.py) on the G4 / G14 inputs, every loss case holds its nine regimes and stays
under the exclusion caps, torch's own float32 evaluation passes every checker (the bounds are not vacuous the other way either: each
planted defect fails one)."""
import numpy as np
import pytest
import torch

import lse_inputs as LI
import policy_inputs as PI
from oracle import ppo_oracle as O

torch.set_num_threads(8)


# ------------------------------------------------------------------------------------------------ the references are the oracle's
@pytest.mark.parametrize("arch", ("impala", "mlp"))
@pytest.mark.parametrize("lse", (False, True), ids=("g4", "g14"))
def test_references_agree_with_the_oracle(arch, lse):
    c = LI.case(arch)
    A = c["A"]
    p = {k: torch.as_tensor(np.asarray(v)).double() for k, v in c["params"].items()}
    with torch.no_grad():
        feat = LI.embed(p, arch, LI.ref_obs(arch, c["frames"][:-1]).double())
    Wh = np.concatenate([c["params"]["fc_policy.weight"], c["params"]["fc_value.weight"]])
    bh = np.concatenate([c["params"]["fc_policy.bias"], c["params"]["fc_value.bias"]])
    n = feat.shape[0]
    u = np.random.default_rng(3).random(n)
    s = PI.sample_reference(feat.numpy(), Wh, bh, u, lse)
    lp_o, v_o = (LI.heads if lse else O.heads)(p, feat)
    np.testing.assert_allclose(s["lp"], lp_o.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(s["value"], v_o.numpy(), rtol=1e-13, atol=1e-13)
    act_o, logp_o = O.sample_actions(lp_o, torch.as_tensor(u))
    assert np.array_equal(s["act"], act_o.numpy()) and np.allclose(s["logp"], logp_o.numpy(), rtol=0, atol=1e-13)
    # the loss: the same head rows through oracle.ppo_loss with autograd to the head outputs
    for xc in (0.0, 0.05):
        hp = dict(PI.HP, x_entropy_coef=xc)
        case = dict(hout=s["hout_t"], idx=np.arange(n), act=c["act"].reshape(-1), old_logp=c["logp"].reshape(-1), old_value=c["val"][:-1].reshape(-1),
                    ret=c["ret"].reshape(-1), adv=c["adv"].reshape(-1), n=n, A=A, lse=lse)
        r = PI.loss_reference(case, hp)
        h = torch.as_tensor(s["hout_t"]).clone().requires_grad_(True)
        lp, v = PI.policy_terms(h, lse)
        t = lambda k: torch.as_tensor(np.asarray(case[k])).double()
        k = PI.hp64(hp)
        L = O.ppo_loss(lp, v, torch.as_tensor(case["act"]), t("old_logp"), t("old_value"), t("ret"), t("adv"), k["eps_clip"], k["value_coef"], k["entropy_coef"],
                       k["x_entropy_coef"], k["entropy_multiplier"])
        L["total"].backward()
        for name in ("pi_loss", "value_loss", "entropy", "x_ent", "total"):
            assert abs(float(L[name].detach()) - float(r["records"][0][name])) < 1e-13, name
        np.testing.assert_allclose(r["dY"], h.grad.numpy(), rtol=0, atol=1e-15)
        if lse:
            assert not r["dY"][:, A].any()


# ------------------------------------------------------------------------------------------------ regimes, caps, torch float32 within the bounds
LOSS_PARAMS = [(A, n, lse) for A in PI.LOSS_A for n in PI.LOSS_N + (sum(PI.SEG_N),) for lse in (False, True)]


@pytest.mark.parametrize("A,n,lse", LOSS_PARAMS)
def test_loss_cases_hold_their_regimes_and_caps(A, n, lse):
    c = PI.loss_case(n, A, lse)
    r = PI.loss_reference(c, PI.HP)
    assert sorted(set(c["idx"].tolist())) != sorted(c["idx"].tolist()) or n < 8          # repeated entries
    assert c["act"].size > n and c["idx"].max() >= n or n == 1
    PI.check_cap(PI.loss_excluded(r, PI.HP), f"loss A={A} n={n}")
    if n >= 63:
        share = PI.loss_regimes(r, PI.HP).mean(axis=1)
        assert (share >= 0.05).all(), dict(zip(PI.REGIMES, share))
    if n >= 16:
        z = c["hout"][:, :A].astype(np.float64)
        gap = (z.max(1) - z.min(1)).max() if A > 1 else 0.0
        assert gap <= 60.0 and (A == 1 or n < PI.POOL_N or gap > 30.0)
    if not lse and n >= 63:
        assert (r["v"] == r["old_v"]).sum() >= 2          # the planted exact ties


@pytest.mark.parametrize("A", PI.LOSS_A)
@pytest.mark.parametrize("lse", (False, True))
@pytest.mark.parametrize("xc,seg", ((0.0, None), (0.05, None), (0.0, PI.SEG_N)), ids=("xc0", "xc0.05", "segments"))
def test_torch_float32_passes_the_loss_checkers(A, lse, xc, seg):
    """torch's float32 loss is within its own 8 x bound per sample, and its block sums and records within the sum bounds -- also over the
    segment table, whose one-sample segment and one-sample last block hold a single term each (a term's error does not shrink with the
    term: the allowance per term is absolute, see policy_inputs)"""
    hp = dict(PI.HP, x_entropy_coef=xc)
    n, ng = (PI.POOL_N, None) if seg is None else (sum(seg), 200)
    c = PI.loss_case(n, A, lse)
    r64, r32 = PI.loss_reference(c, hp, ng, seg), PI.loss_reference(c, hp, ng, seg, dtype=torch.float32)
    keep = ~PI.loss_excluded(r64, hp)
    terr = PI.rel_l2(r32["dY"][keep], r64["dY"][keep])
    assert 0 < terr < 1e-4, terr
    PI.check_measured(r32["dY"], r64["dY"], terr, keep, "torch float32 dY")
    eps_q = PI.term_errors(r32, r64)
    want, got = PI.block_partials(r64, A, eps_q), PI.block_partials(r32, A, eps_q)
    assert want["pi"].want.shape[0] == sum(-(-k // 64) for k in r64["seg"])
    for q in ("pi", "vm", "H", "p"):
        PI.check_sum(got[q].want.astype(np.float32), want[q], f"torch float32 partial {q}")
    for k, rec in enumerate(r32["records"]):
        if rec is None:
            continue
        row = np.zeros(32, np.float32)
        row[:7] = [rec["pi_loss"], rec["value_loss"], rec["entropy"], rec["x_ent"], rec["total"], 0.0, rec["marg"]]
        row[8:8 + A] = rec["q"]
        PI.check_record(row, row[:8], r64, k, A, hp, eps_q, "torch float32")
        # a record that lost one sample's entropy is caught
        s0 = sum(r64["seg"][:k])
        wrong = row.copy(); wrong[2] -= np.float32(r64["H"][s0:s0 + r64["seg"][k]].max() / r64["n_global"])
        if A > 1:
            with pytest.raises(AssertionError):
                PI.check_record(wrong, wrong[:8], r64, k, A, hp, eps_q)


@pytest.mark.parametrize("A", PI.SAMPLE_A)
@pytest.mark.parametrize("spread", PI.SPREADS)
def test_sampler_exclusions_and_float32_walk(A, spread):
    """u within 1e-5 of a CDF edge: under the cap with the planted u = 0 and u = 1 - 2^-24 rows; outside it a float32 walk picks the
    float64 action"""
    for lse in (False, True):
        c = PI.sample_case(4096, 64, A, spread)
        r64, r32 = PI.sample_reference(**c, lse=lse), PI.sample_reference(**c, lse=lse, dtype=torch.float32)
        assert c["u"][0] == 0 and c["u"][-1] == np.float32(1 - 2.0 ** -24) and (c["u"] < 1).all()
        PI.check_cap(r64["edge"], f"sampler A={A} spread={spread}")
        PI.check_actions(r32["act"], r64["act"], r64["edge"], A, "float32 walk")
        PI.check_sum(r32["hout_t"], r64["hout"], "torch float32 hout")
        keep = ~r64["edge"]
        for k in ("lp", "logp") + (("value",) if lse else ()):
            PI.check_measured(r32[k], r64[k], PI.rel_l2(r32[k][keep], r64[k][keep]), keep, k)


@pytest.mark.parametrize("A", PI.SAMPLE_A)
def test_every_sampler_case_is_under_its_cap(A):
    """the GPU test's own shapes: no excluded row below 256 rows, at most 1 % at 256; the planted rows are never excluded"""
    for H in PI.SAMPLE_H:
        for i, n in enumerate(PI.SAMPLE_N):
            c = PI.sample_case(n, H, A, PI.SPREADS[(i + A + H) % 3])
            edge = PI.sample_reference(**c, lse=False)["edge"]
            PI.check_cap(edge, f"A={A} H={H} n={n}")
            assert not edge[0] and not edge[-1] and c["u"][0] == 0 and (n == 1 or c["u"][-1] == np.float32(1 - 2.0 ** -24))


# ------------------------------------------------------------------------------------------------ planted defects
def _loss_pair(A=15, lse=False, n=PI.POOL_N):
    c = PI.loss_case(n, A, lse)
    r64, r32 = PI.loss_reference(c, PI.HP), PI.loss_reference(c, PI.HP, dtype=torch.float32)
    keep = ~PI.loss_excluded(r64, PI.HP)
    return c, r64, r32, keep, PI.rel_l2(r32["dY"][keep], r64["dY"][keep])


def test_defect_swapped_logit_column_fails():
    c = PI.sample_case(20, 64, 3, 4.0)
    r = PI.sample_reference(**c, lse=False)
    got = r["hout_t"].astype(np.float32)
    PI.check_sum(got, r["hout"])
    got[:, [0, 1]] = got[:, [1, 0]]
    with pytest.raises(AssertionError, match="from the float64 value"):
        PI.check_sum(got, r["hout"])


@pytest.mark.parametrize("defect", ("clip_grad", "vswap"))
def test_defect_in_a_gradient_branch_fails(defect):
    """the clip's gradient passed outside the range; the value gradient taken from the smaller of vs1 / vs2 (tie-free rows only differ)"""
    c, r64, r32, keep, terr = _loss_pair()
    bad = PI.loss_reference(c, PI.HP, dtype=torch.float32, defect=defect)
    changed = np.abs(bad["dY"] - r32["dY"]).max(axis=1) > 1e-3 * np.abs(r32["dY"]).max(axis=1)
    inside = np.abs(r64["v"] - r64["old_v"]) <= PI.hp64(PI.HP)["eps_clip"]          # (there vs1 and vs2 differ by a rounding at most)
    assert changed.any() and (defect != "vswap" or not (changed & inside).any())
    np.testing.assert_allclose(bad["pi"], r32["pi"], rtol=1e-6); np.testing.assert_allclose(bad["vm"], r32["vm"], rtol=1e-6)          # the forward is the same
    with pytest.raises(AssertionError, match="relative L2"):
        PI.check_measured(bad["dY"], r64["dY"], terr, keep)
    # one wrong row among 1088 is enough
    one = r32["dY"].copy()
    k = int(np.flatnonzero(changed & keep)[0])
    one[k] = bad["dY"][k]
    with pytest.raises(AssertionError, match="relative L2"):
        PI.check_measured(one, r64["dY"], terr, keep)


def test_defect_row_written_to_its_neighbour_fails():
    c, r64, r32, keep, terr = _loss_pair(A=2)
    got = r32["dY"].copy()
    k = int(np.flatnonzero(keep[:-1] & keep[1:])[5])
    got[[k, k + 1]] = got[[k + 1, k]]
    with pytest.raises(AssertionError, match="relative L2"):
        PI.check_measured(got, r64["dY"], terr, keep)


def test_defect_action_off_by_one_fails():
    c = PI.sample_case(256, 30, 15, 4.0)
    r = PI.sample_reference(**c, lse=False)
    PI.check_actions(r["act"], r["act"], r["edge"], 15)
    bad = PI.sample_reference(**c, lse=False, off_by_one=True)
    with pytest.raises(AssertionError, match="away from every CDF edge"):
        PI.check_actions(bad["act"], r["act"], r["edge"], 15)
    with pytest.raises(AssertionError, match="outside"):
        PI.check_actions(np.full(256, 15), r["act"], r["edge"], 15)


def test_heads_bounds_are_met_by_float32_and_broken_by_a_dropped_row():
    """numpy's float32 products are within the sum bounds at the largest backward shape; a dropped row, a wrong mask and a result without
    the starting values are not"""
    n, H, O = 8193, 256, 16
    c = PI.heads_case(n, H, O)
    for relu_mask in (0, 1):
        df, gW, gb = PI.heads_bwd_reference(c["dY"], c["feat"], c["Wh"], relu_mask, c["gW0"], c["gb0"])
        mask = (c["feat"] > 0) if relu_mask else np.ones_like(c["feat"], bool)
        PI.check_sum(np.where(mask, c["dY"] @ c["Wh"], 0).astype(np.float32), df)
        PI.check_sum((c["gW0"] + c["dY"].T @ c["feat"]).astype(np.float32), gW); PI.check_sum((c["gb0"] + c["dY"].sum(0)).astype(np.float32), gb)
    assert (c["feat"] == 0).mean() > 0.2 and np.signbit(c["feat"][c["feat"] == 0]).any() and (c["feat"] < 0).any()
    with pytest.raises(AssertionError):
        PI.check_sum((c["dY"] @ c["Wh"]).astype(np.float32), df)                                   # the mask ignored
    with pytest.raises(AssertionError):
        PI.check_sum((c["gW0"] + c["dY"][:-1].T @ c["feat"][:-1]).astype(np.float32), gW)           # the last row dropped
    with pytest.raises(AssertionError):
        PI.check_sum((c["dY"].sum(0)).astype(np.float32), gb)                                       # the starting values dropped
    r = PI.heads_fwd_reference(c["feat"][:1039], c["Wh"], c["bh"])
    PI.check_sum((c["feat"][:1039] @ c["Wh"].T + c["bh"]).astype(np.float32), r)
    with pytest.raises(AssertionError):
        PI.check_sum((c["feat"][:1039] @ c["Wh"].T).astype(np.float32), r)                          # the bias dropped
