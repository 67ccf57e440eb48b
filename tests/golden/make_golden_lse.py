#!/usr/bin/env python3
"""Generate G14 (tests/golden/g14_lse_value.npz): the reference's CategoricalPolicy(..., logsumexp_logits_is_v=True)
(common/policy.py:77-78, v = logits.logsumexp(-1)) through PPO.optimize (agents/ppo.py:96-208) and PPO.predict_w_value_saliency
(:83-94).

Runs the reference like make_golden.py (whose import recipe and helpers it reuses; that file is not changed), in the build
container only.

    python tests/golden/make_golden_lse.py

Data only.  Inputs: G4's rollout (frames / observations, rewards, dones, actions, old log-probs), read from g4_*_lossgrad.npz and NOT
stored again; T = 4, E = 8, one minibatch of 32; IMPALA with A = 15 and MLPModel(9, 4, 256, 64) with A = 2.  Parameters: G3's / G7's
(the policy initialises bit-identically from seed 6033; asserted tensor by tensor), except fc_policy.weight, multiplied by one factor per
architecture so that the 32 samples' raw logits have a standard deviation of 1 (the 0.01-gain initialisation gives a nearly uniform
softmax, under which a wrong d v / d logits would hide).  The scaled tensor is stored.  Old values: the reference's own logsumexp values of
the T + 1 steps plus default_rng(29).standard_normal * 0.25 (lse_inputs.NOISE_*), so that the value clip acts on some samples and not on
others; the generator asserts: at least 8 of the 32 samples with |v - old_v| > eps_clip, at least 8 inside, both orders of v_surr1 / v_surr2.

Per architecture, keys under '<arch>/':
  fc_policy.weight, scale, val (T+1, E), adv, ret, logits (Categorical.logits of the 32 samples), value (their logsumexp values)
  raw/, xent/   grad_clip_norm = 1e9, x_entropy_coef = 0 / 0.05: summary; the gradients handed to the optimizer step -- tensors of up to
                4608 elements whole (g/<name>), larger ones as L2 norm, sum and 16 fixed +-1 projections (norm/ sum/ sketch/<name>,
                width_inputs.sketch); none = the names whose grad is None
  step/         grad_clip_norm = 0.5, lr 5e-4, one optimizer step: norm (the pre-clip norm clip_grad_norm_ returned), all parameters
                after it (same storage rule), opt = the optimizer state_dict's structure as G11 records it
  sal           predict_w_value_saliency of the 8 observations of step 0, one call per observation (value.backward() needs one env)
"""
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))      # the repository root, for `oracle` (behind the reference on the path)
import make_golden as G  # noqa: E402  (imports the reference)
import lse_inputs as LI  # noqa: E402
import width_inputs as WI  # noqa: E402

OUT = os.path.join(HERE, "g14_lse_value.npz")
T, E = LI.T, LI.E


def build(arch, scaled_w=None):
    A = LI.ARCHS[arch]["A"]
    torch.manual_seed(6033)
    emb = G.ImpalaModel(in_channels=3) if arch == "impala" else G.MLPModel(9, 4, 256, 64)
    policy = G.CategoricalPolicy(emb, False, A, logsumexp_logits_is_v=True)
    policy.device = G.CPU
    if scaled_w is not None:
        with torch.no_grad():
            policy.fc_policy.weight.copy_(torch.from_numpy(scaled_w))
    return policy


def obs_of(arch, frames):
    f = np.asarray(frames)
    return torch.FloatTensor(G.frames_to_ref_obs(f.reshape(-1, 64, 64, 3))) if arch == "impala" else torch.from_numpy(f.reshape(-1, 9))


def put(out, prefix, tensors):
    for k, v in tensors.items():
        if v.size <= WI.SMALL:
            out[f"{prefix}/g/{k}"] = v
        else:
            out[f"{prefix}/norm/{k}"] = np.float64(np.linalg.norm(v.astype(np.float64)))
            out[f"{prefix}/sum/{k}"] = np.float64(v.astype(np.float64).sum())
            out[f"{prefix}/sketch/{k}"] = WI.sketch(v)


def one_arch(arch, out):
    c = LI.ARCHS[arch]
    A, H = c["A"], c["H"]
    g4 = LI.load(c["g4"])
    r = {k: g4["in/" + k] for k in ("frames", "act", "rew", "done", "logp")}
    base = build(arch)
    ref_p = LI.base_params(arch)
    for k, v in G.sd_numpy(base).items():
        assert np.array_equal(v, ref_p[k]), f"{arch}: {k} differs from the G3 / G7 parameters"
    with torch.no_grad():
        raw = base.fc_policy(base.embedder(obs_of(arch, r["frames"][:T])))
    scale = np.float32(1.0 / float(raw.std()))
    w = (G.sd_numpy(base)["fc_policy.weight"] * scale).astype(np.float32)
    pol = build(arch, w)
    with torch.no_grad():
        hx, m = torch.zeros((T + 1) * E, H), torch.ones((T + 1) * E)
        dist, v_all, _ = pol(obs_of(arch, r["frames"]), hx, m)
        raw = pol.fc_policy(pol.embedder(obs_of(arch, r["frames"][:T])))
    assert abs(float(raw.std()) - 1.0) < 0.05, float(raw.std())
    noise = (np.random.default_rng(LI.NOISE_SEED).standard_normal((T + 1, E)) * LI.NOISE_STD).astype(np.float32)
    r["val"] = (v_all.numpy().reshape(T + 1, E) + noise).astype(np.float32)
    out[f"{arch}/fc_policy.weight"], out[f"{arch}/scale"], out[f"{arch}/val"] = w, scale, r["val"]
    out[f"{arch}/logits"] = dist.logits.numpy()[:T * E]
    out[f"{arch}/value"] = v_all.numpy()[:T * E]

    def storage():
        st = G.Storage((3, 64, 64) if arch == "impala" else (9,), H, T, E, G.CPU)
        G.fill_storage(st, r, T, E, arch == "impala")
        st.compute_estimates(0.999, 0.95, True, True)
        return st

    # the conditions the value-clip branches need (on the CPU, before anything is written)
    st = storage()
    v, oldv, ret = v_all.numpy()[:T * E].astype(np.float64), r["val"][:T].reshape(-1).astype(np.float64), st.return_batch.numpy().reshape(-1).astype(np.float64)
    outside = np.abs(v - oldv) > 0.2
    vs1, vs2 = (v - ret) ** 2, (oldv + np.clip(v - oldv, -0.2, 0.2) - ret) ** 2
    assert outside.sum() >= 8 and (~outside).sum() >= 8, (int(outside.sum()), int((~outside).sum()))
    assert (vs1 > vs2).any() and (vs2 > vs1).any(), "both orders of v_surr1 / v_surr2"
    print(arch, "outside the clip range:", int(outside.sum()), " v_surr1 > v_surr2:", int((vs1 > vs2).sum()), " <:", int((vs2 > vs1).sum()))
    out[f"{arch}/adv"], out[f"{arch}/ret"] = st.adv_batch.numpy().copy(), st.return_batch.numpy().copy()

    names = [k for k, _ in pol.named_parameters()]
    for tag, clip, xc in (("raw", 1e9, 0.0), ("xent", 1e9, 0.05), ("step", 0.5, 0.0)):
        policy, st = build(arch, w), storage()
        hp = dict(G.BASE_HP, epoch=1, n_minibatch=1, mini_batch_size=T * E, grad_clip_norm=clip, x_entropy_coef=xc)
        cap, norms = {}, []
        orig_clip = torch.nn.utils.clip_grad_norm_
        torch.nn.utils.clip_grad_norm_ = lambda params, max_norm, *a, **k: (norms.append(float(orig_clip(params, max_norm, *a, **k))), norms[-1])[1]
        try:
            torch.manual_seed(5)
            agent, summary = G.run_optimize(policy, st, T, E, hp, cap)
        finally:
            torch.nn.utils.clip_grad_norm_ = orig_clip
        g = cap["grads"][0]
        none = [n for n in names if n not in g]
        assert none == list(LI.VALUE_KEYS), none
        if tag != "step":
            out[f"{arch}/{tag}/summary"] = np.frombuffer(json.dumps({k: float(x) for k, x in summary.items()}).encode(), np.uint8)
            out[f"{arch}/{tag}/none"] = np.frombuffer(json.dumps(none).encode(), np.uint8)
            put(out, f"{arch}/{tag}", g)
            continue
        after = cap["params"][0]
        for k in LI.VALUE_KEYS:
            assert np.array_equal(after[k], ref_p[k]), f"{k} changed"
        out[f"{arch}/step/norm"] = np.float64(norms[0])
        put(out, f"{arch}/step", after)
        buf = io.BytesIO()
        torch.save({'model_state_dict': agent.policy.state_dict(), 'optimizer_state_dict': agent.optimizer.state_dict()}, buf)
        buf.seek(0)
        ck = torch.load(buf, map_location="cpu", weights_only=True)
        desc = lambda t: [list(t.shape), str(t.dtype)]
        osd = ck["optimizer_state_dict"]
        opt = {"top_keys": list(ck.keys()), "model": [[k, *desc(t)] for k, t in ck["model_state_dict"].items()], "opt_keys": list(osd.keys()),
               "opt_state": [[int(i), [[k, *desc(t)] for k, t in s.items()], float(s["step"])] for i, s in osd["state"].items()],
               "param_groups": osd["param_groups"], "n_parameters": len(list(agent.policy.parameters()))}
        assert len(opt["opt_state"]) == opt["n_parameters"] - 2
        out[f"{arch}/step/opt"] = np.frombuffer(json.dumps(opt).encode(), np.uint8)

    # saliency: one call per observation of step 0
    policy = build(arch, w)
    agent = G.PPO(None, policy, G._NullLogger(), storage(), G.CPU, 1, n_steps=T, n_envs=E, **dict(G.BASE_HP, epoch=1, n_minibatch=1, mini_batch_size=T * E))
    obs0 = obs_of(arch, r["frames"][0]).numpy()
    sal = []
    for e in range(E):
        _, _, val, _, grad = agent.predict_w_value_saliency(obs0[e:e + 1], np.zeros((1, H), np.float32), np.zeros(1, np.float32))
        assert abs(float(val[0]) - float(v_all[e])) < 1e-5
        sal.append(grad[0])
        policy.zero_grad()
    out[f"{arch}/sal"] = np.stack(sal).astype(np.float32)


def main():
    out = {}
    for arch in ("impala", "mlp"):
        one_arch(arch, out)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 1000000


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
