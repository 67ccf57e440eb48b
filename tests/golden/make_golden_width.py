#!/usr/bin/env python3
"""Generate G12 (tests/golden/g12_impala_width.npz): the reference's IMPALA embedder at output_dim != 256.

Runs the reference like make_golden.py (whose import recipe and helpers it reuses; that file is not changed) in the build
container only.  No weights are stored: the port's ImpalaModel + CategoricalPolicy initialise bit-identically for a seed, so the
tests rebuild them from SEED and check the SHA-256 of the flat parameter vector first.

    python tests/golden/make_golden_width.py

The frames are not stored either: tests/width_inputs.py rebuilds them from seeded generators, and the fixture keeps their SHA-256.
Gradient tensors of up to 4608 elements are stored whole; larger ones as their L2 norm, sum and 16 fixed +-1 projections
(width_inputs.sketch).

Contents (A = 15 actions, seed 6033):
  sha        json {"D64": .., "D128": .., "D512": .., "D128_rec": ..}: flat_sha of the policy (recurrent: with the GRU)
  keys/shapes json: state_dict keys and shapes of the D = 128 policy (non-recurrent)
  frames_sha json {"fwd": .., "rollout": .., "rec": ..}: SHA-256 of width_inputs.frames_fwd / frames_rollout / frames_rec
  fwd/*      D = 128 forward on 8 fixed frames (G3 style): feat, logits, value
  in/*, adv, ret, raw/*   D = 128, one minibatch of B = 32 through PPO.optimize (G4 style, clip 1e9): summary; raw/g/<name> for
             the small gradients, raw/norm/<name>, raw/sum/<name>, raw/sketch/<name> for the large ones
  rec/*      D = 128 recurrent prediction, three steps with carried, done-masked hidden state (G9 style)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (imports the reference)
import width_inputs as WI  # noqa: E402

SEED, A = 6033, 15
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g12_impala_width.npz")


def build(D, recurrent=False):
    torch.manual_seed(SEED)
    policy = G.CategoricalPolicy(G.ImpalaModel(in_channels=3, output_dim=D), recurrent, A)
    policy.device = G.CPU
    return policy


def main():
    out = {}
    shas = {f"D{D}": G.flat_sha(build(D)) for D in (64, 128, 512)}
    shas["D128_rec"] = G.flat_sha(build(128, True))
    out["sha"] = np.frombuffer(json.dumps(shas).encode(), np.uint8)
    sd = build(128).state_dict()
    out["keys"] = np.frombuffer(json.dumps(list(sd.keys())).encode(), np.uint8)
    out["shapes"] = np.frombuffer(json.dumps({k: list(v.shape) for k, v in sd.items()}).encode(), np.uint8)

    # forward (G3 style)
    obs_u8 = WI.frames_fwd()
    policy = build(128)
    with torch.no_grad():
        feat, _, _, _ = policy.embedder.forward_with_attn_indices(torch.FloatTensor(G.frames_to_ref_obs(obs_u8)))
        dist, value = policy.hidden_to_output(feat)
    out["fwd/feat"], out["fwd/logits"], out["fwd/value"] = feat.numpy(), dist.logits.numpy(), value.numpy()

    # one minibatch: losses + every gradient (G4 style, unclipped)
    T, E = 4, 8
    r = G.synth_rollout(np.random.default_rng(11), T, E, A, "frames")
    assert np.array_equal(r["frames"], WI.frames_rollout(T, E))
    for k, v in r.items():
        if k != "frames":
            out["in/" + k] = v
    st = G.Storage((3, 64, 64), 128, T, E, G.CPU)
    G.fill_storage(st, r, T, E, True)
    st.compute_estimates(0.999, 0.95, True, True)
    hp = dict(G.BASE_HP, epoch=1, n_minibatch=1, mini_batch_size=T * E, grad_clip_norm=1e9, x_entropy_coef=0.0)
    cap = {}
    torch.manual_seed(5)
    _, summary = G.run_optimize(build(128), st, T, E, hp, cap)
    out["raw/summary"] = np.frombuffer(json.dumps({k: float(v) for k, v in summary.items()}).encode(), np.uint8)
    for k, v in cap["grads"][0].items():
        if v.size <= WI.SMALL:
            out["raw/g/" + k] = v
        else:
            out["raw/norm/" + k] = np.float64(np.linalg.norm(v.astype(np.float64)))
            out["raw/sum/" + k] = np.float64(v.astype(np.float64).sum())
            out["raw/sketch/" + k] = WI.sketch(v)
    out["adv"], out["ret"] = st.adv_batch.numpy().copy(), st.return_batch.numpy().copy()

    # recurrent prediction (G9 style)
    policy = build(128, True)
    rng = np.random.default_rng(23)
    frames = rng.integers(0, 256, size=(3, E, 64, 64, 3), dtype=np.uint8)
    assert np.array_equal(frames, WI.frames_rec(E))
    done = np.stack([np.zeros(E), (rng.random(E) < 0.4).astype(np.float64), (rng.random(E) < 0.4).astype(np.float64)])
    out["rec/done"] = done.astype(np.float32)
    out["frames_sha"] = np.frombuffer(json.dumps({"fwd": WI.sha(obs_u8), "rollout": WI.sha(r["frames"]), "rec": WI.sha(frames)}).encode(), np.uint8)
    hx = torch.zeros(E, 128)
    with torch.no_grad():
        for t in range(3):
            dist, value, hx = policy(torch.FloatTensor(G.frames_to_ref_obs(frames[t])), hx, torch.FloatTensor(1 - done[t]))
            out[f"rec/logits{t}"], out[f"rec/value{t}"], out[f"rec/hx{t}"] = dist.logits.numpy(), value.numpy(), hx.numpy().copy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
