"""Cases and hashing for tests/test_gpu_pass_pins.py: SHA-256 of what whole update-phase passes leave behind.

Every case builds a fresh Engine, fills the parameters and the whole rollout storage from numpy.random.default_rng with fixed seeds,
runs its entry point TWICE in a row (the second pass accumulates into the same gradient buffer, takes the next index-ring slot and, at
update size, finds the slab table cached: both side-stream forks), then one optimizer_step.  Hashed: the gradients after each pass, the
loss log, the parameters after the step, and what the entry leaves beside them (GRU gradients / tensors, IPL's predictions, the value
saliency's outputs).  The library reduces in fixed orders (no floating-point atomics), so a pass is reproducible bit for bit;
scratch/gen_pass_pins.py records the hashes and refuses a case whose two runs in two fresh engines differ.

Shapes are the smallest that still reach each branch of csrc/engine.hip's update entries: IMPALA contexts T = 2, E = 4, 15 actions; MLP
contexts T = 4, E = 8, obs_dim 4, depth 2, width 64, out_dim 64, 15 actions; the side-stream threshold (n >= 1024) with repeated
indices at max_batch 1040."""
import hashlib
import json
import os

import numpy as np

PIN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pins", "update_pass_sha256.json")
A = 15
LR, CLIP = 5e-4, 0.5

# name -> (entry, spec).  arch "mlp" | "fp32" | "bf16" (the last two IMPALA); hp: keywords of Engine.hparams
CASES = {
    "minibatch-mlp-n24": ("minibatch", dict(arch="mlp", n=24)),
    "minibatch-mlp-n0": ("minibatch", dict(arch="mlp", n=0)),
    "minibatch-impala-fp32-n6-xent-fs": ("minibatch", dict(arch="fp32", n=6, hp=dict(x_entropy_coef=0.02, fs_coef=0.01))),
    "minibatch-impala-fp32-n6": ("minibatch", dict(arch="fp32", n=6)),
    "minibatch-impala-bf16-n6-fs": ("minibatch", dict(arch="bf16", n=6, hp=dict(fs_coef=0.01))),
    "minibatch-impala-bf16-n0": ("minibatch", dict(arch="bf16", n=0)),
    "multi-impala-bf16-n1024-mode0": ("minibatch_multi", dict(arch="bf16", seg=[1024], mode=0)),
    "multi-impala-bf16-n1024-mode2": ("minibatch_multi", dict(arch="bf16", seg=[1024], mode=2)),
    "multi-impala-bf16-n1029-mode0": ("minibatch_multi", dict(arch="bf16", seg=[515, 514], mode=0)),
    "multi-impala-bf16-n1029-mode2": ("minibatch_multi", dict(arch="bf16", seg=[515, 514], mode=2)),
    "finish-impala-bf16-n6-fs": ("minibatch_finish", dict(arch="bf16", n=6, hp=dict(fs_coef=0.01))),
    "finish-mlp-n24": ("minibatch_finish", dict(arch="mlp", n=24)),
    "fused-mlp-n24": ("minibatch_fused", dict(arch="mlp", seg=[24])),
    "fused-mlp-n7+17": ("minibatch_fused", dict(arch="mlp", seg=[7, 17])),
    "rec-mlp": ("minibatch_rec", dict(arch="mlp", envs=[5, 0, 2])),
    "rec-mlp-xent": ("minibatch_rec", dict(arch="mlp", envs=[5, 0, 2], hp=dict(x_entropy_coef=0.02))),
    "rec-impala-bf16": ("minibatch_rec", dict(arch="bf16", envs=[3, 0, 1])),
    "rec-impala-bf16-xent": ("minibatch_rec", dict(arch="bf16", envs=[3, 0, 1], hp=dict(x_entropy_coef=0.02))),
    "ipl-mlp-n24": ("ipl_minibatch", dict(arch="mlp", n=24)),
    "ipl-impala-bf16-n6": ("ipl_minibatch", dict(arch="bf16", n=6)),
    "saliency-impala-bf16": ("value_saliency", dict(arch="bf16", gru=False)),
    "saliency-impala-bf16-gru": ("value_saliency", dict(arch="bf16", gru=True)),
    "saliency-mlp": ("value_saliency", dict(arch="mlp", gru=False)),
    "saliency-mlp-gru": ("value_saliency", dict(arch="mlp", gru=True)),
}
ENTRIES = ("minibatch", "minibatch_multi", "minibatch_finish", "minibatch_fused", "minibatch_rec", "ipl_minibatch", "value_saliency")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def _engine(arch, max_batch, out_dim=None):
    from mi355 import layout
    from mi355.engine import Engine
    if arch == "mlp":
        eng = Engine("mlp", 4, 8, A, max_batch, obs_dim=4, mlp_depth=2, mlp_width=64, out_dim=64)
        shapes = layout.mlp_param_shapes(A, 4, 2, 64, 64)
    else:
        H = out_dim or 256
        eng = Engine("impala", 2, 4, A, max_batch, out_dim=H, precision=arch)
        shapes = layout.impala_param_shapes(A, output_dim=H)
    rng = np.random.default_rng(101)
    params = {k: (rng.standard_normal(s) / np.sqrt(np.prod(s[1:])) if k.endswith("weight") else 0.05 * rng.standard_normal(s)) for k, s in shapes.items()}
    eng.set_params(layout.flatten(shapes, params))
    return eng


def _obs(eng, rng):
    if eng.obs_dim:
        return rng.standard_normal((eng.E, eng.obs_dim)).astype(np.float32)
    return rng.integers(0, 256, size=(eng.E, 64, 64, 3), dtype=np.uint8)


def _fill_storage(eng):
    from mi355 import engine as M
    rng = np.random.default_rng(202)
    T, E = eng.T, eng.E
    for t in range(T + 1):
        eng.put_obs(t, _obs(eng, rng))
        eng.sync()
    eng.write_field(M.F_ACT, rng.integers(0, A, (T, E)).astype(np.float32))
    eng.write_field(M.F_LOGP, (np.log(1 / A) + 0.3 * rng.standard_normal((T, E))).astype(np.float32))
    eng.write_field(M.F_VALUE, (0.5 * rng.standard_normal((T + 1, E))).astype(np.float32))
    eng.write_field(M.F_REW, rng.standard_normal((T, E)).astype(np.float32))
    eng.write_field(M.F_DONE, (rng.random((T, E)) < 0.25).astype(np.float32))
    eng.write_field(M.F_ADV, rng.standard_normal((T, E)).astype(np.float32))
    eng.write_field(M.F_RET, rng.standard_normal((T, E)).astype(np.float32))


def _gru(eng, rng):
    H = eng.H
    return [(rng.standard_normal(s) / np.sqrt(H)).astype(np.float32) for s in eng.gru_shapes()]


def run_case(name):
    """{what: sha256 of its float32 bytes} of one case, in a fresh Engine."""
    entry, s = CASES[name]
    arch, rng = s["arch"], np.random.default_rng(303)
    seg = s.get("seg")
    n = sum(seg) if seg else s.get("n", 0)
    rec = entry == "minibatch_rec"
    eng = _engine(arch, 1040 if n >= 1024 else 32 if arch == "mlp" else 8, out_dim=64 if rec else None)
    TE = eng.T * eng.E
    out = {}
    if entry == "value_saliency":
        if s["gru"]:
            eng.set_gru(*_gru(eng, rng))
            eng.rec_state(0.5 * rng.standard_normal((eng.E, eng.H)), (rng.random(eng.E) < 0.5).astype(np.float32))
        for k in (1, 2):
            act, logp, val, grad = eng.value_saliency(_obs(eng, rng), seed=7, counter=k, u=rng.random(eng.E).astype(np.float32))
            out[f"act{k}"], out[f"logp{k}"], out[f"value{k}"], out[f"grad{k}"] = sha(act), sha(logp), sha(val), sha(grad)
        g = eng.get_grads()
        assert not g.any(), "value_saliency left parameter gradients behind"
        out["grads"] = sha(g)
    else:
        _fill_storage(eng)
        hp = eng.hparams(**s.get("hp", {}))
        if rec:
            eng.set_gru(*_gru(eng, rng))
            eng.gru_train(True)
            envs = np.array(s["envs"])
            h0 = (0.5 * rng.standard_normal((len(envs), eng.H))).astype(np.float32)
        if s.get("mode"):
            eng.set_multirank(s["mode"])
        if entry == "minibatch_finish":
            eng.set_multirank(1)
        ihp = eng.ipl_hparams(0.999, 1.0, 0.01, True, True, True)
        for k in (1, 2):
            idx = rng.integers(0, TE, n) if n >= 1024 else rng.permutation(TE)[:n]
            if entry == "minibatch":
                eng.minibatch(idx, max(n, 6), hp)
            elif entry == "minibatch_multi":
                eng.minibatch_multi(idx, seg, max(seg), hp)
            elif entry == "minibatch_fused":
                eng.minibatch_fused(idx, seg, max(seg), hp)
            elif entry == "minibatch_finish":
                if arch != "mlp":
                    eng.minibatch_positions(np.arange(n))
                eng.minibatch(idx, n, hp)
                eng.minibatch_finish()
            elif rec:
                eng.minibatch_rec(envs if k == 1 else envs[::-1], h0, len(envs) * eng.T, hp)
                out[f"gru_grads{k}"] = sha(*eng.get_gru_grads())
            else:
                eng.ipl_minibatch(idx, n, ihp)
                pred, rew = eng.ipl_read_pred(n)
                out[f"ipl_pred{k}"], out[f"ipl_rew{k}"] = sha(pred), sha(rew)
            out[f"grads{k}"] = sha(eng.get_grads())
        if s.get("mode") == 2:
            eng.loss_log_finalize()
        out["loss_log"] = sha(eng.loss_log())
    eng.optimizer_step(LR, CLIP, 1)
    out["params"] = sha(eng.get_params())
    if rec:
        out["gru"] = sha(*eng.get_gru())
    eng.close()
    return out


def load_pins():
    with open(PIN_FILE) as f:
        return json.load(f)
