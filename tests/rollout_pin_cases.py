"""Cases and hashing for tests/test_gpu_rollout_pins.py: SHA-256 of what whole small rollouts leave behind.

Every case builds a fresh Engine, fills the parameters from numpy.random.default_rng with a fixed seed and runs a whole rollout through
one family of entry points (csrc/rollout.hip): serial steps (mi_policy_step, mi_rollout_step), env groups (mi_rollout_groups / _submit /
_wait), the staged entries (mi_predict_staged + mi_commit_staged, mi_predict_greedy, mi_forward, mi_forward_rec) and the recurrent ones
(mi_set_gru, mi_rec_state, mi_rec_begin, mi_get_hidden_ring, mi_get_hidden).  Hashed: the act / logp / value / rew / done rings, the
observation ring, every array an entry returns (but the action / log-prob outputs of the bootstrap step t == T, which the entries leave
unwritten), and the hidden ring and final hidden state of the GRU cases.  Each of these is a pure function of its inputs: the Philox
counters are t * E + e whatever the grouping, groups own disjoint rows, and the one atomic elects the workgroup that publishes the
ticket.  scratch/gen_rollout_pins.py records the hashes and refuses a case whose two runs in two fresh engines differ.

Shapes: IMPALA contexts T = 3, E = 8, 15 actions, max_batch 12; MLP contexts T = 4, E = 8, obs_dim 4, depth 2, width 64, out_dim 64,
max_batch 32; GRU width 64.  The rew / done handed over at step t and the caller uniforms come from fixed streams and do not depend on
the actions, so the order in which groups are submitted and waited for is free: the group cases run the collector's pipelined schedule
(wait group g's step t, submit its step t + 1) with a submit order and a wait order that differ and change from step to step."""
import hashlib
import json
import os

import numpy as np

PIN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pins", "rollout_sha256.json")
A = 15

# name -> (kind, spec).  arch "mlp" | "fp32" | "bf16" (the last two IMPALA); flags: mi_debug_flags (bit 0: no fused rollout tail, bit 2:
# frames always by DMA); frames "pinned" (mi_host_alloc memory: the pull path) | "pageable"; G: a group count, or the counts of several
# rollouts in a row on one engine
CASES = {
    "policy-step-mlp-u": ("policy_step", dict(arch="mlp", u=True)),
    "policy-step-mlp": ("policy_step", dict(arch="mlp", u=False)),
    "policy-step-fp32-u": ("policy_step", dict(arch="fp32", u=True)),
    "policy-step-bf16-u": ("policy_step", dict(arch="bf16", u=True)),
    "policy-step-bf16": ("policy_step", dict(arch="bf16", u=False)),
    "rollout-step-mlp": ("rollout_step", dict(arch="mlp")),
    "rollout-step-fp32": ("rollout_step", dict(arch="fp32")),
    "rollout-step-bf16": ("rollout_step", dict(arch="bf16")),
    "rollout-step-bf16-notail": ("rollout_step", dict(arch="bf16", flags=1)),
    "groups-bf16-G1-pinned": ("groups", dict(arch="bf16", G=[1], frames="pinned")),
    "groups-bf16-G1-pageable": ("groups", dict(arch="bf16", G=[1], frames="pageable")),
    "groups-bf16-G2-pinned": ("groups", dict(arch="bf16", G=[2], frames="pinned")),
    "groups-bf16-G2-pageable": ("groups", dict(arch="bf16", G=[2], frames="pageable")),
    "groups-bf16-G2-pinned-dma": ("groups", dict(arch="bf16", G=[2], frames="pinned", flags=4)),
    "groups-bf16-G4-pinned": ("groups", dict(arch="bf16", G=[4], frames="pinned")),
    "groups-bf16-G4-pageable": ("groups", dict(arch="bf16", G=[4], frames="pageable")),
    "groups-bf16-G4-notail": ("groups", dict(arch="bf16", G=[4], frames="pinned", flags=1)),
    "groups-mlp-G2-pinned": ("groups", dict(arch="mlp", G=[2], frames="pinned")),
    "groups-mlp-G2-pageable": ("groups", dict(arch="mlp", G=[2], frames="pageable")),
    "groups-fp32-G2-pinned": ("groups", dict(arch="fp32", G=[2], frames="pinned")),
    "groups-fp32-G2-pageable": ("groups", dict(arch="fp32", G=[2], frames="pageable")),
    "groups-bf16-G4-2-4": ("groups", dict(arch="bf16", G=[4, 2, 4], frames="pinned")),
    "staged-mlp": ("staged", dict(arch="mlp")),
    "staged-fp32": ("staged", dict(arch="fp32")),
    "staged-bf16": ("staged", dict(arch="bf16")),
    "forward-rec-mlp": ("forward_rec", dict(arch="mlp")),
    "forward-rec-bf16": ("forward_rec", dict(arch="bf16")),
    "rec-serial-mlp": ("rollout_step", dict(arch="mlp", gru=True)),
    "rec-serial-bf16": ("rollout_step", dict(arch="bf16", gru=True)),
    "rec-groups-mlp-G2": ("groups", dict(arch="mlp", G=[2, 2], frames="pinned", gru=True)),
    "rec-groups-bf16-G2": ("groups", dict(arch="bf16", G=[2, 2], frames="pinned", gru=True)),
}
KINDS = ("policy_step", "rollout_step", "groups", "staged", "forward_rec")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def _engine(arch, gru):
    from mi355 import layout
    from mi355.engine import Engine
    if arch == "mlp":
        eng = Engine("mlp", 4, 8, A, 32, obs_dim=4, mlp_depth=2, mlp_width=64, out_dim=64)
        shapes = layout.mlp_param_shapes(A, 4, 2, 64, 64)
    else:
        H = 64 if gru else 256
        eng = Engine("impala", 3, 8, A, 12, out_dim=H, precision=arch)
        shapes = layout.impala_param_shapes(A, output_dim=H)
    rng = np.random.default_rng(101)
    params = {k: (rng.standard_normal(s) / np.sqrt(np.prod(s[1:])) if k.endswith("weight") else 0.05 * rng.standard_normal(s)) for k, s in shapes.items()}
    eng.set_params(layout.flatten(shapes, params))
    return eng


def _obs_shape(eng):
    return (eng.obs_dim,) if eng.obs_dim else (64, 64, 3)


def _fill_obs(eng, rng, out):
    """out[...] = observations from rng, of the context's kind (fp32 rows or uint8 frames)"""
    if eng.obs_dim:
        out[...] = rng.standard_normal(out.shape).astype(np.float32)
    else:
        out[...] = rng.integers(0, 256, size=out.shape, dtype=np.uint8)
    return out


def _rings(eng, tag=""):
    from mi355 import engine as M
    out = {tag + "obs": sha(*[eng.get_obs(t) for t in range(eng.T + 1)])}
    for k, f in (("act", M.F_ACT), ("logp", M.F_LOGP), ("value", M.F_VALUE), ("rew", M.F_REW), ("done", M.F_DONE)):
        out[tag + k] = sha(eng.read_field(f))
    return out


def _step_sha(t, T, act, logp, val):
    """what one step handed back: the bootstrap step writes the values only"""
    return sha(val) if t == T else sha(act, logp, val)


def _carried_in(eng, rng):
    hid = (0.6 * np.tanh(rng.standard_normal((eng.E, eng.H)))).astype(np.float32)
    done = (np.arange(eng.E) % 3 == 1).astype(np.float32)          # some rows start an episode at t = 0: their state is masked
    return hid, done


def _set_gru(eng, rng):
    eng.set_gru(*[(rng.standard_normal(s) / np.sqrt(eng.H)).astype(np.float32) for s in eng.gru_shapes()])


def _grouped_rollout(eng, G, frames, rew, done, u, seed):
    """One pipelined rollout over G groups -> [sha of what every wait returned, in (t, g) order]"""
    T, E = eng.T, eng.E
    ng = E // G
    rows = lambda g: slice(g * ng, (g + 1) * ng)

    def submit(t, g):
        eng.rollout_submit(t, g, frames[t, rows(g)], None if t == 0 else rew[t - 1, rows(g)], None if t == 0 else done[t - 1, rows(g)],
                           seed=seed, u=u[t, rows(g)] if t % 2 else None)

    got = {}
    for g in np.random.default_rng(7).permutation(G):
        submit(0, int(g))
    for t in range(T + 1):
        order = np.random.default_rng(70 + t).permutation(G)
        for g in (order[::-1] if t % 2 else np.roll(order, 1)):
            g = int(g)
            got[t, g] = _step_sha(t, T, *eng.rollout_wait(g))
            if t < T:
                submit(t + 1, g)
    return [got[k] for k in sorted(got)]


def run_case(name):
    """{what: sha256 of its float32 bytes} of one case, in a fresh Engine."""
    kind, s = CASES[name]
    rng = np.random.default_rng(404)
    gru = s.get("gru", False)
    eng = _engine(s["arch"], gru)
    T, E = eng.T, eng.E
    if s.get("flags"):
        eng.debug_flags(s["flags"])
    if gru or kind == "forward_rec":
        _set_gru(eng, rng)
    rew = rng.standard_normal((T, E)).astype(np.float32)
    done = (rng.random((T, E)) < 0.3).astype(np.float32)
    u = rng.random((T + 1, E)).astype(np.float32)
    out = {}
    if kind == "groups":
        make = eng.pinned if s["frames"] == "pinned" else np.empty
        frames = make((T + 1, E) + _obs_shape(eng), np.float32 if eng.obs_dim else np.uint8)
        for k, G in enumerate(s["G"]):
            _fill_obs(eng, rng, frames)
            eng.rollout_groups(G)
            if gru:          # first rollout: a carried-in state and done flags from the host; later ones: the device's state, done flags only
                hid, d0 = _carried_in(eng, rng)
                eng.rec_begin(hid if k == 0 else None, d0)
            out[f"steps{k}"] = "".join(_grouped_rollout(eng, G, frames, rew, done, u, seed=31 + k))
            out.update(_rings(eng, f"r{k}."))
            if gru:
                out[f"hidden_ring{k}"], out[f"hidden{k}"] = sha(eng.get_hidden_ring(0, T)), sha(eng.get_hidden())
    elif kind in ("policy_step", "rollout_step"):
        obs = _fill_obs(eng, rng, np.empty((T + 1, E) + _obs_shape(eng), np.float32 if eng.obs_dim else np.uint8))
        if gru:
            eng.rec_state(*_carried_in(eng, rng))
        steps = []
        for t in range(T + 1):
            eng.put_obs(t, obs[t])
            if kind == "policy_step":
                steps.append(_step_sha(t, T, *eng.policy_step(t, seed=11, u=u[t] if s["u"] else None)))
                if t == 1:          # no outputs wanted: the step only fills the ring (slot 1 again, same counters)
                    eng.policy_step(t, seed=11, u=u[t] if s["u"] else None, want_outputs=False)
                if t < T:
                    eng.put_step(t, rew[t], done[t])
            else:
                steps.append(_step_sha(t, T, *eng.rollout_step(t, None if t == 0 else rew[t - 1], None if t == 0 else done[t - 1], seed=13,
                                                               u=u[t] if t % 2 else None)))
        out["steps"] = "".join(steps)
        out.update(_rings(eng))
        if gru:
            out["hidden"] = sha(eng.get_hidden())
    elif kind == "staged":
        obs = _fill_obs(eng, rng, np.empty((T + 1, E) + _obs_shape(eng), np.float32 if eng.obs_dim else np.uint8))
        for t in range(T + 1):
            out[f"predict{t}"] = sha(*eng.predict_staged(obs[t], seed=17, counter=t * E, u=u[t] if t % 2 else None))
            eng.commit_staged(t)
        out.update(_rings(eng))
        out["greedy"] = sha(*eng.predict_greedy(obs[1]))
        big = _fill_obs(eng, rng, np.empty((eng.max_batch,) + _obs_shape(eng), obs.dtype))
        out["forward1"] = sha(*eng.forward(big[:1], want_feat=True))
        out["forward_max"] = sha(*eng.forward(big, want_feat=True))
    else:
        obs = _fill_obs(eng, rng, np.empty((2, E) + _obs_shape(eng), np.float32 if eng.obs_dim else np.uint8))
        eng.rec_state(*_carried_in(eng, rng))
        out["forward_rec0"] = sha(*eng.forward_rec(obs[0]))
        out["hidden0"] = sha(eng.get_hidden())
        eng.rec_state(None, None)          # the state the first call left, no row masked
        out["forward_rec1"] = sha(*eng.forward_rec(obs[1]))
        out["hidden1"] = sha(eng.get_hidden())
    eng.close()
    return out


def load_pins():
    with open(PIN_FILE) as f:
        return json.load(f)
