"""Rollout lanes (csrc/lanes.h, rollout.hip g_lanes / mi_rollout_groups; DESIGN.md section 5 "Lanes"): the env groups of every engine in the process run
on at most four shared high-priority streams.  Placement moves no kernel, no ordering edge and no buffer, so every number a pipelined
rollout returns or leaves in the ring stays BIT-equal to the serial mi_put_obs + mi_rollout_step loop -- across lane reuse within an
engine, with two engines alive, and whatever earlier engines of the process created or destroyed -- and the four lanes of an engine
run side by side in whatever hardware-queue budget the process was given.

Shapes: IMPALA bf16, A = 15, T = 3, E = 8 (two envs per group at G = 4): the logic is per stream, not per size.  The minibatch between
rollouts has n = 1024 rows, the smallest size that forks the update's side stream (backward_impala_bf16, n >= 1024), which is lane 0."""
import numpy as np
import pytest

from conftest import load_npz, npz_params

pytestmark = pytest.mark.gpu

T, E, A, NB = 3, 8, 15, 1024
FIELDS = ("act", "logp", "val", "f_act", "f_logp", "f_val", "f_rew", "f_done", "obs", "adv")


def _flat():
    from mi355 import layout
    params = dict(npz_params(load_npz("g3_impala_forward.npz")))
    params["fc_policy.weight"] = params["fc_policy.weight"] * 200.0          # peaked policies: actions differ from env to env
    return layout.flatten(layout.impala_param_shapes(A), params)


def _inputs(k):
    """observations / rewards / dones of rollout number k"""
    rng = np.random.default_rng(170 + k)
    return (rng.integers(0, 256, size=(T + 1, E, 64, 64, 3), dtype=np.uint8), rng.standard_normal((T, E)).astype(np.float32),
            (rng.random((T, E)) < 0.3).astype(np.float32))


def _engine():
    from mi355.engine import Engine
    eng = Engine("impala", T, E, A, NB, precision="bf16")
    eng.set_params(_flat())
    return eng


def _readout(eng, outs):
    from mi355 import engine as M
    r = dict(act=np.stack([o[0] for o in outs[:T]]), logp=np.stack([o[1] for o in outs[:T]]), val=np.stack([o[2] for o in outs]),
             f_act=eng.read_field(M.F_ACT), f_logp=eng.read_field(M.F_LOGP), f_val=eng.read_field(M.F_VALUE),
             f_rew=eng.read_field(M.F_REW), f_done=eng.read_field(M.F_DONE), obs=np.stack([eng.get_obs(t) for t in range(T + 1)]))
    eng.compute_estimates(0.999, 0.95, True, True)
    r["adv"] = eng.read_field(M.F_ADV)
    return r


def _serial(eng, k, seed):
    obs, rew, done = _inputs(k)
    outs = []
    for t in range(T + 1):
        eng.put_obs(t, obs[t])
        outs.append(eng.rollout_step(t, rew[t - 1] if t else None, done[t - 1] if t else None, seed=seed))
    return _readout(eng, outs)


def _pipelined(jobs):
    """jobs = [(engine, groups, rollout number, seed)]: the rollouts of all jobs in ONE host loop, stepped in alternation the way
    PPO._collect_lanes steps its lanes (for t: for g: for lane: wait, submit); returns one readout per job"""
    S = []
    for eng, G, k, seed in jobs:
        if getattr(eng, "n_groups", 1) != G:
            eng.rollout_groups(G)
        ng = E // G
        obs, rew, done = _inputs(k)
        stage = [[eng.pinned(obs[0, :ng].shape, obs.dtype) for _ in range(2)] for _ in range(G)]
        S.append(dict(eng=eng, G=G, ng=ng, obs=obs, rew=rew, done=done, stage=stage, seed=seed, got=[None] * G, outs=[]))
    cat = lambda got: tuple(np.concatenate([x[j] for x in got]) for j in range(3))
    for t in range(T + 1):
        for g in range(max(s["G"] for s in S)):
            for s in S:
                if g >= s["G"]:
                    continue
                eng, ng = s["eng"], s["ng"]
                if t:
                    s["got"][g] = eng.rollout_wait(g)
                sl = slice(g * ng, (g + 1) * ng)
                s["stage"][g][t & 1][...] = s["obs"][t, sl]
                eng.rollout_submit(t, g, s["stage"][g][t & 1], np.ascontiguousarray(s["rew"][t - 1, sl]) if t else None,
                                   np.ascontiguousarray(s["done"][t - 1, sl]) if t else None, seed=s["seed"])
                if t and g == s["G"] - 1:
                    s["outs"].append(cat(s["got"]))
    res = []
    for s in S:
        s["outs"].append(cat([s["eng"].rollout_wait(g) for g in range(s["G"])]))
        res.append(_readout(s["eng"], s["outs"]))
    return res


def _update(eng, k):
    """one minibatch (1024 rows: the side-stream path) + optimizer step on what the rollout left in the ring; returns what it produced"""
    idx = np.random.default_rng(50 + k).integers(0, T * E, NB)
    eng.minibatch(idx, NB, eng.hparams())
    log = eng.loss_log()
    eng.optimizer_step(5e-4, 0.5, k + 1)
    return dict(loss=np.array(log), params=eng.get_params().copy())


def _same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


PLAN = (4, 2, 4)          # env groups of the three rollouts of test 1


@pytest.fixture(scope="module")
def serial_reference():
    """rollout 0, update 0, rollout 1, update 1, rollout 2 through serial steps on one engine: computed once, read by several tests"""
    eng = _engine()
    ref = []
    for k in range(len(PLAN)):
        ref.append(_serial(eng, k, seed=5 + k))
        if k + 1 < len(PLAN):
            ref.append(_update(eng, k))
    eng.close()
    assert len(set(ref[0]["act"].reshape(-1).tolist())) > 1 and np.abs(ref[1]["params"] - _flat()).max() > 0
    return ref


def test_numbers_unchanged_across_lane_reuse(serial_reference):
    """G = 4, then 2, then 4 again on ONE engine (a group keeps its lane; groups 2 and 3 rest during the middle rollout), a side-stream
    minibatch + optimizer step between the rollouts: every returned array, ring field, loss record and parameter is bit-equal to the
    engine that did the same through serial steps."""
    eng = _engine()
    got = []
    for k, G in enumerate(PLAN):
        got.append(_pipelined([(eng, G, k, 5 + k)])[0])
        if k == 0:
            info = eng.lane_info()
            assert len(info) == 4 and len({s for _, s in info}) == 4, info
        if k + 1 < len(PLAN):
            got.append(_update(eng, k))
    assert eng.lane_info() == info          # a group never changes its stream
    eng.close()
    for j, (a, b) in enumerate(zip(serial_reference, got)):
        _same(a, b, j)


def test_two_live_engines_hold_disjoint_lanes(serial_reference):
    """Engines A and B with two groups each, stepped in alternation: each returns what it returns alone, and the two hold four
    different streams.  After A is closed a new engine with four groups gets four different lanes, and B still steps correctly."""
    solo = []
    for k, seed in ((0, 5), (1, 9)):
        e = _engine(); solo.append(_pipelined([(e, 2, k, seed)])[0]); e.close()
    _same(serial_reference[0], solo[0], "solo A")          # (same parameters, inputs and seed as the reference's first rollout)
    a, b = _engine(), _engine()
    ra, rb = _pipelined([(a, 2, 0, 5), (b, 2, 1, 9)])
    _same(solo[0], ra, "A beside B"); _same(solo[1], rb, "B beside A")
    ia, ib = a.lane_info(), b.lane_info()
    assert len(ia) == 2 and len(ib) == 2 and len({s for _, s in ia + ib}) == 4, (ia, ib)
    a.close()
    c = _engine()
    c.rollout_groups(4)
    ic = c.lane_info()
    assert len(ic) == 4 and len({s for _, s in ic}) == 4, ic
    assert b.lane_info() == ib
    rc, rb2 = _pipelined([(c, 4, 0, 5), (b, 2, 1, 9)])          # (4 + 2 groups live on four lanes: two are shared)
    _same(serial_reference[0], rc, "C beside B"); _same(solo[1], rb2, "B beside C")
    b.close(); c.close()


def test_lanes_do_not_depend_on_process_history(serial_reference):
    """Three engines with 4, 2 and 1 groups are opened, stepped once and closed; a fresh engine's G = 4 rollout then equals the reference."""
    for G in (4, 2, 1):
        e = _engine()
        e.rollout_groups(G)
        for g in range(G):
            e.rollout_submit(0, g, None, seed=1)
        for g in range(G):
            e.rollout_wait(g)
        assert len({s for _, s in e.lane_info()}) == G
        e.close()
    eng = _engine()
    got = _pipelined([(eng, 4, 0, 5)])[0]
    assert len({s for _, s in eng.lane_info()}) == 4
    eng.close()
    _same(serial_reference[0], got, "after 4, 2, 1")


def test_the_four_lanes_overlap():
    """One fixed-length sleeping workgroup per lane (mi_debug_lane_probe: nothing it could wait on).  t1 = one lane alone (>= 150 us),
    t4 = all four at once, each the minimum of five probes.  Four lanes on four hardware queues give t4 / t1 of about 1.0, two pairs
    that share queues 2.0, full serialisation 4.0: the bound 1.5 separates the first from the others.  Runs in whatever queue budget
    the process was given."""
    eng = _engine()
    eng.rollout_groups(4)
    eng.debug_lane_probe(0b1111, 64)          # (first launch of the kernel: code object load, queues created)
    iters = 64
    while True:
        t1 = min(eng.debug_lane_probe(1, iters) for _ in range(5))
        if t1 >= 150.0 or iters >= 4096:
            break
        iters *= 2
    assert t1 >= 150.0, (iters, t1)
    single = [min(eng.debug_lane_probe(1 << g, iters) for _ in range(5)) for g in range(4)]
    t4 = min(eng.debug_lane_probe(0b1111, iters) for _ in range(5))
    info = eng.lane_info()
    eng.close()
    print(f"lane probe: iters {iters}, single lanes {single} us, t1 {t1:.1f} us, t4 {t4:.1f} us, t4 / t1 = {t4 / t1:.2f}; lanes {info}")
    assert t4 < 1.5 * t1, (t1, t4, info)
