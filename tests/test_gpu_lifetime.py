"""Who owns what a context allocates (csrc/devpool.h, engine.hip ctx_release): every device buffer, pinned buffer and event of a context --
those of mi_create, of every lazily allocated group and of the SAE agent's state -- goes back when the context is destroyed.
mi_debug_live_resources counts what the pools of the process hold; after close() the three counts are what they were before the
context was made, for each kind of context, twice over.

Shapes: T = 2, E = 4, A = 15, max_batch = 8, out_dim = 64 (the smallest width mi_gru_train accepts); MLP obs_dim = 8, depth 2, width 16.
The counts do not depend on sizes."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, E, A, NB, H = 2, 4, 15, 8, 64
KINDS = ("impala-fp32", "impala-bf16", "mlp")


def _make(kind):
    from mi355.engine import Engine
    if kind == "mlp":
        return Engine("mlp", T, E, A, NB, obs_dim=8, mlp_depth=2, mlp_width=16, out_dim=H)
    return Engine("impala", T, E, A, NB, out_dim=H, precision=kind.split("-")[1])


def _obs(eng, kind, rng):
    if kind == "mlp":
        return rng.standard_normal((E, 8)).astype(np.float32)
    return rng.integers(0, 256, size=(E, 64, 64, 3), dtype=np.uint8)


def _touch_every_lazy_group(eng, kind):
    from mi355.engine import Engine
    rng = np.random.default_rng(5)
    eng.set_params(0.05 * rng.standard_normal(eng.n_params).astype(np.float32))
    obs = _obs(eng, kind, rng)
    assert np.isfinite(eng.value_saliency(obs, seed=1)[3]).all()                 # the saliency buffers (without the GRU)
    eng.ipl_minibatch(np.arange(T * E), T * E, Engine.ipl_hparams())             # the IPL buffers
    if kind != "mlp":
        eng.sae_create(64, 0.05)                                                 # the SAE agent's state, on a non-recurrent IMPALA context
    g = [0.05 * rng.standard_normal(s).astype(np.float32) for s in eng.gru_shapes()]
    eng.set_gru(*g)                                                              # the GRU cell's tensors and state
    eng.rec_begin(np.zeros((E, H), np.float32), np.zeros(E, np.float32))         # the hidden ring, its staging buffer and event
    eng.gru_train(True)                                                          # the GRU's gradients, moments and sequence buffers
    assert np.isfinite(eng.value_saliency(obs, seed=1)[3]).all()                 # the saliency buffers of the pass through the GRU


def test_every_context_kind_returns_what_it_took():
    from mi355.engine import live_resources
    gc.collect()                                         # (engines an earlier test dropped without close() go now, not in the middle)
    base = live_resources()
    for rnd in range(2):
        for kind in KINDS:
            eng = _make(kind)
            _touch_every_lazy_group(eng, kind)
            held = live_resources()
            assert all(h > b for h, b in zip(held, base)), (rnd, kind, held, base)
            eng.close()
            assert live_resources() == base, (rnd, kind, live_resources(), base)


def test_destroy_alone_releases_a_live_sae():
    from mi355.engine import live_resources
    gc.collect()
    base = live_resources()
    eng = _make("impala-bf16")
    plain = live_resources()
    eng.sae_create(64, 0.05)
    assert all(h > p for h, p in zip(live_resources(), plain))
    assert eng.lib.mi_destroy(eng._ctx) == 0             # not Engine.close(): no mi_sae_destroy in front
    eng._ctx, eng.sae_dim = C.c_void_p(), None
    assert live_resources() == base


def test_sae_destroy_is_idempotent():
    from mi355.engine import live_resources
    gc.collect()
    base = live_resources()
    eng = _make("impala-fp32")
    plain = live_resources()
    eng.sae_create(64, 0.05)
    assert eng.lib.mi_sae_destroy(eng._ctx) == 0 and live_resources() == plain
    assert eng.lib.mi_sae_destroy(eng._ctx) == 0 and live_resources() == plain
    eng.sae_create(128, 0.05)                            # and the context can take another one
    eng.close()
    assert live_resources() == base
