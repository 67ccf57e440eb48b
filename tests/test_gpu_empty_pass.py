"""An empty minibatch pass (n = 0: a rank that owns no sample of a global minibatch) on a bf16 IMPALA context.

It is the only way into the separate-launch route of backward_conv_pool_bf16 (csrc/engine.hip): with no sample the fused conv + pool
backward has no workgroup to launch.  The oracle of an empty batch adds nothing to the gradients, so the comparison is exact; test_error_paths
(test_gpu_engine.py) runs the same pass on the MLP."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_empty_bf16_pass_adds_nothing_to_the_gradients():
    from mi355 import layout
    from mi355.engine import Engine

    T, E, A, B = 4, 8, 15, 16
    rng = np.random.default_rng(11)
    shapes = layout.impala_param_shapes(A)
    params = {k: ((rng.standard_normal(s) / np.sqrt(np.prod(s[1:]))) if k.endswith("weight") else 0.05 * rng.standard_normal(s)).astype(np.float32)
              for k, s in shapes.items()}
    eng = Engine("impala", T, E, A, B, precision="bf16")
    eng.set_params(layout.flatten(shapes, params))
    frames = rng.integers(0, 256, size=(T + 1, E, 64, 64, 3), dtype=np.uint8)
    for t in range(T + 1):
        eng.put_obs(t, frames[t])
        eng.policy_step(t, seed=1, u=rng.random(E).astype(np.float32))
        if t < T:
            eng.put_step(t, rng.standard_normal(E).astype(np.float32), (rng.random(E) < 0.1).astype(np.float32))
    eng.compute_estimates(0.999, 0.95, True, True)
    hp = eng.hparams()
    eng.minibatch(rng.permutation(T * E)[:B], B, hp)
    before = eng.get_grads()
    assert np.isfinite(before).all() and np.abs(before).max() > 0
    eng.minibatch(np.zeros(0, np.int64), B, hp)          # empty local share of a global minibatch of B samples
    after = eng.get_grads()
    assert np.array_equal(before, after), "an empty pass changed the gradients"
    assert eng.loss_log(reset=True).shape[0] == 2       # it still logs its (empty) record
    eng.close()
