"""Host view of the device-resident Adam state, in torch.optim.Adam's own state_dict layout.

The reference builds ``optim.Adam(policy.parameters(), lr, eps=1e-5)`` (agents/ppo.py:58), anneals
``param_groups[i]['lr']`` (common/misc_util.py:92-96) and checkpoints ``optimizer.state_dict()``
(agents/ppo.py:271-276, resumed at train.py:260-263).  The moments live in the engine's flat
buffers; a never-stepped torch Adam over the host parameter views is kept purely as the container
that produces / consumes that exact on-disk layout."""
import torch
import torch.optim as optim

from . import layout


class DeviceAdam:
    def __init__(self, policy, engine, lr, eps=1e-5, stateless=()):
        self.policy, self.engine, self.eps = policy, engine, eps
        self._params = [p for n, p in policy.named_parameters() if not n.startswith("gru.")]
        self._names = [n for n, _ in policy.named_parameters() if not n.startswith("gru.")]
        # the container spans ALL policy parameters like the reference's optim.Adam(policy.parameters()) (a frozen GRU
        # never receives gradients there, so it never gets optimiser state either)
        self._adam = optim.Adam(list(policy.parameters()), lr=lr, eps=eps)
        self.step_count = 0
        # logsumexp_logits_is_v: fc_value never receives a gradient (policy.py:77-78), so torch's Adam never creates state for it -- like
        # the frozen GRU it stays in param_groups and out of `state`; the device moments of its slice are and stay zero
        self._stateless = {"fc_value.weight", "fc_value.bias"} if getattr(policy, "logsumexp_logits_is_v", False) else set()
        # `stateless`: further tensors the caller's loss never reaches (the distiller's MSE leaves fc_value.grad None in the reference)
        self._stateless |= set(stateless)

    @property
    def param_groups(self):
        return self._adam.param_groups

    @property
    def lr(self):
        return float(self._adam.param_groups[0]['lr'])

    def zero_grad(self, set_to_none=True):
        pass                                   # gradients are zeroed inside the fused device step

    def step(self, max_grad_norm, want_norm=False):
        self.step_count += 1
        out = self.engine.optimizer_step(self.lr, max_grad_norm, self.step_count, want_norm)
        self.policy.mark_device_updated()
        return out

    def step_eps(self, max_grad_norm=float("inf"), want_norm=False):
        """step() with this optimizer's own eps (mi_optimizer_step_eps; step() is the agents' Adam(eps=1e-5)); inf: no clipping."""
        self.step_count += 1
        out = self.engine.optimizer_step_eps(self.lr, max_grad_norm, self.eps, self.step_count, want_norm)
        self.policy.mark_device_updated()
        return out

    def _gru_trained(self):
        return bool(getattr(self.policy, "_gru_trained", False))

    def state_dict(self):
        if self.step_count > 0:
            shapes = self.policy.param_shapes()
            m, v = self.engine.get_adam_state()
            m, v = layout.unflatten(shapes, m), layout.unflatten(shapes, v)
            for n, p in zip(self._names, self._params):
                if n in self._stateless:
                    continue
                self._adam.state[p] = {'step': torch.tensor(float(self.step_count)),
                                       'exp_avg': torch.from_numpy(m[n]), 'exp_avg_sq': torch.from_numpy(v[n])}
            if self._gru_trained():
                # algo ppo-pure: the GRU's four tensors are trained, so they carry state like every other parameter (they come last
                # in policy.parameters()); the device keeps their moments as one vector {w_ih, w_hh, b_ih, b_hh}
                gm, gv = self.engine.get_gru_adam_state()
                off = 0
                for p in self.policy.gru_parameters():
                    k = p.numel()
                    self._adam.state[p] = {'step': torch.tensor(float(self.step_count)),
                                           'exp_avg': torch.from_numpy(gm[off:off + k].reshape(tuple(p.shape)).copy()),
                                           'exp_avg_sq': torch.from_numpy(gv[off:off + k].reshape(tuple(p.shape)).copy())}
                    off += k
        return self._adam.state_dict()

    def load_state_dict(self, sd):
        self._adam.load_state_dict(sd)
        shapes = self.policy.param_shapes()
        st = self._adam.state
        if len(st) == 0:
            return
        import numpy as np
        zeros = lambda n: np.zeros(shapes[n], np.float32)
        # fc_value's moments are zero in this mode whatever the file holds: a state written in this mode has no entries for it, and one
        # written with the fc_value head (the flag off) carries moments that would go on moving the parameter under a zero gradient
        # (m / (sqrt(v) + eps) != 0).  Such entries are dropped, so that state_dict() gives this mode's layout again.
        for n, p in zip(self._names, self._params):
            if n in self._stateless:
                st.pop(p, None)
        m = {n: zeros(n) if n in self._stateless else st[p]['exp_avg'].numpy() for n, p in zip(self._names, self._params)}
        v = {n: zeros(n) if n in self._stateless else st[p]['exp_avg_sq'].numpy() for n, p in zip(self._names, self._params)}
        self.engine.set_adam_state(layout.flatten(shapes, m), layout.flatten(shapes, v))
        if self._gru_trained():
            gp = self.policy.gru_parameters()
            if all(p in st for p in gp):
                self.engine.set_gru_adam_state(np.concatenate([st[p]['exp_avg'].numpy().ravel() for p in gp]),
                                               np.concatenate([st[p]['exp_avg_sq'].numpy().ravel() for p in gp]))
        self.step_count = int(float(next(st[p]['step'] for p in self._params if p in st)))


class DeviceModelAdam:
    """DeviceAdam for one model of the SAE agent (agents/sae.py:64-65: optim.Adam(self.sae.parameters()) / optim.Adam(self.linear_model
    .parameters()), lr, eps=1e-5): `which` = Engine.SAE or Engine.PROBE selects the flat vector of the mi_sae_* entry points.  The
    moments live on the device; a never-stepped torch Adam over the module's host parameters produces / consumes torch's own
    state_dict layout."""

    def __init__(self, module, engine, which, lr, eps=1e-5):
        self.module, self.engine, self.which = module, engine, which
        self._params = list(module.parameters())
        self._adam = optim.Adam(self._params, lr=lr, eps=eps)
        self.step_count = 0
        self.device_is_newer = False

    @property
    def param_groups(self):
        return self._adam.param_groups

    @property
    def lr(self):
        return float(self._adam.param_groups[0]['lr'])

    def zero_grad(self, set_to_none=True):
        pass                                   # gradients are zeroed inside the fused device step

    def push_params(self):
        import numpy as np
        self.engine.sae_set_params(self.which, np.concatenate([p.detach().cpu().numpy().ravel() for p in self._params]))
        self.device_is_newer = False

    def pull_params(self):
        """The module's host tensors := the device's working copy (before state_dict() / a checkpoint)."""
        if not self.device_is_newer:
            return
        flat, off = self.engine.sae_get_params(self.which), 0
        with torch.no_grad():
            for p in self._params:
                p.copy_(torch.from_numpy(flat[off:off + p.numel()].reshape(tuple(p.shape)).copy()))
                off += p.numel()
        self.device_is_newer = False

    def step(self, max_grad_norm, want_norm=False):
        self.step_count += 1
        out = self.engine.sae_optimizer_step(self.which, self.lr, max_grad_norm, self.step_count, want_norm)
        self.device_is_newer = True
        return out

    def state_dict(self):
        if self.step_count > 0:
            m, v = self.engine.sae_get_adam_state(self.which)
            off = 0
            for p in self._params:
                k = p.numel()
                self._adam.state[p] = {'step': torch.tensor(float(self.step_count)),
                                       'exp_avg': torch.from_numpy(m[off:off + k].reshape(tuple(p.shape)).copy()),
                                       'exp_avg_sq': torch.from_numpy(v[off:off + k].reshape(tuple(p.shape)).copy())}
                off += k
        return self._adam.state_dict()

    def load_state_dict(self, sd):
        import numpy as np
        self._adam.load_state_dict(sd)
        st = self._adam.state
        if len(st) == 0:
            return
        self.engine.sae_set_adam_state(self.which, np.concatenate([st[p]['exp_avg'].numpy().ravel() for p in self._params]),
                                       np.concatenate([st[p]['exp_avg_sq'].numpy().ravel() for p in self._params]))
        self.step_count = int(float(st[self._params[0]]['step']))
