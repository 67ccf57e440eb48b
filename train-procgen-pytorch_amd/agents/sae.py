"""Sparse-autoencoder agent (reference: agents/sae.py:10-286, `algo: sae`) on the MI355X engine.

Stage 1 trains a sparse autoencoder on the 2048 block-3 features (ImpalaModel.forward_to_pool) of a FROZEN, trained IMPALA policy;
stage 2 trains a linear probe (fc_policy, fc_value) that acts from the autoencoder's codes.  Same constructor arguments, defaults and
public methods; what differs is where things live: the features never leave the device -- every rollout step writes them, the
policy's logits, the value and the action into device rings (mi_sae_step), a minibatch is an index vector (mi_sae_minibatch /
mi_sae_probe_minibatch), Adam and the clip run on the device.  The policy runs in --precision fp32 or bf16; all SAE / probe
arithmetic is fp32.

Supported: ImpalaModel, non-recurrent, one GPU, serial rollout steps (no env groups).  Everything else is refused by name.

Reference behaviours kept on purpose (each marked where it happens): `self.t` is shared by the two stages; `collect_rollouts` does
not hand the next observation back; `anneal_lr` anneals `self.optimizer` (the SAE's) in both stages; the value loss of the probe is
the reference's (n,1) - (n,) broadcast (see mi_sae_probe_minibatch)."""
import os

import numpy as np
import torch

from common.misc_util import adjust_lr
from common.model import LinearSAEProbe, SparseAutoencoder, as_device_obs
from mi355.engine import Engine
from mi355.optim import DeviceModelAdam
from .base_agent import BaseAgent


def check_supported(policy, n_envs, env=None, sae_dim=1024):
    """The combinations the engine's SAE path is built for; any other is refused with the option's name."""
    if getattr(policy, "arch", None) != "impala":
        raise NotImplementedError("algo sae with architecture mlpmodel is not supported: encoded_dim / forward_to_pool exist only on "
                                  "ImpalaModel (architecture: impala)")
    if policy.is_recurrent():
        raise NotImplementedError("algo sae with recurrent: True is not supported (the reference's SAE agent never carries a hidden state)")
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        raise NotImplementedError(f"algo sae runs on a single GPU: WORLD_SIZE (world size) = {world} is not supported")
    if env is not None and len(getattr(env, "env_groups", ())) > 1:
        raise NotImplementedError("algo sae runs serial rollout steps: rollout_groups > 1 (env groups) is not supported")
    if int(sae_dim) not in Engine.SAE_DIMS:
        raise NotImplementedError(f"sae_dim={sae_dim} is not supported: sae_dim must be a multiple of 64 in [64, 4096]")


class SAE(BaseAgent):
    def __init__(self, env, policy, logger, storage, device, n_checkpoints, env_valid=None, storage_valid=None,
                 n_steps=128, n_envs=8, epoch=3, mini_batch_per_epoch=8, mini_batch_size=32 * 8, gamma=0.99, lmbda=0.95,
                 learning_rate=2.5e-4, grad_clip_norm=0.5, eps_clip=0.2, value_coef=0.5, entropy_coef=0.01, normalize_adv=True,
                 normalize_rew=True, use_gae=True, l1_coef=0., anneal_lr=True, sae_dim=1024, rho=0.05, sparse_coef=1e-3,
                 close_envs=True, **kwargs):
        super().__init__(env, policy, logger, storage, device, n_checkpoints, env_valid, storage_valid)
        check_supported(policy, n_envs, env, sae_dim)
        if env_valid is not None and len(getattr(env_valid, "env_groups", ())) > 1:
            raise NotImplementedError("algo sae runs serial rollout steps: rollout_groups > 1 (env groups) is not supported")
        self.close_envs = close_envs
        self.sparse_coef, self.rho, self.sae_dim = sparse_coef, rho, sae_dim
        self.anneal_lr = anneal_lr
        self.n_steps, self.n_envs = n_steps, n_envs
        self.epoch, self.mini_batch_per_epoch, self.mini_batch_size = epoch, mini_batch_per_epoch, mini_batch_size
        self.learning_rate = learning_rate
        self.grad_clip_norm = grad_clip_norm
        self.seed = int(kwargs.get("seed", 0))
        self.precision = kwargs.get("precision", "fp32")
        # agents/sae.py:60-63 (same construction order: the SAE draws its weights first, then the probe)
        self.sae = SparseAutoencoder(input_dim=policy.embedder.encoded_dim, hidden_dim=sae_dim, rho=rho)
        self.linear_model = LinearSAEProbe(sae_dim, policy.action_size)
        self.engine = self._make_engine(policy, device, min(mini_batch_size, max(1, n_steps * n_envs // mini_batch_per_epoch)))
        policy.attach_engine(self.engine)
        self.engine.sae_create(sae_dim, rho)
        storage.attach_engine(self.engine)
        if storage_valid is not None:
            storage_valid.attach_engine(self.engine, ring=False)      # validation steps do not store (mi_sae_step, store = 0)
        # agents/sae.py:64-65
        self.optimizer = DeviceModelAdam(self.sae, self.engine, Engine.SAE, learning_rate, eps=1e-5)
        self.l_optimizer = DeviceModelAdam(self.linear_model, self.engine, Engine.PROBE, learning_rate, eps=1e-5)
        self.optimizer.push_params()
        self.l_optimizer.push_params()
        self._calls = 0

    def _make_engine(self, policy, device, max_batch):
        dev_index = device.index if isinstance(device, torch.device) and device.index is not None else 0
        return Engine("impala", self.n_steps, self.n_envs, policy.action_size, max_batch=max(max_batch, self.n_envs),
                      out_dim=policy.embedder.output_dim, device=dev_index, precision=self.precision,
                      value_from_logits=policy.logsumexp_logits_is_v)

    def _sampler_seed(self):
        return self.seed * 1000003 + 1

    # ------------------------------------------------------------------ acting
    def _step(self, obs, storage, t, policy=None):
        """One engine step on ring slot t of `storage` (stores unless it is the validation storage) -> (act, value)."""
        store = bool(getattr(storage, "ring", True))
        act, value = self.engine.sae_step(t, as_device_obs(obs, "impala"), act_from_probe=policy is not None, store=store,
                                          seed=self._sampler_seed())
        if store:
            storage.note_stepped(t)
        return act, value

    def get_hidden_and_acts(self, obs, policy=None):
        """agents/sae.py:73-86 -> (act, hidden (E, 2048), the policy's logits (E, A), value).  Stores nothing."""
        act, value = self.engine.sae_step(0, as_device_obs(obs, "impala"), act_from_probe=policy is not None, store=False,
                                          seed=self._sampler_seed())
        return act, self.engine.sae_get_hidden(-1), self.engine.sae_get_logits(-1), value

    def predict(self, obs, hidden_state, done):
        """agents/sae.py:88-97: the frozen policy's own step."""
        self._calls += 1
        act, logp, value = self.engine.predict_staged(as_device_obs(obs, "impala"), seed=self._sampler_seed() + 1,
                                                      counter=self._calls * self.n_envs)
        return act, logp, value, np.asarray(hidden_state)

    def predict_w_value_saliency(self, obs, hidden_state, done):
        """agents/sae.py:99-110 through the engine's value-saliency pass (mi_value_saliency)."""
        self._calls += 1
        act, logp, value, grad = self.engine.value_saliency(as_device_obs(obs, "impala"), seed=self._sampler_seed() + 1,
                                                            counter=self._calls * self.n_envs)
        return act, logp, value, np.asarray(hidden_state), np.ascontiguousarray(grad.transpose(0, 3, 1, 2))

    def predict_for_logit_saliency(self, obs, act, all_acts=False):
        raise NotImplementedError("SAE.predict_for_logit_saliency is not supported on the engine (no logit-saliency backward pass)")

    def predict_for_rew_saliency(self, obs, done):
        raise NotImplementedError("SAE.predict_for_rew_saliency is not supported on the engine (it returns autograd tensors)")

    # ------------------------------------------------------------------ updates
    def _accumulation(self):
        """agents/sae.py:137-141 -> grad_accumulation_steps (a float, compared with `cnt % steps == 0` as there)."""
        batch_size = self.n_steps * self.n_envs // self.mini_batch_per_epoch
        if batch_size < self.mini_batch_size:
            self.mini_batch_size = batch_size
        return batch_size / self.mini_batch_size

    def _optimize(self, minibatch, optimizer):
        steps, cnt, logs = self._accumulation(), 1, []
        for _ in range(self.epoch):
            for idx in self.storage.fetch_train_generator(mini_batch_size=self.mini_batch_size, recurrent=False):
                logs.append(minibatch(idx))
                if cnt % steps == 0:             # let the model handle a large batch with little memory (:158-162)
                    optimizer.step(self.grad_clip_norm)
                    optimizer.zero_grad()
                cnt += 1
        return np.asarray(logs, dtype=np.float64).reshape(-1, 3)

    def optimize_sae(self):
        log = self._optimize(lambda idx: self.engine.sae_minibatch(idx, self.sparse_coef), self.optimizer)      # rows (recon, KL, loss)
        return {'Loss/total': np.mean(log[:, 2]), 'Loss/recon': np.mean(log[:, 0]), 'Loss/sparsity': np.mean(log[:, 1])}

    def optimize_linear_model(self):
        log = self._optimize(self.engine.sae_probe_minibatch, self.l_optimizer)                                # rows (value, logit, loss)
        return {'Loss/total_linear': np.mean(log[:, 2]), 'Loss/value': np.mean(log[:, 0]), 'Loss/logit': np.mean(log[:, 1])}

    # ------------------------------------------------------------------ train
    def train(self, num_timesteps):
        self.train_model(self.sae, self.optimizer, self.optimize_sae, num_timesteps, "sae")
        # reference behaviour kept (agents/sae.py:221-222): self.t is shared by the two stages, so stage 2 starts at num_timesteps and
        # runs to 2 * num_timesteps
        self.train_model(self.linear_model, self.l_optimizer, self.optimize_linear_model, num_timesteps + num_timesteps, "linear")
        if self.close_envs:
            self.env.close()
            if self.env_valid is not None:
                self.env_valid.close()

    def train_model(self, model, optimizer, optimize_func, num_timesteps, model_type):
        save_every = num_timesteps // self.num_checkpoints
        checkpoint_cnt = 0
        obs = self.env.reset()
        if self.env_valid is not None:
            obs_v = self.env_valid.reset()
        action_policy = True if model_type == 'linear' else None
        while self.t < num_timesteps:
            # reference behaviour kept (agents/sae.py:242, 272-279): collect_rollouts does not hand the last observation back, so `obs`
            # stays the reset observation and every rollout starts from it while the env itself has moved on
            self.collect_rollouts(obs, self.storage, self.env, action_policy)
            if self.env_valid is not None:
                self.collect_rollouts(obs_v, self.storage_valid, self.env_valid, action_policy)
            summary = optimize_func()
            self.t += self.n_steps * self.n_envs
            rew_batch, done_batch, true_average_reward = self.storage.fetch_log_data()
            if self.storage_valid is not None:
                rew_batch_v, done_batch_v, true_average_reward_v = self.storage_valid.fetch_log_data()
            else:
                rew_batch_v = done_batch_v = true_average_reward_v = None
            if self.anneal_lr:                   # (:257-258: always self.optimizer, the SAE's, also in stage 2 -- kept)
                self.optimizer, lr = adjust_lr(self.optimizer, self.learning_rate, self.t, num_timesteps)
            else:
                lr = self.learning_rate
            self.logger.feed(rew_batch, done_batch, true_average_reward, rew_batch_v, done_batch_v, true_average_reward_v)
            self.logger.dump(summary, lr)
            if self.t > ((checkpoint_cnt + 1) * save_every):
                print("Saving model.")
                optimizer.pull_params()
                torch.save({'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict()},
                           self.logger.logdir + f'/{model_type}_{self.t}.pth')
                checkpoint_cnt += 1

    def collect_rollouts(self, obs, storage, env, policy=None):
        for _ in range(self.n_steps):
            act, value = self._step(obs, storage, storage.step, policy)
            next_obs, rew, done, info = env.step(act)
            storage.store(obs, None, act, rew, done, info, None, value)      # hidden / logits are in the device ring already
            obs = next_obs
        _, value = self._step(obs, storage, self.n_steps, policy)
        storage.store_last(obs, None, value)

    def explore(self, env, steps, policy=None):
        obs = env.reset()
        for _ in range(steps):
            act, _ = self.engine.sae_step(0, as_device_obs(obs, "impala"), act_from_probe=policy is not None, store=False,
                                          seed=self._sampler_seed())
            obs, rew, done, info = env.step(act)
