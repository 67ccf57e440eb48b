"""IPL agent (reference: agents/IPL.py:11-303) on the MI355X engine.

The reference's constructor and public methods.  The rollout ring, the network passes, clip, Adam and the checkpoint layout are PPO's
(this class reuses PPO's engine set-up and collector: the ring fields IPL needs are a subset of PPO's); IPL's own arithmetic -- a loss
that reads the network at obs[t] AND obs[t + 1] -- is mi_ipl_minibatch (csrc/ipl.hip): three forward and two backward passes per
minibatch, one 8-float record per minibatch in the device loss log, read once per ``optimize()``.

Built: what the shipped sets `hard-500-ipl` and `ipl_cartpole` reach, plus entropy_modified / reward_incentive / adv_incentive /
accumulate_all_grads / alpha / entropy_coef and ``predict(greedy=True)``.  Refused by name (check_supported): learned_gamma and
learned_temp (they need CategoricalPolicy(extra_params=True), which the reference's factory never passes), the greedy env
(--use_greedy_env: a third env, storage and logger column set), recurrent policies, logsumexp_logits_is_v, more than one rank.
Reference quirks kept: 'Loss/alpha' is the mean of an empty list (nan); ``mini_batch_size`` is shrunk to T*E/n_minibatch; the optimizer
steps by the float rule cnt % (batch_size / mini_batch_size) == 0, or once per epoch with accumulate_all_grads; validation rollouts
are collected and logged, never trained on.
"""
import os

import numpy as np
import torch

from common.model import as_device_obs
from .ppo import PPO


def check_supported(hp=None, policy=None, env_greedy=None, storage_greedy=None, use_greedy_env=False):
    """Every IPL option outside the built scope, refused by name -- from train.py before any engine is built, and from IPL.__init__."""
    hp = hp or {}
    for k in ("learned_gamma", "learned_temp"):
        if hp.get(k, False):
            raise NotImplementedError(f"algo IPL with {k}=True is not supported: it needs CategoricalPolicy(extra_params=True), "
                                      "which stays refused")
    if use_greedy_env or env_greedy is not None or storage_greedy is not None:
        raise NotImplementedError("algo IPL with a greedy env (--use_greedy_env / env_greedy / storage_greedy) is not supported: "
                                  "predict(greedy=True) is, the third env + storage + logger column set is not")
    if hp.get("recurrent", False) or (policy is not None and policy.is_recurrent()):
        raise NotImplementedError("algo IPL with recurrent: True is not supported (the reference's IPL never passes a hidden state)")
    if hp.get("logsumexp_logits_is_v", False) or (policy is not None and getattr(policy, "logsumexp_logits_is_v", False)):
        raise NotImplementedError("algo IPL with logsumexp_logits_is_v is not supported")
    if int(os.environ.get("WORLD_SIZE", 1)) > 1:
        raise NotImplementedError(f"algo IPL runs on a single GPU: WORLD_SIZE (world size) = {os.environ['WORLD_SIZE']} is not supported")


class IPL(PPO):
    def __init__(self, env, policy, logger, storage, device, n_checkpoints, env_valid=None, storage_valid=None,
                 n_steps=128, n_envs=8, epoch=3, n_minibatch=8, mini_batch_size=32 * 8, gamma=0.99, lmbda=0.95,
                 learning_rate=2.5e-4, grad_clip_norm=0.5, normalize_adv=True, normalize_rew=True, increasing_lr=False,
                 env_greedy=None, storage_greedy=None, learned_gamma=False, learned_temp=False, reward_incentive=False,
                 adv_incentive=False, accumulate_all_grads=False, alpha_learning_rate=2.5e-4, target_entropy_coef=0.5, alpha=1,
                 entropy_coef=0, entropy_modified=False, **kwargs):
        check_supported({"learned_gamma": learned_gamma, "learned_temp": learned_temp}, policy, env_greedy, storage_greedy)
        for k in ("eps_clip", "value_coef", "x_entropy_coef", "use_gae", "entropy_scaling", "sparsity_coef", "fs_coef", "merge_accumulation"):
            kwargs.pop(k, None)                                   # (PPO's own terms: not part of this loss)
        super().__init__(env, policy, logger, storage, device, n_checkpoints, env_valid=env_valid, storage_valid=storage_valid,
                         n_steps=n_steps, n_envs=n_envs, epoch=epoch, n_minibatch=n_minibatch, mini_batch_size=mini_batch_size,
                         gamma=gamma, lmbda=lmbda, learning_rate=learning_rate, grad_clip_norm=grad_clip_norm, entropy_coef=entropy_coef,
                         normalize_adv=normalize_adv, normalize_rew=normalize_rew, increasing_lr=increasing_lr,
                         merge_accumulation=False, **kwargs)
        self.entropy_modified, self.entropy_coef, self.alpha = entropy_modified, entropy_coef, alpha
        self.target_entropy = self.policy.target_entropy * target_entropy_coef
        self.adv_incentive, self.reward_incentive = adv_incentive, reward_incentive
        self.learned_temp, self.learned_gamma = False, False
        self.accumulate_all_grads = accumulate_all_grads
        self.env_greedy = self.storage_greedy = None
        self.last_predicted_reward = self.last_reward = None
        self.optimizer_steps = 0                                  # optimizer steps taken by optimize() so far (tests count them)

    # ------------------------------------------------------------------ predict
    def predict(self, obs, greedy=False):
        """agents/IPL.py:82-94 -> (act, value).  The observation is staged on the device: the IPLStorage.store / store_last that
        follows with the same array commits it into its slot."""
        dev_obs = as_device_obs(obs, self.policy.arch)
        if greedy:
            act, logp, value = self.engine.predict_greedy(dev_obs)
        else:
            self._predict_calls = getattr(self, "_predict_calls", 0) + 1
            act, logp, value = self.engine.predict_staged(dev_obs, seed=self.seed * 1000003 + self._iter,
                                                          counter=self._predict_calls * self.n_envs)
        self.storage.note_predicted(-1, obs, act, logp, value)
        return act, value

    # predict_w_value_saliency(obs, hidden_state, done) is PPO's: the existing engine call (mi_value_saliency)

    # ------------------------------------------------------------------ optimize
    def _ipl_hparams(self):
        return self.engine.ipl_hparams(self.gamma, self.alpha, self.entropy_coef, self.entropy_modified, self.reward_incentive,
                                       self.adv_incentive)

    def optimize(self):
        batch_size = self.n_steps * self.n_envs // self.n_minibatch
        if batch_size < self.mini_batch_size:
            self.mini_batch_size = batch_size
        grad_accumulation_steps = batch_size / self.mini_batch_size
        grad_accumulation_cnt = 1
        eng, hp = self.engine, self._ipl_hparams()
        n_last = 0

        def step():
            gn = self.optimizer.step(self.grad_clip_norm, want_norm=self.detect_nan)
            self.optimizer_steps += 1
            if self.detect_nan and not np.isfinite(gn):
                raise RuntimeError(f"Found NaN / Inf in the gradient norm of optimizer step {self.optimizer.step_count}: {gn}")

        for _ in range(self.epoch):
            for idx in self.storage.minibatch_index_stream(self.mini_batch_size, False):
                eng.ipl_minibatch(idx, len(idx), hp)
                n_last = len(idx)
                if not self.accumulate_all_grads and grad_accumulation_cnt % grad_accumulation_steps == 0:
                    step()
                grad_accumulation_cnt += 1
            if self.accumulate_all_grads:
                step()
        log = eng.loss_log(reset=True)
        if self.detect_nan and not np.isfinite(log[:, [0, 1, 2, 7]]).all():
            raise RuntimeError("Found NaN / Inf in the loss terms of this update")
        n = len(log)
        summary = {'Loss/entropy': float(np.mean(log[:, 0])), 'Loss/mutual_info': float(np.mean(log[:, 1])),
                   'Loss/total': float(np.mean(log[:, 2])), 'Loss/rew_corr': float(np.mean(log[:, 3])),
                   'Loss/gamma': float(np.mean([self.gamma] * n)),
                   'Loss/alpha': float("nan"),                    # np.mean([]) of the reference: the temperature is not learned
                   'alpha': float(np.mean([self.alpha] * n)), 'Loss/pred_reward': float(np.mean(log[:, 7]))}
        self.last_predicted_reward, self.last_reward = eng.ipl_read_pred(n_last)
        return summary

    def draw_permutation_ahead(self):
        self.storage.draw_permutation_ahead(self.n_steps * self.n_envs)

    # ------------------------------------------------------------------ rollout + train
    def _collect(self, env, engine, storage, obs, hidden_state=None, done=None):
        if self._can_pipeline(env):
            return self._collect_pipelined(env, engine, storage, obs, hidden_state, done)
        for _ in range(self.n_steps):
            act, _, value, _ = self._predict_into(engine, storage, storage.step, obs)
            next_obs, rew, done, info = env.step(act)
            storage.store(obs, act, rew, done, info, value)
            obs = next_obs
        _, _, last_val, _ = self._predict_into(engine, storage, self.n_steps, obs)
        storage.store_last(obs, last_val)
        return obs, hidden_state, done

    def collect_data(self, obs, storage, env, greedy=False):
        """agents/IPL.py:295-303.  Sampled actions on the agent's own storages go through PPO's collector (env groups included);
        greedy=True, or a storage of the caller's, runs the reference's loop on predict()."""
        engine = self.engine if storage is self.storage else self.engine_valid if storage is self.storage_valid else None
        if not greedy and engine is not None:
            return self._collect(env, engine, storage, obs, self._h0(), np.zeros(self.n_envs))[0]
        if storage is not self.storage:
            raise NotImplementedError("IPL.collect_data(greedy=True) is built for the agent's own storage only")
        for _ in range(self.n_steps):
            act, value = self.predict(obs, greedy)
            next_obs, rew, done, info = env.step(act)
            storage.store(obs, act, rew, done, info, value)
            obs = next_obs
        _, last_val = self.predict(obs, greedy)
        storage.store_last(obs, last_val)
        return obs

    def _h0(self):
        return np.zeros((self.n_envs, 0), np.float32)

    def train(self, num_timesteps):
        self.total_timesteps = num_timesteps
        save_every = num_timesteps // self.num_checkpoints
        checkpoints = sorted((i + 1) * save_every for i in range(self.num_checkpoints))
        checkpoint_cnt = 0
        obs = self.env.reset()
        if self.env_valid is not None:
            obs_v = self.env_valid.reset()
        while self.t < num_timesteps:
            self._iter += 1
            obs = self.collect_data(obs, self.storage, self.env)
            if self.env_valid is not None:
                self.engine_valid.copy_params_from(self.engine)
                obs_v = self.collect_data(obs_v, self.storage_valid, self.env_valid)
            summary = self.optimize()
            self.t += self.n_steps * self.n_envs
            rew_batch, done_batch, true_average_reward = self.storage.fetch_log_data()
            if (done_batch > 0).any():
                print(f"Mean Reward:{np.mean(rew_batch[done_batch > 0]):.2f}")
            if self.storage_valid is not None:
                rew_batch_v, done_batch_v, true_average_reward_v = self.storage_valid.fetch_log_data()
            else:
                rew_batch_v = done_batch_v = true_average_reward_v = None
            self.logger.feed(rew_batch, done_batch, true_average_reward, rew_batch_v, done_batch_v, true_average_reward_v, None, None, None)
            self.optimizer, lr = self.adjust_lr(self.optimizer, self.learning_rate, self.t, num_timesteps)
            self.logger.dump(summary, lr)
            self.draw_permutation_ahead()
            if checkpoint_cnt < len(checkpoints) and self.t > checkpoints[checkpoint_cnt]:
                print("Saving model.")
                torch.save({'model_state_dict': self.policy.state_dict(), 'optimizer_state_dict': self.optimizer.state_dict()},
                           self.logger.logdir + '/model_' + str(self.t) + '.pth')
                checkpoint_cnt += 1
        self.env.close()
        if self.env_valid is not None:
            self.env_valid.close()
