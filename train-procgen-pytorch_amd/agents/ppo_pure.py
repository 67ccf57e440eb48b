"""PPOPure (reference: agents/ppo_pure.py:11-247) on the MI355X engine: the PPO loss without the feature-sparsity / attention
terms, and -- what algo: ppo does not do -- a recurrent policy trained THROUGH its GRU.

The reference's optimize() calls ``self.policy(obs_batch, hidden_state_batch, mask_batch)`` (:126); for a recurrent policy that is
the training branch of GRU.forward (common/model.py:226-277): the hidden state is recomputed over the whole trajectory of the
minibatch's envs, from hidden_states_batch[0, envs], and the gradient runs back through time.  Here that is one
``mi_minibatch_rec`` per env group (the GRU over the sequence is one forward and one backward kernel, csrc/gru_seq.hip); the GRU's
four tensors get gradients, Adam state and their share of the global clip norm on the device (``mi_gru_train``).

Rollout, estimates, logging, checkpoints and the LR schedule are PPO's (agents/ppo.py here).  The training mask is the reference's:
m[t] = 1 - done_batch[t], the done stored WITH step t (:124, common/storage.py:105), where the rollout masks step t with the done of
step t - 1.  A recurrent policy trains on a single GPU only."""
import numpy as np

from .ppo import PPO


class PPOPure(PPO):
    def __init__(self, env, policy, logger, storage, device, n_checkpoints, env_valid=None, storage_valid=None,
                 n_steps=128, n_envs=8, epoch=3, n_minibatch=8, mini_batch_size=32 * 8, gamma=0.99, lmbda=0.95,
                 learning_rate=2.5e-4, grad_clip_norm=0.5, eps_clip=0.2, value_coef=0.5, entropy_coef=0.01,
                 x_entropy_coef=0., normalize_adv=True, normalize_rew=True, use_gae=True, entropy_scaling=None,
                 increasing_lr=False, sparsity_coef=0., fs_coef=0., **kwargs):
        recurrent = policy.is_recurrent()
        if recurrent and getattr(policy, "logsumexp_logits_is_v", False):
            raise NotImplementedError("algo: ppo-pure with a recurrent policy and logsumexp_logits_is_v: training through the GRU with the "
                                      "logsumexp value head is not built (use algo: ppo, or a non-recurrent policy)")
        if recurrent:
            self._check_recurrent(n_steps, n_envs, n_minibatch, mini_batch_size)
            # a recurrent minibatch is whole trajectories: the engine's batch capacity must hold one env group x T steps (PPO sizes it
            # from mini_batch_size), and accumulated minibatches stay separate passes
            kwargs = dict(kwargs, merge_accumulation=False)
        # ppo-pure has no feature-sparsity term (agents/ppo_pure.py:149-153 -- fs_coef is stored and never used)
        super().__init__(env, policy, logger, storage, device, n_checkpoints, env_valid, storage_valid, n_steps=n_steps, n_envs=n_envs,
                         epoch=epoch, n_minibatch=n_minibatch, mini_batch_size=mini_batch_size, gamma=gamma, lmbda=lmbda,
                         learning_rate=learning_rate, grad_clip_norm=grad_clip_norm, eps_clip=eps_clip, value_coef=value_coef,
                         entropy_coef=entropy_coef, x_entropy_coef=x_entropy_coef, normalize_adv=normalize_adv,
                         normalize_rew=normalize_rew, use_gae=use_gae, entropy_scaling=entropy_scaling, increasing_lr=increasing_lr,
                         sparsity_coef=sparsity_coef, fs_coef=0., **kwargs)
        self.fs_coef = 0.
        if recurrent:
            if self.coll.active:
                raise NotImplementedError("algo: ppo-pure with a recurrent policy trains the GRU on a single GPU only (world_size must be 1)")
            policy.enable_gru_training()

    @staticmethod
    def rec_plan(n_steps, n_envs, n_minibatch, mini_batch_size):
        """-> (mini_batch_size after the reference's shrink, envs per recurrent minibatch, minibatches per optimizer step):
        agents/ppo_pure.py:110-113 and common/storage.py:94-95."""
        n_total = n_steps * n_envs
        batch_size = n_total // n_minibatch
        mbs = min(mini_batch_size, batch_size)
        per = n_envs // (n_total // mbs)
        return mbs, per, batch_size / mbs

    @classmethod
    def _check_recurrent(cls, n_steps, n_envs, n_minibatch, mini_batch_size):
        mbs, per, _ = cls.rec_plan(n_steps, n_envs, n_minibatch, mini_batch_size)
        if per < 1 or per * n_steps != mbs:
            raise ValueError(f"recurrent ppo-pure: a minibatch is whole trajectories, so mini_batch_size ({mbs} after the shrink to T*E/n_minibatch) "
                             f"must be a multiple of n_steps = {n_steps} that gives at least one env per minibatch (got {per} envs)")

    def optimize(self):
        if not self.policy.is_recurrent():
            summary = super().optimize()                         # the existing minibatch path; fs_coef is 0
        else:
            summary = self._optimize_recurrent()
        return {k: summary[k] for k in ('Loss/pi', 'Loss/v', 'Loss/entropy', 'Loss/x_entropy', 'Loss/total')}

    def _optimize_recurrent(self):
        if self.entropy_scaling == "reward_based":
            mean_rew = np.mean(self.logger.episode_reward_buffer)
            self.entropy_multiplier = 1 - ((mean_rew - self.min_rew) / (self.max_rew - self.min_rew))
        elif self.entropy_scaling == "time_based":
            self.entropy_multiplier = 1 - (self.t / self.total_timesteps)
        batch_size = self.n_steps * self.n_envs // self.n_minibatch
        if batch_size < self.mini_batch_size:
            self.mini_batch_size = batch_size
        grad_accumulation_steps = batch_size / self.mini_batch_size
        eng, hp = self.engine, self._hparams()
        cnt = 1
        for _ in range(self.epoch):
            for envs, h0 in self.storage.recurrent_minibatch_stream(self.mini_batch_size):
                eng.minibatch_rec(envs, h0, len(envs) * self.n_steps, hp)
                if cnt % grad_accumulation_steps == 0:
                    gn = self.optimizer.step(self.grad_clip_norm, want_norm=self.detect_nan)
                    if self.detect_nan and not np.isfinite(gn):
                        raise RuntimeError(f"Found NaN / Inf in the gradient norm of optimizer step {self.optimizer.step_count}: {gn}")
                cnt += 1
        log = eng.loss_log(reset=True)
        if self.detect_nan and not np.isfinite(log[:, :5]).all():
            bad = np.argwhere(~np.isfinite(log[:, :5]))
            raise RuntimeError(f"Found NaN / Inf in the loss terms (minibatch, term) {bad[:8].tolist()} of this update")
        return {'Loss/pi': float(np.mean(-log[:, 0])), 'Loss/v': float(np.mean(-log[:, 1])),
                'Loss/entropy': float(np.mean(log[:, 2])), 'Loss/x_entropy': float(np.mean(log[:, 3])),
                'Loss/total': float(np.mean(log[:, 4]))}
