#!/usr/bin/env python3
"""Policy distillation (reference: distill.py:22-234) on the MI355X engine: a blank student policy explores the env with its OWN actions,
a trained teacher labels every observation the student visited with its normalised logits, and the student is fitted to those labels
with MSELoss and plain Adam over several epochs per exploration (DAgger-style).

    python distill.py --model_file logs/train/coinrun/x/<run>/model_200015872.pth --env_name coinrun --param_name hard-500 --output_dim 64

`--model_file` is the teacher's checkpoint (model_<timesteps>.pth of train.py) and `--teacher_param_name` the hyper-parameter set it was
trained with (default: --param_name); `--param_name` is the STUDENT's set (the reference hard-codes hard-500-impalavqmha, which is not
built here: the default is hard-500) and `--output_dim` narrows its embedder.  Envs, policies and engines come from train.py's own
factories, as in evaluate.py.  Everything expensive runs on the device: the student explores through PPO's own collector into its
engine's ring (T = explore_size // n_envs steps: env groups and the serial vector envs work unchanged), the teacher -- a second engine
context whose ring holds the validation rollout it acted itself, max(1, explore_size // 32 // n_envs) steps -- labels the student's
ring in place (mi_distill_label), every batch is one mi_distill_minibatch + mi_optimizer_step_eps (eps = 1e-8, torch's default, no
gradient clipping), and the validation loss is one forward-only mi_distill_loss.  The value head takes no part in the loss: fc_value
never changes and the checkpoint's optimizer state has no entries for it, as in the reference (its .grad is None there).

Kept from the reference: its flags with their defaults, one permutation of the rows per exploration, contiguous batches in the same
order every epoch with the tail shorter than a batch dropped, `Loss` = the mean batch loss of the LAST epoch, `Valid_Loss` after the
last epoch only, log-append.csv with the columns Exploration, Epoch, Loss, Valid_Loss, Mean_Reward (Mean_Reward = mean(rew[done]) of
the exploration), a checkpoint {model_state_dict, optimizer_state_dict} model_<n>.pth when n > (checkpoints so far + 1) * (n_explore //
num_checkpoints).

Different on purpose:
  * Exploration rows.  The reference's collect_obs stores explore_size + n_envs - 1 rows: it duplicates the first block, drops one
    single row ([1:]) and starts every exploration from the stale first observation.  Here an exploration is the student's ordinary
    T x E ring, and the env carries on where the previous exploration left it.
  * Labelling batch.  predict_in_batches drops a tail shorter than 256 rows, so the last targets are missing there; here every row is
    labelled.
  * CSV.  perf_dict exists in the reference only under --use_wandb, and writer.writerow(log) writes the DataFrame's column names; here
    the values row is always written.
  * A last checkpoint model_<n_explore>.pth is written when the run ends (the reference's condition never fires for the final
    exploration, so its fitted student is lost unless num_checkpoints is large).
  * `--device` defaults to gpu and cpu is refused (there is no CPU fallback); the permutation comes from a generator seeded with --seed.
  * The reference's __main__ runs the distillation twice with a hard-coded teacher directory; here it runs once, on --model_file.
From Python: distill(args, logdir_trained=None) as in the reference (logdir_trained: a run directory whose newest model_<n>.pth is the
teacher when --model_file is not given), or Distiller(args) to drive the explorations one by one (explore(n), finish(), close()).
Refused by name before any engine exists: recurrent: True on either side, WORLD_SIZE > 1, --device cpu, logsumexp_logits_is_v on the
student, student and teacher with different observation shapes or action counts."""
import argparse
import csv
import os
import random
import re
import time

import numpy as np

COLUMNS = ("Exploration", "Epoch", "Loss", "Valid_Loss", "Mean_Reward")
ADAM_EPS = 1e-8                        # torch.optim.Adam's default (distill.py:165 passes lr only)
NO_VALUE_STATE = ("fc_value.weight", "fc_value.bias")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    # ---- the reference's flags and defaults (distill.py:243-262; --device: see the module docstring)
    p.add_argument('--start_level', type=int, default=0, help='start-level for environment')
    p.add_argument('--num_levels', type=int, default=500, help='number of training levels for environment')
    p.add_argument('--distribution_mode', type=str, default='easy', help='distribution mode for environment')
    p.add_argument('--device', type=str, default='gpu')
    p.add_argument('--gpu_device', type=int, default=0)
    p.add_argument('--seed', type=int, default=random.randint(0, 9999), help='Random generator seed')
    p.add_argument('--num_checkpoints', type=int, default=1, help='number of checkpoints to store')
    p.add_argument('--use_wandb', action="store_true")
    p.add_argument('--mirror_env', action="store_true", default=False)
    p.add_argument('--wandb_tags', type=str, nargs='+')
    p.add_argument('--lr', type=float, default=1e-4, help='learning rate')
    p.add_argument('--batch_size', type=int, default=8192, help='batch size')
    p.add_argument('--nb_epoch', type=int, default=10, help='number of epochs per exploration')
    p.add_argument('--explore_size', type=int, default=256 * 256, help='size of each exploration')
    p.add_argument('--n_explore', type=int, default=300, help='number of explorations')
    p.add_argument('--num_threads', type=int, default=8)
    # ---- new flags
    p.add_argument('--env_name', type=str, default='coinrun')
    p.add_argument('--param_name', type=str, default='hard-500', help="the STUDENT's hyper-parameter set")
    p.add_argument('--model_file', type=str, default=None, help="the teacher's checkpoint (model_<timesteps>.pth of train.py); required")
    p.add_argument('--teacher_param_name', type=str, default=None, help="the set the teacher was trained with (default: --param_name)")
    p.add_argument('--precision', type=str, default=None, choices=['fp32', 'bf16'], help="IMPALA activation storage of both engines (default: the sets')")
    p.add_argument('--n_envs', type=int, default=None, help="envs of the exploration and of the validation rollout (default: the student set's)")
    p.add_argument('--output_dim', type=int, default=None, help="the student's embedder width (default: the student set's)")
    return p.parse_args(argv)


def newest_checkpoint(logdir):
    """The reference's load_policy rule (distill.py:36-39): model_<n>.pth with the largest n in `logdir`."""
    found = [(int(m.group(1)), f) for f in os.listdir(logdir) for m in [re.fullmatch(r"model_(\d+)\.pth", f)] if m]
    if not found:
        raise FileNotFoundError(f"{logdir}: no model_<timesteps>.pth in this directory")
    return os.path.join(logdir, max(found)[1])


def check_args(args, logdir_trained=None):
    """Everything that can be refused before an env or a GPU is touched -> (student set, teacher set, env name, teacher checkpoint)."""
    import train
    if args.device != 'gpu':
        raise NotImplementedError(f"--device must be 'gpu', not {args.device}: distill.py runs on the MI355X engine, there is no CPU fallback")
    if int(os.environ.get("WORLD_SIZE", 1)) > 1:
        raise NotImplementedError(f"distill.py runs on a single GPU: WORLD_SIZE = {os.environ['WORLD_SIZE']} is not supported")
    model_file = args.model_file
    if model_file is None and logdir_trained is not None:
        model_file = newest_checkpoint(logdir_trained)
    if not model_file:
        raise ValueError("--model_file is required: the teacher is the policy of a checkpoint (model_<timesteps>.pth of train.py)")
    if not os.path.isfile(model_file):
        raise FileNotFoundError(f"--model_file {model_file}: no such file")
    hp_s = train.get_hyperparams(args.param_name)
    hp_t = train.get_hyperparams(args.teacher_param_name or args.param_name)
    for k, v in (("n_envs", args.n_envs), ("precision", args.precision)):
        if v is not None:
            hp_s[k] = hp_t[k] = v
    if args.output_dim is not None:
        hp_s["output_dim"] = args.output_dim
    for who, hp in (("student", hp_s), ("teacher", hp_t)):
        if hp.get("recurrent", False):
            raise NotImplementedError(f"recurrent: True on the {who} is not supported: the distillation passes run no GRU")
    if hp_s.get("logsumexp_logits_is_v", False):
        raise NotImplementedError("logsumexp_logits_is_v on the student is not supported: its value IS the logits the loss fits "
                                  "(the teacher may use it)")
    kind = lambda hp: "frames" if hp.get("architecture", "impala") == "impala" else "rows"
    if kind(hp_s) != kind(hp_t):
        raise NotImplementedError(f"student and teacher read different observation shapes: architecture {hp_s.get('architecture', 'impala')} "
                                  f"({kind(hp_s)}) against {hp_t.get('architecture', 'impala')} ({kind(hp_t)})")
    if args.explore_size < hp_s.get("n_envs", 256):
        raise ValueError(f"--explore_size {args.explore_size} is smaller than n_envs = {hp_s.get('n_envs', 256)}: an exploration is at least one step of every env")
    if args.batch_size < 1 or args.nb_epoch < 1 or args.n_explore < 1 or args.num_checkpoints < 1:
        raise ValueError("--batch_size, --nb_epoch, --n_explore and --num_checkpoints must be at least 1")
    return hp_s, hp_t, hp_s.get("env_name", args.env_name), model_file


def check_pair(env, teacher_state):
    """Student and teacher act in the same env: the teacher's checkpoint must name the env's actions and read its observations."""
    A, obs_shape = env.action_space.n, tuple(env.observation_space.shape)
    A_t = int(teacher_state["fc_policy.weight"].shape[0])
    if A_t != A:
        raise NotImplementedError(f"student and teacher have different action counts: the env (and so the student) has {A}, the teacher's checkpoint {A_t}")
    first = next(iter(teacher_state.values()))              # the embedder's first weight: (cout, cin, 3, 3) or (width, obs_dim)
    if int(first.shape[1]) != obs_shape[0]:
        raise NotImplementedError(f"student and teacher read different observation shapes: the env's is {obs_shape}, the teacher's first layer "
                                  f"takes {int(first.shape[1])} inputs")


def _env_args(args):
    """train.py's flag set at its defaults with this script's flags on top: what train.make_env reads."""
    import train
    t = train.add_training_args(argparse.ArgumentParser()).parse_args([])
    for k in ("env_name", "start_level", "num_levels", "distribution_mode", "num_threads", "mirror_env", "seed", "gpu_device"):
        setattr(t, k, getattr(args, k))
    t.use_valid_env = False            # (the automatic env-group count: each of the two rollouts here runs on its own)
    return t


def predict(policy, obs, hidden_state, done, with_grad=False):
    """distill.py:22-32: (the policy's normalised logits, one sampled action per row).  The forward pass runs on the policy's engine, so
    there is no autograd graph whatever with_grad says: the fit differentiates on the device (mi_distill_minibatch)."""
    dist, _, _ = policy(obs, hidden_state, hidden_state)
    return dist.logits, dist.sample().cpu().numpy()


def load_policy(model_file, device, env, hp):
    """distill.py:35-65, the part that is the teacher: the set's policy with the checkpoint's weights, in eval mode.  Refuses a checkpoint
    that does not fit the env (check_pair) before anything is built."""
    import torch
    import train
    state = torch.load(model_file, map_location="cpu", weights_only=True)["model_state_dict"]
    check_pair(env, state)
    _, _, policy = train.initialize_model(device, env, hp)
    policy.load_state_dict(state)
    policy.eval()
    return policy


def _make_agent(env, policy, obs_shape, hp, n_steps, max_batch, device, seed):
    """PPO's collector, engine and optimizer plumbing around `policy`: T = n_steps, one engine whose passes carry max_batch rows."""
    from agents.ppo import PPO
    from common.logger import Logger
    from common.storage import Storage
    n_envs = hp["n_envs"]
    hp = dict(hp, n_steps=n_steps, n_minibatch=1, mini_batch_size=max(1, min(max_batch, n_steps * n_envs)), merge_accumulation=False)
    for k in ("fused_update", "resident_rollout", "seed"):
        hp.pop(k, None)
    storage = Storage(obs_shape, policy.embedder.output_dim, n_steps, n_envs, device)
    return PPO(env, policy, Logger(n_envs, None), storage, device, 0, seed=seed, **hp)


class _Lane:
    """One env with the agent that acts in it and where its rollout stands."""
    def __init__(self, agent, env):
        self.agent, self.env = agent, env
        self.obs = env.reset()
        self.hidden_state = np.zeros((agent.n_envs, agent.storage.hidden_state_size))
        self.done = np.zeros(agent.n_envs)


def collect_obs(lane):
    """distill.py:68-88: the lane's policy acts for T steps of every env, through PPO's collector, into its engine's ring (the
    observations stay on the device) -> (rew (T, E), done (T, E)) as the host mirrors hold them."""
    a = lane.agent
    a._iter += 1
    lane.obs, lane.hidden_state, lane.done = a._collect(lane.env, a.engine, a.storage, lane.obs, lane.hidden_state, lane.done)
    return np.array(a.storage._rew), np.array(a.storage._done)


def collect_validation_data(teacher_lane):
    """distill.py:91-103: the TEACHER acts in the validation env, and its ring -- observations and its own normalised logits as
    targets -- is the validation set from then on."""
    collect_obs(teacher_lane)
    eng = teacher_lane.agent.engine
    eng.distill_label(eng)
    return eng


def validate(student_engine, valid_engine):
    """distill.py:106-113: MSELoss(student(valid_X).logits, valid_Y_gold), forward only (mi_distill_loss)."""
    return student_engine.distill_loss(valid_engine)


class Distiller:
    """The run of distill(): construction builds the envs, both policies and both engines and collects the validation set; explore(n)
    is one exploration (rollout, labels, fit, validation loss, the CSV row, a checkpoint when one is due); finish() writes the last
    checkpoint; close() releases envs and engines.  student / teacher are PPO agents (their .engine, .policy, .storage are the parts)."""

    def __init__(self, args, logdir_trained=None):
        hp_s, hp_t, env_name, model_file = check_args(args, logdir_trained)
        import torch
        import train
        from mi355.optim import DeviceAdam
        train.set_global_seeds(args.seed)
        self.args, self.hp = args, hp_s
        device = torch.device("cuda", args.gpu_device)
        n_envs = hp_s["n_envs"] = hp_t["n_envs"] = hp_s.get("n_envs", 256)
        T = args.explore_size // n_envs
        T_valid = max(1, args.explore_size // 32 // n_envs)
        targs = _env_args(args)
        A_hint = 9 if hp_s.get("architecture", "impala") == "impala" else 2          # (the synthetic env's action count, as train.py)
        self.env = train.make_env(env_name, n_envs, args.seed, A_hint, targs, hp_s)
        self.env_valid = train.make_env(env_name, n_envs, args.seed + 1, A_hint, targs, hp_t, is_valid=True)
        print("Loading the teacher from %s" % model_file)
        teacher_policy = load_policy(model_file, device, self.env_valid, hp_t)     # (refuses a mismatch before any engine exists)
        _, obs_shape, student_policy = train.initialize_model(device, self.env, hp_s)
        self.student = _make_agent(self.env, student_policy, obs_shape, hp_s, T, args.batch_size, device, args.seed)
        self.teacher = _make_agent(self.env_valid, teacher_policy, obs_shape, hp_t, T_valid, args.batch_size, device, args.seed + 1)
        self.student.optimizer = DeviceAdam(student_policy, self.student.engine, args.lr, eps=ADAM_EPS, stateless=NO_VALUE_STATE)
        self.logdir = os.path.join('logs', 'distill', env_name, 'distill', time.strftime("%Y-%m-%d__%H-%M-%S") + f'__seed_{args.seed}')
        os.makedirs(self.logdir, exist_ok=True)
        print(f'Logging to {self.logdir}')
        np.save(os.path.join(self.logdir, "hyperparameters.npy"), hp_s)
        self.wandb = None
        if args.use_wandb:
            import wandb
            cfg = dict(vars(args)); cfg.update(hp_s)
            wandb.init(project="distill", config=cfg, tags=args.wandb_tags, resume="allow",
                       name=f"{hp_s.get('architecture', 'impala')}-distill-{np.random.randint(1e5)}")
            self.wandb = wandb
        collect_validation_data(_Lane(self.teacher, self.env_valid))
        self.lane = _Lane(self.student, self.env)
        self.rng = np.random.default_rng(args.seed)
        self.n_rows = T * n_envs
        self.batch = min(args.batch_size, self.n_rows)
        self.save_every = args.n_explore // args.num_checkpoints
        self.checkpoint_cnt, self.saved = 0, []

    def _save(self, n):
        import torch
        path = os.path.join(self.logdir, f"model_{n}.pth")
        torch.save({'model_state_dict': self.student.policy.state_dict(), 'optimizer_state_dict': self.student.optimizer.state_dict()}, path)
        self.saved.append(path)

    def explore(self, n_explores):
        args, eng, teng = self.args, self.student.engine, self.teacher.engine
        rew, done = collect_obs(self.lane)
        eng.distill_label(teng)
        perm = self.rng.permutation(self.n_rows)
        for epoch in range(args.nb_epoch):
            for i in range(self.n_rows // self.batch):
                eng.distill_minibatch(perm[i * self.batch:(i + 1) * self.batch], self.batch)
                self.student.optimizer.step_eps()
            epoch_loss = float(np.mean(eng.loss_log(reset=True)[:, 0], dtype=np.float64))      # (the last epoch's stays: distill.py:178-205)
        valid_loss = validate(eng, teng)
        mean_rew = float(np.mean(rew[done > 0])) if (done > 0).any() else float("nan")
        print(f'Epoch {epoch}: total train loss: {epoch_loss:.5f}, valid loss: {valid_loss:.5f}')
        perf = {"Exploration": n_explores, "Epoch": epoch, "Loss": epoch_loss, "Valid_Loss": valid_loss, "Mean_Reward": mean_rew}
        if self.wandb is not None:
            self.wandb.log(perf)
        with open(os.path.join(self.logdir, 'log-append.csv'), 'a') as f:
            writer = csv.writer(f)
            if f.tell() == 0:
                writer.writerow(COLUMNS)
            writer.writerow([perf[k] for k in COLUMNS])
        if n_explores > ((self.checkpoint_cnt + 1) * self.save_every):
            print("Saving model.")
            self._save(n_explores)
            self.checkpoint_cnt += 1
        return perf

    def finish(self):
        self._save(self.args.n_explore)
        if self.wandb is not None:
            self.wandb.finish()
        print(f"Wrote {os.path.join(self.logdir, 'log-append.csv')} and {len(self.saved)} checkpoint(s), the last {self.saved[-1]}")

    def close(self):
        for e in (self.env, self.env_valid):
            e.close()
        for a in (self.student, self.teacher):
            for e in (a.engine, a.engine_valid):
                if e is not None:
                    e.close()


def distill(args, logdir_trained=None):
    """distill.py:128-234 -> (the last exploration's train loss, its mean reward)."""
    d = Distiller(args, logdir_trained)
    try:
        for n_explores in range(args.n_explore):
            perf = d.explore(n_explores)
        d.finish()
    finally:
        d.close()
    return perf["Loss"], perf["Mean_Reward"]


if __name__ == "__main__":
    distill(parse_args())
