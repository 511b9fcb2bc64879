"""Device-side TD3 training loop: BASELINE.json config 5 assembled end to end (e, f1, f2).

The batched counterpart of the reference's `Trainer.warmup` / `Trainer.train` (reference src/trainer.py:90-286): every
time step is ONE engine launch + ONE batched SET forward for all environments of this rank (rollout.py `Rollout`), the
per-environment bookkeeping of the reference loop runs as tensor ops (`RoundCollector`), transitions travel to the
learner rank in one gather and land in device-resident per-morphology ring buffers (`TransitionSink`,
`DeviceReplayBuffer`), and when every environment of every rank has finished its first episode of the round the learner
runs the reference's update schedule -- `per_morph_iter = sum(episode_timesteps) // num_envs` TD3 updates for each
morphology in turn (trainer.py:244-251) -- through `td3.Agent`, then all ranks reset and start the next round.

Multi-GPU: environments are sharded by rank (no collective in the step); the learner (rank `dst`) owns buffers and
optimizers; after its updates the actor's parameters are broadcast (one flat 18.9 MB `broadcast`) so that every
rank's rollout uses the new policy.  Single rank: no process group needed.
"""
import numpy as np
import torch

from . import graph as G
from .replay import DeviceReplayBuffer
from .rollout import TRAV, Rollout, TransitionSink
from .td3 import Agent, default_train_args


class DeviceTrainer(object):
    def __init__(self, env_names, envs_per_morph, args=None, seed=0, device="cuda:0", max_buffer_size=1000000,
                 batch_size=None, dst=0, graph_updates=False, tune_gemms=False, rollout=None, lag_flag=True, device_sampler=False,
                 device_noise=False, graph_hip_kernels=False, store_all_episodes=False, true_next_obs=False, **env_kw):
        """graph_updates: replay the TD3 update from hipGraphs (td3.GraphedUpdates; td3.GraphedMlpUpdates
        for an `mlp` agent); graph_hip_kernels (with graph_updates; ignored for `mlp`): td3.GraphedUpdates(hip_kernels=True) -- a
        swat or smp agent keeps its HIP target chain and its `*_train_kernels` switch under the graphs instead of being switched
        to plain PyTorch; tune_gemms: let PyTorch's TunableOp pick
        the rocBLAS / hipBLASLt algorithm per GEMM shape on first use (the defaults choose 256 x 256 tiles for the 700-row
        weight-gradient GEMMs of a 100-row update: 50 -> 38 ms per update, round 1).  batch_size: rows per TD3 update, default
        args.agent_batch_size = 256 (the reference's trainer.py:289-291).  lag_flag (GPU ranks): the round-finished flag is read one
        step late instead of synchronising every collection step (rollout.TransitionSink); False = the immediate flag.
        device_sampler (learner): every update of update_after_round takes its batch and its target-policy noise from ONE library call
        (replay.DeviceReplayBuffer.sample_into, include/sgrl_replay.h) with seed = `seed` and draw = a counter incremented once per
        update, instead of sample(generator=self.gen) and normal_().  Off by default: it changes which rows a seeded run samples,
        and the learning curves have not been re-run on the new stream.  A reference-format snapshot
        (snapshot.py) has no field for the draw counter: assigning tot_env_steps (how a run resumed from one restores its count)
        restarts it at draw = tot_env_steps.  A checkpoint (save_checkpoint / load_checkpoint) carries the counter itself.
        device_noise (the training rollout only; evaluation never adds noise): the exploration noise and the warm-up actions of
        collect_step come from ONE library call each (Rollout.explore_into / random_actions, include/sgrl_explore.h) as a function of
        (`seed`, the rollout's noise_step, global environment number, slot), instead of torch.randn / uniform_ on the rollout's
        generator.  Off by default for the same reason: it changes what a seeded run explores, and the learning curves have not
        been re-run on it.  noise_step follows the same rule as the draw counter: a snapshot has no field for it and assigning
        tot_env_steps sets the rollout's noise_step to the restored value; a checkpoint carries it.
        store_all_episodes: the replay rings receive every row of every episode of a round, not only each environment's first episode
        (rollout.RoundCollector store_all; DESIGN section 5: at config 5 about 70 of 250 simulated steps per environment are kept
        otherwise).  Round end, updates per morphology and the train statistics are those of the default; tot_env_steps counts what is
        stored, so it grows faster.  true_next_obs: the `next_obs` stored for the last transition of an episode is the observation the
        episode ended on, not the next episode's reset observation (which the reference stores, subproc_vec_env.py:12-15, and which
        a time-limit cut with done_bool = 0 bootstraps from): collect_step steps with auto_reset=False, pushes, then restarts the
        finished environments (Rollout.reset_where) -- one more launch per launch group, no synchronisation; an injected rollout
        driver without reset_where is a ValueError.  Both are independent, constructor arguments like device_noise (a checkpoint is
        taken at a round end, where the collector's state is fresh, and carries neither), and off by default: they change what a
        seeded run learns from, and NO learning curve has been run with either."""
        import torch.distributed as dist
        self.dist = dist
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.dst = dst
        self.args = args if args is not None else default_train_args()
        self.env_names = list(env_names)
        self.seed = int(seed)
        self.eval_rollouts = {}      # tuple of names -> (settings, Rollout, DeviceEvaluator) of evaluate()
        self.demo_rollouts = {}      # tuple of names -> (settings, Rollout, max_episode_steps) of save_video_demo()
        if getattr(self.args, "actor_type", "set") == "mlp":
            if getattr(self.args, "mlp_num_limbs", None) is None and getattr(self.args, "graphs", None) is None:
                # the reference sizes the network for the LAST training morphology (MLPActor.py:42)
                from .vec_env import resolve_models
                xml = env_kw.get("xml_paths")
                self.args.mlp_num_limbs = resolve_models(self.env_names[-1:], None if xml is None else xml[-1:])[0].num_limbs
        if getattr(self.args, "seed", None) is None:
            self.args.seed = int(seed)        # what the agent seeds its dropout masks with (td3.Agent.dropout_seed)
        torch.manual_seed(seed)               # same initial weights on every rank
        self.agent = Agent(self.args, device=device)
        if tune_gemms:
            torch.cuda.tunable.enable(True)
        # `rollout`: a ready-made driver with the Rollout surface (env, graph_dicts, reset / step / random_actions / policy_forward /
        # add_exploration_noise, actions) or a callable (policy, rank) -> driver; the engine-backed Rollout by default.  The
        # multi-rank control flow of this class (round schedule, counters, actor broadcast) is covered on CPU ranks by
        # tests/test_trainer_multirank.py with a scripted driver injected here -- the product itself never builds one.
        if rollout is not None:
            self.ro = rollout(self.agent.actor, self.rank) if callable(rollout) else rollout
        else:
            # the actor's parameters change only in update_after_round (updates on the learner, the broadcast on the others): the
            # rollout holds its packed weights across a collection round
            self.ro = Rollout(self.env_names, envs_per_morph, policy=self.agent.actor, seed=seed, device=device, rank=self.rank,
                              max_episode_steps=self.args.max_episode_steps, hold_weights=True, device_noise=device_noise, **env_kw)
        # an injected driver without explore_into keeps the tensor-op path
        self.device_noise = bool(device_noise) and hasattr(self.ro, "explore_into")
        self.store_all_episodes = bool(store_all_episodes)
        self.true_next_obs = bool(true_next_obs)
        if self.true_next_obs and not hasattr(self.ro, "reset_where"):
            raise ValueError("true_next_obs=True needs a rollout driver with reset_where(mask) and step(actions, auto_reset=False); "
                             "%s has none" % type(self.ro).__name__)
        env = self.ro.env
        self.device = env.device
        self.graph_dicts = self.ro.graph_dicts
        self.is_learner = self.rank == dst
        # rows per TD3 update: the reference's trainer samples `agent_batch_size` (configs/default.py:61 = 256, main.py:164-171,
        # trainer.py:289-291); args.batch_size (100) is only the policies' unused constructor argument
        self.batch_size = int(batch_size if batch_size is not None else getattr(self.args, "agent_batch_size", 256))
        self.buffers = None
        if self.is_learner:     # one ring buffer per morphology (reference main.py:141-155), rows cut to 41 L / 3 L
            self.buffers = [DeviceReplayBuffer(41 * L, 3 * L, max_buffer_size, device=self.device) for L in env.num_limbs]
        self.sink = TransitionSink(env.env_morph, env.num_limbs, env.obs_max_len, env.action_max_len,
                                   max_episode_steps=self.args.max_episode_steps, device=self.device, buffers=self.buffers,
                                   dst=dst, lag_flag=lag_flag, store_all=self.store_all_episodes)
        self.prev_obs = torch.zeros_like(env.obs)
        self.num_envs_global = env.num_envs * self.world
        self._updates = 0            # TD3 updates so far (the reference adds them to tot_env_steps: trainer.py:250)
        self._tot_synced = 0         # non-learner ranks: the learner's count as of the last round end
        self._tot_base = 0           # count restored from a snapshot (tot_env_steps setter)
        self.rounds = 0
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed) * 7919 + 13)
        self.device_sampler = bool(device_sampler) and self.is_learner
        self.sample_seed = int(seed)
        self.draw = 0                # draw number of the next update's batch (device_sampler)
        self._eager_slots = {}       # morphology -> (batch tensors, noise) of the eager device-sampled updates
        self.last_losses = {}
        self.graphed = None
        self._graphed_lazy = False   # td3.GraphedMlpUpdates: needs no warm() before its first update
        if graph_updates and self.is_learner:
            from .td3 import GraphedMlpUpdates, GraphedUpdates
            # an mlp agent's update is entirely library launches: one shared slot, no warm-up of its own (the first update of each
            # kind runs eagerly inside the ordinary schedule), so the (morphology, it, draw) sequence is the eager trainer's
            mlp = getattr(self.args, "actor_type", "set") == "mlp"
            self.graphed = GraphedMlpUpdates(self.agent, self.batch_size) if mlp else \
                GraphedUpdates(self.agent, self.batch_size, hip_kernels=bool(graph_hip_kernels))
            self._graphed_lazy = mlp
        self._steps_in_round = 0     # collect_step calls since the last begin_round (a checkpoint is taken at 0 only)
        self.begin_round()

    @property
    def tot_env_steps(self):
        """Stored transitions + updates (trainer.py:229, 250).  The learner's count: reading it there folds the device-side
        ingest counters in (one synchronisation -- nothing in the per-step path reads it); the other ranks hold the value the
        learner broadcast at the last round end."""
        if self.is_learner:
            return self._tot_base + self.sink.stored + self._updates
        return self._tot_synced

    @tot_env_steps.setter
    def tot_env_steps(self, v):
        """Resume from a snapshot (snapshot.load_snapshot returns the count, reference common/trainer.py:296-322): the restored
        value becomes the base the live counters are added to.  The two counter-RNG positions a snapshot has no field for restart
        at the restored value; load_checkpoint, whose files carry them, assigns the saved positions after this rule."""
        if self.is_learner:
            self._tot_base = int(v) - (self.sink.stored + self._updates)
        self._tot_synced = int(v)
        self.draw = int(v)           # a snapshot has no draw counter: a run resumed from one starts at draw = tot_env_steps
        if hasattr(self.ro, "noise_step"):
            self.ro.noise_step = int(v)      # ... and no exploration step number: same rule

    def sync_step_count(self):
        """Every rank learns the learner's count (called at the round ends and after the warm-up: rank-local logic that reads the
        count before the first update then agrees with the learner)."""
        if self.world > 1:
            t = torch.tensor([self.tot_env_steps if self.is_learner else 0], dtype=torch.long, device=self.device)
            self.dist.broadcast(t, src=self.dst)
            self._tot_synced = int(t.item())

    # ---- collection ----------------------------------------------------------------------------------
    def begin_round(self):
        """`obs_list = envs.reset()` + fresh done / timestep lists (trainer.py:155-160, 268-275)."""
        self.ro.reset()
        self.sink.begin_round()
        self._steps_in_round = 0

    def collect_step(self, random_actions=False):
        """One time step of every environment + replay push.  Returns True when the collection round is complete."""
        env = self.ro.env
        self._steps_in_round += 1
        self.prev_obs.copy_(env.obs)
        if random_actions:                       # Trainer.warmup: uniform actions (trainer.py:95-102)
            a = self.ro.random_actions()
        else:                                    # select_action + exploration noise (trainer.py:173-196)
            a = self.ro.policy_forward(self.prev_obs)
            if self.device_noise and self.args.expl_noise != 0:
                a = self.ro.explore_into(a, self.args.expl_noise)      # one launch, straight into ro.actions
            else:
                if self.args.expl_noise != 0:
                    a = self.ro.add_exploration_noise(a, self.args.expl_noise)
                self.ro.actions.copy_(a)
                a = self.ro.actions
        if self.true_next_obs:
            # the packer copies the observation every episode really ended on; only then do the finished environments start anew
            obs, rew, done, _ = self.ro.step(a, auto_reset=False)
            finished = self.sink.push(self.prev_obs, a, obs, rew, done)
            self.ro.reset_where(done)
            return finished
        obs, rew, done, _ = self.ro.step(a)
        return self.sink.push(self.prev_obs, a, obs, rew, done)    # the round-finished flag (GPU: read one step late, no stall)

    def warmup(self, timesteps):
        """reference Trainer.warmup (trainer.py:90-138): `timesteps` batched steps of uniform random actions; finished
        rounds only reset the environments (no updates)."""
        for _ in range(int(timesteps)):
            if self.collect_step(random_actions=True):
                self.begin_round()
        self.sync_step_count()

    # ---- learning --------------------------------------------------------------------------------------
    def update_after_round(self, max_iters=None):
        """The update schedule of trainer.py:240-251 on the learner, then the weight broadcast.  Returns per_morph_iter."""
        per_morph_iter = self.sink.total_episode_timesteps() // self.num_envs_global
        if max_iters is not None:
            per_morph_iter = min(per_morph_iter, int(max_iters))
        if self.is_learner:
            self.agent.models2train()
            start = [0] * len(self.env_names)
            if self.graphed is not None and not self._graphed_lazy:
                # every morphology runs eagerly before any graph bakes a pointer (capture protocol of td3.GraphedUpdates): the
                # FIRST iterations of its schedule serve as those eager runs -- same number of updates as the reference's
                # schedule, in the first such round the morphologies' first two iterations come before everybody's remaining ones
                for k in range(len(self.env_names)):
                    if k not in self.graphed.warmed and self.buffers[k].max_sample_size >= self.batch_size and per_morph_iter > 0:
                        n = min(2, per_morph_iter)
                        if self.device_sampler:
                            outs = self.graphed.warm_from(k, self.graph_dicts[k], self.ro.env.num_limbs[k], self.buffers[k],
                                                          self.sample_seed, self.draw, iters=n)
                            self.draw += n
                        else:
                            outs = self.graphed.warm(k, self.graph_dicts[k], self.ro.env.num_limbs[k],
                                                     lambda k=k: self.buffers[k].sample(self.batch_size, generator=self.gen), iters=n)
                        self.last_losses[self.env_names[k]] = outs[-1]
                        start[k] = n
                        self._updates += n
            for k, name in enumerate(self.env_names):
                self.agent.change_morphology(self.graph_dicts[k])
                for it in range(start[k], per_morph_iter):
                    if self.device_sampler:
                        self.last_losses[name] = self._device_sampled_update(k, it)
                        self._updates += 1
                        continue
                    batch = self.buffers[k].sample(self.batch_size, generator=self.gen)
                    if self.graphed is not None and (self._graphed_lazy or k in self.graphed.warmed):
                        self.last_losses[name] = self.graphed.update(k, self.graph_dicts[k], self.ro.env.num_limbs[k], batch, it)
                    else:
                        self.last_losses[name] = self.agent.update(batch, it)
                    self._updates += 1                         # the reference counts updates too (trainer.py:250)
            self.agent.models2eval()
        self.sync_step_count()               # every rank reports the learner's step count (checkpoints, stopping rule)
        self.broadcast_actor()
        if hasattr(self.ro, "weights_changed"):
            self.ro.weights_changed()          # with the weights every rank rolls out next
        self.rounds += 1
        return per_morph_iter

    def _device_sampled_update(self, k, it):
        """One update of morphology k on a batch drawn by sample_into with (sample_seed, draw); the counter moves once per update."""
        draw, buf, L = self.draw, self.buffers[k], self.ro.env.num_limbs[k]
        self.draw += 1
        if self.graphed is not None and (self._graphed_lazy or k in self.graphed.warmed):
            return self.graphed.update_from(k, self.graph_dicts[k], L, buf, it, self.sample_seed, draw)
        sl = self._eager_slots.get(k)
        if sl is None:               # per-morphology tensors kept by the trainer: nothing is allocated per update
            z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.device)
            B = self.batch_size
            sl = self._eager_slots[k] = ({"obs": z(B, 41 * L), "action": z(B, 3 * L), "next_obs": z(B, 41 * L), "reward": z(B, 1),
                                          "done": z(B, 1)}, z(B, 3 * L))
        batch, noise = sl
        n = buf.sample_into(batch, self.batch_size, self.sample_seed, draw, noise=noise, noise_std=self.args.policy_noise)
        if n < self.batch_size:      # buffer not yet filled: the k rows there are (views of the kept tensors)
            batch, noise = {name: t[:n] for name, t in batch.items()}, noise[:n]
        return self.agent.update(batch, it, noise=noise)

    def broadcast_actor(self):
        if self.world == 1:
            return
        params = list(self.agent.actor.parameters())
        flat = torch.cat([p.data.reshape(-1) for p in params])
        self.dist.broadcast(flat, src=self.dst)
        if not self.is_learner:
            off = 0
            for p in params:
                n = p.numel()
                p.data.copy_(flat[off:off + n].view_as(p))     # in place: the HIP actor reads the live storage
                off += n

    # ---- evaluation ------------------------------------------------------------------------------------
    def evaluate(self, num_eval_trajectories=10, max_trajectory_length=1000, env_names=None, **env_kw):
        """Periodic evaluation of the deterministic policy (reference common/trainer.py:80-146), all trajectories in one batched pass
        on the device (evaluate.DeviceEvaluator): `num_eval_trajectories` environments per morphology, trajectory t = environment t of
        every morphology.  env_names=None: the training morphologies; any other list: zero-shot evaluation on those (xml_paths= and
        the other environment keywords pass through `env_kw`).  The environments are an evaluation Rollout of this trainer's own,
        built on first use and kept per tuple of names: the training environments, their observations and the round's counters are
        never touched.  That Rollout shares `self.agent.actor` and reads its live weights on every forward (it holds no packed copy),
        so it always evaluates the current policy.  Returns the DeviceEvaluator dictionary: `performance/eval_return`,
        `performance/eval_length` and the same two per morphology name.  RANK-LOCAL: no collective is issued -- every rank that calls
        it evaluates its own copy of the actor on its own device, and a rank may call it alone."""
        from .evaluate import DeviceEvaluator
        names = tuple(self.env_names if env_names is None else env_names)
        n_traj = int(num_eval_trajectories)
        settings = (n_traj, repr(sorted(env_kw.items())))      # what the cached environments were built with
        entry = self.eval_rollouts.get(names)
        if entry is None or entry[0] != settings:
            kw = dict(max_episode_steps=self.args.max_episode_steps)
            kw.update(env_kw)
            ro = Rollout(list(names), n_traj, policy=self.agent.actor, seed=self.seed + 7001, device=self.device, rank=self.rank,
                         hold_weights=False, **kw)
            ev = DeviceEvaluator(ro, num_eval_trajectories=n_traj, max_trajectory_length=max_trajectory_length,
                                 max_episode_steps=kw["max_episode_steps"])
            entry = self.eval_rollouts[names] = (settings, ro, ev)
        entry[2].max_trajectory_length = int(max_trajectory_length)
        return entry[2].evaluate()

    def save_video_demo(self, out_dir, width=500, height=500, max_trajectory_length=1000, env_names=None, **env_kw):
        """The reference's `save_video_demo` (common/trainer.py:149-258): roll the deterministic policy out in ONE environment per
        morphology until every one has finished its first episode (or `max_trajectory_length` steps) and write one `<i>.gif` per
        environment into `out_dir`, every frame rendered on the device (evaluate.VideoDemo, evaluate.write_demo_gifs).  Built like
        evaluate(): the environments are a Rollout of this trainer's own, kept per tuple of names, that shares `self.agent.actor` and
        reads its live weights; the training environments and the round's counters are never touched; env_names: zero-shot demos on
        held-out morphologies; RANK-LOCAL (no collective).  Returns the list of written paths."""
        from .evaluate import VideoDemo, write_demo_gifs
        names = tuple(self.env_names if env_names is None else env_names)
        settings = repr(sorted(env_kw.items()))
        entry = self.demo_rollouts.get(names)
        if entry is None or entry[0] != settings:
            kw = dict(max_episode_steps=self.args.max_episode_steps)
            kw.update(env_kw)
            ro = Rollout(list(names), 1, policy=self.agent.actor, seed=self.seed + 7002, device=self.device, rank=self.rank,
                         hold_weights=False, **kw)
            entry = self.demo_rollouts[names] = (settings, ro, kw["max_episode_steps"])
        demo = VideoDemo(entry[1], width=width, height=height, max_trajectory_length=max_trajectory_length, max_episode_steps=entry[2])
        frames, overlay, _ = demo.run()
        return write_demo_gifs(frames, overlay, str(out_dir))

    def train_round(self, max_steps=None, max_iters=None):
        """Collect until every environment has finished one episode (or max_steps), update, reset.  Returns a summary."""
        steps = 0
        while True:
            steps += 1
            if self.collect_step() or (max_steps is not None and steps >= max_steps):
                break
        returns = self.sink.collector.episode_reward.mean().item()
        lengths = self.sink.collector.episode_timesteps.float().mean().item()
        iters = self.update_after_round(max_iters=max_iters)
        self.begin_round()
        return {"steps": steps, "per_morph_iter": iters, "performance/train_return": returns,
                "performance/train_length": lengths, "tot_env_steps": self.tot_env_steps}

    # ---- checkpoints -----------------------------------------------------------------------------------
    def save_checkpoint(self, ckpt_dir, replay="reference"):
        """Everything that decides what this run does next, written at a ROUND BOUNDARY (after train_round() has returned, after a
        warmup() that ended with a round, straight after construction; RuntimeError otherwise): checkpoint.save_checkpoint has
        the file list and the contract.  Every rank calls it.  Returns the list of paths this rank wrote."""
        from . import checkpoint
        return checkpoint.save_checkpoint(self, ckpt_dir, replay=replay)

    def load_checkpoint(self, ckpt_dir):
        """Restore a checkpoint IN PLACE into this trainer (built with the constructor arguments of the one that saved it; any
        mismatch is a ValueError before anything is written): no parameter, Adam or ring tensor moves, captured update graphs stay
        valid.  A trainer that goes on from here computes bit for bit what the saved one went on to compute
        (checkpoint.load_checkpoint).  Every rank calls it.  Returns tot_env_steps."""
        from . import checkpoint
        return checkpoint.load_checkpoint(self, ckpt_dir)
