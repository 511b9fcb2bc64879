"""Batched evaluator: the bookkeeping of the reference's `BaseTrainer.evaluate`
(reference src/common/trainer.py:80-146) over a whole batch of environments at once.

The reference steps `num_envs_train` sub-environments (one per morphology) through an auto-resetting VecEnv for up to
`max_trajectory_length` steps per trajectory and keeps, per sub-environment,

  * `episode_timesteps`: steps until the FIRST done (the time limit `max_episode_steps` counts as done, :124-125),
  * `episode_reward`: the reward accumulated up to the first done -- latched only while it is still exactly 0 (:126-128;
    later dones of the auto-reset episodes re-latch only if the latched value is 0, with the accumulator restarted),
  * a trajectory contributes its per-env (length, return) pairs only if EVERY sub-environment was done at least once
    before `max_trajectory_length` (:139-145); otherwise it contributes nothing.

`evaluate()` returns the same dictionary (`performance/eval_return`, `performance/eval_length`: means over all
contributed pairs).  Arrays stay on the device of the environment; the only host sync per step is the `all(done)` test,
which the reference also performs.

`DeviceEvaluator` lays the trajectories of one evaluation side by side instead: every environment belongs to a trajectory GROUP,
the bookkeeping above is ONE launch per step (include/sgrl_eval.h sgrl_eval_record) with the `all(done)` test as a property of a
group, and the number of open groups is read a step late through pinned memory -- at most `max_trajectory_length` engine steps
per evaluation instead of up to `num_eval_trajectories` times that, and no host synchronisation in the loop.  `reduce_groups`
turns the resulting state into the reference's dictionary.

`VideoDemo` is the reference's `save_video_demo` (common/trainer.py:149-258) on the same machinery: one environment per morphology,
the evaluator's rule with one group, and after every step a frame of every environment rendered on the device
(BatchedModularVecEnv.get_images_device) into a frame chunk that crosses to the host in one copy.  `write_demo_gifs` writes the
frames with the reference's four text lines as one GIF per environment (host only, PIL).
"""
import ctypes

import numpy as np
import torch

from . import _lib


class BatchedEvaluator(object):
    def __init__(self, env, act_fn, num_eval_trajectories=10, max_trajectory_length=1000, max_episode_steps=1000):
        """env: object with reset() -> obs [n, obs_len] and step(actions) -> (obs, reward [n], done [n], info);
        act_fn(obs) -> actions [n, action_len] (deterministic policy: Agent.select_action, reference agent.py:189-198).
        Tensors or NumPy arrays are accepted (NumPy is converted)."""
        self.env, self.act_fn = env, act_fn
        self.num_eval_trajectories = int(num_eval_trajectories)
        self.max_trajectory_length = int(max_trajectory_length)
        self.max_episode_steps = int(max_episode_steps)

    @torch.no_grad()
    def evaluate(self):
        returns, lengths = [], []
        for _ in range(self.num_eval_trajectories):
            obs = self.env.reset()
            n = int(obs.shape[0])
            dev = obs.device if torch.is_tensor(obs) else torch.device("cpu")
            done_ever = torch.zeros(n, dtype=torch.bool, device=dev)
            ep_reward = torch.zeros(n, dtype=torch.float64, device=dev)      # episode_reward_list
            ep_steps = torch.zeros(n, dtype=torch.int64, device=dev)         # episode_timesteps_list
            acc = torch.zeros(n, dtype=torch.float64, device=dev)            # episode_reward_list_buffer
            for _step in range(self.max_trajectory_length):
                obs, rew, done, _info = self.env.step(self.act_fn(obs))
                rew = torch.as_tensor(rew, device=dev).to(torch.float64).reshape(n)
                cur = torch.as_tensor(done, device=dev).to(torch.bool).reshape(n).clone()
                acc += rew
                cur |= (ep_steps + 1) == self.max_episode_steps
                latch = cur & (ep_reward == 0)
                ep_reward = torch.where(latch, acc, ep_reward)
                acc = torch.where(latch, torch.zeros_like(acc), acc)
                ep_steps += (~done_ever).to(torch.int64)
                done_ever |= cur
                if bool(done_ever.all()):
                    lengths.extend(ep_steps.tolist())
                    returns.extend(ep_reward.tolist())
                    break
        # np.mean of an empty list is nan (with a warning) in the reference as well
        return {"performance/eval_return": float(np.mean(returns)) if returns else float("nan"),
                "performance/eval_length": float(np.mean(lengths)) if lengths else float("nan")}


class _EvalState(ctypes.Structure):
    """sgrl_eval_state of include/sgrl_eval.h: a host struct of device pointers."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("group", "done_ever", "ep_steps", "ep_reward", "acc", "remaining", "close_step",
                                                     "open")]


def _bind(L):
    """The entry points of include/sgrl_eval.h (declared there, not in sgrl.h)."""
    if getattr(L, "_eval_bound", False):
        return
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.sgrl_eval_begin.argtypes = [ctypes.POINTER(_EvalState), ci, ci, vp]
    L.sgrl_eval_begin.restype = ci
    L.sgrl_eval_record.argtypes = [ctypes.POINTER(_EvalState), vp, vp, vp, ci, ci, ci, ci, vp]
    L.sgrl_eval_record.restype = ci
    L.sgrl_eval_record_launches.argtypes = []
    L.sgrl_eval_record_launches.restype = ci
    L.sgrl_eval_last_error.argtypes = []
    L.sgrl_eval_last_error.restype = ctypes.c_char_p
    L._eval_bound = True


def _host(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=dtype).reshape(-1)


def reduce_groups(ep_reward, ep_steps, group, close_step, env_morph=None, names=None):
    """The reference's evaluation dictionary from the state of a grouped evaluation (tensors or NumPy arrays, any device; the
    reduction itself runs on the host in float64): means of `ep_reward` / `ep_steps` over the environments whose group completed
    (`close_step[group] != 0`) -- a trajectory in which some sub-environment never finished contributes nothing (reference
    common/trainer.py:139-145) -- and NaN when no group completed, as np.mean of the reference's empty lists.  With `env_morph`
    (morphology id per environment) and `names` also `performance/eval_return/<name>` and `performance/eval_length/<name>`: the
    same means over the environments of one morphology."""
    ret, length = _host(ep_reward, np.float64), _host(ep_steps, np.float64)
    grp, closed = _host(group, np.int64), _host(close_step, np.int64) != 0
    keep = closed[grp]

    def mean(a, m):
        return float(a[m].mean()) if m.any() else float("nan")
    out = {"performance/eval_return": mean(ret, keep), "performance/eval_length": mean(length, keep)}
    if env_morph is not None and names is not None:
        morph = _host(env_morph, np.int64)
        for k, name in enumerate(names):
            m = keep & (morph == k)
            out["performance/eval_return/%s" % name] = mean(ret, m)
            out["performance/eval_length/%s" % name] = mean(length, m)
    return out


class DeviceEvaluator(object):
    """All trajectories of one evaluation in one batched pass on the device (there is no CPU fallback)."""

    def __init__(self, ro, act_fn=None, num_eval_trajectories=10, max_trajectory_length=1000, max_episode_steps=1000, group=None):
        """ro: a rollout.Rollout built with envs_per_morph = num_eval_trajectories (or anything with its surface: `device`,
        `env.num_envs` / `env.env_morph` / `env.env_names` / `env.morph_slices`, `reset()`, `step(actions)`, `policy_forward(obs)`).
        act_fn(obs) -> actions; default ro.policy_forward, the deterministic policy (no exploration noise).  group: trajectory
        group id per environment; default = an environment's index within its morphology's slice, so that every group holds one
        environment of every morphology -- the reference's set of sub-environments."""
        self.ro = ro
        self.act_fn = act_fn if act_fn is not None else ro.policy_forward
        self.num_eval_trajectories = int(num_eval_trajectories)
        self.max_trajectory_length = int(max_trajectory_length)
        self.max_episode_steps = int(max_episode_steps)
        env = ro.env
        n, n_groups = int(env.num_envs), self.num_eval_trajectories
        if n_groups < 1 or self.max_trajectory_length < 1 or self.max_episode_steps < 1:
            raise ValueError("num_eval_trajectories, max_trajectory_length and max_episode_steps must be at least 1")
        if group is None:
            g = np.zeros(n, dtype=np.int64)
            for sl in env.morph_slices:
                g[sl] = np.arange(sl.stop - sl.start)
        else:
            g = np.asarray(group.detach().cpu().numpy() if torch.is_tensor(group) else group)
            if g.dtype.kind not in "iu":
                raise ValueError("group ids must be integers, not %s" % g.dtype)
            if g.shape != (n,):
                raise ValueError("group must hold one id per environment (%d), not shape %s" % (n, g.shape))
        if g.min() < 0 or g.max() >= n_groups:
            raise ValueError("group ids must lie in 0 .. %d (num_eval_trajectories - 1)" % (n_groups - 1))
        members = np.bincount(g, minlength=n_groups)
        if (members == 0).any():
            raise ValueError("trajectory group(s) %s have no environment: they could never complete" % np.nonzero(members == 0)[0].tolist())
        self.device = torch.device(ro.device)
        if self.device.type != "cuda":
            raise _lib.SgrlError("DeviceEvaluator needs a rollout on the GPU (no CPU fallback exists)")
        self.n_env, self.n_groups = n, n_groups
        self.env_morph = np.asarray(env.env_morph, dtype=np.int64)
        self.names = list(env.env_names)
        z = lambda m, dtype: torch.zeros(m, dtype=dtype, device=self.device)
        self.group = torch.from_numpy(g.astype(np.int32)).to(self.device)
        self.done_ever, self.ep_steps = z(n, torch.uint8), z(n, torch.int64)
        self.ep_reward, self.acc = z(n, torch.float64), z(n, torch.float64)
        self.remaining, self.close_step, self.open = z(n_groups, torch.int32), z(n_groups, torch.int32), z(1, torch.int32)
        self._state = _EvalState(*[t.data_ptr() for t in (self.group, self.done_ever, self.ep_steps, self.ep_reward, self.acc,
                                                          self.remaining, self.close_step, self.open)])
        # the open-group count of a step, fetched behind an event and read one step late (rollout.TransitionSink's lag_flag)
        self._lag_slots = [(torch.zeros(1, dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(2)]
        self.early_stop = True
        self.last_steps = 0
        self._L = _lib.lib()
        _bind(self._L)

    def _check(self, rc, what):
        if rc != 0:
            raise _lib.SgrlError("%s failed (%d): %s" % (what, rc, self._L.sgrl_eval_last_error().decode()))

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def begin(self):
        self._check(self._L.sgrl_eval_begin(ctypes.byref(self._state), self.n_env, self.n_groups, self._stream()), "sgrl_eval_begin")

    def record(self, reward, done, step):
        """One step's reward (float32, or float64 for parity tests) and done (bool / uint8) of every environment: one launch."""
        if reward.dtype not in (torch.float32, torch.float64) or not reward.is_contiguous():
            reward = reward.to(torch.float32).contiguous()
        if done.dtype == torch.bool:
            done = done.contiguous().view(torch.uint8)
        elif done.dtype != torch.uint8 or not done.is_contiguous():
            done = (done != 0).contiguous().view(torch.uint8)
        if reward.numel() != self.n_env or done.numel() != self.n_env or reward.device != self.device or done.device != self.device:
            raise _lib.SgrlError("record: reward and done must hold one value per environment on %s" % self.device)
        p = ctypes.c_void_p(reward.data_ptr())
        f32 = reward.dtype == torch.float32
        self._check(self._L.sgrl_eval_record(ctypes.byref(self._state), p if f32 else None, None if f32 else p,
                                             ctypes.c_void_p(done.data_ptr()), self.n_env, self.n_groups, int(step),
                                             self.max_episode_steps, self._stream()), "sgrl_eval_record")

    @torch.no_grad()
    def evaluate(self, early_stop=None):
        """reset, then at most max_trajectory_length steps of act_fn / step / record; the loop ends when the open-group count read
        one step late is 0 (steps taken after the last group closed change nothing: their groups are frozen); ONE synchronisation
        after the loop, then reduce_groups.  early_stop=False runs all max_trajectory_length steps.  `last_steps`: steps taken."""
        early_stop = self.early_stop if early_stop is None else bool(early_stop)
        obs = self.ro.reset()
        self.begin()
        stream = torch.cuda.current_stream(self.device)
        prev, steps = None, 0
        for step in range(self.max_trajectory_length):
            obs, rew, done = self.ro.step(self.act_fn(obs))[:3]
            self.record(rew, done, step)
            steps += 1
            if not early_stop:
                continue
            host, ev = self._lag_slots[step & 1]
            host.copy_(self.open, non_blocking=True)
            ev.record(stream)
            if prev is not None:
                prev[1].synchronize()           # recorded a whole step ago
                if int(prev[0][0]) == 0:
                    break
            prev = (host, ev)
        self.last_steps = steps
        stream.synchronize()
        return reduce_groups(self.ep_reward, self.ep_steps, self.group, self.close_step, self.env_morph, self.names)


CHUNK_BYTES = 256 * 1000 * 1000      # default ceiling of one device frame chunk


class VideoDemo(object):
    """The rollout of the reference's `save_video_demo` (common/trainer.py:149-258) with every frame rendered on the device (there is
    no CPU fallback): reset, frame 0, then per step the deterministic policy, the engine step, the bookkeeping of :191-201 -- the
    evaluator's rule, `DeviceEvaluator.record` with ONE group holding every environment -- and a frame of every environment
    (finished ones auto-reset and keep being rendered, as in the reference) until every environment has finished its first episode
    or `max_trajectory_length` steps were taken."""

    def __init__(self, ro, act_fn=None, width=500, height=500, max_trajectory_length=1000, max_episode_steps=1000, chunk_frames=None):
        """ro: a rollout.Rollout with ONE environment per morphology (the reference's `eval_env`); act_fn(obs) -> actions, default
        ro.policy_forward.  chunk_frames: frames per device chunk, default as many as stay under CHUNK_BYTES (256 MB) -- 1001
        frames of 23 environments at 500 x 500 do not fit on the device in one piece."""
        self.ro = ro
        self.act_fn = act_fn if act_fn is not None else ro.policy_forward
        self.width, self.height = int(width), int(height)
        self.max_trajectory_length = int(max_trajectory_length)
        self.max_episode_steps = int(max_episode_steps)
        if self.width < 1 or self.height < 1:
            raise ValueError("width and height must be at least 1")
        n = int(ro.env.num_envs)
        self.ev = DeviceEvaluator(ro, act_fn=self.act_fn, num_eval_trajectories=1, max_trajectory_length=self.max_trajectory_length,
                                  max_episode_steps=self.max_episode_steps, group=np.zeros(n, dtype=np.int64))
        self.device, self.n_env = self.ev.device, n
        frame_bytes = n * self.height * self.width * 3
        if chunk_frames is None:
            chunk_frames = max(1, CHUNK_BYTES // frame_bytes)
        self.chunk_frames = max(1, min(int(chunk_frames), self.max_trajectory_length + 1))
        self.last_dones = None       # uint8 [T, n]: the environments' own done flags of the kept steps (before the time-limit rule)
        self.last_steps = 0          # engine steps taken, the lagged extra ones included

    @torch.no_grad()
    def run(self):
        """-> (frames uint8 [T + 1, n, H, W, 3] on the host, overlay float64 [T, n, 4] on the host, close_step).  Overlay row t =
        (dist, reward, episode reward buffer, episode timesteps) of every environment after step t: what the reference draws on frame
        t + 1.  close_step: the number of steps after which every environment had finished its first episode, 0 when that did not
        happen within max_trajectory_length; T = close_step, or max_trajectory_length then.  The stop flag is read one step late
        (DeviceEvaluator), so one or two steps more than T are taken; their frames and rows are dropped.  No host synchronisation per
        step: a full frame chunk goes to pinned memory in one copy, and the host waits for it while the next chunk renders."""
        ro, ev, env = self.ro, self.ev, self.ro.env
        n, H, W, C, max_len = self.n_env, self.height, self.width, self.chunk_frames, self.max_trajectory_length
        dev, stream = self.device, torch.cuda.current_stream(self.device)
        chunk = torch.empty((C, n, H, W, 3), dtype=torch.uint8, device=dev)
        stage = [(torch.empty((C, n, H, W, 3), dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(2)]
        frames = np.empty((max_len + 1, n, H, W, 3), dtype=np.uint8)       # pages are touched only as far as frames arrive
        overlay = torch.zeros((max_len, n, 4), dtype=torch.float64, device=dev)
        dones = torch.zeros((max_len, n), dtype=torch.uint8, device=dev)
        pending = []                 # [(stage slot, first frame, count)] copies in flight, at most two

        def drain(keep=0):
            while len(pending) > keep:
                k, first, cnt = pending.pop(0)
                stage[k][1].synchronize()
                frames[first:first + cnt] = stage[k][0][:cnt].numpy()

        def flush(first, cnt, k):
            stage[k][0][:cnt].copy_(chunk[:cnt], non_blocking=True)      # slot k was drained a whole chunk ago
            stage[k][1].record(stream)
            pending.append((k, first, cnt))
            drain(keep=1)            # the chunk before this one: its copy ran while this one rendered

        obs = ro.reset()
        ev.begin()
        env.get_images_device(None, W, H, out=chunk[0])
        n_frames, first, flushed = 1, 0, 0
        prev, steps = None, 0
        for step in range(max_len):
            obs, rew, done, dist = ro.step(self.act_fn(obs))[:4]
            ev.record(rew, done, step)
            if n_frames - first == C:
                flush(first, C, flushed & 1)
                first, flushed = n_frames, flushed + 1
            env.get_images_device(None, W, H, out=chunk[n_frames - first])
            n_frames += 1
            row = overlay[step]
            row[:, 0], row[:, 1], row[:, 2], row[:, 3] = dist, rew, ev.acc, ev.ep_steps
            dones[step] = done.view(torch.uint8) if done.dtype == torch.bool else done
            steps += 1
            host, lag = ev._lag_slots[step & 1]
            host.copy_(ev.open, non_blocking=True)
            lag.record(stream)
            if prev is not None:
                prev[1].synchronize()           # recorded a whole step ago
                if int(prev[0][0]) == 0:
                    break
            prev = (host, lag)
        if n_frames > first:
            flush(first, n_frames - first, flushed & 1)
        drain()
        stream.synchronize()
        close_step = int(ev.close_step[0])
        T = close_step if close_step != 0 else steps
        self.last_steps = steps
        self.last_dones = dones[:T].cpu().numpy()
        return frames[:T + 1], overlay[:T].cpu().numpy(), close_step


def _demo_font():
    from PIL import ImageFont
    try:
        return ImageFont.truetype("./misc/sans-serif.ttf", 20)      # the reference's font, where a run directory ships it
    except OSError:
        return ImageFont.load_default()


def write_demo_gifs(frames, overlay, out_dir, fps=60, text=True):
    """One `<i>.gif` per environment in `out_dir` from VideoDemo.run()'s (frames [T + 1, n, H, W, 3] uint8, overlay [T, n, 4]); host
    only.  text: the reference's four yellow lines at (100, 10 / 32 / 54 / 76) on every frame but the first
    (common/trainer.py:213-232).  The frames are written as they are: the reference's rot90(k=2) undoes the upside-down off-screen
    buffer of MuJoCo's renderer, and this repository's ray caster renders upright.  Returns the list of written paths."""
    import os
    from PIL import Image, ImageDraw
    frames, overlay = np.asarray(frames), np.asarray(overlay)
    if frames.ndim != 5 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
        raise ValueError("frames must be uint8 [T + 1, n, H, W, 3]")
    if overlay.shape != (frames.shape[0] - 1, frames.shape[1], 4):
        raise ValueError("overlay must be [T, n, 4] for frames [T + 1, n, H, W, 3], not %s" % (overlay.shape,))
    os.makedirs(out_dir, exist_ok=True)
    font = _demo_font() if text else None
    labels = ("Distance: ", "Instant Reward: ", "Episode Reward: ", "Episode Timesteps: ")
    paths = []
    for i in range(frames.shape[1]):
        imgs = []
        for t in range(frames.shape[0]):
            img = Image.fromarray(frames[t, i], "RGB")
            if text and t > 0:
                draw = ImageDraw.Draw(img)
                dist, rew, acc, ts = overlay[t - 1, i]
                for k, v in enumerate((str(float(dist)), str(float(rew)), str(float(acc)), str(int(ts)))):
                    draw.text((100, 10 + 22 * k), labels[k] + v, (255, 255, 0), font=font)
            imgs.append(img)
        path = os.path.join(out_dir, "%d.gif" % i)
        imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=max(1, int(round(1000.0 / fps))), loop=0)
        paths.append(path)
    return paths
