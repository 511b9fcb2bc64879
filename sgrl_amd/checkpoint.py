"""Checkpoints of a `train_loop.DeviceTrainer`: save at a round end, resume bit for bit.

A reference-format snapshot (snapshot.py: `save.pth` + `.npy` rings) holds the four networks, the rings and one integer -- what the
reference's `--save_freq` / `--load_buffer` keep.  A checkpoint is that snapshot plus a sidecar per rank with everything else that
decides what the run does next: both Adam states, the counter-RNG positions (`DeviceTrainer.draw`, `Rollout.noise_step`, the
agent's dropout step), the generator states (`DeviceTrainer.gen`, `Rollout.gen`, torch's CPU and CUDA generators), the engine's
records and counters (the episode number keys every later reset draw) with its observation buffer, and the trainer's counters.

    <dir>/save.pth, save_<env>_{obs,action,next_obs,reward,done}_buffer.npy     learner; snapshot.save_snapshot writes them, so the
                                                 directory still loads with snapshot.load_snapshot and with the reference
                                                 (replay="reference" only: the other modes write save.pth alone)
    <dir>/resume_rank<r>.pth                     every rank; ONE torch.save of tensors, ints, floats, strings, None and lists / dicts of
                                                 those: torch.load(..., weights_only=True) reads it, and the loader uses that mode
    <dir>/resume_<env>_{obs,action,next_obs,reward,done}.npy                    learner, replay="filled": rows [0, max_sample_size) only
                                                 (a ring of 1 M rows of a 14-limb morphology is about 5 GB, a young ring mostly empty)

Every file is written under a temporary name and renamed into place: an interrupted save leaves each file of the previous
checkpoint in that directory either as it was or complete and new.

WHEN: at a round boundary only -- `begin_round()` has just reset the environments and the sink's per-round state is zero: after
`train_round()` has returned, after a `warmup()` that ended with a round, or straight after construction.
`DeviceTrainer._steps_in_round` counts the collection steps since the last `begin_round()`; a save with a non-zero count is a
RuntimeError.

CONTRACT.  Trainer A runs R1 rounds, saves, runs R2 more.  Trainer B, built with the same constructor arguments in the same or a
new process, loads and runs R2 rounds.  Then A and B hold equal BITS in every parameter, every Adam tensor, every ring row and
ring pointer and every engine record and counter, and their `train_round()` summaries are equal -- whenever two uninterrupted
copies of A agree with each other (the run's own reproducibility, which a checkpoint neither adds nor removes).  Loading into the
same live trainer restores IN PLACE: no parameter, Adam or ring tensor changes its data_ptr(), so the address tables of
td3.clip_and_step, the binds of mlp_hip.HipMlpOptim and every captured update graph stay valid (`graphed.stale(...)` stays False,
nothing is captured again); the host mirrors of device counters are dropped or re-read (td3.restore_optimizer,
HipMlpOptim.resync, TransitionSink.rings_loaded).
Not covered: the evaluation and demo rollouts (`eval_rollouts`, `demo_rollouts` keep engines of their own), TunableOp's choices,
and -- for `graph_updates=True` with an agent other than `mlp` and more than one morphology -- the ORDER of a fresh trainer's first
round of updates, whose first two iterations per morphology are the graphs' eager warm-up (train_loop.update_after_round): a
trainer that goes on with warmed graphs and a fresh one that loads its checkpoint then take the morphologies in different order.
A checkpoint from before the first update loaded into a trainer that HAS stepped deletes Adam state; a GraphedUpdates then forgets
its graphs and warms again (td3.GraphedUpdates.forget_graphs).
"""
import os

import numpy as np
import torch

from .snapshot import load_snapshot, save_snapshot

FORMAT_VERSION = 1
_RING_FIELDS = ("obs", "action", "next_obs", "reward", "done")
_IDENTITY = ("world", "rank", "env_names", "envs_per_morph", "seed", "actor_type", "critic_type", "td", "bu", "max_episode_steps")


def _identity(tr):
    env, args = tr.ro.env, tr.args
    counts = np.bincount(np.asarray(env.env_morph, dtype=np.int64), minlength=len(tr.env_names))
    return {"world": int(tr.world), "rank": int(tr.rank), "env_names": [str(n) for n in tr.env_names],
            "envs_per_morph": [int(c) for c in counts], "seed": int(tr.seed),
            "actor_type": str(getattr(args, "actor_type", "set")), "critic_type": str(getattr(args, "critic_type", "set")),
            "td": int(bool(args.td)), "bu": int(bool(args.bu)), "max_episode_steps": int(args.max_episode_steps)}


def _sidecar_path(ckpt_dir, rank):
    return os.path.join(ckpt_dir, "resume_rank%d.pth" % rank)


def _ring_paths(ckpt_dir, name, filled):
    if filled:
        return [os.path.join(ckpt_dir, "resume_%s_%s.npy" % (name, f)) for f in _RING_FIELDS]
    return [os.path.join(ckpt_dir, "save_%s_%s_buffer.npy" % (name, f)) for f in _RING_FIELDS]


def _write_atomic(path, write):
    """write(file object) under a temporary name in the same directory, then one rename."""
    tmp = "%s.tmp%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            write(f)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _engine_env(ro):
    env = getattr(ro, "env", None)
    if env is not None and all(hasattr(env, a) for a in ("get_records", "set_records", "refresh_device")):
        return env
    return None


def save_checkpoint(trainer, ckpt_dir, replay="reference"):
    """replay: "reference" -- the full-capacity rings in the reference's files; "filled" -- rows [0, max_sample_size) of each ring
    as resume_<env>_<field>.npy, no reference ring files; None -- no rows (load_checkpoint then leaves the rings as they are).
    Every rank calls it (one barrier at the end when world > 1; no other collective).  Returns the paths this rank wrote."""
    tr = trainer
    if replay not in ("reference", "filled", None):
        raise ValueError("replay must be 'reference', 'filled' or None (got %r)" % (replay,))
    if tr._steps_in_round != 0:
        raise RuntimeError("save_checkpoint at a round boundary only: %d collection steps since the last begin_round() "
                           "(save after train_round() has returned)" % tr._steps_in_round)
    ckpt_dir = str(ckpt_dir)
    os.makedirs(ckpt_dir, exist_ok=True)
    written = []
    tot = int(tr.tot_env_steps)
    side = {"format_version": FORMAT_VERSION, "rounds": int(tr.rounds), "tot_env_steps": tot}
    side.update(_identity(tr))
    ro = tr.ro
    env = _engine_env(ro)
    if env is not None:
        rec, cnt = env.get_records()
        side["engine_rec"], side["engine_cnt"] = torch.from_numpy(np.array(rec)), torch.from_numpy(np.array(cnt))
        side["engine_obs"] = env.obs.detach().cpu().clone()      # the reset observation the next step acts on (see load_checkpoint)
    elif hasattr(ro, "state_dict") and hasattr(ro, "load_state_dict"):
        side["driver"] = ro.state_dict()
    if hasattr(ro, "noise_step"):
        side["noise_step"] = int(ro.noise_step)
    if hasattr(ro, "gen"):
        side["ro_gen"] = ro.gen.get_state()
    side["torch_rng"] = torch.get_rng_state()
    side["cuda_rng"] = torch.cuda.get_rng_state(tr.device) if torch.device(tr.device).type == "cuda" else None
    if tr.is_learner:
        side.update({"updates": int(tr._updates), "draw": int(tr.draw), "trainer_gen": tr.gen.get_state(),
                     "agent": tr.agent.resume_state(), "replay": replay if replay is not None else "none",
                     "rings": [{"curr": int(b.curr), "max_sample_size": int(b.max_sample_size), "capacity": int(b.max_buffer_size)}
                               for b in tr.buffers]})
        names = tr.env_names
        # the learner's snapshot, by the function that defines the format; into a directory of its own first, then renamed in
        tmp_dir = os.path.join(ckpt_dir, ".snapshot.tmp%d" % os.getpid())
        try:
            if replay == "reference":
                save_snapshot(tmp_dir, tr.agent.state_dict(), tot, names, dict(zip(names, tr.buffers)))
            else:
                save_snapshot(tmp_dir, tr.agent.state_dict(), tot, [], {})
            for fn in sorted(os.listdir(tmp_dir), key=lambda fn: (fn == "save.pth", fn)):       # save.pth last
                os.replace(os.path.join(tmp_dir, fn), os.path.join(ckpt_dir, fn))
                written.append(os.path.join(ckpt_dir, fn))
        finally:
            if os.path.isdir(tmp_dir):
                for fn in os.listdir(tmp_dir):
                    os.remove(os.path.join(tmp_dir, fn))
                os.rmdir(tmp_dir)
        if replay == "filled":
            for name, b in zip(names, tr.buffers):
                fill = int(b.max_sample_size)
                for f, path in zip(_RING_FIELDS, _ring_paths(ckpt_dir, name, True)):
                    arr = getattr(b, f + "_buffer")[:fill].detach().cpu().numpy()
                    _write_atomic(path, lambda fh, arr=arr: np.save(fh, arr, allow_pickle=False))
                    written.append(path)
    _write_atomic(_sidecar_path(ckpt_dir, tr.rank), lambda fh: torch.save(side, fh))
    written.append(_sidecar_path(ckpt_dir, tr.rank))
    if tr.is_learner:
        # ring files of another mode left by an earlier save into this directory do not belong to this checkpoint
        for name in tr.env_names:
            for filled in (False, True):
                if (replay == "filled") != filled or replay is None:
                    for path in _ring_paths(ckpt_dir, name, filled):
                        if os.path.exists(path):
                            os.remove(path)
    if torch.device(tr.device).type == "cuda":
        torch.cuda.synchronize(tr.device)
    if tr.world > 1:
        tr.dist.barrier()
    return written


def _validate(tr, side):
    if side.get("format_version") != FORMAT_VERSION:
        raise ValueError("checkpoint format_version: the files hold %r, this library reads %r" % (side.get("format_version"), FORMAT_VERSION))
    mine = _identity(tr)
    for k in _IDENTITY:
        if side.get(k) != mine[k]:
            raise ValueError("checkpoint %s: the files hold %r, this trainer has %r" % (k, side.get(k), mine[k]))
    if tr.is_learner:
        if "agent" not in side:
            raise ValueError("checkpoint rank: the sidecar of rank %d was not written by a learner (dst = %d here)" % (tr.rank, tr.dst))
        caps = [int(r["capacity"]) for r in side["rings"]]
        have = [int(b.max_buffer_size) for b in tr.buffers]
        if caps != have:
            raise ValueError("checkpoint max_buffer_size: the files hold %r, this trainer has %r" % (caps, have))
        for which in ("actor_optimizer", "critic_optimizer"):
            n_saved = len(side["agent"][which]["state"])
            n_have = len(getattr(tr.agent, which).param_groups[0]["params"])
            if n_saved != n_have:
                raise ValueError("checkpoint %s: the files hold %d parameters, this trainer has %d" % (which, n_saved, n_have))


def load_checkpoint(trainer, ckpt_dir):
    """Restore IN PLACE (module docstring).  Every rank calls it with a directory that holds save.pth and its own sidecar
    (FileNotFoundError naming the missing file); the identity fields are validated first (ValueError naming the field and both
    values, before anything has been written into the trainer).  Ring rows come from whichever ring files are there -- the set
    the sidecar names first, else the other, else none: the rings and their pointers then stay as they are.  One barrier at the
    end when world > 1.  Returns tot_env_steps."""
    tr = trainer
    ckpt_dir = str(ckpt_dir)
    side_path, model_path = _sidecar_path(ckpt_dir, tr.rank), os.path.join(ckpt_dir, "save.pth")
    for path in (side_path, model_path):
        if not os.path.exists(path):
            raise FileNotFoundError("checkpoint file not found: %s" % path)
    side = torch.load(side_path, map_location="cpu", weights_only=True)
    _validate(tr, side)
    names = tr.env_names
    ring_mode = None
    if tr.is_learner:
        present = {filled: all(os.path.exists(p) for n in names for p in _ring_paths(ckpt_dir, n, filled)) for filled in (False, True)}
        for filled in ((True, False) if side["replay"] == "filled" else (False, True)):
            if present[filled] and ring_mode is None:
                ring_mode = "filled" if filled else "reference"
    # ---- networks (and, in the reference's files, the rings): into the existing tensors
    if ring_mode == "reference":
        state, _ = load_snapshot(model_path, names, dict(zip(names, tr.buffers)))
    else:
        state, _ = load_snapshot(model_path)
    tr.agent.load_state_dict(state)
    if tr.is_learner:
        # ---- optimizers, the agent's counters
        if tr.agent.load_resume_state(side["agent"]) and hasattr(tr.graphed, "forget_graphs"):
            tr.graphed.forget_graphs()
        # ---- rings
        if ring_mode == "filled":
            for name, b, r in zip(names, tr.buffers, side["rings"]):
                fill = int(r["max_sample_size"])
                for f, path in zip(_RING_FIELDS, _ring_paths(ckpt_dir, name, True)):
                    arr = np.load(path)
                    t = getattr(b, f + "_buffer")
                    if arr.shape[0] != fill or tuple(arr.shape[1:]) != tuple(t.shape[1:]):
                        raise ValueError("checkpoint ring file %s: shape %s, expected %s" % (path, arr.shape, (fill,) + tuple(t.shape[1:])))
                    t[:fill].copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(t.dtype))
                    t[fill:].zero_()         # rows a fresh ring has never written
                b.max_sample_size, b.curr = fill, int(r["curr"])
        if ring_mode is not None:
            tr.sink.rings_loaded()
    # ---- environments: the records, then the observation the saved run was about to act on
    ro = tr.ro
    env = _engine_env(ro)
    if env is not None and "engine_rec" in side:
        # set_records, then refresh_device: kinematics and observations of the restored state (gym's set_state -> sim.forward).
        # The refresh normalises the root quaternion IN PLACE, as every kinematics pass does, and normalising a normalised
        # quaternion again may move its last bit: the records are therefore written once more after it, and the observation
        # buffer takes the saved run's own bits
        rec, cnt = side["engine_rec"].numpy(), side["engine_cnt"].numpy()
        env.set_records(rec, cnt)
        ro.obs = env.refresh_device()
        env.set_records(rec, cnt)
        if "engine_obs" in side:
            env.obs.copy_(side["engine_obs"])
    elif "driver" in side and hasattr(ro, "load_state_dict"):
        ro.load_state_dict(side["driver"])
    tr.sink.begin_round()                # per-round state is zero at a round boundary; a pending lagged flag belongs to nobody
    tr._steps_in_round = 0
    # ---- counters: the total first, then the SAVED counter-RNG positions (the setter's rule draw = tot_env_steps is for snapshots)
    tot = int(side["tot_env_steps"])
    tr.rounds = int(side["rounds"])
    if tr.is_learner:
        tr._updates = int(side["updates"])
        tr._tot_base = tot - (tr.sink.stored + tr._updates)
        tr.draw = int(side["draw"])
        tr.gen.set_state(side["trainer_gen"])
    tr._tot_synced = tot
    if "noise_step" in side and hasattr(ro, "noise_step"):
        ro.noise_step = int(side["noise_step"])
    if "ro_gen" in side and hasattr(ro, "gen"):
        ro.gen.set_state(side["ro_gen"])
    torch.set_rng_state(side["torch_rng"])
    if side.get("cuda_rng") is not None and torch.device(tr.device).type == "cuda":
        torch.cuda.set_rng_state(side["cuda_rng"], tr.device)
    if hasattr(ro, "weights_changed"):
        ro.weights_changed()             # the copy_ above has bumped the versions already; explicit all the same
    if torch.device(tr.device).type == "cuda":
        torch.cuda.synchronize(tr.device)
    if tr.world > 1:
        tr.dist.barrier()
    return tot
