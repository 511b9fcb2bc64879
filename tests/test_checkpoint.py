"""`DeviceTrainer.save_checkpoint` / `load_checkpoint` (sgrl_amd/checkpoint.py) on CPU: a trainer over a SCRIPTED driver with the
`Rollout` surface (the engine has no CPU implementation), in the manner of tests/test_trainer_multirank.py, but with a policy
forward and a reward that depends on the actions, so that the networks decide what the next round stores.

What is compared is BITS: every parameter of the four networks, every Adam tensor of both optimizers, every ring row and ring
pointer and the trainer's counters of a run that was interrupted (saved, loaded into another trainer, continued) against the
run that went on.  CPU PyTorch with one thread is reproducible; the round-trip test asserts that first, so that a failure of the
comparison points at the checkpoint."""
import os
import shutil
import socket
import types

import numpy as np
import pytest
import torch

LIMBS = [3, 4]
PER = 3
T_MAX = 12
CAP = 40             # ring capacity: after two rounds the second morphology's ring has wrapped, the first one's has not
NETS = ("actor", "actor_target", "critic", "critic_target")
RINGS = ("obs_buffer", "action_buffer", "next_obs_buffer", "reward_buffer", "done_buffer")


class ScriptedRollout(object):
    """The surface DeviceTrainer uses of sgrl_amd.rollout.Rollout, without an engine.  Its whole state is the step number `t`
    (state_dict / load_state_dict: what a checkpoint keeps of an injected driver without an engine) and the generator `gen`."""

    def __init__(self, policy, rank):
        from sgrl_amd import graph as G
        self.rank = rank
        self.policy = policy
        self.actor = None
        n = PER * len(LIMBS)
        Lmax = max(LIMBS)
        parents = {3: [-1, 0, 1], 4: [-1, 0, 1, 1]}
        self.graph_dicts = [G.getGraphDict(parents[L], ["pre", "inlcrs", "postlcrs"], [], device=torch.device("cpu")) for L in LIMBS]
        self.env = types.SimpleNamespace(num_envs=n, env_morph=np.repeat(np.arange(len(LIMBS)), PER), num_limbs=list(LIMBS),
                                         obs_max_len=41 * Lmax, action_max_len=3 * Lmax, device=torch.device("cpu"),
                                         obs=torch.zeros((n, 41 * Lmax)), row_overflow_envs=lambda: 0)
        self.actions = torch.zeros((n, 3 * Lmax))
        self.act_mask = torch.zeros((n, 3 * Lmax))
        for i, k in enumerate(self.env.env_morph):
            self.act_mask[i, :3 * LIMBS[k]] = 1.0
        self.t = 0
        self.gen = torch.Generator().manual_seed(100 + rank)

    def state_dict(self):
        return {"t": int(self.t)}

    def load_state_dict(self, d):
        self.t = int(d["t"])
        self.env.obs.copy_(self._obs())

    def _obs(self):
        g = torch.Generator().manual_seed(7919 * self.rank + self.t)
        o = torch.rand((self.env.num_envs, self.env.obs_max_len), generator=g)
        for i, k in enumerate(self.env.env_morph):
            o[i, 41 * LIMBS[k]:] = 0
        return o

    def reset(self):
        self.env.obs.copy_(self._obs())
        return self.env.obs

    def random_actions(self):
        self.actions.uniform_(-1, 1, generator=self.gen)
        self.actions.mul_(self.act_mask)
        return self.actions

    def policy_forward(self, obs=None):
        obs = self.env.obs if obs is None else obs
        out = torch.zeros_like(self.actions)
        with torch.no_grad():
            for k, L in enumerate(LIMBS):
                sl = slice(k * PER, (k + 1) * PER)
                self.policy.change_morphology(self.graph_dicts[k])
                out[sl, :3 * L] = self.policy(obs[sl, :41 * L])
        return out

    def add_exploration_noise(self, actions, expl_noise):
        noise = torch.randn(actions.shape, generator=self.gen) * expl_noise
        return ((actions + noise).clamp_(-1.0, 1.0)) * self.act_mask

    def step(self, a):
        self.t += 1
        n = self.env.num_envs
        self.env.obs.copy_(self._obs())
        rew = 0.25 * (self.rank + 1) + 0.01 * a.sum(dim=1)
        # the second morphology's episodes are longer: its ring fills (and wraps) faster than the first one's
        done = torch.tensor([(self.t + i + 2 * self.rank) % ((3 if i < PER else 9) + i % 3) == 0 for i in range(n)])
        return self.env.obs, rew, done, torch.zeros(n)


def _trainer(rollout=ScriptedRollout, names=("m3", "m4"), **arg_over):
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    # a SET agent with ONE attention layer instead of three: every code path of the restore at a third of the time
    args = default_train_args(batch_size=8, max_episode_steps=T_MAX, attention_layers=1, **arg_over)
    return DeviceTrainer(list(names), PER, args=args, seed=5, device="cpu", max_buffer_size=CAP, batch_size=8, rollout=rollout)


def _adam(opt):
    out = []
    for p in opt.param_groups[0]["params"]:
        st = opt.state.get(p) or {}
        out.append({k: st[k] for k in ("step", "exp_avg", "exp_avg_sq") if k in st})
    return out


def _tensors(tr):
    """Every tensor the contract names, live (not copied): name -> tensor."""
    out = {}
    for nm in NETS:
        for k, p in getattr(tr.agent, nm).named_parameters():
            out["%s.%s" % (nm, k)] = p
    for nm in ("actor_optimizer", "critic_optimizer"):
        for i, st in enumerate(_adam(getattr(tr.agent, nm))):
            for k, v in st.items():
                out["%s[%d].%s" % (nm, i, k)] = v
    for i, b in enumerate(tr.buffers):
        for f in RINGS:
            out["ring%d.%s" % (i, f)] = getattr(b, f)
    return out


def _state(tr):
    """A copy of that, plus the pointers and counters."""
    st = {k: v.detach().clone() for k, v in _tensors(tr).items()}
    st["pointers"] = [(b.curr, b.max_sample_size) for b in tr.buffers]
    st["counters"] = (tr.tot_env_steps, tr._updates, tr.rounds, tr.draw, tr.ro.t)
    return st


def _assert_same(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _round(tr):
    return tr.train_round(max_iters=2)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Trainer A: a checkpoint at construction, two rounds, checkpoints in every replay mode, two more rounds.  Computed once and
    left unchanged."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    root = tmp_path_factory.mktemp("ckpt")
    d = {k: str(root / k) for k in ("fresh", "reference", "filled", "none")}
    a = _trainer()
    a.save_checkpoint(d["fresh"])
    out = {"dirs": d, "summaries": [], "states": {0: _state(a)}}
    for r in (1, 2):
        out["summaries"].append(_round(a))
        out["states"][r] = _state(a)
    out["written"] = {"reference": a.save_checkpoint(d["reference"]), "filled": a.save_checkpoint(d["filled"], replay="filled"),
                      "none": a.save_checkpoint(d["none"], replay=None)}
    assert _state(a)["counters"] == out["states"][2]["counters"]           # saving moved nothing
    for r in (3, 4):
        out["summaries"].append(_round(a))
        out["states"][r] = _state(a)
    yield out
    torch.set_num_threads(threads)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_resumes_bit_for_bit(run):
    control = _trainer()
    summaries = [_round(control) for _ in range(4)]
    assert summaries == run["summaries"]                                   # two uninterrupted copies agree ...
    _assert_same(_state(control), run["states"][4], "control")             # ... bit for bit: the precondition of what follows
    # the shapes the interchange test relies on: the second ring has wrapped at the save, the first has not; updates have run
    (c0, f0), (c1, f1) = run["states"][2]["pointers"]
    assert f0 < CAP and c0 == f0 and f1 == CAP and run["states"][2]["counters"][1] == 8
    b = _trainer()
    assert b.load_checkpoint(run["dirs"]["reference"]) == run["states"][2]["counters"][0]
    _assert_same(_state(b), run["states"][2], "after load")
    assert b.sink.device_pointers() == (None, 0)                           # a CPU sink keeps no device pointers, nothing pending
    resumed = [_round(b) for _ in range(2)]
    assert resumed == run["summaries"][2:]
    _assert_same(_state(b), run["states"][4], "resumed")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def test_load_restores_in_place(run):
    b = _trainer()
    _round(b)                                                              # it has updated: every tensor exists
    before = {k: v.data_ptr() for k, v in _tensors(b).items()}
    assert any(k.endswith("exp_avg") for k in before)
    b.load_checkpoint(run["dirs"]["reference"])
    after = {k: v.data_ptr() for k, v in _tensors(b).items()}
    assert after == before
    _assert_same(_state(b), run["states"][2], "after load")
    for opt in (b.agent.actor_optimizer, b.agent.critic_optimizer):
        mirror = getattr(opt, "_sgrl_step_class", None)
        assert mirror is None or all(mirror[id(p)] == int(opt.state[p]["step"]) for p in opt.param_groups[0]["params"])
    _round(b), _round(b)
    _assert_same(_state(b), run["states"][4], "resumed in place")


def test_restore_optimizer_keeps_the_form_of_the_group():
    """A capturable group gets (and keeps) float32 step tensors on the parameter's device, a plain group 0-dim CPU tensors; stale
    host mirrors are dropped."""
    from sgrl_amd.td3 import optimizer_state, restore_optimizer
    w = torch.nn.Parameter(torch.arange(6.0).reshape(2, 3))
    src = torch.optim.Adam([w], lr=3e-4)
    w.grad = torch.ones_like(w)
    src.step(), src.step()
    rec = optimizer_state(src)
    assert rec["state"][0]["step"] == 2.0 and rec["group"]["lr"] == 3e-4
    for capturable in (False, True):
        v = torch.nn.Parameter(torch.zeros(2, 3))
        dst = torch.optim.Adam([v], lr=1e-3)
        dst.param_groups[0]["capturable"] = capturable
        dst._sgrl_step_class = {id(v): 7}
        assert restore_optimizer(dst, rec) is False
        st = dst.state[v]
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"], src.state[w]["exp_avg"]) and torch.equal(st["exp_avg_sq"], src.state[w]["exp_avg_sq"])
        # the stale mirror is gone: a plain group keeps none, device counters get one that holds the restored count
        assert dst.param_groups[0]["lr"] == 3e-4 and getattr(dst, "_sgrl_step_class", None) == ({id(v): 2} if capturable else None)
        ptrs = [st[k].data_ptr() for k in ("step", "exp_avg", "exp_avg_sq")]
        assert restore_optimizer(dst, rec) is False and [st[k].data_ptr() for k in ("step", "exp_avg", "exp_avg_sq")] == ptrs
        assert restore_optimizer(dst, {"group": rec["group"], "state": [None]}) is True and len(dst.state.get(v, {})) == 0
    with pytest.raises(ValueError, match="parameters"):
        restore_optimizer(src, {"group": rec["group"], "state": []})


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_empty_optimizer_state_both_ways(run):
    # a checkpoint from before the first update, into a trainer that HAS stepped: its Adam state is gone again
    b = _trainer()
    _round(b)
    assert len(b.agent.critic_optimizer.state) > 0
    b.load_checkpoint(run["dirs"]["fresh"])
    assert all(len(st) == 0 for opt in (b.agent.actor_optimizer, b.agent.critic_optimizer) for st in _adam(opt))
    _assert_same(_state(b), run["states"][0], "after load of the fresh checkpoint")
    assert _round(b) == run["summaries"][0]
    _assert_same(_state(b), run["states"][1], "first round after the fresh checkpoint")
    # a checkpoint with state, into a fresh trainer: created, in the form torch.optim.Adam creates for a plain group
    c = _trainer()
    assert len(c.agent.critic_optimizer.state) == 0
    c.load_checkpoint(run["dirs"]["reference"])
    for opt in (c.agent.actor_optimizer, c.agent.critic_optimizer):
        states = [st for st in _adam(opt) if st]                          # (a parameter that never takes a gradient has none)
        assert states
        for st in states:
            assert st["step"].device.type == "cpu" and st["step"].dim() == 0 and st["step"].dtype == torch.float32
    assert _round(c) == run["summaries"][2]
    _assert_same(_state(c), run["states"][3], "first round after the checkpoint with state")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_interchange_and_replay_modes(run):
    from sgrl_amd.replay import DeviceReplayBuffer
    from sgrl_amd.snapshot import load_snapshot
    names, dirs, s2 = ["m3", "m4"], run["dirs"], run["states"][2]
    # the reference's format: a checkpoint directory is a snapshot directory
    bufs = {n: DeviceReplayBuffer(41 * L, 3 * L, CAP) for n, L in zip(names, LIMBS)}
    state, tot = load_snapshot(os.path.join(dirs["reference"], "save.pth"), names, bufs)
    assert tot == s2["counters"][0] and set(state) == set(_trainer().agent.state_dict())
    for i, n in enumerate(names):
        assert (bufs[n].curr, bufs[n].max_sample_size) == s2["pointers"][i]
        for f in RINGS:
            assert torch.equal(getattr(bufs[n], f), s2["ring%d.%s" % (i, f)]), (n, f)
    assert sorted(os.path.basename(p) for p in run["written"]["reference"]) == sorted(
        ["save.pth", "resume_rank0.pth"] + ["save_%s_%s.npy" % (n, f) for n in names for f in RINGS])
    # filled: no reference ring files, exactly max_sample_size rows per file, and a load reproduces the ring
    files = sorted(os.listdir(dirs["filled"]))
    assert files == sorted(["save.pth", "resume_rank0.pth"] + ["resume_%s_%s.npy" % (n, f[:-7]) for n in names for f in RINGS])
    for i, n in enumerate(names):
        for f in RINGS:
            assert np.load(os.path.join(dirs["filled"], "resume_%s_%s.npy" % (n, f[:-7]))).shape[0] == s2["pointers"][i][1]
    b = _trainer()
    _round(b), _round(b), _round(b)                                        # other rows, more of them, other pointers
    b.load_checkpoint(dirs["filled"])
    _assert_same(_state(b), s2, "filled")
    # None: save.pth and the sidecar only; the rings stay as they are
    assert sorted(os.listdir(dirs["none"])) == ["resume_rank0.pth", "save.pth"]
    c = _trainer()
    _round(c)
    rings = {k: v for k, v in _state(c).items() if k.startswith("ring") or k == "pointers"}
    c.load_checkpoint(dirs["none"])
    got = _state(c)
    for k, v in rings.items():
        assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert got["counters"] == s2["counters"]
    _assert_same({k: v for k, v in got.items() if k not in rings}, {k: v for k, v in s2.items() if k not in rings}, "none")


def test_a_save_over_another_mode_leaves_one_set_of_ring_files(run, tmp_path):
    d = str(tmp_path / "both")
    shutil.copytree(run["dirs"]["reference"], d)
    b = _trainer()
    b.load_checkpoint(d)
    b.save_checkpoint(d, replay="filled")
    assert not [f for f in os.listdir(d) if f.endswith("_buffer.npy") or ".tmp" in f]
    c = _trainer()
    c.load_checkpoint(d)
    _assert_same(_state(c), run["states"][2], "filled over reference")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_refusals(run, tmp_path):
    b = _trainer()
    b.collect_step(random_actions=True)
    with pytest.raises(RuntimeError, match="1 collection step"):
        b.save_checkpoint(str(tmp_path / "mid"))
    assert not os.path.exists(str(tmp_path / "mid" / "save.pth"))

    class FourPer(ScriptedRollout):
        def __init__(self, policy, rank):
            ScriptedRollout.__init__(self, policy, rank)
            self.env.env_morph = np.array([0, 0, 1, 1, 1, 1])

    side = torch.load(os.path.join(run["dirs"]["reference"], "resume_rank0.pth"), weights_only=True)
    world2 = str(tmp_path / "world2")
    shutil.copytree(run["dirs"]["reference"], world2)
    torch.save(dict(side, world=2), os.path.join(world2, "resume_rank0.pth"))
    cases = [("env_names", _trainer(names=("m3", "other")), run["dirs"]["reference"]),
             ("envs_per_morph", _trainer(rollout=FourPer), run["dirs"]["reference"]),
             ("actor_type", _trainer(actor_type="swat"), run["dirs"]["reference"]),
             ("world", _trainer(), world2)]
    for field, tr, d in cases:
        before = _state(tr)
        with pytest.raises(ValueError, match="checkpoint %s: the files hold .* this trainer has " % field):
            tr.load_checkpoint(d)
        _assert_same(_state(tr), before, field)
    with pytest.raises(FileNotFoundError, match="resume_rank0.pth"):
        _trainer().load_checkpoint(str(tmp_path / "nowhere"))
    with pytest.raises(ValueError, match="replay"):
        _trainer().save_checkpoint(str(tmp_path / "bad"), replay="all")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_the_sidecar_loads_with_weights_only(run):
    for d in run["dirs"].values():
        side = torch.load(os.path.join(d, "resume_rank0.pth"), weights_only=True)
        assert side["format_version"] == 1 and side["env_names"] == ["m3", "m4"] and side["envs_per_morph"] == [PER, PER]
    assert side["rounds"] == 2 and side["updates"] == 8 and side["driver"] == {"t": run["states"][2]["counters"][4]}
    assert side["agent"]["dropout_step"] is None and side["cuda_rng"] is None and side["replay"] == "none"
    assert len(side["agent"]["actor_optimizer"]["state"]) == len(list(_trainer().agent.actor.parameters()))


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy()


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        ckpt = os.path.join(out_dir, "ckpt")
        a = _trainer()
        _round(a)
        written = a.save_checkpoint(ckpt)                # both ranks; the barrier inside: every file is there when it returns
        out = {"n_written": len(written), "files": np.array(sorted(os.listdir(ckpt)))}
        _round(a)
        out["a_actor"], out["a_tot"] = _flat(a.agent.actor), a.tot_env_steps
        b = _trainer()                                   # a fresh pair
        out["b_loaded_tot"] = b.load_checkpoint(ckpt)
        out["b_actor_at_load"] = _flat(b.agent.actor)
        _round(b)
        out["b_actor"], out["b_tot"], out["b_rounds"] = _flat(b.agent.actor), b.tot_env_steps, b.rounds
        if rank == 0:
            out["a_critic"], out["b_critic"] = _flat(a.agent.critic), _flat(b.agent.critic)
            out["a_fill"] = np.array([x.max_sample_size for x in a.buffers])
            out["b_fill"] = np.array([x.max_sample_size for x in b.buffers])
        if rank == 1:                                    # alone: the refusal comes before any collective
            lone = os.path.join(out_dir, "lone")
            os.makedirs(lone)
            for fn in ("save.pth", "resume_rank0.pth"):
                shutil.copy(os.path.join(ckpt, fn), os.path.join(lone, fn))
            try:
                _trainer().load_checkpoint(lone)
                out["missing"] = "no error"
            except FileNotFoundError as e:
                out["missing"] = str(e)
        dist.barrier()
        np.savez(os.path.join(out_dir, "rank_%d.npz" % rank), **out)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_save_and_a_fresh_pair_resumes(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(os.path.join(str(tmp_path), "rank_%d.npz" % r)) for r in (0, 1))
    assert {"resume_rank0.pth", "resume_rank1.pth", "save.pth"} <= set(r0["files"]) and r1["n_written"] == 1 < r0["n_written"]
    for r in (r0, r1):
        assert (r["b_actor"] == r["a_actor"]).all() and r["b_tot"] == r["a_tot"] == r0["a_tot"] and r["b_rounds"] == 2
        assert np.abs(r["b_actor"] - r["b_actor_at_load"]).max() > 0       # the round after the load did update
    assert (r0["a_actor"] == r1["a_actor"]).all() and (r0["b_actor_at_load"] == r1["b_actor_at_load"]).all()
    assert (r0["b_critic"] == r0["a_critic"]).all() and (r0["b_fill"] == r0["a_fill"]).all()
    assert "resume_rank1.pth" in str(r1["missing"])
