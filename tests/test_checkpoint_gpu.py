"""`DeviceTrainer.save_checkpoint` / `load_checkpoint` (sgrl_amd/checkpoint.py) on the MI355X: the in-place restore under the
raw-pointer consumers (td3.clip_and_step's tables, mlp_hip.HipMlpOptim's binds and counters, the sink's device-side ring
pointers, the rollout's held weight pack) and under captured update graphs, and the engine's records.

Shapes: `3d_hopper_3_shin` (light: steps two environments to a wavefront) and `3d_walker_7_full` (not), three environments each --
a pair and a single per block --, episodes of 12 steps, batches of 8 rows, rings of 64 rows (they wrap within a test), warmup(10),
device_sampler and device_noise on unless a test is about the torch generators.

1  MLP agent, eager, every half of the update on HIP (library launches with fixed summation orders): A runs 2 + 2 rounds, B loads
   A's checkpoint -- as a fresh trainer, and as one that has already stepped -- and runs 2: every parameter, Adam tensor, ring row
   and pointer, engine record and counter and the summaries are equal bit for bit, with no proviso
2  SET agent, eager, both morphologies: two uninterrupted copies first, then the resumed copy against them; and what holds
   regardless: the state straight after the load is the state at the save, and a further round of pure collection is equal
3  the torch-generator path (device_sampler / device_noise off): the resumed copy samples the same rows and explores with the same
   noise -- `DeviceTrainer.gen`, `Rollout.gen` and the global CUDA generator
4  graphs survive an in-place load: an MLP trainer (GraphedMlpUpdates) and a SWAT trainer with dropout on the HIP kernels
   (GraphedUpdates): `stale` stays False (asserted BEFORE anything is replayed: a replay through a freed address is a memory
   fault, not an exception), nothing is captured again, and the round after the load reproduces the round after the save
5  engine state: `env.obs` after a load is the saved run's observation, and 14 steps with the same actions -- across the time
   limit's auto-reset, whose draw is keyed by the restored episode number -- keep obs, rew, done and the records equal
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ["3d_hopper_3_shin", "3d_walker_7_full"]
NETS = ("actor", "actor_target", "critic", "critic_target")
RINGS = ("obs_buffer", "action_buffer", "next_obs_buffer", "reward_buffer", "done_buffer")


def _trainer(kind, names=NAMES, warm=True, **kw):
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    over = {}
    if kind == "mlp":
        over = dict(actor_type="mlp", critic_type="mlp", mlp_hip_grads=True, mlp_hip_optim=True)
    elif kind == "swat":
        over = dict(actor_type="swat", critic_type="swat", swat_train_kernels=True, dropout_rate=0.1, swat_hip_dropout=True)
    args = default_train_args(max_episode_steps=12, batch_size=8, **over)
    kw.setdefault("device_sampler", True)
    kw.setdefault("device_noise", True)
    tr = DeviceTrainer(list(names), 3, args=args, seed=3, device=DEV, max_buffer_size=64, batch_size=8, **kw)
    if warm:
        tr.warmup(10)
    return tr


def _adam(opt):
    out = []
    for p in opt.param_groups[0]["params"]:
        st = opt.state.get(p) or {}
        out.append({k: st[k] for k in ("step", "exp_avg", "exp_avg_sq") if k in st})
    return out


def _tensors(tr):
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
    """Everything the contract names, copied: parameters, Adam tensors, ring rows and pointers (host and device side), engine
    records and counters, the observation the next step acts on, the trainer's counters."""
    st = {k: v.detach().clone() for k, v in _tensors(tr).items()}
    st["pointers"] = [(b.curr, b.max_sample_size) for b in tr.buffers]
    rec, cnt = tr.ro.env.get_records()
    st["engine.rec"], st["engine.cnt"] = torch.from_numpy(rec.copy()), torch.from_numpy(cnt.copy())
    st["env.obs"] = tr.ro.env.obs.detach().clone()
    step = tr.agent._dropout_step
    st["counters"] = (tr.tot_env_steps, tr._updates, tr.rounds, tr.draw, tr.ro.noise_step, None if step is None else int(step))
    return st


def _diff(a, b):
    bad = sorted(set(a) ^ set(b))
    for k in a:
        if k in b:
            same = (a[k].dtype == b[k].dtype and torch.equal(a[k], b[k])) if torch.is_tensor(a[k]) else a[k] == b[k]
            if not same:
                bad.append(k)
    return bad


def _assert_same(a, b, what):
    bad = _diff(a, b)
    assert not bad, (what, len(bad), bad[:8])


def _pointers_current(tr):
    """The sink's device-side write pointers are the rings' `curr` (or not made yet) and nothing is pending."""
    pos, pending = tr.sink.device_pointers()
    assert pending == 0 and (pos is None or pos == [b.curr for b in tr.buffers]), (pos, pending, [b.curr for b in tr.buffers])


def _run(tr, rounds, **kw):
    return [tr.train_round(**kw) for _ in range(rounds)]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mlp_run(tmp_path_factory):
    """Trainer A of test 1: 2 rounds, a checkpoint in each ring format, 2 more rounds.  Computed once, left unchanged."""
    root = tmp_path_factory.mktemp("mlp")
    a = _trainer("mlp", names=NAMES[:1])
    out = {"dirs": {"reference": str(root / "reference"), "filled": str(root / "filled")}, "summaries": _run(a, 2)}
    out["saved"] = _state(a)
    a.save_checkpoint(out["dirs"]["reference"])
    a.save_checkpoint(out["dirs"]["filled"], replay="filled")
    _assert_same(_state(a), out["saved"], "saving moved something")
    assert a.agent._mlp_optim is not None and a.agent._mlp_grads is not None          # the update did run on the HIP halves
    assert out["saved"]["counters"][1] >= 4                                           # updates of both kinds have run
    out["summaries"] += _run(a, 2)
    out["final"] = _state(a)
    print("mlp run: pointers at the save", out["saved"]["pointers"], "at the end", out["final"]["pointers"], "counters", out["final"]["counters"])
    assert all(f == 64 for _, f in out["final"]["pointers"])                          # the ring has wrapped within the test
    return out


@pytest.mark.parametrize("stepped,replay", [(False, "reference"), (True, "filled")])
def test_mlp_agent_resumes_bit_for_bit(mlp_run, stepped, replay):
    b = _trainer("mlp", names=NAMES[:1], warm=stepped)
    if stepped:                      # a live trainer somewhere else in its run: other weights, counts, rows, records, generators
        _run(b, 1)
        before = {k: v.data_ptr() for k, v in _tensors(b).items()}
    assert b.load_checkpoint(mlp_run["dirs"][replay]) == mlp_run["saved"]["counters"][0]
    _assert_same(_state(b), mlp_run["saved"], "after load")
    _pointers_current(b)
    o = b.agent._mlp_optim
    if stepped:
        assert {k: v.data_ptr() for k, v in _tensors(b).items()} == before
        assert o is not None and o.counts_current(True, True)
    else:
        assert o is None             # no update yet: the first one binds the restored state
    assert _run(b, 2) == mlp_run["summaries"][2:]
    _assert_same(_state(b), mlp_run["final"], "resumed")
    assert b.agent._mlp_optim.counts_current(True, True)
    _pointers_current(b)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def test_set_agent_resumes(tmp_path):
    a, control = _trainer("set"), _trainer("set")
    sa, sc = _run(a, 2, max_iters=3), _run(control, 2, max_iters=3)
    saved = _state(a)
    a.save_checkpoint(str(tmp_path), replay="filled")
    sa += _run(a, 2, max_iters=3)
    sc += _run(control, 2, max_iters=3)
    final = _state(a)
    reproducible = sa == sc and not _diff(final, _state(control))
    print("two uninterrupted SET trainers agree bit for bit:", reproducible, _diff(final, _state(control))[:6])
    b = _trainer("set", warm=False)
    b.load_checkpoint(str(tmp_path))
    _assert_same(_state(b), saved, "after load")          # deterministic whatever the updates do
    _pointers_current(b)
    assert reproducible, "the SET update is not reproducible run to run: see the printed keys"
    sb = _run(b, 2, max_iters=3)
    assert sb == sa[2:]
    _assert_same(_state(b), final, "resumed")
    # collection alone (no update): another round of both
    assert _run(a, 1, max_iters=0) == _run(b, 1, max_iters=0)
    _assert_same(_state(b), _state(a), "a round of pure collection")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_torch_generator_path_resumes(tmp_path):
    kw = dict(names=NAMES[:1], device_sampler=False, device_noise=False)
    a = _trainer("mlp", **kw)
    _run(a, 2)
    a.save_checkpoint(str(tmp_path), replay="filled")
    summary = _run(a, 1)
    final = _state(a)
    b = _trainer("mlp", **kw)
    _run(b, 1)                       # every generator has moved on from where a fresh trainer's stand
    b.load_checkpoint(str(tmp_path))
    assert _run(b, 1) == summary
    got = _state(b)
    _assert_same({k: v for k, v in got.items() if k.startswith("ring")}, {k: v for k, v in final.items() if k.startswith("ring")},
                 "the rows the next round stored (Rollout.gen)")
    _assert_same(got, final, "the parameters after it (DeviceTrainer.gen, the global CUDA generator)")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_mlp_graphs_survive_an_in_place_load(tmp_path):
    tr = _trainer("mlp", names=NAMES[:1], graph_updates=True)
    g = tr.graphed
    for _ in range(4):
        _run(tr, 1)
        if not g.stale(0) and not g.stale(1):
            break
    assert not g.stale(0) and not g.stale(1)
    tr.save_checkpoint(str(tmp_path), replay="filled")
    graphs = {flag: id(gr) for flag, gr in g.slots[None]["graphs"].items()}
    ptrs = {k: v.data_ptr() for k, v in _tensors(tr).items()}
    replays = g.replays
    summary = _run(tr, 1)
    n = summary[0]["per_morph_iter"]
    assert n >= 2 and g.replays - replays == n                             # every update of that round was a replay
    s1 = _state(tr)
    tr.load_checkpoint(str(tmp_path))
    assert {k: v.data_ptr() for k, v in _tensors(tr).items()} == ptrs
    assert not g.stale(0) and not g.stale(1)                               # before anything is replayed
    assert tr.agent._mlp_optim.counts_current(True, True)
    replays = g.replays
    assert _run(tr, 1) == summary
    assert g.replays - replays == n and {flag: id(gr) for flag, gr in g.slots[None]["graphs"].items()} == graphs
    _assert_same(_state(tr), s1, "the round after the load against the round after the save")


def _stale_in_update(tr, keys):
    """`stale` as the next update would see it: the stamp of a dropout graph carries the networks' `training` flags, and the
    trainer runs its updates in training mode (update_after_round) and everything else in eval mode."""
    tr.agent.models2train()
    try:
        return [key for key in keys if tr.graphed.stale(*key)]
    finally:
        tr.agent.models2eval()


def test_swat_dropout_graphs_survive_an_in_place_load(tmp_path):
    tr = _trainer("swat", graph_updates=True, graph_hip_kernels=True)
    g = tr.graphed
    assert g.dropout and g.hip_kernels
    keys = [(k, flag) for k in range(len(NAMES)) for flag in (0, 1)]
    for _ in range(4):                                                     # warm() runs inside the ordinary schedule
        _run(tr, 1, max_iters=4)
        if all(flag in g.slots.get(k, {"graphs": {}})["graphs"] for k, flag in keys):
            break
    assert set(g.warmed) == {0, 1} and all(flag in g.slots[k]["graphs"] for k, flag in keys)
    assert not _stale_in_update(tr, keys)
    step_ptr = tr.agent._dropout_step.data_ptr()
    tr.save_checkpoint(str(tmp_path), replay="filled")
    captures, ptrs = dict(g.captures), {k: v.data_ptr() for k, v in _tensors(tr).items()}
    summary = _run(tr, 1, max_iters=4)
    s1 = _state(tr)
    assert g.captures == captures and s1["counters"][5] > 0
    tr.load_checkpoint(str(tmp_path))
    assert {k: v.data_ptr() for k, v in _tensors(tr).items()} == ptrs and tr.agent._dropout_step.data_ptr() == step_ptr
    assert not _stale_in_update(tr, keys)                                  # before anything is replayed
    assert _run(tr, 1, max_iters=4) == summary
    assert g.captures == captures                                          # nothing was captured again
    _assert_same(_state(tr), s1, "the round after the load against the round after the save")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_engine_state_is_restored(tmp_path):
    a = _trainer("set")
    _run(a, 1, max_iters=0)
    a.save_checkpoint(str(tmp_path), replay=None)
    b = _trainer("set", warm=False)
    cnt_fresh = b.ro.env.get_records()[1].copy()
    b.load_checkpoint(str(tmp_path))
    ea, eb = a.ro.env, b.ro.env
    cnt = ea.get_records()[1]
    assert (cnt[:, 1] > cnt_fresh[:, 1]).all()                             # the saved run is episodes ahead of a fresh engine
    assert ea.paired_envs == 2 and ea.num_envs == 6                        # a pair and a single of the light morphology
    assert torch.equal(ea.obs, eb.obs)
    for x, y in zip(ea.get_records(), eb.get_records()):
        assert np.array_equal(x, y)
    gen = torch.Generator().manual_seed(11)
    resets = 0
    for t in range(14):
        act = (torch.rand((ea.num_envs, ea.action_max_len), generator=gen) * 2 - 1).to(DEV) * a.ro.act_mask
        outs = [[v.clone() for v in env.step_device(act.contiguous())[:3]] for env in (ea, eb)]
        for name, x, y in zip(("obs", "rew", "done"), outs[0], outs[1]):
            assert torch.equal(x, y), (t, name)
        for x, y in zip(ea.get_records(), eb.get_records()):
            assert np.array_equal(x, y), t
        resets += int(outs[0][2].sum())
    assert resets >= ea.num_envs                                           # every environment crossed an auto-reset
