"""Graphed SWAT / SMP updates on the HIP kernels, on the MI355X: the loss kernels (csrc/td3_loss.hip through the C ABI and through
train_ops.twin_mse / neg_mean) against the float64 restatement of tests/td3_loss_restate.py; td3.GraphedUpdates(hip_kernels=True)
replaying a SWAT and an SMP update -- HIP target chain, training kernels, loss kernels, table optimizer -- against the same agent
updated eagerly, to the bit; a graph made stale by a regrown workspace; td3.Agent(loss_kernels=True) against float64 modules; a
DeviceTrainer round with graph_hip_kernels=True.

Bars.  Loss kernels: 1 float32 ulp of the float32-rounded restatement -- the sums are float64 over at most 1e5 terms (relative error
<= n 2^-53, far below 2^-24), so only the final rounding can differ, by at most one ulp.  Replay against eager: identity
(torch.equal) -- a replay issues the same kernels with the same arguments in the same stream order (tests/test_mlp_graph_gpu.py
holds the MLP graphs to the same bar).  Loss switch: per loss max(4 x the switch-off agent's relative deviation from float64, 1e-5),
the bar of tests/test_swat_train_gpu.py for the same comparison."""
import copy
import ctypes

import numpy as np
import pytest

import td3_loss_restate as R

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
NS = [1, 63, 64, 65, 255, 256, 257, 3 * 12, 7 * 12, 15 * 257, 100003]
GUARD = 64


# ---- 1: the loss kernels ---------------------------------------------------------------------------------------------------------
def _within_one_ulp(got, ref64):
    """got (float32) against the float32-rounded float64 reference: at most one float32 ulp apart, element by element."""
    got = np.asarray(got, dtype=np.float32).reshape(-1)
    ref = np.asarray(ref64, dtype=np.float64).reshape(-1).astype(np.float32)
    ulp = np.spacing(np.abs(ref))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    return bool(np.all(np.isfinite(got)) and np.all(err <= ulp.astype(np.float64))), float(np.max(err / ulp.astype(np.float64)))


def _guarded(n):
    """A NaN-filled buffer of n + GUARD floats: the kernel may write its first n only."""
    import torch
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda:0")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("g", [1.0, -0.37])
def test_loss_kernels_match_the_restatement(n, g):
    import torch
    from sgrl_amd import train_ops
    L = train_ops._L()
    rs = np.random.RandomState(n)
    q1, q2, t = [(0.6 * rs.standard_normal(n)).astype(np.float32) for _ in range(3)]
    dq1, dq2, dq, gt = (torch.from_numpy(x).cuda() for x in (q1, q2, t, np.asarray([g], dtype=np.float32)))
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        loss, nm = _guarded(1), _guarded(1)
        o1, o2, o3 = _guarded(n), _guarded(n), _guarded(n)
        assert L.sgrl_td3_twin_mse_forward(p(dq1), p(dq2), p(dq), n, p(loss), st) == 0
        assert L.sgrl_td3_twin_mse_backward(p(dq1), p(dq2), p(dq), n, p(gt), p(o1), p(o2), st) == 0
        assert L.sgrl_td3_neg_mean_forward(p(dq1), n, p(nm), st) == 0
        assert L.sgrl_td3_neg_mean_backward(n, p(gt), p(o3), st) == 0
        torch.cuda.synchronize()
        outs = [x.cpu().numpy() for x in (loss, nm, o1, o2, o3)]
        for x, used in zip(outs, (1, 1, n, n, n)):
            assert np.isnan(x[used:]).all() and x[used:].size == GUARD          # the guard band is intact
        runs.append([x[:used] for x, used in zip(outs, (1, 1, n, n, n))])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))             # the same bits run to run
    loss, nm, o1, o2, o3 = runs[0]
    g32 = float(np.float32(g))                                                  # the upstream gradient as the device scalar holds it
    r1, r2 = R.twin_mse_backward(q1, q2, t, g32)
    worst = []
    for got, ref in ((loss, R.twin_mse_forward(q1, q2, t)), (nm, R.neg_mean_forward(q1)), (o1, r1), (o2, r2), (o3, R.neg_mean_backward(n, g32))):
        ok, w = _within_one_ulp(got, ref)
        worst.append(w)
        assert ok, (n, g, w)
    print("n %d g %g: worst error in ulps: loss %.3g neg_mean %.3g dq1 %.3g dq2 %.3g dq %.3g" % ((n, g) + tuple(worst)))
    # the autograd functions over the same entry points: the same bits as the raw calls
    a, b = dq1.clone().requires_grad_(), dq2.clone().requires_grad_()
    tl = train_ops.twin_mse(a, b, dq)
    assert type(tl.grad_fn).__name__ == "_TwinMseFnBackward" and tl.shape == ()
    (tl * g).backward()
    c = dq1.clone().requires_grad_()
    nl = train_ops.neg_mean(c)
    assert type(nl.grad_fn).__name__ == "_NegMeanFnBackward" and nl.shape == ()
    (nl * g).backward()
    for got, want in ((tl.detach().reshape(1), loss), (nl.detach().reshape(1), nm), (a.grad, o1), (b.grad, o2), (c.grad, o3)):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_loss_functions_fall_back_where_the_kernels_do_not_apply():
    import torch
    import torch.nn.functional as F
    from sgrl_amd import train_ops
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    q1, q2, t = (torch.randn((12, 7), device="cuda:0", generator=gen) for _ in range(3))
    with torch.no_grad():
        assert torch.equal(train_ops.twin_mse(q1, q2, t), F.mse_loss(q1, t) + F.mse_loss(q2, t))
        assert torch.equal(train_ops.neg_mean(q1), -q1.mean())
    a = q1.clone().requires_grad_()
    assert type(train_ops.twin_mse(a.t(), q2.t(), t.t()).grad_fn).__name__ == "AddBackward0"                 # non-contiguous
    assert type(train_ops.neg_mean(a.t()).grad_fn).__name__ == "NegBackward0"
    assert type(train_ops.twin_mse(a.double(), q2.double(), t.double()).grad_fn).__name__ == "AddBackward0"   # float64
    with pytest.warns(UserWarning, match="target size"):                                                      # a broadcast target, as F.mse_loss takes it
        assert type(train_ops.twin_mse(a, q2, t[:, :1]).grad_fn).__name__ == "AddBackward0"
    assert type(train_ops.twin_mse(a, q2, t).grad_fn).__name__ == "_TwinMseFnBackward"


# ---- 2, 3: replay equals eager ---------------------------------------------------------------------------------------------------
def _graph_dicts(names):
    import torch
    from sgrl_amd import graph as G, mjcf
    return [G.getGraphDict(mjcf.load_asset(n).parents, TRAV, [], device=torch.device("cuda:0")) for n in names]


def _args(atype, **over):
    from sgrl_amd.td3 import default_train_args
    kw = dict(actor_type=atype, critic_type=atype)
    if atype == "smp":
        kw.update(td=True, bu=True)
    kw.update(over)
    return default_train_args(**kw)


def _pair(atype, seed):
    """(graphed-to-be agent, eager agent) from one state_dict, targets away from the online networks, both with the training
    kernels and the loss kernels on; the eager one with capturable Adam groups (what GraphedUpdates sets on the other)."""
    import torch
    from sgrl_amd.td3 import Agent
    kw = {atype + "_train_kernels": True, "loss_kernels": True}
    torch.manual_seed(seed)
    a = Agent(_args(atype), device=torch.device("cuda:0"), **kw)
    b = Agent(_args(atype), device=torch.device("cuda:0"), **kw)
    with torch.no_grad():
        gen = torch.Generator(device="cuda:0").manual_seed(seed + 1)
        for mod in (a.actor_target, a.critic_target):
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.02)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    for opt in (b.actor_optimizer, b.critic_optimizer):
        for g in opt.param_groups:
            g["capturable"] = True
    a.models2train()
    b.models2train()
    return a, b


def _batch(L, B, seed):
    import torch
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    r = lambda *s: torch.rand(s, device="cuda:0", generator=gen)
    return {"obs": torch.randn((B, 41 * L), device="cuda:0", generator=gen), "next_obs": torch.randn((B, 41 * L), device="cuda:0", generator=gen),
            "action": r(B, 3 * L) * 2 - 1, "reward": r(B, 1) * 2 - 1, "done": (r(B, 1) < 0.3).float()}


def _switches(agent, atype):
    return (getattr(agent, "use_%s_hip" % atype), getattr(agent, "use_%s_train_kernels" % atype), agent.actor.train_kernels,
            agent.critic.train_kernels, agent.actor_target.train_kernels, agent.critic_target.train_kernels, agent.use_loss_kernels)


def _eager_twin_step(eager, gu, key, gd, batch, it):
    """The update the graphed agent has just made on slot `key`, made eagerly with the trainer-path arguments and the slot's noise."""
    eager.change_morphology(gd)
    return eager.update(batch, it, noise=gu.slots[key]["noise"].clone(), lazy_stats=True, skip_unused_critic_grads=True)


def _assert_same_state(graphed, eager, what):
    import torch
    for nm in ("actor", "critic", "actor_target", "critic_target"):
        for (name, p), q in zip(getattr(graphed, nm).named_parameters(), getattr(eager, nm).parameters()):
            assert torch.equal(p, q), (what, nm, name, float((p - q).abs().max()))
    for nm in ("actor_optimizer", "critic_optimizer"):
        og, oe = getattr(graphed, nm), getattr(eager, nm)
        net = graphed.actor if nm == "actor_optimizer" else graphed.critic
        names = {id(p): n for n, p in net.named_parameters()}
        pairs = list(zip(og.param_groups[0]["params"], oe.param_groups[0]["params"]))
        assert len(og.state) == len(oe.state) > 0
        for p, q in pairs:
            sg, se = og.state.get(p, {}), oe.state.get(q, {})
            assert sg.keys() == se.keys(), (what, nm, names[id(p)])
            for k in sg:
                assert torch.equal(sg[k], se[k]), (what, nm, names[id(p)], k)


def _same_losses(out, ref, what):
    import torch
    assert out.keys() == ref.keys(), what
    for k in out:
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])), (what, k, float(out[k]), float(ref[k]))


@pytest.mark.parametrize("atype", ["swat", "smp"])
def test_replay_equals_the_eager_update_to_the_bit(atype):
    import torch
    from sgrl_amd.td3 import GraphedUpdates
    names = ["3d_hopper_3_shin", "3d_walker_7_full"]         # 36 and 84 rows at B = 12: a chain and a branching tree
    B = 12
    graphed, eager = _pair(atype, seed=50)
    before = _switches(graphed, atype)
    assert before == (True, True, True, True, False, False, True)
    gu = GraphedUpdates(graphed, B, hip_kernels=True)
    assert _switches(graphed, atype) == before == _switches(eager, atype)       # the constructor touched no switch
    morphs = [(gd, len(gd["parents"])) for gd in _graph_dicts(names)]
    start = [p.detach().clone() for p in graphed.critic.parameters()]
    for key, (gd, L) in enumerate(morphs):                   # two warm-up updates per morphology, mirrored one by one
        for it in range(2):
            batch = _batch(L, B, seed=100 * key + it)
            out = gu.warm(key, gd, L, batch, iters=1, first_it=it)[0]
            _same_losses(out, _eager_twin_step(eager, gu, key, gd, batch, it), ("warm", key, it))
    _assert_same_state(graphed, eager, "after the warm-up")
    assert gu.captures == {}
    for it in range(4):                                      # alternating keys: the handles switch batch structure between replays
        for key, (gd, L) in enumerate(morphs):
            batch = _batch(L, B, seed=100 * key + 10 + it)
            assert not gu.stale(key, it % 2)
            out = gu.update(key, gd, L, batch, it)
            _same_losses(out, _eager_twin_step(eager, gu, key, gd, batch, it), (key, it))
    torch.cuda.synchronize()
    assert gu.captures == {(0, 0): 1, (0, 1): 1, (1, 0): 1, (1, 1): 1}          # each graph captured once, replayed afterwards
    _assert_same_state(graphed, eager, "after four iterations per morphology")
    assert _switches(graphed, atype) == before
    moved = max(float((p.detach() - s0).abs().max()) for p, s0 in zip(graphed.critic.parameters(), start))
    assert moved > 1e-4


# ---- 4: stale graphs -------------------------------------------------------------------------------------------------------------
# (the SMP agent's default max_children = 3 does not admit the cheetah's five-child torso: its handles regrow on 64 rows of walker_7)
@pytest.mark.parametrize("atype,big_name", [("swat", "3d_cheetah_14_full"), ("smp", "3d_walker_7_full")])
def test_a_stale_graph_is_captured_again_not_replayed(atype, big_name):
    import torch
    from sgrl_amd.td3 import GraphedUpdates
    B = 12
    graphed, eager = _pair(atype, seed=60)
    gu = GraphedUpdates(graphed, B, hip_kernels=True)
    gd, big = _graph_dicts(["3d_hopper_3_shin", big_name])
    L, Lb = len(gd["parents"]), len(big["parents"])
    for it in range(2):
        batch = _batch(L, B, seed=200 + it)
        gu.warm(0, gd, L, batch, iters=1, first_it=it)
        _eager_twin_step(eager, gu, 0, gd, batch, it)
    for it in range(2):
        batch = _batch(L, B, seed=210 + it)
        gu.update(0, gd, L, batch, it)
        _eager_twin_step(eager, gu, 0, gd, batch, it)
    assert gu.captures == {(0, 0): 1, (0, 1): 1} and not gu.stale(0, 0) and not gu.stale(0, 1)
    # the agent's own target object on a 64-row batch of a larger morphology: its handles regrow their workspaces
    targets = graphed._hip_targets(batch["next_obs"])
    assert targets is gu.slots[0]["targets"]
    wide = _batch(Lb, 64, seed=220)
    targets.target_q(wide["next_obs"], torch.zeros((64, 3 * Lb), device="cuda:0"), wide["reward"], wide["done"], big,
                     graphed.args.noise_clip, graphed.args.discount)
    torch.cuda.synchronize()
    for flag in (0, 1):
        if not gu.stale(0, flag):
            pytest.fail("the stamp of graph (0, %d) did not follow the regrown workspaces: nothing is replayed" % flag)
    batch = _batch(L, B, seed=230)
    out = gu.update(0, gd, L, batch, 2)
    ref = _eager_twin_step(eager, gu, 0, gd, batch, 2)
    torch.cuda.synchronize()
    assert gu.captures == {(0, 0): 2, (0, 1): 1} and not gu.stale(0, 0) and gu.stale(0, 1)
    _same_losses(out, ref, "after the regrowth")
    _assert_same_state(graphed, eager, "after the regrowth")


# ---- 5: the loss switch at agent level ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("atype", ["swat", "smp"])
def test_loss_switch_stays_on_float64(atype, monkeypatch):
    import torch
    from sgrl_amd import train_ops
    from sgrl_amd.td3 import Agent
    dev = torch.device("cuda:0")
    torch.manual_seed(70)
    on = Agent(_args(atype), device=dev, loss_kernels=True)
    off = Agent(_args(atype), device=dev, loss_kernels=False)
    f64 = Agent(_args(atype), device=dev, use_hip=False)
    off.load_state_dict(on.state_dict())
    f64.load_state_dict(on.state_dict())
    f64.double()
    assert on.use_loss_kernels and not off.use_loss_kernels and not f64.use_loss_kernels
    g = _graph_dicts(["3d_walker_7_full"])[0]
    g64 = dict(g)
    g64["relation"] = g["relation"].double()
    calls = {"twin_mse": 0, "neg_mean": 0}
    for name in calls:
        def counted(*a, _f=getattr(train_ops, name), _n=name):
            out = _f(*a)
            calls[_n] += type(out.grad_fn).__name__ in ("_TwinMseFnBackward", "_NegMeanFnBackward")
            return out
        monkeypatch.setattr(train_ops, name, counted)
    losses = {"on": [], "off": [], "float64": []}
    for it in range(3):
        batch = _batch(7, 16, seed=300 + it)
        noise = torch.randn((16, 21), device=dev, generator=torch.Generator(device="cuda:0").manual_seed(310 + it)) * 0.2
        for tag, agent, gd in (("on", on, g), ("off", off, g), ("float64", f64, g64)):
            agent.change_morphology(gd)
            agent.models2train()
            b, n = ({k: v.double() for k, v in batch.items()}, noise.double()) if tag == "float64" else (batch, noise)
            out = agent.update(b, it, noise=n)
            losses[tag].append({k: float(torch.as_tensor(v).double()) for k, v in out.items() if k.startswith("loss/")})
    assert calls == {"twin_mse": 3, "neg_mean": 2}           # the switch-on agent's losses did run on the kernels
    for it in range(3):
        for k, ref in losses["float64"][it].items():
            d_on, d_off = abs(losses["on"][it][k] - ref) / abs(ref), abs(losses["off"][it][k] - ref) / abs(ref)
            print("%s it %d %s: float64 %.9g  switch off rel dev %.3g  switch on rel dev %.3g" % (atype, it, k, ref, d_off, d_on))
            assert np.isfinite(losses["on"][it][k]) and d_on <= max(4 * d_off, 1e-5), (it, k, d_on, d_off)


# ---- 6: DeviceTrainer ------------------------------------------------------------------------------------------------------------
def test_device_trainer_replays_swat_updates_on_the_kernels():
    import torch
    from sgrl_amd.swat_hip import HipSwatActor
    from sgrl_amd.td3 import GraphedUpdates
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full"]
    args = _args("swat", swat_train_kernels=True, loss_kernels=True, max_episode_steps=40)
    tr = DeviceTrainer(names, 4, args=args, seed=3, device="cuda:0", graph_updates=True, graph_hip_kernels=True, max_buffer_size=1024,
                       batch_size=16)
    agent = tr.agent
    assert isinstance(tr.graphed, GraphedUpdates) and tr.graphed.hip_kernels and isinstance(tr.ro.actor, HipSwatActor)
    assert agent.use_swat_hip and agent.use_swat_train_kernels and agent.use_loss_kernels
    assert agent.actor.train_kernels and agent.critic.train_kernels
    assert not agent.actor_target.train_kernels and not agent.critic_target.train_kernels
    tr.warmup(30)
    assert all(b.max_sample_size >= 16 for b in tr.buffers)
    obs = tr.ro.env.obs.clone()
    before = [p.detach().clone() for p in agent.actor.parameters()]
    out = tr.train_round(max_steps=60, max_iters=4)
    assert out["per_morph_iter"] >= 3                        # two eager warm-up iterations per morphology, then graphed ones
    for name in names:
        loss = tr.last_losses[name]
        assert all(np.isfinite(float(v)) for v in loss.values()), loss
    assert max(float((p.detach() - q).abs().max()) for p, q in zip(agent.actor.parameters(), before)) > 0
    assert tr.graphed.captures and all(v == 1 for v in tr.graphed.captures.values())
    assert agent.use_swat_hip and agent.use_swat_train_kernels and agent._targets is not None
    # the rollout's HIP forward reads the live weights: it equals the module's forward on the same observations
    a1 = tr.ro.policy_forward(obs).clone()
    env, row = tr.ro.env, 0
    for gd, c in zip(tr.graph_dicts, env.counts):
        L = len(gd["parents"])
        agent.actor.change_morphology(gd)
        with torch.no_grad():
            want = agent.actor(obs[row:row + c, :41 * L])
        assert float((a1[row:row + c, :3 * L] - want).abs().max()) < 1e-5
        row += c
