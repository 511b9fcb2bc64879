"""Dropout inside the HIP forwards of the SWAT networks (csrc/swat_actor.hip, include/sgrl_swat.h sgrl_swat_forward_dropout /
_forward_q_dropout / _td_target_dropout) on the MI355X: single networks and the TD3 target chain against float64 copies of the
PyTorch modules in training mode under the same train_ops.dropout_rng, the agent's `swat_hip_dropout` switch through three updates,
capture of the chain alone, graphed dropout updates (td3.GraphedUpdates(hip_kernels=True)) against an eager twin, and a two-round
DeviceTrainer.

The bar of every comparison with float64 ("bar 1" below): max(4 x the float32 MODULE's own deviation from float64 under the same
masks, 2e-5 x max(1, |ref|max)) -- the second term is what tests/test_swat_critic_gpu.py holds the plain forwards to."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import test_graphed_kernels_gpu as K
import test_swat_train_gpu as T

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567
STEP = 5
SITE0 = 5
ERR_ARG = -1
# 18 nodes: no multiple of the embed kernel's 8 nor of the row kernels' 4, L^2 = 9 puts the attention indices across Philox quads;
# 133 nodes: just past one 128-row product tile
SHAPES = {3: ("3d_walker_3_left_knee_right_knee", 6), 7: ("3d_walker_7_full", 19)}


def _step(value=STEP):
    import torch
    return torch.tensor([value], dtype=torch.int64, device="cuda:0")


def _perturb(mod, seed):
    """Default initialisation, biases and LayerNorm parameters away from 0 / 1 (as tests/test_swat_dropout_gpu.py)."""
    import torch
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n.endswith("bias") or "norm" in n:
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.1)


def _bar(dev32, ref):
    return max(4 * dev32, 2e-5 * max(1.0, float(ref.abs().max())))


@functools.lru_cache(maxsize=None)
def _case(L, cond, p):
    """One actor (41 -> 3) and one twin critic (44 -> 1 each) with dropout p in training mode, inputs for SHAPES[L], and -- computed
    ONCE -- the float64 modules' outputs under dropout_rng(SEED, STEP) from site SITE0 and the float32 modules' deviations from them."""
    import torch
    from sgrl_amd import train_ops
    from sgrl_amd.set_policy import default_args
    from sgrl_amd.swat_policy import CriticStructurePolicy, StructurePolicy
    name, B = SHAPES[L]
    g = T._graphs([name])[0]
    args = default_args(dropout_rate=p, condition_decoder_on_features=cond, transformer_norm=1)
    torch.manual_seed(10 * L + cond)
    pol = StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False, args).to("cuda:0").train()
    crit = CriticStructurePolicy(41, 3, 32, 1, 3, True, False, False, args).to("cuda:0").train()
    _perturb(pol, 1)
    _perturb(crit, 2)
    gen = torch.Generator(device="cuda:0").manual_seed(L)
    obs = torch.randn((B, 41 * L), device="cuda:0", generator=gen)
    act = torch.rand((B, 3 * L), device="cuda:0", generator=gen) * 2 - 1
    step = _step()
    c = dict(L=L, B=B, g=g, pol=pol, crit=crit, obs=obs, act=act, step=step, p=p)

    def run(mods, gd, dt):
        pol_, crit_ = mods
        pol_.change_morphology(gd)
        crit_.change_morphology(gd)
        out = []
        for f in (lambda: pol_(obs.to(dt)), lambda: crit_.Q1(obs.to(dt), act.to(dt))):
            with torch.no_grad(), train_ops.dropout_rng(SEED, step) as rng:
                rng.reserve(SITE0)
                out.append(f().double())
                assert rng.site == SITE0 + (13 if p > 0 else 0)
        return out

    c["ref"] = run((copy.deepcopy(pol).double(), copy.deepcopy(crit).double()), T._g64(g), torch.float64)
    f32 = run((pol, crit), g, torch.float32)
    c["dev32"] = [float((a - r).abs().max()) for a, r in zip(f32, c["ref"])]
    return c


def _hip_pair(c, **kw):
    """(actor output, Q1 output) of the case's networks through the dropout entries."""
    drop = (c["p"], SEED, c["step"], SITE0)
    a = c["pol"].hip_handle()
    a.configure([c["g"]], [c["B"]])
    q = c["crit"].hip_handle()
    q.configure([c["g"]], [c["B"]])
    return a.forward_batch(c["obs"], dropout=drop, **kw).clone(), q.q1.forward_q(c["obs"], c["act"], dropout=drop, **kw).clone()


# ---- 1, 2: single networks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("cond", [0, 1])
@pytest.mark.parametrize("L", [3, 7])
def test_single_networks_match_the_float64_modules_in_training_mode(L, cond, p):
    import torch
    from sgrl_amd import _lib
    c = _case(L, cond, p)
    lib = c["pol"].hip_handle().L
    assert lib.sgrl_swat_dropout_sites() == 13 and lib.sgrl_swat_dropout_launches() == 25 and lib.sgrl_swat_launches() == 22
    got = _hip_pair(c)
    for what, y, ref, dev32 in zip(("forward_dropout 41 -> 3", "forward_q_dropout 44 -> 1"), got, c["ref"], c["dev32"]):
        assert y.shape == ref.shape
        err, bar = float((y.double() - ref).abs().max()), _bar(dev32, ref)
        print("%s L %d B %d cond %d p %g: |hip - f64| %.3g  |module f32 - f64| %.3g  bar %.3g" % (what, L, c["B"], cond, p, err, dev32, bar))
        assert torch.isfinite(y).all() and err <= bar, (what, err, bar)
    # dropout acted: the eval-mode forward of the same weights is another function
    c["pol"].eval(), c["crit"].eval()
    try:
        a = c["pol"].hip_handle().forward_batch(c["obs"])
        q = c["crit"].hip_handle().q1.forward_q(c["obs"], c["act"])
    finally:
        c["pol"].train(), c["crit"].train()
    assert float((a - got[0]).abs().max()) > 1e-3 and float((q - got[1]).abs().max()) > 1e-3
    # without the argument a module in training mode is still refused, in today's words
    with pytest.raises(_lib.SgrlError, match=r"has no dropout.*call eval\(\)"):
        c["pol"].hip_handle().forward_batch(c["obs"])
    # the same (seed, step, site0) again: the same bits; another step on the device: other masks
    again = _hip_pair(c)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    c["step"].add_(1)
    try:
        other = _hip_pair(c)
    finally:
        c["step"].sub_(1)
    assert not torch.equal(other[0], got[0]) and not torch.equal(other[1], got[1])


# ---- 3: every site is live and separately numbered -----------------------------------------------------------------------------------
def test_every_site_of_a_network_draws_from_its_own_number():
    """site_map (tests only, include/sgrl_swat.h): the identity map is the NULL map bit for bit, and moving ONE of the 13 sites to
    another number (the others fixed) changes the output -- no site is skipped and none reads another's stream."""
    import torch
    c = _case(3, 0, 0.5)
    base = _hip_pair(c)
    ident = _hip_pair(c, site_map=list(range(13)))
    assert torch.equal(ident[0], base[0]) and torch.equal(ident[1], base[1])
    for k in range(13):
        sm = list(range(13))
        sm[k] += 1000
        moved = _hip_pair(c, site_map=sm)
        assert not torch.equal(moved[0], base[0]), ("actor", k)
        assert not torch.equal(moved[1], base[1]), ("critic", k)
    # two sites swapped: the streams are the sites', not the kernels'
    sm = list(range(13))
    sm[2], sm[4] = sm[4], sm[2]
    assert not torch.equal(_hip_pair(c, site_map=sm)[0], base[0])


# ---- 4: the ends of p ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 7])
def test_p_zero_is_the_plain_entry_bit_for_bit(L):
    import torch
    c = _case(L, 1, 0.0)                 # a module with rate 0 is served by the plain entries in training mode too
    a, q = _hip_pair(c)
    assert torch.equal(a, c["pol"].hip_handle().forward_batch(c["obs"]))
    assert torch.equal(q, c["crit"].hip_handle().q1.forward_q(c["obs"], c["act"]))


@pytest.mark.parametrize("L", [3, 7])
def test_p_one_drops_everything_and_stays_finite(L):
    import torch
    c = _case(L, 0, 1.0)
    for y, ref, dev32 in zip(_hip_pair(c), c["ref"], c["dev32"]):
        err, bar = float((y.double() - ref).abs().max()), _bar(dev32, ref)
        print("p = 1, L %d: |hip - f64| %.3g  |module f32 - f64| %.3g  bar %.3g" % (L, err, dev32, bar))
        assert torch.isfinite(y).all() and err <= bar


# ---- 5: the chain --------------------------------------------------------------------------------------------------------------------
def _agent(seed, p=0.1, cond=0, **kw):
    import torch
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(seed)
    args = default_train_args(actor_type="swat", critic_type="swat", dropout_rate=p, seed=77, condition_decoder_on_features=cond)
    agent = Agent(args, device=torch.device("cuda:0"), **kw)
    for k, mod in enumerate((agent.actor_target, agent.critic_target)):      # targets away from the online networks and each other
        _perturb(mod, seed + k)
        with torch.no_grad():
            gen = torch.Generator(device="cuda:0").manual_seed(seed + 10 + k)
            for q in mod.parameters():
                q.add_(torch.randn(q.shape, device="cuda:0", generator=gen) * 0.02)
    return agent


def _chain_batch(L, B, seed):
    """Noise beyond the clip, rewards of both signs (test_swat_critic_gpu._batch's draw), done 0 in one row at least and 1 in one."""
    batch, noise = T._batch(L, B, seed)
    done = batch["done"]
    if float(done.min()) == float(done.max()):
        done[0], done[1] = 0.0, 1.0
    assert 0 < float(done.sum()) < B and float(noise.abs().max()) > 0.5
    assert float(batch["reward"].min()) < 0 < float(batch["reward"].max())
    return batch, noise


def _module_targets(agent, gd, batch, noise, step, site0, dtype):
    """Agent.update_targets through the MODULES (the agent's switch is off, or it is float64) under dropout_rng from site0."""
    import torch
    from sgrl_amd import train_ops
    agent.change_morphology(gd)
    with train_ops.dropout_rng(SEED, step) as rng:
        rng.reserve(site0)
        _, t = agent.update_targets({k: v.to(dtype) for k, v in batch.items()}, noise.to(dtype))
        assert rng.site == site0 + 39
    return t.double()


@pytest.mark.parametrize("L,cond", [(3, 0), (7, 1)])
def test_chain_matches_float64_update_targets(L, cond):
    import torch
    from sgrl_amd.swat_hip import HipSwatTargets
    name, B = SHAPES[L]
    g = T._graphs([name])[0]
    agent = _agent(4 + L, cond=cond)
    agent.models2train()
    assert not agent.swat_hip_dropout and agent._hip_targets(torch.zeros(B, 41 * L, device="cuda:0")) is None
    a64 = copy.deepcopy(agent).double()
    a64.use_swat_hip = False
    hip = HipSwatTargets(agent.actor_target, agent.critic_target)
    lib = hip.L
    assert hip.dropout_launches() == lib.sgrl_swat_td_target_dropout_launches() == 3 * lib.sgrl_swat_dropout_launches() == 75
    assert hip.launches() == 66
    batch, noise = _chain_batch(L, B, seed=L)
    step = _step()
    a = agent.args
    run = lambda p=0.1: hip.target_q(batch["next_obs"], noise, batch["reward"], batch["done"], g, a.noise_clip, a.discount,
                                     dropout=(p, SEED, step, 7)).clone()
    got = run()
    for k in range(2):                                   # this step, then the step moved ON THE DEVICE
        ref = _module_targets(a64, T._g64(g), batch, noise, step, 7, torch.float64)
        dev32 = float((_module_targets(agent, g, batch, noise, step, 7, torch.float32) - ref).abs().max())
        err, bar = float((got.double() - ref).abs().max()), _bar(dev32, ref)
        print("chain L %d B %d cond %d step %d: max|target| %.3g  |hip - f64| %.3g  |modules f32 - f64| %.3g  bar %.3g"
              % (L, B, cond, int(step), float(ref.abs().max()), err, dev32, bar))
        assert got.shape == ref.shape == (B, L) and err <= bar, (err, bar)
        ended = batch["done"].reshape(-1) == 1
        assert torch.equal(got[ended], batch["reward"].reshape(-1)[ended][:, None].expand(-1, L))
        assert float((got[~ended] - batch["reward"][~ended]).abs().max()) > 1e-4
        assert torch.equal(run(), got)                   # the same (seed, step): the same bits
        if k == 0:
            first = got
            step.add_(1)
            got = run()
            assert not torch.equal(got, first)
    # p = 0 through the dropout entry: the plain chain's bits (the plain entry serves the modules in eval mode)
    agent.models2eval()
    plain = hip.target_q(batch["next_obs"], noise, batch["reward"], batch["done"], g, a.noise_clip, a.discount).clone()
    agent.models2train()
    assert torch.equal(run(0.0), plain)


# ---- 6: through the agent --------------------------------------------------------------------------------------------------------------
def test_three_updates_with_the_switch_on_stay_on_float64(monkeypatch):
    """Three Agent.update iterations of walker_3 at batch 6, dropout_rate 0.1: `swat_hip_dropout` on, off, and float64 PyTorch, one
    state_dict, the same batches, noise and seed.  The bar of test_swat_dropout_gpu.test_three_updates_with_dropout_stay_on_float64:
    every loss within max(4 x the switch-off agent's relative deviation, 1e-5) of float64, the parameters per tensor within
    max(4 x the switch-off deviation, 1e-5 x the largest float64 parameter)."""
    import torch
    from sgrl_amd import swat_hip, train_ops
    g = T._graphs([SHAPES[3][0]])[0]
    on, off, f64 = _agent(30, swat_hip_dropout=True), _agent(30), _agent(30, use_hip=False)
    off.load_state_dict(on.state_dict())
    f64.load_state_dict(on.state_dict())
    f64.double()
    assert on.swat_hip_dropout and on.use_swat_hip and not off.swat_hip_dropout and off.use_swat_hip and not f64.swat_hip_dropout
    agents = (("on", on, g), ("off", off, g), ("float64", f64, T._g64(g)))
    for _, agent, gd in agents:
        agent.change_morphology(gd)
        agent.models2train()
    assert isinstance(on._hip_targets(torch.zeros(6, 41 * 3, device="cuda:0")), swat_hip.HipSwatTargets)
    chain = []
    inner = swat_hip.HipSwatTargets.target_q
    monkeypatch.setattr(swat_hip.HipSwatTargets, "target_q", lambda self, *a, **k: chain.append(k.get("dropout")) or inner(self, *a, **k))
    data = [T._batch(3, 6, seed=40 + it) for it in range(3)]
    cast = lambda tag, b, n: ({k: v.double() for k, v in b.items()}, n.double()) if tag == "float64" else (b, n)
    losses = {tag: [] for tag, _, _ in agents}
    for it in range(3):
        for tag, agent, _ in agents:
            b, n = cast(tag, *data[it])
            before = dict(train_ops.dropout_calls)
            out = agent.update(b, it, noise=n)
            used = {key: train_ops.dropout_calls[key] - before[key] for key in before}
            online = (4 if it % 2 == 0 else 2) * 13        # two critics (+ actor and Q1 on a policy step): today's counts
            if tag == "on":                                # the modules' no-grad passes are gone
                assert used == dict(kernel=online, attention_kernel=0, counter=0, torch=0), (it, used)
            elif tag == "off":
                assert used == dict(kernel=online, attention_kernel=0, counter=39, torch=0), (it, used)
            assert int(agent._dropout_step) == it + 1
            losses[tag].append({k: float(torch.as_tensor(v).double()) for k, v in out.items() if k.startswith("loss/")})
    assert [d[:2] + d[3:] for d in chain] == [(on.dropout_rate, 77, 0)] * 3 and all(d[2] is on._dropout_step for d in chain)
    for it in range(3):
        for k, ref in losses["float64"][it].items():
            d_on, d_off = abs(losses["on"][it][k] - ref) / abs(ref), abs(losses["off"][it][k] - ref) / abs(ref)
            print("it %d %s: float64 %.9g  switch off rel dev %.3g  switch on rel dev %.3g" % (it, k, ref, d_off, d_on))
            assert np.isfinite(losses["on"][it][k]) and d_on <= max(4 * d_off, 1e-5), (it, k, d_on, d_off)
    named = lambda a: [("actor." + n, p) for n, p in a.actor.named_parameters()] + [("critic." + n, p) for n, p in a.critic.named_parameters()]
    ref = [p.detach().double().cpu() for _, p in named(f64)]
    scale = max(float(r.abs().max()) for r in ref)
    worst, failed = 0.0, []
    for (pname, a), (_, b), r in zip(named(on), named(off), ref):
        d_on, d_off = float((a.detach().double().cpu() - r).abs().max()), float((b.detach().double().cpu() - r).abs().max())
        bar = max(4 * d_off, 1e-5 * scale)
        worst = max(worst, d_on / bar)
        if not (np.isfinite(d_on) and d_on <= bar):
            failed.append((pname, d_on, d_off, bar))
    print("parameters after three updates: %d tensors, largest |p64| %.3g, worst deviation / bar %.3g" % (len(ref), scale, worst))
    assert not failed, failed


# ---- 7: capture of the chain alone ---------------------------------------------------------------------------------------------------
def test_captured_chain_moves_its_masks_with_the_device_step():
    import torch
    from sgrl_amd.swat_hip import HipSwatTargets
    L, (name, B) = 7, SHAPES[7]
    g = T._graphs([name])[0]
    agent = _agent(21)
    agent.models2train()
    hip = HipSwatTargets(agent.actor_target, agent.critic_target)
    batch, noise = _chain_batch(L, B, seed=6)
    step = _step()
    a = agent.args

    def run(out=None):
        return hip.target_q(batch["next_obs"], noise, batch["reward"], batch["done"], g, a.noise_clip, a.discount, out=out,
                            dropout=(0.1, SEED, step, 0))

    eager = run().clone()                                      # the handles' first calls: outside any capture
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    step.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    second = out.clone()
    assert torch.equal(second, run()) and not torch.equal(second, eager)


# ---- 8: graphed dropout updates ------------------------------------------------------------------------------------------------------
def test_graphed_dropout_updates_equal_the_eager_twin_to_the_bit():
    """The comparison of tests/test_graphed_kernels_gpu.test_replay_equals_the_eager_update_to_the_bit -- losses, parameters and
    optimizer state torch.equal to an eager twin's with the same switches, state, batches, noise and seed -- for a dropout agent."""
    import torch
    from sgrl_amd.td3 import GraphedUpdates
    B, key = 16, 0
    kw = dict(swat_hip_dropout=True, swat_train_kernels=True, loss_kernels=True)
    graphed, eager = _agent(50, **kw), _agent(50, **kw)
    eager.load_state_dict(copy.deepcopy(graphed.state_dict()))
    for opt in (eager.actor_optimizer, eager.critic_optimizer):
        for grp in opt.param_groups:
            grp["capturable"] = True
    graphed.models2train()
    eager.models2train()
    gu = GraphedUpdates(graphed, B, hip_kernels=True)
    assert gu.dropout and graphed.use_swat_hip and graphed.swat_hip_dropout and graphed.use_swat_train_kernels
    gd = K._graph_dicts([SHAPES[3][0]])[0]
    L = len(gd["parents"])
    for it in range(2):
        batch = K._batch(L, B, seed=100 + it)
        out = gu.warm(key, gd, L, batch, iters=1, first_it=it)[0]
        K._same_losses(out, K._eager_twin_step(eager, gu, key, gd, batch, it), ("warm", it))
    assert gu.captures == {} and gu.slots[key]["dropout_step"] is graphed._dropout_step
    for it in range(4):
        batch = K._batch(L, B, seed=110 + it)
        assert not gu.stale(key, it % 2)
        out = gu.update(key, gd, L, batch, it)
        K._same_losses(out, K._eager_twin_step(eager, gu, key, gd, batch, it), it)
    torch.cuda.synchronize()
    assert gu.captures == {(key, 0): 1, (key, 1): 1}
    assert int(graphed._dropout_step) == int(eager._dropout_step) == 6          # every replay moved the step: 2 eager + 4 graphed
    K._assert_same_state(graphed, eager, "after four graphed dropout updates")
    # the passes an update runs depend on the networks' modes: part of the stamp
    graphed.models2eval()
    assert gu.stale(key, 0) and gu.stale(key, 1)
    graphed.models2train()
    assert not gu.stale(key, 0) and not gu.stale(key, 1)
    # a step tensor that is not the warmed one: no capture on it
    graphed._dropout_step = graphed._dropout_step.clone()
    assert gu.stale(key, 0)
    with pytest.raises(RuntimeError, match="step tensor"):
        gu.update(key, gd, L, K._batch(L, B, seed=120), 0)


def test_graphed_updates_still_refuse_a_dropout_agent_without_the_chain():
    from sgrl_amd.td3 import GraphedUpdates
    for agent, hip_kernels in ((_agent(1), True), (_agent(1), False), (_agent(1, swat_hip_dropout=True), False)):
        with pytest.raises(NotImplementedError, match="dropout"):
            GraphedUpdates(agent, 16, hip_kernels=hip_kernels)


# ---- 9: the trainer --------------------------------------------------------------------------------------------------------------------
def test_device_trainer_trains_graphed_with_dropout():
    import torch
    from sgrl_amd import train_ops
    from sgrl_amd.td3 import GraphedUpdates, default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full"]
    args = default_train_args(actor_type="swat", critic_type="swat", swat_train_kernels=True, dropout_rate=0.1, max_episode_steps=40,
                              swat_hip_dropout=True)
    tr = DeviceTrainer(names, 2, args=args, seed=3, device="cuda:0", max_buffer_size=1024, batch_size=16, graph_updates=True,
                       graph_hip_kernels=True)
    agent = tr.agent
    assert isinstance(tr.graphed, GraphedUpdates) and tr.graphed.hip_kernels and tr.graphed.dropout
    assert agent.swat_hip_dropout and agent.use_swat_train_kernels and agent.dropout_seed == 3
    tr.warmup(30)
    before = [p.detach().clone() for p in agent.actor.parameters()]
    calls = dict(train_ops.dropout_calls)
    updates = 0
    for _ in range(2):
        out = tr.train_round(max_steps=60, max_iters=4)
        assert out["per_morph_iter"] >= 3
        updates += out["per_morph_iter"] * len(names)
        for name in names:
            assert all(np.isfinite(float(v)) for v in tr.last_losses[name].values()), tr.last_losses[name]
        assert not agent.actor.training and not agent.critic_target.training           # collection runs in eval mode
    assert int(agent._dropout_step) == updates
    assert tr.graphed.captures and all(v == 1 for v in tr.graphed.captures.values())
    # no target chain ran the modules: that is 39 restated calls per update.  (The few there are belong to the online passes, as
    # they do without the switch: site 0 of Q1 in an eager or recorded policy step, whose critic parameters take no gradient.)
    assert train_ops.dropout_calls["counter"] - calls["counter"] < 39 and updates >= 6 and train_ops.dropout_calls["torch"] == calls["torch"]
    assert max(float((p.detach() - q).abs().max()) for p, q in zip(agent.actor.parameters(), before)) > 0


# ---- 10: argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    import torch
    from sgrl_amd.swat_hip import HipSwatTargets
    L, B = 3, 6
    g3, g7 = T._graphs([SHAPES[3][0], SHAPES[7][0]])
    agent = _agent(9)
    hip = HipSwatTargets(agent.actor_target, agent.critic_target)
    hip.configure([g3], [B])
    for h in (hip.actor, hip.critic.q1, hip.critic.q2):
        h.sync_weights(dropout=True)
    lib = hip.L
    batch, noise = _chain_batch(L, B, seed=3)
    obs, act = batch["next_obs"], batch["action"]
    step = _step()
    vp, cf, u64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64
    ptr = lambda t: vp(None if t is None else t.data_ptr())
    st = vp(torch.cuda.current_stream().cuda_stream)
    out_a = torch.full((B, 3 * L), 7.5, device="cuda:0")
    out_q = torch.full((B, L), 7.5, device="cuda:0")
    a, q1, q2 = hip.actor.h, hip.critic.q1.h, hip.critic.q2.h
    entries = {
        "sgrl_swat_forward_dropout": lambda p, s, site0, o=obs: lib.sgrl_swat_forward_dropout(
            a, ptr(o), 41 * L, ptr(out_a), 3 * L, cf(1.0), cf(p), u64(SEED), ptr(s), site0, vp(None), st),
        "sgrl_swat_forward_q_dropout": lambda p, s, site0, o=obs: lib.sgrl_swat_forward_q_dropout(
            q1, ptr(o), 41 * L, ptr(act), 3 * L, 3, ptr(out_q), L, cf(p), u64(SEED), ptr(s), site0, vp(None), st),
        "sgrl_swat_td_target_dropout": lambda p, s, site0, o=obs: lib.sgrl_swat_td_target_dropout(
            a, q1, q2, ptr(o), 41 * L, ptr(noise), 3 * L, ptr(batch["reward"]), ptr(batch["done"]), cf(1.0), cf(0.5), cf(0.99), ptr(out_q), L,
            cf(p), u64(SEED), ptr(s), site0, st)}
    last = {"sgrl_swat_forward_dropout": (1 << 24) - 13, "sgrl_swat_forward_q_dropout": (1 << 24) - 13,
            "sgrl_swat_td_target_dropout": (1 << 24) - 39}           # the largest site0 whose last site is 2^24 - 1

    def refused(name, *args, **kw):
        assert entries[name](*args, **kw) == ERR_ARG, (name, args)
        assert name.encode() in lib.sgrl_swat_last_error(), (name, args, lib.sgrl_swat_last_error())

    for name in entries:
        for p in (-0.01, 1.01, float("nan"), float("inf")):
            refused(name, p, step, 0)
        refused(name, 0.1, None, 0)                      # a null step_dev
        refused(name, 0.1, step, -1)
        refused(name, 0.1, step, last[name] + 1)
        refused(name, 0.1, step, (1 << 31) - 1)          # no overflow on the way to the last site
        refused(name, 0.1, step, 0, o=None)              # what the plain entry refuses
    bad_map = (ctypes.c_int32 * 13)(*([0] * 12 + [-1]))
    assert lib.sgrl_swat_forward_dropout(a, ptr(obs), 41 * L, ptr(out_a), 3 * L, cf(1.0), cf(0.1), u64(SEED), ptr(step), 0,
                                         ctypes.cast(bad_map, vp), st) == ERR_ARG
    # more than one morphology in the batch structure
    hip.configure([g3, g7], [2, 4])
    wide = torch.zeros((6, 41 * 7), device="cuda:0")
    wide_act = torch.zeros((6, 3 * 7), device="cuda:0")
    big_a, big_q = torch.full((6, 21), 7.5, device="cuda:0"), torch.full((6, 7), 7.5, device="cuda:0")
    rc = [lib.sgrl_swat_forward_dropout(a, ptr(wide), 41 * 7, ptr(big_a), 21, cf(1.0), cf(0.1), u64(SEED), ptr(step), 0, vp(None), st),
          lib.sgrl_swat_forward_q_dropout(q1, ptr(wide), 41 * 7, ptr(wide_act), 21, 3, ptr(big_q), 7, cf(0.1), u64(SEED), ptr(step), 0, vp(None), st),
          lib.sgrl_swat_td_target_dropout(a, q1, q2, ptr(wide), 41 * 7, ptr(wide_act), 21, ptr(batch["reward"]), ptr(batch["done"]), cf(1.0),
                                          cf(0.5), cf(0.99), ptr(big_q), 7, cf(0.1), u64(SEED), ptr(step), 0, st)]
    assert rc == [ERR_ARG] * 3 and b"one morphology" in lib.sgrl_swat_last_error()
    torch.cuda.synchronize()
    for t in (out_a, out_q, big_a, big_q):
        assert bool((t == 7.5).all())
    # the ends are valid: p = 1 at the last site0 launches and writes
    hip.configure([g3], [B])
    for name in entries:
        assert entries[name](1.0, step, last[name]) == 0, lib.sgrl_swat_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_a).all()) and bool(torch.isfinite(out_q).all()) and not bool((out_a == 7.5).any())
