"""The one-call TD3 target chain of a SET agent (set_hip.HipSetTargets over sgrl_set_td_target) on the device.

Yardstick: the COMPOSED path on the same handles -- `forward_batch`, the float32 PyTorch element-wise operations of
td3.Agent.update_targets (clamp, +, clamp), `forward_q` twice, torch.min and the Bellman line.  The chain must equal it bit for bit:
its epilogue modes run the same operations, one IEEE float32 operation each, on the values the heads' last kernels hold.  Weights:
full rank (tests/set_targets_restate.py, weight set 3); inputs qualified by tests/test_set_targets.py on the CPU.

Against float64 (test_chain_against_the_float64_restatement): the composed path -- the forwards as they were before the chain --
deviates from tests/set_targets_restate.py by 5.9e-8 (walker x 5, bound 2.98e-5) and 4.0e-8 / 5.1e-8 / 5.9e-8 (the mixed batch's
hopper / cheetah / walker rows, bounds 2.62e-5 / 2.49e-5 / 2.48e-5): far below half the project's bound set_full_rank_ref.TOL_Q x
max |target_ref|, which therefore is the bar the chain is held to (measured chain deviation: the same figures, bit for bit).

Agent level (the last three tests).  The switch-off agent's `critic_target(...)` under no_grad runs, by the module's default
(set_policy.TWIN_TARGETS = True), BOTH target critics in one pass of the training kernels (set_policy.twin_forward) -- not two HIP
forwards -- so its values differ from the composed path's, and from the chain's, by float32 rounding (measured with the chain
forced on there: max |target on - off| 0 / 0 / 3.0e-8 over three updates, max parameter difference 7.5e-9 after three eager and
1.5e-8 after five graphed updates).  The switch promises the switch-off agent's results, so Agent._hip_targets lets the chain run only
where that agent takes two forwards, and yields to the twin pass elsewhere.  The agent tests run on both routes and assert the same
bit identity of all four networks: `two_forwards` pins TWIN_TARGETS = False and the chain must have run; `module_default` leaves the
module as it is and the chain must have yielded."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _pair(seed):
    """(SEPolicy, SECritic) on the device at weight set `seed` of tests/set_targets_restate.py."""
    import set_targets_restate as S
    from sgrl_amd.set_policy import make_critic, make_policy
    pol = S.apply_actor(seed)(make_policy(device=DEV, use_hip=True, max_action=S.MAX_ACTION).eval())
    crit = S.apply_critic(seed)(make_critic(device=DEV).eval())
    return pol, crit


class Ctx(object):
    def __init__(self):
        import torch
        import set_full_rank_ref as R
        import set_targets_restate as S
        from sgrl_amd.set_hip import HipSetTargets
        assert torch.cuda.is_available()
        self.torch, self.R, self.S = torch, R, S
        self.pol, self.crit = _pair(S.SEED)
        self.targets = HipSetTargets(self.pol, self.crit)
        self._graphs, self._f64 = {}, None

    def graph(self, name):
        if name not in self._graphs:
            self._graphs[name] = self.R.graph_dict(name, DEV)
        return self._graphs[name]

    def batch(self, names, counts, seed=0, pad_nan=False, Lmax=None):
        """(next_obs [B, 41 Lmax], noise [B, 3 Lmax], reward [B], done [B], blocks) on the device; rows of shorter morphologies are
        padded with zeros (observations) and zeros or NaN (noise)."""
        t, S = self.torch, self.S
        blocks, reward, done = S.inputs(names, counts, seed)
        Lmax = Lmax or max(b[1] for b in blocks)
        B = sum(counts)
        obs = np.zeros((B, 41 * Lmax), dtype=np.float32)
        noise = np.full((B, 3 * Lmax), np.nan if pad_nan else 0.0, dtype=np.float32)
        r = 0
        for n, L, c, o, nz in blocks:
            obs[r:r + c, :41 * L], noise[r:r + c, :3 * L] = o, nz
            r += c
        dev = lambda a: t.from_numpy(a).to(DEV)
        return dev(obs), dev(noise), dev(reward), dev(done), blocks

    def f64(self):
        if self._f64 is None:
            self._f64 = self.S.cpu_pair(self.S.SEED)
        return self._f64


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def composed(tg, graphs, counts, obs, noise, reward, done, noise_clip, discount):
    """td3.Agent.update_targets' own lines over the handles' forwards (the path that exists without the chain)."""
    import torch
    tg.configure(graphs, counts)
    max_action = float(tg.actor.policy.max_action)
    noise = noise.clamp(-noise_clip, noise_clip)
    next_action = (tg.actor.forward_batch(obs) + noise).clamp(-max_action, max_action)
    q1, q2 = tg.q1.forward_q(obs, next_action), tg.q2.forward_q(obs, next_action)
    target_q = torch.min(q1, q2)
    return reward.reshape(-1, 1) + ((1.0 - done.reshape(-1, 1)) * discount * target_q)


def _same(t, got, ref, what):
    diff = float((got - ref).abs().max())
    print("SETTARGETS %s | max |chain - composed| %.3e | max |composed| %.3e" % (what, diff, float(ref.abs().max())))
    assert not bool(t.isnan(got).any()) and t.equal(got, ref), what


def _one_morph(ctx, name, B, seed=0):
    S = ctx.S
    obs, noise, reward, done, _ = ctx.batch([name], [B], seed)
    g = ctx.graph(name)
    chain = ctx.targets.target_q(obs, noise, reward, done, g, S.NOISE_CLIP, S.DISCOUNT).clone()
    return chain, composed(ctx.targets, [g], [B], obs, noise, reward, done, S.NOISE_CLIP, S.DISCOUNT)


# ---- 1, 2 ---------------------------------------------------------------------------------------------------------------------
def test_small_batch_path_equals_the_composed_path(ctx):
    chain, ref = _one_morph(ctx, "3d_walker_7_full", 5)
    assert ctx.targets.actor.num_nodes == 35 and chain.shape == (5, 7)
    _same(ctx.torch, chain, ref, "walker x 5, small-batch path")
    assert float(chain.abs().max()) > 0.5


def test_tile_path_equals_the_composed_path(ctx):
    tg = ctx.targets
    try:
        for h in (tg.actor, tg.q1, tg.q2):
            h.debug_small_nodes(0)
        chain, ref = _one_morph(ctx, "3d_walker_7_full", 5)
    finally:
        for h in (tg.actor, tg.q1, tg.q2):
            h.debug_small_nodes(-1)
    _same(ctx.torch, chain, ref, "walker x 5, tile path (k_head_out2)")
    small, _ = _one_morph(ctx, "3d_walker_7_full", 5)
    assert float((small - chain).abs().max()) < 2e-5 * float(small.abs().max())       # the two paths agree to rounding


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def _mixed(ctx, q_ld=16):
    """(chain [6, 16] on the mixed batch with NaN noise padding, [(name, row 0, c, L, composed [c, L])])"""
    S = ctx.S
    names, counts = S.MIXED
    obs, noise, reward, done, blocks = ctx.batch(names, counts, pad_nan=True)
    tg = ctx.targets
    chain = tg.target_q(obs, noise, reward, done, [ctx.graph(n) for n in names], S.NOISE_CLIP, S.DISCOUNT, counts=counts, q_ld=q_ld).clone()
    assert tg.actor.max_limbs == 14 and tg.actor.num_nodes == 44
    parts, r = [], 0
    for n, L, c, _, _ in blocks:
        ref = composed(tg, [ctx.graph(n)], [c], obs[r:r + c, :41 * L].contiguous(), noise[r:r + c, :3 * L].contiguous(),
                       reward[r:r + c], done[r:r + c], S.NOISE_CLIP, S.DISCOUNT)
        parts.append((n, r, c, L, ref))
        r += c
    return chain, parts


def test_mixed_batch_with_nan_beyond_the_noise_rows(ctx):
    t = ctx.torch
    chain, parts = _mixed(ctx)
    assert chain.shape == (6, 16)
    assert not bool(t.isnan(chain).any())
    for n, r, c, L, ref in parts:
        _same(t, chain[r:r + c, :L], ref, "mixed batch, " + n)
        assert bool((chain[r:r + c, L:] == 0).all()), n


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_two_half_forward_equals_the_composed_path(ctx):
    S, tg = ctx.S, ctx.targets
    name, B = "3d_cheetah_14_full", 147
    obs, noise, reward, done, _ = ctx.batch([name], [B], seed=2)
    g = ctx.graph(name)
    chain = tg.target_q(obs, noise, reward, done, g, S.NOISE_CLIP, S.DISCOUNT).clone()
    assert tg.actor.num_nodes == 2058 and tg.actor.last_split() > 0
    ref = composed(tg, [g], [B], obs, noise, reward, done, S.NOISE_CLIP, S.DISCOUNT)
    _same(ctx.torch, chain, ref, "cheetah x 147, two-half forward")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
def test_edges(ctx, B):
    t, S, tg = ctx.torch, ctx.S, ctx.targets
    name = "3d_walker_7_full"
    obs, noise, reward, done, _ = ctx.batch([name], [B], seed=3)
    g = ctx.graph(name)
    run = lambda **kw: tg.target_q(obs, kw.get("noise", noise), kw.get("reward", reward), kw.get("done", done), g,
                                   kw.get("clip", S.NOISE_CLIP), kw.get("discount", S.DISCOUNT)).clone()
    base = run()
    rows = reward.reshape(-1, 1).expand(B, 7)
    assert t.equal(run(done=t.ones_like(done)), rows)                   # every row done: the reward, broadcast exactly
    assert t.equal(run(discount=0.0), rows)
    assert t.equal(run(clip=0.0), run(noise=t.zeros_like(noise)))
    assert not t.equal(run(noise=t.zeros_like(noise)), base)
    assert t.equal(run(reward=reward.reshape(B, 1), done=done.reshape(B, 1)), base)
    _same(t, base, composed(tg, [g], [B], obs, noise, reward, done, S.NOISE_CLIP, S.DISCOUNT), "walker x %d" % B)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_critic_handles_in_the_other_order(ctx):
    tg = ctx.targets
    chain, ref = _one_morph(ctx, "3d_cheetah_14_full", 5)
    tg.q1, tg.q2 = tg.q2, tg.q1
    try:
        swapped, ref2 = _one_morph(ctx, "3d_cheetah_14_full", 5)
    finally:
        tg.q1, tg.q2 = tg.q2, tg.q1
    assert tg.q1 is tg.critic.q1
    _same(ctx.torch, chain, ref, "cheetah x 5, (q1, q2)")
    _same(ctx.torch, swapped, chain, "cheetah x 5, (q2, q1) against (q1, q2)")
    assert ctx.torch.equal(ref2, ref)


# ---- 7, 8: modules of their own (the weights are changed in place) ------------------------------------------------------------
@pytest.fixture(scope="module")
def live():
    from sgrl_amd.set_hip import HipSetTargets
    import set_targets_restate as S
    pol, crit = _pair(S.SEED + 1)
    return pol, crit, HipSetTargets(pol, crit)


def _scale(t, mods, f):
    with t.no_grad():
        for m in mods:
            for p in m.parameters():
                p.mul_(f)


def test_live_weights_and_a_storage_move(ctx, live):
    t, S = ctx.torch, ctx.S
    pol, crit, tg = live
    name, B = "3d_walker_7_full", 5
    obs, noise, reward, done, _ = ctx.batch([name], [B], seed=4)
    g = ctx.graph(name)
    run = lambda: tg.target_q(obs, noise, reward, done, g, S.NOISE_CLIP, S.DISCOUNT).clone()
    ref = lambda: composed(tg, [g], [B], obs, noise, reward, done, S.NOISE_CLIP, S.DISCOUNT)
    before = run()
    _same(t, before, ref(), "live: start")
    bound = tg.q1._bound
    _scale(t, (pol, crit), 1.03)
    after = run()
    assert tg.q1._bound == bound                                    # no rebinding: the values are read where they live
    _same(t, after, ref(), "live: after mul_ in place")
    assert not t.equal(after, before)
    crit.to("cpu")
    crit.to(DEV)
    moved = run()                                                   # sync_weights compares the addresses and binds again where they moved
    _same(t, moved, ref(), "live: after a .to() round trip")
    assert t.equal(moved, after)


def test_capture_replays_the_chain_on_refilled_inputs_and_scaled_weights(ctx, live):
    from sgrl_amd.td3 import _no_finalizers_during_capture
    t, S = ctx.torch, ctx.S
    pol, crit, tg = live
    name, B = "3d_walker_7_full", 5
    g = ctx.graph(name)
    obs, noise, reward, done, _ = ctx.batch([name], [B], seed=5)
    out = t.zeros((B, 7), device=DEV)
    run = lambda: tg.target_q(obs, noise, reward, done, g, S.NOISE_CLIP, S.DISCOUNT, out=out)
    s = t.cuda.Stream()
    s.wait_stream(t.cuda.current_stream())
    with t.cuda.stream(s):
        run()                                                       # the chain's first calls on these handles: outside any capture
    t.cuda.current_stream().wait_stream(s)
    t.cuda.synchronize()
    gens = [h.generation() for h in (tg.actor, tg.q1, tg.q2)]
    graph = t.cuda.CUDAGraph()
    with _no_finalizers_during_capture(), t.cuda.graph(graph):
        run()
    assert [h.generation() for h in (tg.actor, tg.q1, tg.q2)] == gens
    obs2, noise2, reward2, done2, _ = ctx.batch([name], [B], seed=6)
    for dst, src in ((obs, obs2), (noise, noise2), (reward, reward2), (done, done2)):
        dst.copy_(src)
    _scale(t, (pol, crit), 0.98)
    out.zero_()
    graph.replay()
    t.cuda.synchronize()
    got = out.clone()
    _same(t, got, composed(tg, [g], [B], obs, noise, reward, done, S.NOISE_CLIP, S.DISCOUNT), "replay against the eager composed path")
    assert [h.generation() for h in (tg.actor, tg.q1, tg.q2)] == gens


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(ctx):
    t, tg = ctx.torch, ctx.targets
    g7, g14 = ctx.graph("3d_walker_7_full"), ctx.graph("3d_cheetah_14_full")
    tg.configure([g7], [3])
    for h in (tg.actor, tg.q1, tg.q2):
        h.sync_weights()
    L = tg.L
    z = lambda *sh: t.zeros(sh, device=DEV)
    obs, nz, rw, dn = z(3, 41 * 7), z(3, 21), z(3), z(3)
    q = t.full((3, 7), 7.25, device=DEV)
    vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    st = ctypes.c_void_p(t.cuda.current_stream().cuda_stream)
    err = lambda: L.sgrl_set_last_error()

    def td(a=tg.actor.h, c1=tg.q1.h, c2=tg.q2.h, o=obs, old=41 * 7, n=nz, nld=21, r=rw, d=dn, ma=1.0, clip=0.5, out=q, qld=7):
        return L.sgrl_set_td_target(a, c1, c2, vp(o), old, vp(n), nld, vp(r), vp(d), ma, clip, 0.99, vp(out), qld, st)

    for kw in (dict(a=None), dict(c1=None), dict(c2=None), dict(o=None), dict(n=None), dict(r=None), dict(d=None), dict(out=None)):
        assert td(**kw) == -1 and b"null" in err(), kw
    assert td(c1=tg.actor.h) == -1 and td(c2=tg.q1.h) == -1
    for kw in (dict(old=41 * 7 - 1), dict(nld=20), dict(qld=6)):
        assert td(**kw) == -1 and b"Lmax" in err(), kw
    assert td(clip=-0.1) == -1 and b"noise_clip" in err()
    assert td(ma=0.0) == -1 and td(ma=-1.0) == -1
    tg.q2.configure([g14], [3])                                      # Lmax and node count differ
    assert td() == -1 and b"different batch structures" in err()
    tg.q2.configure([g7], [2])                                       # n_env differs
    assert td() == -1 and b"different batch structures" in err()
    tg.q2.configure([g7], [3])
    t.cuda.synchronize()
    assert bool((q == 7.25).all())                                   # nothing was launched
    assert td() == 0
    t.cuda.synchronize()
    assert bool(t.isfinite(q).all()) and not bool((q == 7.25).any())


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def test_chain_against_the_float64_restatement(ctx):
    """The composed path's deviation is measured first; the chain is held to R.TOL_Q x max |target_ref| where the composed path sits
    below half of it (it does: module docstring), else to twice the composed path's deviation."""
    t, R, S = ctx.torch, ctx.R, ctx.S
    pol64, crit64 = ctx.f64()
    bad = []

    def check(what, chain, ref_composed, ref64):
        tol = R.TOL_Q * np.abs(ref64).max()
        dev_c = float(np.abs(ref_composed.double().cpu().numpy() - ref64).max())
        dev = float(np.abs(chain.double().cpu().numpy() - ref64).max())
        bar = tol if dev_c < 0.5 * tol else 2.0 * dev_c
        print("SETTARGETS float64 %s | composed %.3e | chain %.3e | TOL_Q bound %.3e | bar %.3e" % (what, dev_c, dev, tol, bar))
        if not dev < bar:
            bad.append((what, dev, bar))

    chain, ref = _one_morph(ctx, "3d_walker_7_full", 5)
    (_, _, _, _, d), = S.restate_case(pol64, crit64, *S.WALKER)
    check("walker x 5", chain, ref, d["target"])
    chain, parts = _mixed(ctx)
    for (n, r, c, L, ref), (_, _, _, _, d) in zip(parts, S.restate_case(pol64, crit64, *S.MIXED)):
        check("mixed " + n, chain[r:r + c, :L], ref, d["target"])
    assert not bad, bad


# ---- 11 -----------------------------------------------------------------------------------------------------------------------
def _agents(seed, B):
    import copy
    import torch
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(seed)
    on = Agent(default_train_args(batch_size=B), device=DEV, set_hip_targets=True)
    off = Agent(default_train_args(batch_size=B), device=DEV, set_hip_targets=False)
    off.load_state_dict(copy.deepcopy(on.state_dict()))
    assert on.use_set_hip and not off.use_set_hip
    return on, off


def _update_batch(L, B, seed):
    import torch
    from oracle.formula import scripted_batch
    return {k: torch.from_numpy(v).to(DEV) for k, v in scripted_batch(L, B, seed).items()}


def _same_params(t, a, b, what):
    worst = 0.0
    for nm in ("actor", "critic", "actor_target", "critic_target"):
        for (k, p), q in zip(getattr(a, nm).named_parameters(), getattr(b, nm).parameters()):
            worst = max(worst, float((p.detach() - q.detach()).abs().max()))
    print("SETTARGETS %s | max parameter difference %.3e" % (what, worst))
    for nm in ("actor", "critic", "actor_target", "critic_target"):
        for (k, p), q in zip(getattr(a, nm).named_parameters(), getattr(b, nm).parameters()):
            assert t.equal(p, q), (what, nm, k)


@pytest.fixture(params=["two_forwards", "module_default"])
def target_route(request, monkeypatch):
    """How the switch-off agent's `critic_target(...)` runs under no_grad: as two HIP forwards through SECritic.forward
    (set_policy.TWIN_TARGETS = False -- the composed path this file's yardstick is), or as the module does by default."""
    from sgrl_amd import set_policy
    if request.param == "two_forwards":
        monkeypatch.setattr(set_policy, "TWIN_TARGETS", False)
    return request.param


def test_agent_updates_are_those_of_the_switch_off_agent(ctx, target_route):
    """Three eager updates from the same weights and noise: all four networks bit-identical, on either route of the switch-off
    agent's target critics (module docstring)."""
    from sgrl_amd.set_hip import HipSetTargets
    t, B, L = ctx.torch, 8, 7
    on, off = _agents(70, B)
    g = ctx.graph("3d_walker_7_full")
    for a in (on, off):
        a.change_morphology(g)
        a.models2train()
    for it in range(3):
        batch = _update_batch(L, B, 300 + it)
        noise = t.from_numpy(np.random.RandomState(310 + it).normal(0, 0.2, size=(B, 3 * L)).astype(np.float32)).to(DEV)
        r_on, tq_on = on.update_targets(batch, noise)
        r_off, tq_off = off.update_targets(batch, noise)
        print("SETTARGETS agent %s it %d | max |target on - off| %.3e" % (target_route, it, float((tq_on - tq_off).abs().max())))
        on.update(batch, it, noise=noise)
        off.update(batch, it, noise=noise)
    assert off._targets is None
    if target_route == "two_forwards":
        assert isinstance(on._targets, HipSetTargets)               # the chain ran
    else:
        assert on._targets is None                                   # the chain yielded to the twin pass
    _same_params(t, on, off, "eager agents, " + target_route)


def test_graphed_updates_with_the_switch_are_those_without_it(ctx, target_route):
    """GraphedUpdates with the switch against GraphedUpdates without it, 2 warm + 3 replayed updates: all four networks
    bit-identical, on either route (module docstring)."""
    from sgrl_amd.td3 import GraphedUpdates
    t, B, L = ctx.torch, 8, 7
    on, off = _agents(71, B)
    g = ctx.graph("3d_walker_7_full")
    gus = [GraphedUpdates(a, B) for a in (on, off)]
    for a in (on, off):
        a.models2train()
    for it in range(5):                                              # 2 warm + 3 replayed
        batch = _update_batch(L, B, 400 + it)
        for gu in gus:
            t.manual_seed(500 + it)                                  # the slot's noise draw: the same on both sides
            if it < 2:
                gu.warm(0, g, L, batch, iters=1, first_it=it)
            else:
                gu.update(0, g, L, batch, it)
    t.cuda.synchronize()
    assert gus[0].captures == gus[1].captures == {(0, 0): 1, (0, 1): 1}          # it = 2, 4 replay graph 0; it = 3 graph 1
    assert gus[0].slots[0]["targets"] is on._targets and gus[1].slots[0]["targets"] is None
    assert (on._targets is not None) == (target_route == "two_forwards")
    _same_params(t, on, off, "graphed agents, " + target_route)


def test_a_replaced_target_module_makes_the_next_capture_raise(ctx, monkeypatch):
    import copy
    from sgrl_amd import set_policy
    from sgrl_amd.td3 import GraphedUpdates
    monkeypatch.setattr(set_policy, "TWIN_TARGETS", False)           # the route on which the chain runs
    t, B, L = ctx.torch, 8, 7
    on, _ = _agents(72, B)
    g = ctx.graph("3d_walker_7_full")
    gu = GraphedUpdates(on, B)
    on.models2train()
    gu.warm(0, g, L, _update_batch(L, B, 600), iters=1)
    warmed = gu.slots[0]["targets"]
    assert warmed is on._targets and warmed is not None
    on.critic_target = copy.deepcopy(on.critic_target)               # a new module: its handles have run nothing yet
    with pytest.raises(RuntimeError, match="not the one morphology"):
        gu.update(0, g, L, _update_batch(L, B, 601), 1)
    gu.warm(0, g, L, _update_batch(L, B, 602), iters=1, first_it=1)
    assert gu.slots[0]["targets"] is not warmed
    out = gu.update(0, g, L, _update_batch(L, B, 603), 2)
    t.cuda.synchronize()
    assert np.isfinite(float(out["loss/critic_loss"]))
