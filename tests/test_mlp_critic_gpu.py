"""HIP MLP twin critic (twin and Q1 only) and the one-launch TD3 target chain (csrc/mlp_actor.hip k_mlp_critic / k_mlp_chain through
sgrl_amd/mlp_hip.py HipMlpCritic / HipMlpTargets and td3.Agent.update_targets) on the MI355X: against the fixtures of the executed
reference, against float64 restatements (tests/mlp_restate.py forward64 on module_linears) with full-rank seeded weights at every
path of the kernels (ragged row tiles, widths that are no multiple of a tile, 1 .. 4 hidden layers, the 1-, 2- and 4-chunk variants,
panel depth 8, an actor and a critic of different depth and chunk count), leading dimensions and sentinels, live and held weights,
one launch under graph capture, inside Agent.update and the device trainer, and the argument errors of the C ABI.

Error bar: 2e-5 * max(1, max|ref|) against float64, the bar tests/test_smp_critic_gpu.py and tests/test_swat_critic_gpu.py give a
HIP critic (the fixtures: the same bar against the stored float32 values of the executed reference).  Every comparison prints its
measured error and the float32 PyTorch module's error against the same float64 before it asserts.

The chain tests pass noise_clip = 1.5 with noise ~ N(0, 1): with max_action = 1 both the noise clip and the action clamp then bind on
some entries and not on others whatever the actor's output scale (asserted from the float64 values).

Measured on the MI355X (all 44 tests): |HIP - float64| at most 4.6e-7 on actions, Q values and targets of magnitude <= 1.5 (cheetah_14,
hidden [1, 7]; bar 2e-5 and up), the float32 PyTorch modules at most 6.2e-7 against the same float64; the reference's two recorded updates replayed: critic loss to 1.9e-7 and
1.1e-7 relative."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from mlp_restate import apply_seeded_, forward64, module_linears

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
MORPHS = {3: "3d_hopper_3_shin", 7: "3d_walker_7_full", 14: "3d_cheetah_14_full"}
BAR = 2e-5
TILE = 32
COUNTS = (1, TILE - 1, TILE + 1, 2 * TILE + 2)
HIDDEN = [(256, 256), (40, 72), (1, 7), (64, 48, 80, 33), (1024, 1000)]
NETS = [(L, h) for L in (3, 7, 14) for h in HIDDEN]
NET_IDS = ["L%d-%s" % (L, "x".join(str(x) for x in h)) for L, h in NETS]
# (limbs, actor hidden, critic hidden): the pairs of NETS, then pairs of different depth and chunk count (1 against 2, 1 against 4)
PAIRS = [(L, h, h) for L, h in NETS] + [(7, (64,), (300, 512)), (3, (64, 48, 80, 33), (600,)), (14, (300, 512), (24,))]
PAIR_IDS = ["L%d-%s-%s" % (L, "x".join(str(x) for x in a), "x".join(str(x) for x in c)) for L, a, c in PAIRS]
CLIP, DISCOUNT = 1.5, 0.99


def _graph(L):
    from sgrl_amd import graph as G, mjcf
    return G.getGraphDict(mjcf.load_asset(MORPHS[L]).parents, TRAV, [], device=torch.device("cuda:0"))


def _args(L, actor_hidden=(256, 256), critic_hidden=(256, 256), **over):
    from sgrl_amd.td3 import default_train_args
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L, **over)
    args.agent.policy_network = {"hidden_dims": list(actor_hidden)}
    args.agent.q_network = {"hidden_dims": list(critic_hidden)}
    return args


def _policy(L, hidden=(256, 256), seed=5):
    from sgrl_amd.mlp_policy import MlpPolicy
    return apply_seeded_(MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, _args(L, actor_hidden=hidden)).eval(), seed).to("cuda:0")


def _critic(L, hidden=(256, 256), seed=5):
    from sgrl_amd.mlp_policy import MlpCritic
    return apply_seeded_(MlpCritic(41, 3, 32, 100, 3, True, False, False, _args(L, critic_hidden=hidden)).eval(), seed).to("cuda:0")


def _randn(n, width, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, width), generator=g, dtype=torch.float32) * scale).cuda()


def _np64(t):
    return t.double().cpu().numpy()


def _q64(crit, obs, act):
    x = np.concatenate([_np64(obs), _np64(act)], axis=1)
    return forward64(module_linears(crit.critic1), x), forward64(module_linears(crit.critic2), x)


def _check_q(what, got, crit, obs, act):
    """|HIP - float64| < BAR * max(1, max|ref|) per head; prints it with the float32 PyTorch module's error first."""
    ref = _q64(crit, obs, act)
    with torch.no_grad():
        f32 = crit(obs, act)
    worst = 0.0
    for k in range(len(got)):
        mx = float(np.abs(ref[k]).max())
        err = float(np.abs(_np64(got[k]) - ref[k]).max())
        e32 = float(np.abs(_np64(f32[k]) - ref[k]).max())
        bar = BAR * max(1.0, mx)
        print("%s q%d: max|q_ref| %.3g  |HIP - float64| %.3g  torch f32 %.3g  bar %.3g" % (what, k + 1, mx, err, e32, bar))
        assert got[k].shape == (obs.shape[0], 1)
        assert err < bar, (what, k, err, bar)
        worst = max(worst, err)
    return ref


def _batch(L, n, seed):
    """next_obs ~ N(0, 1); noise ~ N(0, 1) (clip 1.5, max_action 1: both clamps bind on some entries); reward with both signs; done
    with zeros and ones (n >= 2)."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.rand(s, generator=g)
    b = {"obs": torch.randn((n, 41 * L), generator=g), "next_obs": torch.randn((n, 41 * L), generator=g), "action": r(n, 3 * L) * 2 - 1,
         "reward": r(n, 1) * 2 - 1, "done": (r(n, 1) < 0.3).float()}
    if n >= 2:
        b["done"][0, 0], b["done"][1, 0] = 0.0, 1.0
    noise = torch.randn((n, 3 * L), generator=g)
    return {k: v.cuda() for k, v in b.items()}, noise.cuda()


def _chain64(pol, crit, next_obs, noise, reward, done, clip=CLIP, discount=DISCOUNT, max_action=1.0):
    """float64 restatement of the chain -> (action [n, 3 L], target [n, 1], clip binds [n, 3 L] bool, clamp binds [n, 3 L] bool)."""
    x, nz = _np64(next_obs), _np64(noise)
    pre = forward64(module_linears(pol.actor), x, max_action=max_action) + np.clip(nz, -clip, clip)
    act = np.clip(pre, -max_action, max_action)
    xa = np.concatenate([x, act], axis=1)
    q = np.minimum(forward64(module_linears(crit.critic1), xa), forward64(module_linears(crit.critic2), xa))
    return act, _np64(reward).reshape(-1, 1) + (1.0 - _np64(done).reshape(-1, 1)) * discount * q, np.abs(nz) > clip, np.abs(pre) > max_action


def _chain32(pol, crit, next_obs, noise, reward, done, clip=CLIP, discount=DISCOUNT, max_action=1.0):
    """The float32 PyTorch chain of td3.Agent.update_targets on the same modules."""
    with torch.no_grad():
        a = (pol(next_obs) + noise.clamp(-clip, clip)).clamp(-max_action, max_action)
        q1, q2 = crit(next_obs, a)
        return a, reward.reshape(-1, 1) + (1.0 - done.reshape(-1, 1)) * discount * torch.min(q1, q2)


def _check_chain(what, act, tq, pol, crit, b, noise):
    ref_a, ref_t = _chain64(pol, crit, b["next_obs"], noise, b["reward"], b["done"])[:2]
    a32, t32 = _chain32(pol, crit, b["next_obs"], noise, b["reward"], b["done"])
    ea, ea32 = float(np.abs(_np64(act) - ref_a).max()), float(np.abs(_np64(a32) - ref_a).max())
    print("%s action: |HIP - float64| %.3g  torch f32 %.3g  bar %.3g" % (what, ea, ea32, BAR))
    assert ea < BAR, (what, "action", ea)                  # |a| <= max_action = 1
    mx = float(np.abs(ref_t).max())
    bar = BAR * max(1.0, mx)
    et, et32 = float(np.abs(_np64(tq) - ref_t).max()), float(np.abs(_np64(t32) - ref_t).max())
    print("%s target: max|target| %.3g  |HIP - float64| %.3g  torch f32 %.3g  bar %.3g" % (what, mx, et, et32, bar))
    assert tq.shape == (b["next_obs"].shape[0], 1)
    assert et < bar, (what, "target", et, bar)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 7])
def test_critic_matches_the_reference_fixture(golden_dir, L):
    from sgrl_amd.mlp_hip import HipMlpCritic
    z = np.load(os.path.join(golden_dir, "mlp_forward.npz"))
    name = MORPHS[L]
    obs, act = torch.from_numpy(z[name + "/obs"]).cuda(), torch.from_numpy(z[name + "/act_in"]).cuda()
    crit = _critic(L, seed=int(z["seed"]))
    hip = HipMlpCritic(crit)
    hip.configure([_graph(L)], [obs.shape[0]])
    q1, q2 = (q.clone() for q in hip.forward_q(obs, act))
    only = hip.forward_q(obs, act, twin=False)
    with torch.no_grad():
        f32 = crit(obs, act)
    for h, (key, got) in enumerate((("q1", q1), ("q2", q2))):
        want = z[name + "/" + key]
        bar = BAR * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got.cpu().numpy() - want).max())
        e32 = float(np.abs(f32[h].cpu().numpy() - want).max())
        print("fixture %s %s: max|q| %.3g  |HIP - stored| %.3g  torch f32 %.3g  bar %.3g" % (name, key, float(np.abs(want).max()), err, e32, bar))
        assert got.shape == want.shape == (obs.shape[0], 1) and err < bar, (name, key, err, bar)
    assert torch.equal(only, q1) and not torch.equal(q1, q2)
    assert hip.forward_single(obs, act, _graph(L), twin=False).shape == (obs.shape[0], 1)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hidden", NETS, ids=NET_IDS)
def test_critic_against_float64(L, hidden):
    from sgrl_amd.mlp_hip import HipMlpCritic
    g = _graph(L)
    crit = _critic(L, hidden)
    hip = HipMlpCritic(crit)
    assert hip.dims == [44 * L] + list(hidden) + [1] and hip.launches() == 1
    biggest = 0.0
    for n in COUNTS:
        obs, act = _randn(n, 41 * L, seed=n), _randn(n, 3 * L, seed=100 + n).clamp(-1, 1)
        hip.configure([g], [n])
        q1, q2 = (q.clone() for q in hip.forward_q(obs, act))
        ref = _check_q("L %d hidden %s rows %d" % (L, list(hidden), n), (q1, q2), crit, obs, act)
        assert torch.equal(hip.forward_q(obs, act, twin=False), q1)
        biggest = max(biggest, float(np.abs(ref[0]).max()), float(np.abs(ref[1]).max()))
    assert biggest > 1e-3                                   # non-trivial outputs
    p = hip.plan()
    assert p["tiles"] == 3 and p["lds_bytes"] <= 160 * 1024


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,ah,ch", PAIRS, ids=PAIR_IDS)
def test_chain_against_float64_stage_by_stage(L, ah, ch):
    from sgrl_amd.mlp_hip import HipMlpTargets, chain_plan
    g = _graph(L)
    pol, crit = _policy(L, ah, seed=7), _critic(L, ch, seed=8)
    hip = HipMlpTargets(pol, crit)
    assert hip.plan() == chain_plan([41 * L] + list(ah) + [3 * L], [44 * L] + list(ch) + [1])
    clip_binds = clamp_binds = total = 0
    for n in COUNTS:
        b, noise = _batch(L, n, seed=n)
        act = torch.full((n, 3 * L), 9.0, device="cuda:0")
        tq = hip.target_q(b["next_obs"], noise, b["reward"], b["done"], g, CLIP, DISCOUNT, action_out=act).clone()
        _check_chain("L %d actor %s critic %s rows %d" % (L, list(ah), list(ch), n), act, tq, pol, crit, b, noise)
        again = hip.target_q(b["next_obs"], noise, b["reward"], b["done"], g, CLIP, DISCOUNT)      # action_out=None: the workspace
        assert torch.equal(again, tq)
        cb, mb = _chain64(pol, crit, b["next_obs"], noise, b["reward"], b["done"])[2:]
        clip_binds, clamp_binds, total = clip_binds + int(cb.sum()), clamp_binds + int(mb.sum()), total + cb.size
        ended = b["done"].reshape(-1) == 1
        assert torch.equal(tq[ended], b["reward"][ended])                 # (1 - done) = 0: the reward alone, exactly
        if n >= 2:
            assert 0 < int(ended.sum()) < n and float(b["reward"].min()) < 0 < float(b["reward"].max())
            assert float((tq[~ended] - b["reward"][~ended]).abs().max()) > 1e-4    # the critics contribute elsewhere
    assert 0 < clip_binds < total and 0 < clamp_binds < total, (clip_binds, clamp_binds, total)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_leading_dimensions_padding_and_sentinels():
    from sgrl_amd.mlp_hip import HipMlpTargets
    L, n, guard, sentinel = 7, 37, 64, 12345.0
    g = _graph(L)
    pol, crit = _policy(L, seed=7), _critic(L, seed=8)
    hip = HipMlpTargets(pol, crit)
    b, noise = _batch(L, n, seed=4)
    obs_wide = torch.full((n, 287 + 13), float("nan"), device="cuda:0")          # beyond 41 L: never read
    obs_wide[:, :287] = b["next_obs"]
    noise_wide = torch.full((n, 21 + 5), float("nan"), device="cuda:0")          # beyond 3 L: never read
    noise_wide[:, :21] = noise
    act_ld = 21 + 70                                                              # more padding than a wave's 64 lanes cover in one pass
    aflat = torch.full((guard + n * act_ld + guard,), sentinel, device="cuda:0")
    act = aflat[guard:guard + n * act_ld].view(n, act_ld)
    qflat = torch.full((guard + n + guard,), sentinel, device="cuda:0")
    tq = qflat[guard:guard + n].view(n, 1)
    hip.target_q(obs_wide[:, :287], noise_wide[:, :21], b["reward"], b["done"], g, CLIP, DISCOUNT, out=tq, action_out=act)
    _check_chain("wide rows", act[:, :21], tq, pol, crit, b, noise)
    assert torch.equal(act[:, 21:], torch.zeros_like(act[:, 21:]))
    for flat, m in ((aflat, n * act_ld), (qflat, n)):
        assert bool((flat[:guard] == sentinel).all()) and bool((flat[guard + m:] == sentinel).all())
    narrow = hip.target_q(b["next_obs"], noise, b["reward"], b["done"], g, CLIP, DISCOUNT)
    assert torch.equal(narrow, tq)                          # the leading dimensions change nothing
    # the critic alone: NaN beyond 41 L / 3 L of its rows, sentinels around q1 and q2
    a_wide = torch.full((n, 21 + 5), float("nan"), device="cuda:0")
    a_wide[:, :21] = act[:, :21]
    c = hip.critic
    q1, q2 = (q.clone() for q in c.forward_q(obs_wide[:, :287], a_wide[:, :21]))
    _check_q("wide rows", (q1, q2), crit, b["next_obs"], act[:, :21].contiguous())
    want = b["reward"] + (1.0 - b["done"]) * DISCOUNT * torch.min(q1, q2)
    assert float((want - tq).abs().max()) < BAR * max(1.0, float(tq.abs().max()))      # chain and critic agree on the same actions
    qq = torch.full((2, guard + n + guard), sentinel, device="cuda:0")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert c.L.sgrl_mlp_critic_forward(c.h, vp(obs_wide), 300, vp(a_wide), 26, vp(qq[0, guard:]), vp(qq[1, guard:]), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(qq[0, guard:guard + n], q1.reshape(-1)) and torch.equal(qq[1, guard:guard + n], q2.reshape(-1))
    assert bool((qq[:, :guard] == sentinel).all()) and bool((qq[:, guard + n:] == sentinel).all())


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def _step(mod, k=0):
    """An in-place optimizer-style update of every parameter."""
    with torch.no_grad():
        for i, p in enumerate(mod.parameters()):
            p.add_(0.05 * torch.sin(torch.arange(p.numel(), device=p.device, dtype=torch.float32) + i + k).view_as(p))


def test_live_target_weights_show_in_the_next_chain():
    from sgrl_amd.mlp_hip import HipMlpTargets
    L, n = 3, 40
    g = _graph(L)
    pol, crit = _policy(L, seed=7), _critic(L, seed=8)
    hip = HipMlpTargets(pol, crit)
    b, noise = _batch(L, n, seed=2)

    def run(what):
        act = torch.empty((n, 3 * L), device="cuda:0")
        tq = hip.target_q(b["next_obs"], noise, b["reward"], b["done"], g, CLIP, DISCOUNT, action_out=act).clone()
        _check_chain("live weights, " + what, act, tq, pol, crit, b, noise)
        return act, tq

    a0, t0 = run("initial")
    _step(crit)                                            # the critic alone: the action stays, the target moves
    a1, t1 = run("critic stepped")
    assert torch.equal(a1, a0) and float((t1 - t0).abs().max()) > 1e-3
    _step(pol)                                             # the actor: both move
    a2, t2 = run("actor stepped")
    assert float((a2 - a1).abs().max()) > 1e-3 and float((t2 - t1).abs().max()) > 1e-4
    src = _critic(L, seed=13)                              # an in-place soft update (reference common/functional.py:7-10)
    with torch.no_grad():
        for p, q in zip(crit.parameters(), src.parameters()):
            p.data.copy_(0.5 * p.data + 0.5 * q.data)
    _, t3 = run("soft update")
    assert float((t3 - t2).abs().max()) > 1e-4
    crit.load_state_dict(_critic(L, seed=14).state_dict())
    _, t4 = run("load_state_dict")
    assert float((t4 - t3).abs().max()) > 1e-4
    assert hip.critic._bound == tuple(p.data_ptr() for p in hip.critic._params())


def test_critic_hold_weights_and_weights_changed():
    from sgrl_amd.mlp_hip import HipMlpCritic
    L, n = 3, 40
    g = _graph(L)
    crit = _critic(L)
    hip = HipMlpCritic(crit)
    hip.configure([g], [n])
    obs, act = _randn(n, 123, seed=1), _randn(n, 9, seed=2).clamp(-1, 1)
    fwd = lambda: torch.stack([q.clone() for q in hip.forward_q(obs, act)])
    q0 = fwd()
    _check_q("hold: initial", q0, crit, obs, act)
    hip.hold_weights(True)
    assert torch.equal(fwd(), q0)                           # the first forward of a hold packs
    _step(crit)
    assert torch.equal(fwd(), q0)                           # holding, nobody said the weights changed: the packed copy
    hip.weights_changed()
    q1 = fwd()
    _check_q("hold: weights_changed", q1, crit, obs, act)
    assert float((q1 - q0).abs().max()) > 1e-3
    hip.hold_weights(False)
    _step(crit, 3)
    q2 = fwd()
    _check_q("hold: released", q2, crit, obs, act)
    assert float((q2 - q1).abs().max()) > 1e-3


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_one_launch_and_graph_capture():
    from sgrl_amd.mlp_hip import HipMlpTargets
    L, n = 7, 70
    g = _graph(L)
    pol, crit = _policy(L, seed=7), _critic(L, seed=8)
    hip = HipMlpTargets(pol, crit)
    assert hip.launches() == 1 and int(hip.L.sgrl_mlp_td_target_launches()) == 1 and int(hip.L.sgrl_mlp_critic_forward_launches()) == 1
    assert hip.critic.launches() == 1 and hip.critic.pack_launches() == 1
    b, noise = _batch(L, n, seed=1)
    static = {k: b[k].clone() for k in ("next_obs", "reward", "done")}
    snoise = noise.clone()
    out = torch.zeros((n, 1), device="cuda:0")

    def run(o=None):
        return hip.target_q(static["next_obs"], snoise, static["reward"], static["done"], g, CLIP, DISCOUNT, out=o)

    eager = run().clone()                                   # eager first: it sizes the critic handle's action workspace
    torch.cuda.synchronize()
    gen = (hip.actor.generation(), hip.critic.generation())
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):             # single stream, no parallel branches
            run(out)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    for seed in (2, 3):                                     # new inputs, copied into the static tensors
        b2, noise2 = _batch(L, n, seed=seed)
        for k in static:
            static[k].copy_(b2[k])
        snoise.copy_(noise2)
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        fresh = run()
        assert torch.equal(replayed, fresh) and not torch.equal(replayed, eager)
    assert (hip.actor.generation(), hip.critic.generation()) == gen      # nothing the graph points into was freed


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def _agent(use_hip=True, seed=0, device="cuda:0", **over):
    from sgrl_amd.td3 import Agent
    torch.manual_seed(seed)
    return Agent(_args(7, **over), device=torch.device(device), use_hip=use_hip)


def _perturb_targets(agent, seed):
    """Targets that differ from the online networks, as in the middle of a run."""
    with torch.no_grad():
        for k, mod in enumerate((agent.actor_target, agent.critic_target)):
            gen = torch.Generator(device="cuda:0").manual_seed(seed + k)
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.02)


def _double(batch):
    return {k: v.double() for k, v in batch.items()}


def _copy_agent(agent, dtype):
    """A PyTorch-only deep copy of the agent in `dtype` (never builds a handle)."""
    a = copy.deepcopy(agent).to(dtype)
    a.use_mlp_hip = False
    return a


@pytest.mark.parametrize("B", [256, 33])
def test_agent_update_targets_through_the_chain_and_on_float64(B):
    """Three updates (the first and third with the delayed actor step) of an mlp + mlp agent whose target chain runs on HIP, of the
    same agent with use_hip=False and of a float64 copy, from the same weights, batches and target noise: every update's target
    values, computed from each agent's OWN (updated) target networks, within the bar; finite losses."""
    from sgrl_amd.mlp_hip import HipMlpTargets
    g = _graph(7)
    hip_agent = _agent(seed=30, noise_clip=CLIP)
    for mod, seed in ((hip_agent.actor, 3), (hip_agent.critic, 4), (hip_agent.actor_target, 3), (hip_agent.critic_target, 4)):
        apply_seeded_(mod, seed)
    _perturb_targets(hip_agent, 33)
    f64_agent = _copy_agent(hip_agent, torch.float64)
    pt_agent = _agent(use_hip=False, seed=30, noise_clip=CLIP)
    pt_agent.load_state_dict(hip_agent.state_dict())
    assert hip_agent.use_mlp_hip and not pt_agent.use_mlp_hip and not f64_agent.use_mlp_hip
    for agent in (hip_agent, pt_agent, f64_agent):
        agent.change_morphology(g)
        agent.models2train()
    for it in range(3):
        batch, noise = _batch(7, B, seed=60 + it)
        _, tq = hip_agent.update_targets(batch, noise)
        _, tq32 = pt_agent.update_targets(batch, noise)
        _, ref = f64_agent.update_targets(_double(batch), noise.double())
        bar = BAR * max(1.0, float(ref.abs().max()))
        err, e32 = float((tq.double() - ref).abs().max()), float((tq32.double() - ref).abs().max())
        print("B %d update %d: max|target| %.3g  |HIP agent - float64 agent| %.3g  torch f32 agent %.3g  bar %.3g"
              % (B, it, float(ref.abs().max()), err, e32, bar))
        assert tq.shape == ref.shape == (B, 1)
        assert err < bar, (it, err, bar)
        if it == 0:                                         # the same weights still: both clamps bind on some entries, not on others
            cb, mb = _chain64(hip_agent.actor_target, hip_agent.critic_target, batch["next_obs"], noise, batch["reward"], batch["done"])[2:]
            assert 0 < int(cb.sum()) < cb.size and 0 < int(mb.sum()) < mb.size
        losses = {}
        for tag, agent in (("hip", hip_agent), ("pytorch", pt_agent), ("float64", f64_agent)):
            b, n = (_double(batch), noise.double()) if tag == "float64" else (batch, noise)
            out = agent.update(b, it, noise=n)
            assert all(np.isfinite(float(v)) for v in out.values()), (tag, out)
            losses[tag] = float(out["loss/critic_loss"])
        print("B %d update %d critic loss: float64 %.9g  pytorch f32 %.9g  hip targets %.9g" % (B, it, losses["float64"], losses["pytorch"], losses["hip"]))
    assert isinstance(hip_agent._targets, HipMlpTargets) and hip_agent.actor_target._mlp_hip is not None
    assert hip_agent.critic_target._mlp_hip is not None and hip_agent.critic._mlp_hip is None
    assert pt_agent._targets is None and pt_agent.actor_target._mlp_hip is None and pt_agent.critic_target._mlp_hip is None
    assert f64_agent._targets is None and f64_agent.critic_target._mlp_hip is None
    # replaced target modules: the agent builds new handles
    old = hip_agent._targets
    hip_agent.critic_target = copy.deepcopy(hip_agent.critic_target)
    batch, noise = _batch(7, B, seed=70)
    _, tq = hip_agent.update_targets(batch, noise)
    ref = _chain64(hip_agent.actor_target, hip_agent.critic_target, batch["next_obs"], noise, batch["reward"], batch["done"],
                   discount=hip_agent.args.discount)[1]
    assert hip_agent._targets is not old and hip_agent._targets.critic.module is hip_agent.critic_target
    assert float(np.abs(_np64(tq) - ref).max()) < BAR * max(1.0, float(np.abs(ref).max()))


def test_hip_agent_replays_the_reference_update(golden_dir):
    """tests/golden/td3_update_mlp.npz (the executed reference's Agent.update) through an agent whose target chain runs on HIP:
    critic_loss within 1e-4 relative for both iterations, the tolerance of test_mlp_policy.test_update_matches_the_reference_on_cpu."""
    from sgrl_amd.td3 import Agent, default_train_args
    z = np.load(os.path.join(golden_dir, "td3_update_mlp.npz"))
    hyper = dict(zip([str(k) for k in z["hyper_keys"]], z["hyper_vals"]))
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=7, lr=hyper["lr"], policy_noise=hyper["policy_noise"],
                              noise_clip=hyper["noise_clip"], discount=hyper["discount"], policy_freq=int(hyper["policy_freq"]),
                              grad_clipping_value=hyper["grad_clipping_value"], max_action=hyper["max_action"])
    args.agent.target_smoothing_tau, args.agent.reward_scale = hyper["target_smoothing_tau"], hyper["reward_scale"]
    agent = Agent(args, device=torch.device("cuda:0"))
    apply_seeded_(agent.actor, int(z["seed"]))
    apply_seeded_(agent.critic, int(z["seed"]))
    with torch.no_grad():
        for tgt, src in ((agent.actor_target, agent.actor), (agent.critic_target, agent.critic)):
            for tp, sp in zip(tgt.parameters(), src.parameters()):
                tp.copy_(0.97 * sp)
    agent.change_morphology(_graph(7))
    agent.models2train()
    for it in range(2):
        tag = "it%d/" % it
        batch = {k: torch.from_numpy(z[tag + k]).cuda() for k in ("obs", "action", "next_obs", "reward", "done")}
        loss = agent.update(batch, it, noise=torch.from_numpy(z[tag + "noise"]).cuda())
        ref_cl, got = float(z[tag + "critic_loss"]), float(loss["loss/critic_loss"])
        print("reference update %d: critic_loss %.9g  reference %.9g  relative difference %.3g" % (it, got, ref_cl, abs(got - ref_cl) / abs(ref_cl)))
        assert abs(got - ref_cl) < 1e-4 * abs(ref_cl), it
        assert agent._targets is not None


def test_device_trainer_trains_through_the_chain():
    from sgrl_amd.mlp_hip import HipMlpTargets
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    args = default_train_args(actor_type="mlp", critic_type="mlp")
    tr = DeviceTrainer(["3d_hopper_3_shin"], 4, args=args, seed=2, device="cuda:0", max_buffer_size=4096, batch_size=64)
    assert tr.agent.use_mlp_hip and tr.agent._targets is None
    tr.warmup(8)
    s = tr.train_round(max_steps=40, max_iters=2)
    assert s["per_morph_iter"] == 2
    assert isinstance(tr.agent._targets, HipMlpTargets) and tr.agent._targets.actor.n_env > 0
    assert tr.agent._targets.critic.module is tr.agent.critic_target
    losses = tr.last_losses["3d_hopper_3_shin"]
    assert all(np.isfinite(float(v)) for v in losses.values())


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_returned_before_any_launch():
    from sgrl_amd import _lib
    from sgrl_amd.mlp_hip import HipMlpActor, HipMlpCritic, HipMlpTargets
    L7, n = 7, 5
    g7, g3 = _graph(7), _graph(3)
    pol, crit = _policy(L7, seed=7), _critic(L7, seed=8)
    tg = HipMlpTargets(pol, crit)
    actor, c = tg.actor, tg.critic
    tg.configure([g7], [n])
    L = c.L
    z = lambda w: torch.zeros((n, w), device="cuda:0")
    obs, act = z(287), z(21)
    rw = torch.zeros(n, device="cuda:0")
    q1, q2, aout = torch.full((n,), 7.0, device="cuda:0"), torch.full((n,), 7.0, device="cuda:0"), torch.full((n, 21), 7.0, device="cuda:0")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(None)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = lambda: L.sgrl_mlp_last_error()
    fq = lambda h, o=vp(obs), old=287, a=vp(act), ald=21, o1=vp(q1), o2=vp(q2): L.sgrl_mlp_critic_forward(h, o, old, a, ald, o1, o2, st)
    td = lambda a, cc, o=vp(obs), old=287, nz=vp(act), nld=21, r=vp(rw), d=vp(rw), out=vp(q1), ao=vp(aout), ald=21: \
        L.sgrl_mlp_td_target(a, cc, o, old, nz, nld, r, d, 1.0, 0.5, 0.99, out, ao, ald, st)
    ERR = -1
    # handles of the wrong kind
    assert fq(actor.h) == ERR and b"not bound as a critic" in err()
    assert L.sgrl_mlp_forward(c.h, vp(obs), 287, vp(aout), 21, ctypes.c_float(1.0), st) == ERR and b"not bound as an actor" in err()
    assert td(c.h, c.h) == ERR and b"not bound as an actor" in err()
    assert td(actor.h, actor.h) == ERR and b"not bound as a critic" in err()
    assert not hasattr(c, "forward_batch") and not hasattr(actor, "forward_q")      # siblings: each handle has its own forward only
    # rows too narrow
    assert fq(c.h, old=286) == ERR and b"narrow" in err()
    assert fq(c.h, ald=20) == ERR and b"narrow" in err()
    assert td(actor.h, c.h, old=286) == ERR and b"narrow" in err()
    assert td(actor.h, c.h, nld=20) == ERR and b"narrow" in err()
    assert td(actor.h, c.h, ald=20) == ERR and b"narrow" in err()
    # null pointers (a null action_out is allowed, a null q2 means Q1 only)
    assert fq(null) == ERR and b"null" in err()
    assert fq(c.h, o=null) == ERR and fq(c.h, a=null) == ERR and fq(c.h, o1=null) == ERR and b"null" in err()
    assert td(null, c.h) == ERR and td(actor.h, null) == ERR and b"null" in err()
    for kw in ("o", "nz", "r", "d", "out"):
        assert td(actor.h, c.h, **{kw: null}) == ERR and b"null" in err(), kw
    # binding: count, last width, null
    arr = (ctypes.c_void_p * 12)(*[p.data_ptr() for p in c._params()])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    dims = np.asarray([308, 256, 256, 1], dtype=np.int32)
    bad = np.asarray([308, 256, 256, 2], dtype=np.int32)
    npp = lambda a: ctypes.c_void_p(a.ctypes.data)
    h = ctypes.c_void_p()
    assert L.sgrl_mlp_create(ctypes.byref(h)) == 0
    try:
        assert fq(h) == ERR and b"not bound as a critic" in err()                    # nothing bound yet
        assert L.sgrl_mlp_set_critic_params(h, null, 12, npp(dims), 4) == ERR and b"null" in err()
        assert L.sgrl_mlp_set_critic_params(h, cast(arr), 6, npp(dims), 4) == ERR and b"expected 12" in err()
        assert L.sgrl_mlp_set_critic_params(h, cast(arr), 12, npp(bad), 4) == ERR and b"last width must be 1" in err()
        assert L.sgrl_mlp_set_critic_params(h, cast(arr), 12, npp(dims), 4) == 0
        assert fq(h) == ERR and b"batch structure" in err()                          # bound, not configured
        la, ca = np.asarray([3], dtype=np.int32), np.asarray([n], dtype=np.int32)
        assert L.sgrl_mlp_configure(h, 1, npp(la), npp(ca), 41, 3) == ERR            # 3 limbs on a 7-limb critic
        la = np.asarray([7], dtype=np.int32)
        assert L.sgrl_mlp_configure(h, 1, npp(la), npp(ca), 41, 4) == ERR            # (41 + 4) * 7 is not 308
        assert L.sgrl_mlp_configure(h, 1, npp(la), npp(ca), 41, 3) == 0
        # the last bind decides: the same handle as an actor, then a critic again
        arr6 = (ctypes.c_void_p * 6)(*[p.data_ptr() for p in actor._params()])
        adims = np.asarray([287, 256, 256, 21], dtype=np.int32)
        assert L.sgrl_mlp_set_params(h, cast(arr6), 6, npp(adims), 4) == 0
        assert fq(h) == ERR and b"not bound as a critic" in err()
        assert L.sgrl_mlp_set_critic_params(h, cast(arr), 12, npp(dims), 4) == 0
        assert L.sgrl_mlp_configure(h, 1, npp(la), npp(ca), 41, 3) == 0
        # different n_env
        ca2 = np.asarray([n + 1], dtype=np.int32)
        assert L.sgrl_mlp_configure(h, 1, npp(la), npp(ca2), 41, 3) == 0
        assert td(actor.h, h) == ERR and b"different batch structures" in err()
    finally:
        L.sgrl_mlp_destroy(h)
    # a critic whose input is not the actor's input + output width
    other = HipMlpCritic(_critic(3, seed=9))
    other.configure([g3], [n])
    other.sync_weights()
    assert td(actor.h, other.h) == ERR and b"input + output" in err()
    with pytest.raises(_lib.SgrlError, match="input \\+ output"):
        HipMlpTargets(pol, other.module)
    with pytest.raises(ValueError):
        c.configure([g3], [n])
    torch.cuda.synchronize()
    assert bool((q1 == 7).all()) and bool((q2 == 7).all()) and bool((aout == 7).all())      # none of the refused calls wrote anything
    # and the well-formed calls go through, on the same handles
    assert fq(c.h) == 0 and fq(c.h, o2=null) == 0 and td(actor.h, c.h) == 0 and td(actor.h, c.h, ao=null, ald=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q1).all()) and bool(torch.isfinite(q2).all()) and not bool((q2 == 7).any()) and not bool((aout == 7).any())
    b, noise = _batch(L7, n, seed=5)
    act_out = torch.empty((n, 21), device="cuda:0")
    tq = tg.target_q(b["next_obs"], noise, b["reward"], b["done"], g7, CLIP, DISCOUNT, action_out=act_out)
    _check_chain("after the refusals", act_out, tq, pol, crit, b, noise)
    assert isinstance(actor, HipMlpActor)
