"""HIP SWAT critic forward (single and twin) and the fused TD3 target chain (csrc/swat_actor.hip through sgrl_amd/swat_hip.py
HipSwatCritic / HipSwatTargets and td3.Agent.update_targets) on the MI355X: against the fixtures of the executed reference,
against float64 copies of the PyTorch modules at full size, twin against singles bit for bit, with live weights, under graph
capture, inside Agent.update, and the argument errors of the C ABI.  Reads fixtures and this repository only."""
import copy
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
WALKERS = sorted(["3d_walker_2_right_leg_left_knee", "3d_walker_3_left_leg_right_foot", "3d_walker_3_left_knee_right_knee",
                  "3d_walker_4_right_knee_left_foot", "3d_walker_5_foot", "3d_walker_5_left_knee",
                  "3d_walker_6_right_foot", "3d_walker_7_full"])
HELD = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
        "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}
MIXED = ["3d_hopper_3_shin", "3d_walker_7_full", "3d_humanoid_9_full"]
TARGET_MORPHS = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full", "3d_cheetah_14_full"]     # 2, 7 and 14 limbs


def _critic(cond=0, tnorm=1, seed=0):
    import torch
    from sgrl_amd.set_policy import default_args
    from sgrl_amd.swat_policy import CriticStructurePolicy
    torch.manual_seed(seed)
    return CriticStructurePolicy(41, 3, 32, 1, 3, True, False, False,
                                 default_args(condition_decoder_on_features=cond, transformer_norm=tnorm)).eval()


def _graphs(names):
    import torch
    from sgrl_amd import graph as G, mjcf
    return [G.getGraphDict(mjcf.load_asset(n).parents, TRAV, [], device=torch.device("cuda:0")) for n in names]


def _g64(g):
    g64 = dict(g)
    g64["relation"] = g["relation"].double()
    return g64


def _reference(crit, graphs, counts, obs, act, q_ld):
    """CriticStructurePolicy.forward per morphology on a float64 copy of the module -> (q1, q2), zero padded to q_ld."""
    import torch
    c64 = copy.deepcopy(crit).double()
    out = torch.zeros((2, obs.shape[0], q_ld), dtype=torch.float64, device=obs.device)
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        c64.change_morphology(_g64(g))
        with torch.no_grad():
            q1, q2 = c64(obs[row:row + c, :41 * L].double(), act[row:row + c, :3 * L].double())
        out[0, row:row + c, :L], out[1, row:row + c, :L] = q1, q2
        row += c
    return out[0], out[1]


def _inputs(counts, graphs, seed=1):
    """obs ~ N(0, 1), action ~ U(-1, 1) in the limbs' slots, zeros beyond."""
    import torch
    Lmax = max(len(g["parents"]) for g in graphs)
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    n = int(sum(counts))
    obs = torch.zeros((n, 41 * Lmax), dtype=torch.float32, device="cuda:0")
    act = torch.zeros((n, 3 * Lmax), dtype=torch.float32, device="cuda:0")
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        obs[row:row + c, :41 * L] = torch.randn((c, 41 * L), device="cuda:0", generator=gen)
        act[row:row + c, :3 * L] = torch.rand((c, 3 * L), device="cuda:0", generator=gen) * 2 - 1
        row += c
    return obs, act


def _padding_is_zero(q, graphs, counts):
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        if q.shape[1] > L:
            assert bool((q[row:row + c, L:] == 0).all())
        row += c


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", [0, 1])
def test_fixture_morphologies_alone_and_in_one_batch(cond, golden_dir):
    import torch
    from oracle.formula import apply_formula_
    from sgrl_amd.swat_hip import HipSwatCritic
    z = np.load(os.path.join(golden_dir, "swat_forward.npz"))
    crit = _critic(cond)
    apply_formula_(crit)
    crit.to("cuda:0")
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("cond%d/" % cond)})
    assert len(names) == 5
    graphs = _graphs(names)
    hip = HipSwatCritic(crit)
    for name, g in zip(names, graphs):
        tag = "cond%d/%s/" % (cond, name)
        obs, act = torch.from_numpy(z[tag + "obs"]).cuda(), torch.from_numpy(z[tag + "act_in"]).cuda()
        hip.configure([g], [obs.shape[0]])
        q1, q2 = hip.forward_batch(obs, act)
        for got, key in ((q1, "q1"), (q2, "q2")):
            want = z[tag + key]
            tol = 1e-5 * max(1.0, float(np.abs(want).max()))
            err = float(np.abs(got.cpu().numpy() - want).max())
            print("fixture cond%d %s %s: err %.3g tol %.3g" % (cond, name, key, err, tol))
            assert got.shape == want.shape and err <= tol, (name, key, err, tol)
    Lmax = max(len(g["parents"]) for g in graphs)
    obs = torch.zeros((4 * len(names), 41 * Lmax), dtype=torch.float32)
    act = torch.zeros((4 * len(names), 3 * Lmax), dtype=torch.float32)
    want = np.zeros((2, 4 * len(names), Lmax + 2), dtype=np.float32)
    for k, name in enumerate(names):
        tag = "cond%d/%s/" % (cond, name)
        o, a = z[tag + "obs"], z[tag + "act_in"]
        obs[4 * k:4 * k + 4, :o.shape[1]] = torch.from_numpy(o)
        act[4 * k:4 * k + 4, :a.shape[1]] = torch.from_numpy(a)
        want[0, 4 * k:4 * k + 4, :z[tag + "q1"].shape[1]] = z[tag + "q1"]
        want[1, 4 * k:4 * k + 4, :z[tag + "q2"].shape[1]] = z[tag + "q2"]
    hip.configure(graphs, [4] * len(names))
    got = hip.forward_batch(obs.cuda(), act.cuda(), q_ld=Lmax + 2)
    for k in range(2):
        tol = 1e-5 * max(1.0, float(np.abs(want[k]).max()))
        g = got[k].cpu().numpy()
        err = float(np.abs(g - want[k]).max())
        print("fixture cond%d mixed q%d: err %.3g tol %.3g" % (cond, k + 1, err, tol))
        assert err <= tol, (k, err, tol)
        assert bool((g[want[k] == 0] == 0).all())          # padding columns: exact zeros
        _padding_is_zero(got[k], graphs, [4] * len(names))


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tnorm", [1, 0])
@pytest.mark.parametrize("workload", ["config3", "config5_share"])
def test_full_size_mixed_batches_against_float64(workload, tnorm):
    import torch
    from sgrl_amd import mjcf
    from sgrl_amd.swat_hip import HipSwatCritic
    if workload == "config3":
        names, counts = WALKERS, [1024] * len(WALKERS)
    else:
        names = sorted(n for n in mjcf.list_assets() if n not in HELD)
        assert len(names) == 23
        counts = [8188 // len(names)] * len(names)
    graphs = _graphs(names)
    crit = _critic(tnorm=tnorm, seed=5).to("cuda:0")
    hip = HipSwatCritic(crit)
    hip.configure(graphs, counts)
    obs, act = _inputs(counts, graphs)
    q_ld = hip.max_limbs + 3                     # wider than needed: the extra slots are padding too
    got = hip.forward_batch(obs, act, q_ld=q_ld)
    ref = _reference(crit, graphs, counts, obs, act, q_ld)
    for k in range(2):
        bar = 2e-5 * max(1.0, float(ref[k].abs().max()))
        err = float((got[k].double() - ref[k]).abs().max())
        print("%s tnorm %d q%d: max|q_ref| %.3g err %.3g bar %.3g" % (workload, tnorm, k + 1, float(ref[k].abs().max()), err, bar))
        assert err < bar, (k, err, bar)
        _padding_is_zero(got[k], graphs, counts)
        assert float(got[k].abs().max()) > 1e-3                   # a non-trivial output


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_twin_equals_the_two_single_forwards_bit_for_bit():
    import torch
    from sgrl_amd.swat_hip import HipSwatCritic
    counts = [37, 129, 64]
    graphs = _graphs(MIXED)
    crit = _critic(cond=1, seed=8).to("cuda:0")
    hip = HipSwatCritic(crit)
    hip.configure(graphs, counts)
    assert hip.launches() == 2 * hip.q1.launches() == 44
    obs, act = _inputs(counts, graphs, seed=3)
    t1, t2 = (t.clone() for t in hip.forward_batch(obs, act))
    s1 = hip.q1.forward_q(obs, act).clone()
    s2 = hip.q2.forward_q(obs, act).clone()
    assert torch.equal(t1, s1) and torch.equal(t2, s2)
    assert not torch.equal(t1, t2)
    only1, = hip.forward_batch(obs, act, which=(1,))
    assert torch.equal(only1, t1)
    only2, = hip.forward_batch(obs, act, which=(2,))
    assert torch.equal(only2, t2)
    # forward_single: one morphology, rows exactly L wide
    g = graphs[1]
    a1, a2 = hip.forward_single(obs[37:166, :41 * 7], act[37:166, :3 * 7], g)
    assert a1.shape == (129, 7) and torch.equal(a1, t1[37:166, :7]) and torch.equal(a2, t2[37:166, :7])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def _agent(use_hip=True, seed=0, **over):
    import torch
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(seed)
    return Agent(default_train_args(actor_type="swat", critic_type="swat", **over), device=torch.device("cuda:0"), use_hip=use_hip)


def _batch(L, B, seed):
    import torch
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    r = lambda *s: torch.rand(s, device="cuda:0", generator=gen)
    batch = {"obs": torch.randn((B, 41 * L), device="cuda:0", generator=gen), "next_obs": torch.randn((B, 41 * L), device="cuda:0", generator=gen),
             "action": r(B, 3 * L) * 2 - 1, "reward": r(B, 1) * 2 - 1, "done": (r(B, 1) < 0.3).float()}
    noise = torch.randn((B, 3 * L), device="cuda:0", generator=gen) * 0.4         # noise_clip 0.5: a fifth of the draws are clipped
    return batch, noise


def _double(batch):
    return {k: v.double() for k, v in batch.items()}


def test_target_chain_against_float64_update_targets():
    import torch
    from sgrl_amd.swat_hip import HipSwatTargets
    agent = _agent(seed=4)
    # targets that differ from each other and from the online networks
    with torch.no_grad():
        for k, mod in enumerate((agent.actor_target, agent.critic_target)):
            gen = torch.Generator(device="cuda:0").manual_seed(40 + k)
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.02)
    hip = HipSwatTargets(agent.actor_target, agent.critic_target)
    assert hip.launches() == 66
    a64 = copy.deepcopy(agent).double()
    args = agent.args
    for name, g in zip(TARGET_MORPHS, _graphs(TARGET_MORPHS)):
        L = len(g["parents"])
        batch, noise = _batch(L, 256, seed=L)
        assert float(noise.abs().max()) > args.noise_clip and 0 < float(batch["done"].sum()) < 256
        assert float(batch["reward"].min()) < 0 < float(batch["reward"].max()) and float(batch["reward"].abs().max()) <= 1
        a64.change_morphology(_g64(g))
        _, ref = a64.update_targets(_double(batch), noise.double())
        got = hip.target_q(batch["next_obs"], noise, batch["reward"], batch["done"], g, args.noise_clip, args.discount)
        assert got.shape == ref.shape == (256, L)
        bar = 2e-5 * max(1.0, float(ref.abs().max()))
        err = float((got.double() - ref).abs().max())
        print("target chain %s: max|target| %.3g err %.3g bar %.3g" % (name, float(ref.abs().max()), err, bar))
        assert err < bar, (name, err, bar)
        ended = batch["done"].reshape(-1) == 1
        assert torch.equal(got[ended], batch["reward"].reshape(-1)[ended][:, None].expand(-1, L))
        assert float((got[~ended] - batch["reward"][~ended]).abs().max()) > 1e-4       # the critics do contribute elsewhere
        # the same through the agent (its own handle objects, created by this call)
        agent.change_morphology(g)
        _, via_agent = agent.update_targets(batch, noise)
        assert torch.equal(via_agent, got)
    # mixed morphologies in one call, wider rows
    graphs = _graphs(TARGET_MORPHS)
    counts = [50, 100, 106]
    Lmax = 14
    nobs, _ = _inputs(counts, graphs, seed=9)
    batch, noise = _batch(Lmax, 256, seed=77)
    got = hip.target_q(nobs, noise, batch["reward"], batch["done"], graphs, args.noise_clip, args.discount, counts=counts, q_ld=Lmax + 1)
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        a64.change_morphology(_g64(g))
        sub = {"action": batch["action"][row:row + c, :3 * L], "next_obs": nobs[row:row + c, :41 * L],
               "reward": batch["reward"][row:row + c], "done": batch["done"][row:row + c]}
        _, ref = a64.update_targets(_double(sub), noise[row:row + c, :3 * L].double())
        err = float((got[row:row + c, :L].double() - ref).abs().max())
        assert err < 2e-5 * max(1.0, float(ref.abs().max())), (L, err)
        assert bool((got[row:row + c, L:] == 0).all())
        row += c


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_live_weights_are_read_on_every_forward():
    import torch
    from sgrl_amd.swat_hip import HipSwatCritic
    counts = [5, 7, 3]
    graphs = _graphs(MIXED)
    crit = _critic(seed=11).to("cuda:0")
    hip = HipSwatCritic(crit)
    hip.configure(graphs, counts)
    obs, act = _inputs(counts, graphs, seed=4)

    def check(what):
        got = hip.forward_batch(obs, act)
        ref = _reference(crit, graphs, counts, obs, act, got[0].shape[1])
        for k in range(2):
            err = float((got[k].double() - ref[k]).abs().max())
            assert err < 2e-5 * max(1.0, float(ref[k].abs().max())), (what, k, err)
        return torch.stack(got).clone()

    q0 = check("initial")
    opt = torch.optim.Adam(crit.parameters(), lr=1e-2)          # an optimizer step through the PyTorch module
    crit.change_morphology(graphs[1])
    sum(q.square().sum() for q in crit(obs[5:12, :41 * 7], act[5:12, :3 * 7])).backward()
    opt.step()
    q1 = check("adam")
    assert float((q1 - q0).abs().max()) > 1e-4
    other = _critic(seed=12).to("cuda:0")
    crit.load_state_dict(other.state_dict())
    q2 = check("load_state_dict")
    assert float((q2 - q1).abs().max()) > 1e-4
    crit.cpu()                                                  # the storage moves: the next forward re-binds by itself
    crit.to("cuda:0")
    q3 = check(".to() round trip")
    assert torch.equal(q3, q2)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_target_chain_replays_the_eager_result():
    import torch
    from sgrl_amd.swat_hip import HipSwatTargets
    agent = _agent(seed=21)
    g = _graphs(["3d_walker_7_full"])[0]
    batch, noise = _batch(7, 256, seed=6)
    hip = HipSwatTargets(agent.actor_target, agent.critic_target)
    a = agent.args

    def run(out=None):
        return hip.target_q(batch["next_obs"], noise, batch["reward"], batch["done"], g, a.noise_clip, a.discount, out=out)

    eager = run().clone()
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
    with torch.no_grad():                                       # the captured chain reads the parameters too
        agent.critic_target.critic2.decoder.bias.sub_(0.25)
        agent.actor_target.actor.decoder.bias.add_(0.1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, run())
    assert not torch.equal(out, eager)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_agent_update_uses_the_hip_chain_and_stays_on_float64():
    """The critic loss of one update from identical weights, batch and noise: float64 PyTorch (the reference), float32 PyTorch,
    float32 with the HIP target chain.  The HIP agent may deviate from float64 by at most max(4 x the PyTorch agent's own
    deviation, 1e-5) relative."""
    import torch
    from sgrl_amd.swat_hip import HipSwatTargets
    g = _graphs(["3d_walker_7_full"])[0]
    batch, noise = _batch(7, 256, seed=31)
    hip_agent = _agent(seed=30)
    with torch.no_grad():            # targets away from the online networks, as in the middle of a run
        gen = torch.Generator(device="cuda:0").manual_seed(33)
        for mod in (hip_agent.actor_target, hip_agent.critic_target):
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.02)
    pt_agent = _agent(use_hip=False, seed=30)
    pt_agent.load_state_dict(hip_agent.state_dict())
    f64_agent = _agent(use_hip=False, seed=30)
    f64_agent.load_state_dict(hip_agent.state_dict())
    f64_agent.double()
    assert hip_agent.use_swat_hip and not pt_agent.use_swat_hip
    losses = {}
    for tag, agent in (("hip", hip_agent), ("pytorch", pt_agent), ("float64", f64_agent)):
        agent.change_morphology(_g64(g) if tag == "float64" else g)
        agent.models2train()
        before = [[p.detach().clone() for p in mod.parameters()] for mod in (agent.actor, agent.critic)]
        b, n = (_double(batch), noise.double()) if tag == "float64" else (batch, noise)
        out = agent.update(b, 0, noise=n)
        losses[tag] = float(out["loss/critic_loss"].double())
        assert all(np.isfinite(float(v)) for v in out.values()), out
        for mod, old in zip((agent.actor, agent.critic), before):
            assert max(float((p.detach() - q).abs().max()) for p, q in zip(mod.parameters(), old)) > 0
    assert isinstance(hip_agent._targets, HipSwatTargets) and hip_agent.actor_target._swat_hip is not None
    assert pt_agent._targets is None and pt_agent.critic_target._swat_hip is None
    assert f64_agent._targets is None
    ref = losses["float64"]
    dev_hip, dev_pt = abs(losses["hip"] - ref) / abs(ref), abs(losses["pytorch"] - ref) / abs(ref)
    print("critic loss: float64 %.9g  pytorch f32 %.9g (rel dev %.3g)  hip targets %.9g (rel dev %.3g)"
          % (ref, losses["pytorch"], dev_pt, losses["hip"], dev_hip))
    assert dev_hip <= max(4 * dev_pt, 1e-5), (dev_hip, dev_pt)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_returned_not_faults():
    import torch
    from sgrl_amd import _lib
    from sgrl_amd.swat_hip import HipSwatCritic, HipSwatTargets
    agent = _agent(seed=2)
    tg = HipSwatTargets(agent.actor_target, agent.critic_target)
    crit, actor = tg.critic, tg.actor
    g7, g2 = _graphs(["3d_walker_7_full", "3d_walker_2_right_leg_left_knee"])
    tg.configure([g7], [3])
    for h in (crit.q1, crit.q2, actor):
        h.sync_weights()
    L = crit.L
    z = lambda w: torch.zeros((3, w), device="cuda:0")
    obs, act, q, q_b = z(41 * 7), z(3 * 7), z(7), z(7)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = lambda: L.sgrl_swat_last_error()
    # rows too narrow
    assert L.sgrl_swat_forward_q(crit.q1.h, vp(obs), 41 * 7, vp(act), 3 * 7, 3, vp(q), 6, st) == -1 and b"narrow" in err()
    assert L.sgrl_swat_forward_q(crit.q1.h, vp(obs), 41 * 7, vp(act), 3 * 7 - 1, 3, vp(q), 7, st) == -1 and b"narrow" in err()
    assert L.sgrl_swat_forward_twin(crit.q1.h, crit.q2.h, vp(obs), 41 * 7 - 1, vp(act), 3 * 7, 3, vp(q), vp(q_b), 7, st) == -1 and b"narrow" in err()
    # act_feature outside 1 .. feature - 1
    for bad in (0, 44):
        assert L.sgrl_swat_forward_q(crit.q1.h, vp(obs), 41 * 7, vp(act), 3 * 7, bad, vp(q), 7, st) == -1 and b"act_feature" in err()
    # an actor handle is not a critic
    assert L.sgrl_swat_forward_q(actor.h, vp(obs), 41 * 7, vp(act), 3 * 7, 3, vp(q), 7, st) == -1 and b"not bound as a critic" in err()
    assert L.sgrl_swat_forward_twin(crit.q1.h, actor.h, vp(obs), 41 * 7, vp(act), 3 * 7, 3, vp(q), vp(q_b), 7, st) == -1 and b"critic" in err()
    with pytest.raises(_lib.SgrlError, match="not bound as a critic"):
        actor.forward_q(obs, act)
    rw = torch.zeros(3, device="cuda:0")
    td = lambda a, c1, c2, nld, qld: L.sgrl_swat_td_target(a, c1, c2, vp(obs), 41 * 7, vp(act), nld, vp(rw), vp(rw), 1.0, 0.5, 0.99, vp(q), qld, st)
    assert td(actor.h, actor.h, crit.q2.h, 21, 7) == -1
    assert td(crit.q1.h, crit.q1.h, crit.q2.h, 21, 7) == -1
    assert td(actor.h, crit.q1.h, crit.q2.h, 20, 7) == -1 and b"narrow" in err()
    assert td(actor.h, crit.q1.h, crit.q2.h, 21, 6) == -1 and b"narrow" in err()
    # handles with different batch structures
    crit.q2.configure([g2], [3])
    assert L.sgrl_swat_forward_twin(crit.q1.h, crit.q2.h, vp(obs), 41 * 7, vp(act), 3 * 7, 3, vp(q), vp(q_b), 7, st) == -1
    assert b"different batch structures" in err()
    assert td(actor.h, crit.q1.h, crit.q2.h, 21, 7) == -1 and b"different batch structures" in err()
    crit.q2.configure([g7], [3])
    # and the well-formed calls go through
    assert L.sgrl_swat_forward_twin(crit.q1.h, crit.q2.h, vp(obs), 41 * 7, vp(act), 3 * 7, 3, vp(q), vp(q_b), 7, st) == 0
    assert td(actor.h, crit.q1.h, crit.q2.h, 21, 7) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q).all())
