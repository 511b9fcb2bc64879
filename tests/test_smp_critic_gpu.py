"""HIP SMP critic forward (twin and Q1 only) and the fused TD3 target chain (csrc/smp_actor.hip through sgrl_amd/smp_hip.py
HipSmpCritic / HipSmpTargets and td3.Agent.update_targets) on the MI355X: against the fixtures of the executed reference, against
float64 copies of the PyTorch modules at full size, with live weights, under graph capture, inside Agent.update, the launch counts
and the argument errors of the C ABI.  Reads fixtures and this repository only.

Launches: one twin forward 6 D + 3 (Q1 only: 6 D + 2), one target chain 12 D + 3, D = tree levels of the deepest morphology of the
batch, whatever the number of morphologies, environments or limbs.

Error bar: 2e-5 * max(1, max|ref|) against a float64 copy of the PyTorch module, the bar tests/test_swat_critic_gpu.py gives a HIP
critic (the fixtures: the same bar against the stored float32 values of the executed reference).  Every test prints its measured
error and the float32 PyTorch module's error against the same float64 copy before it asserts.  The fixtures' weights are applied
per morphology, see the header of tests/test_smp_hip_gpu.py.

Measured figures: none yet.  This file has not run on an MI355X (no device was obtainable when it was written); the figures each
test prints belong here and in DESIGN.md section 4.4 after its first run.
"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
BAR = 2e-5
WALKERS = sorted(["3d_walker_2_right_leg_left_knee", "3d_walker_3_left_leg_right_foot", "3d_walker_3_left_knee_right_knee",
                  "3d_walker_4_right_knee_left_foot", "3d_walker_5_foot", "3d_walker_5_left_knee",
                  "3d_walker_6_right_foot", "3d_walker_7_full"])
HELD = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
        "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}
MIXED = ["3d_hopper_3_shin", "3d_walker_7_full", "3d_humanoid_9_full"]
TARGET_MORPHS = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full", "3d_cheetah_14_full"]     # 2, 7 and 14 limbs
MC = 5


def _critic(mc=MC, seed=None, td=True, bu=True):
    """seed None: torch's default initialisation from the generator as it stands."""
    import torch
    from sgrl_amd.smp_policy import CriticGraphPolicy
    if seed is not None:
        torch.manual_seed(seed)
    return CriticGraphPolicy(41, 3, 32, 1, mc, True, td, bu, None).eval()


def _graphs(names):
    import torch
    from sgrl_amd import graph as G, mjcf
    return [G.getGraphDict(mjcf.load_asset(n).parents, TRAV, [], device=torch.device("cuda:0")) for n in names]


def _torch_q(crit, graphs, counts, obs, act, dtype):
    """CriticGraphPolicy.forward per morphology on a copy of the module in `dtype` -> (q1, q2) [n_env, 1]."""
    import torch
    crit.clear_buffer()               # the last forward's outputs (non-leaf tensors) cannot be deep-copied
    c = copy.deepcopy(crit).to(dtype)
    out = torch.zeros((2, obs.shape[0], 1), dtype=dtype, device=obs.device)
    row = 0
    for g, n in zip(graphs, counts):
        L = len(g["parents"])
        c.change_morphology(g)
        with torch.no_grad():
            q1, q2 = c(obs[row:row + n, :41 * L].to(dtype), act[row:row + n, :3 * L].to(dtype))
        out[0, row:row + n], out[1, row:row + n] = q1, q2
        row += n
    return out


def _check(what, got, crit, graphs, counts, obs, act):
    """Asserts |HIP - float64| < BAR * max(1, max|ref|) per head; prints it with the float32 PyTorch module's error first."""
    import torch
    ref = _torch_q(crit, graphs, counts, obs, act, torch.float64)
    f32 = _torch_q(crit, graphs, counts, obs, act, torch.float32)
    for k in range(len(got)):
        mx = float(ref[k].abs().max())
        err = float((got[k].double() - ref[k]).abs().max())
        e32 = float((f32[k].double() - ref[k]).abs().max())
        bar = BAR * max(1.0, mx)
        print("%s q%d: max|q_ref| %.3g  |HIP - float64| %.3g  torch f32 %.3g  bar %.3g" % (what, k + 1, mx, err, e32, bar))
        assert e32 < bar, "the float32 PyTorch module itself misses the bar on this input: choose another input"
        assert err < bar, (what, k, err, bar)
    return ref


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


def _config5_share():
    from sgrl_amd import mjcf
    names = sorted(n for n in mjcf.list_assets() if n not in HELD)
    assert len(names) == 23
    return names, [8188 // len(names)] * len(names)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def test_fixture_morphologies_alone_and_in_one_batch(golden_dir):
    import torch
    from oracle.formula import apply_formula_
    from sgrl_amd.smp_hip import HipSmpCritic
    z = np.load(os.path.join(golden_dir, "smp_forward.npz"))
    with open(os.path.join(golden_dir, "smp_state_dict_keys.json")) as f:
        mc = json.load(f)["max_children"]
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("td1_bu1/")})
    assert len(names) == 5
    graphs = _graphs(names)
    crit = _critic(mc).to("cuda:0")
    hip = HipSmpCritic(crit)
    Lmax = max(len(g["parents"]) for g in graphs)
    obs_all = torch.zeros((4 * len(names), 41 * Lmax), dtype=torch.float32)
    act_all = torch.zeros((4 * len(names), 3 * Lmax), dtype=torch.float32)
    for k, name in enumerate(names):
        o, a = z["td1_bu1/%s/obs" % name], z["td1_bu1/%s/act_in" % name]
        obs_all[4 * k:4 * k + 4, :o.shape[1]] = torch.from_numpy(o)
        act_all[4 * k:4 * k + 4, :a.shape[1]] = torch.from_numpy(a)
    obs_all, act_all = obs_all.cuda(), act_all.cuda()
    for k, (name, g) in enumerate(zip(names, graphs)):
        crit.change_morphology(g)         # this morphology's listing of the shared module: see the header
        apply_formula_(crit)
        tag = "td1_bu1/%s/" % name
        obs, act = torch.from_numpy(z[tag + "obs"]).cuda(), torch.from_numpy(z[tag + "act_in"]).cuda()
        hip.configure([g], [obs.shape[0]])
        alone = [q.clone() for q in hip.forward_q(obs, act)]
        hip.configure(graphs, [4] * len(names))
        batch = [q[4 * k:4 * k + 4].clone() for q in hip.forward_q(obs_all, act_all)]
        f32 = _torch_q(crit, [g], [4], obs, act, torch.float32)
        for h, key in enumerate(("q1", "q2")):
            want = z[tag + key]
            bar = BAR * max(1.0, float(np.abs(want).max()))
            err = float(np.abs(alone[h].cpu().numpy() - want).max())
            e32 = float(np.abs(f32[h].cpu().numpy() - want).max())
            print("fixture %s %s: max|q| %.3g  |HIP - stored| %.3g  torch f32 %.3g  bar %.3g"
                  % (name, key, float(np.abs(want).max()), err, e32, bar))
            assert alone[h].shape == want.shape == (4, 1) and err < bar, (name, key, err, bar)
            assert torch.equal(alone[h], batch[h])        # a morphology's rows do not depend on what else is in the batch


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5, 6])
@pytest.mark.parametrize("workload", ["config3", "config5_share"])
def test_full_size_mixed_batches_against_float64(workload, seed):
    import torch
    from sgrl_amd.smp_hip import HipSmpCritic
    names, counts = (WALKERS, [1024] * len(WALKERS)) if workload == "config3" else _config5_share()
    graphs = _graphs(names)
    crit = _critic(seed=seed).to("cuda:0")
    hip = HipSmpCritic(crit)
    hip.configure(graphs, counts)
    obs, act = _inputs(counts, graphs, seed=seed)
    q1, q2 = (q.clone() for q in hip.forward_q(obs, act))
    assert q1.shape == q2.shape == (int(sum(counts)), 1)
    _check("%s seed %d" % (workload, seed), (q1, q2), crit, graphs, counts, obs, act)
    only = hip.forward_q(obs, act, twin=False)
    assert torch.equal(only, q1) and not torch.equal(q1, q2)
    assert float(q1.abs().max()) > 1e-3 and float(q2.abs().max()) > 1e-3      # non-trivial outputs


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def _agent(use_hip=True, seed=0, device="cuda:0", **over):
    import torch
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(seed)
    kw = dict(actor_type="smp", critic_type="smp", td=True, bu=True, max_children=MC)
    kw.update(over)
    return Agent(default_train_args(**kw), device=torch.device(device), use_hip=use_hip)


def _perturb_targets(agent, seed):
    """Targets that differ from the online networks, as in the middle of a run."""
    import torch
    with torch.no_grad():
        for k, mod in enumerate((agent.actor_target, agent.critic_target)):
            gen = torch.Generator(device="cuda:0").manual_seed(seed + k)
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.02)


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


def _copy_agent(agent, dtype):
    """A PyTorch-only deep copy of the agent in `dtype` (never builds a handle)."""
    for m in (agent.actor, agent.actor_target, agent.critic, agent.critic_target):
        m.clear_buffer()
    a = copy.deepcopy(agent).to(dtype)
    a.use_smp_hip = False
    return a


def test_target_chain_against_float64_update_targets():
    import torch
    from sgrl_amd.smp_hip import HipSmpTargets
    agent = _agent(seed=4)
    _perturb_targets(agent, 40)
    hip = HipSmpTargets(agent.actor_target, agent.critic_target)
    a64, a32 = _copy_agent(agent, torch.float64), _copy_agent(agent, torch.float32)
    args = agent.args
    graphs = _graphs(TARGET_MORPHS)
    for name, g in zip(TARGET_MORPHS, graphs):
        L = len(g["parents"])
        batch, noise = _batch(L, 256, seed=L)
        assert float(noise.abs().max()) > args.noise_clip and 0 < float(batch["done"].sum()) < 256
        assert float(batch["reward"].min()) < 0 < float(batch["reward"].max())
        a64.change_morphology(g)
        a32.change_morphology(g)
        _, ref = a64.update_targets(_double(batch), noise.double())
        _, t32 = a32.update_targets(batch, noise)
        got = hip.target_q(batch["next_obs"], noise, batch["reward"], batch["done"], g, args.noise_clip, args.discount)
        assert got.shape == ref.shape == (256, 1)
        bar = BAR * max(1.0, float(ref.abs().max()))
        err, e32 = float((got.double() - ref).abs().max()), float((t32.double() - ref).abs().max())
        print("target chain %s: max|target| %.3g  |HIP - float64| %.3g  torch f32 %.3g  bar %.3g"
              % (name, float(ref.abs().max()), err, e32, bar))
        assert e32 < bar and err < bar, (name, err, e32, bar)
        ended = batch["done"].reshape(-1) == 1
        assert torch.equal(got[ended], batch["reward"][ended])
        assert float((got[~ended] - batch["reward"][~ended]).abs().min()) > 0            # the critic contributes everywhere else
        assert float((got[~ended] - batch["reward"][~ended]).abs().max()) > 1e-3
        # the same through the agent (the same cached handles, its own HipSmpTargets)
        agent.change_morphology(g)
        _, via_agent = agent.update_targets(batch, noise)
        assert torch.equal(via_agent, got) and agent._targets is not None and agent._targets is not hip
    # mixed morphologies in one call, rows as wide as the largest
    counts = [50, 100, 106]
    nobs, _ = _inputs(counts, graphs, seed=9)
    batch, noise = _batch(14, 256, seed=77)
    got = hip.target_q(nobs, noise, batch["reward"], batch["done"], graphs, args.noise_clip, args.discount, counts=counts)
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        a64.change_morphology(g)
        sub = {"action": batch["action"][row:row + c, :3 * L], "next_obs": nobs[row:row + c, :41 * L],
               "reward": batch["reward"][row:row + c], "done": batch["done"][row:row + c]}
        _, ref = a64.update_targets(_double(sub), noise[row:row + c, :3 * L].double())
        err = float((got[row:row + c].double() - ref).abs().max())
        print("target chain, mixed call, %d limbs: max|target| %.3g  |HIP - float64| %.3g" % (L, float(ref.abs().max()), err))
        assert err < BAR * max(1.0, float(ref.abs().max())), (L, err)
        row += c


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_live_weights_are_read_on_every_forward():
    import torch
    from sgrl_amd.smp_hip import HipSmpCritic
    counts = [5, 7, 3]
    graphs = _graphs(MIXED)
    crit = _critic(4, seed=11).to("cuda:0")
    hip = HipSmpCritic(crit)
    hip.configure(graphs, counts)
    obs, act = _inputs(counts, graphs, seed=4)

    def check(what):
        got = [q.clone() for q in hip.forward_q(obs, act)]
        _check("live weights, " + what, got, crit, graphs, counts, obs, act)
        return torch.stack(got)

    q0 = check("initial")
    opt = torch.optim.Adam(crit.parameters(), lr=1e-2)          # an in-place optimizer step through the PyTorch module
    crit.change_morphology(graphs[1])
    sum(q.square().sum() for q in crit(obs[5:12, :41 * 7], act[5:12, :3 * 7])).backward()
    opt.step()
    q1 = check("adam")
    assert float((q1 - q0).abs().max()) > 1e-4
    src = _critic(4, seed=13).to("cuda:0")                      # an in-place soft update (reference common/functional.py:7-10)
    with torch.no_grad():
        for p, q in zip(crit.parameters(), src.parameters()):
            p.data.copy_(0.5 * p.data + 0.5 * q.data)
    q2 = check("soft update")
    assert float((q2 - q1).abs().max()) > 1e-4
    other = _critic(4, seed=12).to("cuda:0")
    other.change_morphology(graphs[1])                          # the same listing of the shared module, so the keys agree
    crit.load_state_dict(other.state_dict())
    q3 = check("load_state_dict")
    assert float((q3 - q2).abs().max()) > 1e-4
    crit.clear_buffer()
    crit.cpu()                                                  # the storage moves: the next forward re-binds by itself
    crit.to("cuda:0")
    q4 = check(".to() round trip")
    assert torch.equal(q4, q3)
    assert hip._bound == tuple(p.data_ptr() for p in hip._params())


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_target_chain_replays_the_eager_result():
    import torch
    from sgrl_amd.smp_hip import HipSmpTargets
    agent = _agent(seed=21)
    _perturb_targets(agent, 50)
    g = _graphs(["3d_walker_7_full"])[0]
    batch, noise = _batch(7, 256, seed=6)
    static = {k: batch[k].clone() for k in ("next_obs", "reward", "done")}
    snoise = noise.clone()
    hip = HipSmpTargets(agent.actor_target, agent.critic_target)
    a = agent.args

    def run(out=None):
        return hip.target_q(static["next_obs"], snoise, static["reward"], static["done"], g, a.noise_clip, a.discount, out=out)

    eager = run().clone()                                       # the eager run comes first: it sizes the workspaces
    torch.cuda.synchronize()
    gen = (hip.actor.generation(), hip.critic.generation())
    out = torch.zeros_like(eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    batch2, noise2 = _batch(7, 256, seed=8)                     # new inputs, copied into the static tensors
    for k in static:
        static[k].copy_(batch2[k])
    snoise.copy_(noise2)
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    fresh = run()
    assert torch.equal(replayed, fresh) and not torch.equal(replayed, eager)
    assert (hip.actor.generation(), hip.critic.generation()) == gen      # nothing the graph points into was freed


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_agent_update_runs_through_the_chain_and_stays_on_float64():
    """Three updates (the first and third with the delayed actor step) of an smp + smp agent whose target chain runs on HIP, and of
    a float64 agent from the same weights fed the same batches and target noise: every update's target values, computed from each
    agent's OWN (updated) target networks, within the bar; finite losses."""
    import torch
    from sgrl_amd.smp_hip import HipSmpTargets
    g = _graphs(["3d_walker_7_full"])[0]
    hip_agent = _agent(seed=30)
    _perturb_targets(hip_agent, 33)
    f64_agent = _copy_agent(hip_agent, torch.float64)
    pt_agent = _agent(use_hip=False, seed=30)
    pt_agent.load_state_dict(hip_agent.state_dict())
    assert hip_agent.use_smp_hip and not pt_agent.use_smp_hip and not f64_agent.use_smp_hip
    for agent in (hip_agent, pt_agent, f64_agent):
        agent.change_morphology(g)
        agent.models2train()
    for it in range(3):
        batch, noise = _batch(7, 256, seed=60 + it)
        _, tq = hip_agent.update_targets(batch, noise)
        _, tq32 = pt_agent.update_targets(batch, noise)
        _, ref = f64_agent.update_targets(_double(batch), noise.double())
        bar = BAR * max(1.0, float(ref.abs().max()))
        err, e32 = float((tq.double() - ref).abs().max()), float((tq32.double() - ref).abs().max())
        print("update %d: max|target| %.3g  |HIP agent - float64 agent| %.3g  torch f32 agent %.3g  bar %.3g"
              % (it, float(ref.abs().max()), err, e32, bar))
        assert err < bar, (it, err, bar)
        losses = {}
        for tag, agent in (("hip", hip_agent), ("pytorch", pt_agent), ("float64", f64_agent)):
            b, n = (_double(batch), noise.double()) if tag == "float64" else (batch, noise)
            out = agent.update(b, it, noise=n)
            assert all(np.isfinite(float(v)) for v in out.values()), (tag, out)
            losses[tag] = float(out["loss/critic_loss"])
        print("update %d critic loss: float64 %.9g  pytorch f32 %.9g  hip targets %.9g" % (it, losses["float64"], losses["pytorch"], losses["hip"]))
    assert isinstance(hip_agent._targets, HipSmpTargets) and hip_agent.actor_target._smp_hip is not None
    assert pt_agent._targets is None and pt_agent.actor_target._smp_hip is None and pt_agent.critic_target._smp_hip is None
    assert f64_agent._targets is None and f64_agent.critic_target._smp_hip is None
    # a CPU agent never constructs a handle either
    cpu_agent = _agent(seed=1, device="cpu")
    cpu_agent.change_morphology({"parents": list(g["parents"])})
    cb = {k: v[:8].cpu() for k, v in _batch(7, 8, seed=3)[0].items()}
    cpu_agent.update_targets(cb)
    assert cpu_agent._targets is None and cpu_agent.actor_target._smp_hip is None
    # the td-only mode keeps PyTorch
    td_only = _agent(seed=1, bu=False)
    td_only.change_morphology(g)
    td_only.update_targets(_batch(7, 8, seed=3)[0])
    assert not td_only.use_smp_hip and td_only._targets is None


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_launch_counts_depend_on_the_deepest_tree_and_twin_only():
    from sgrl_amd.smp_hip import HipSmpTargets
    agent = _agent(seed=2)
    tg = HipSmpTargets(agent.actor_target, agent.critic_target)

    def launches(names, counts):
        tg.configure(_graphs(names), counts)
        D = tg.critic.num_levels
        assert tg.critic.launches() == tg.critic.launches(twin=True) == 6 * D + 3
        assert tg.critic.launches(twin=False) == 6 * D + 2
        assert tg.launches() == 12 * D + 3 == tg.actor.launches() + tg.critic.launches()
        return tg.launches(), D

    assert launches(["3d_walker_7_full"], [3]) == (51, 4)
    assert launches(WALKERS, [16] * len(WALKERS)) == (51, 4)              # a mixed batch of the same depth: the same count
    assert launches(["3d_hopper_5_full"], [7]) == (63, 5)                  # a deeper tree: more
    assert launches(["3d_walker_2_right_leg_left_knee"], [4]) == (27, 2)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_returned_not_faults():
    import torch
    from sgrl_amd import _lib
    from sgrl_amd.smp_hip import HipSmpActor, HipSmpCritic, HipSmpTargets
    agent = _agent(seed=2)
    tg = HipSmpTargets(agent.actor_target, agent.critic_target)
    crit, actor = tg.critic, tg.actor
    g7, g2 = _graphs(["3d_walker_7_full", "3d_walker_2_right_leg_left_knee"])
    tg.configure([g7], [3])
    crit.sync_weights()
    actor.sync_weights()
    L = crit.L
    z = lambda w: torch.zeros((3, w), device="cuda:0")
    obs, act = z(41 * 7), z(3 * 7)
    rw = torch.zeros(3, device="cuda:0")
    q1, q2 = torch.full((3,), 7.0, device="cuda:0"), torch.full((3,), 7.0, device="cuda:0")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(None)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = lambda: L.sgrl_smp_last_error()
    fq = lambda h, o=vp(obs), old=41 * 7, a=vp(act), ald=3 * 7, o1=vp(q1), o2=vp(q2): L.sgrl_smp_forward_q(h, o, old, a, ald, o1, o2, st)
    td = lambda a, c, old=41 * 7, nld=3 * 7, n=vp(act), out=vp(q1): L.sgrl_smp_td_target(a, c, vp(obs), old, n, nld, vp(rw), vp(rw), 1.0, 0.5,
                                                                                       0.99, out, st)
    # a critic call on an actor-bound handle and vice versa
    assert fq(actor.h) == -1 and b"not bound as a critic" in err()
    assert L.sgrl_smp_forward(crit.h, vp(obs), 41 * 7, vp(act), 3 * 7, ctypes.c_float(1.0), st) == -1 and b"not bound as an actor" in err()
    assert td(crit.h, crit.h) == -1 and b"not bound as an actor" in err()
    assert td(actor.h, actor.h) == -1 and b"not bound as a critic" in err()
    with pytest.raises(_lib.SgrlError, match="forward_q"):
        crit.forward_batch(obs)
    # rows too narrow
    assert fq(crit.h, old=41 * 7 - 1) == -1 and b"narrow" in err()
    assert fq(crit.h, ald=3 * 7 - 1) == -1 and b"narrow" in err()
    assert td(actor.h, crit.h, old=41 * 7 - 1) == -1 and b"narrow" in err()
    assert td(actor.h, crit.h, nld=3 * 7 - 1) == -1 and b"narrow" in err()
    # null pointers
    assert fq(null) == -1 and b"null" in err()
    assert fq(crit.h, o=null) == -1 and b"null" in err()
    assert fq(crit.h, a=null) == -1 and b"null" in err()
    assert fq(crit.h, o1=null) == -1 and b"null" in err()
    assert td(null, crit.h) == -1 and td(actor.h, null) == -1 and b"null" in err()
    assert td(actor.h, crit.h, n=null) == -1 and td(actor.h, crit.h, out=null) == -1 and b"null" in err()
    arr = (ctypes.c_void_p * 24)(*[p.data_ptr() for p in crit._params()])
    bind = lambda h, a, n, mc, f, af: L.sgrl_smp_bind_critic_params(h, a, n, mc, f, af)
    assert bind(crit.h, null, 24, MC, 44, 3) == -1 and b"null" in err()
    assert bind(crit.h, ctypes.cast(arr, ctypes.c_void_p), 18, MC, 44, 3) == -1 and b"expected 24" in err()
    assert bind(crit.h, ctypes.cast(arr, ctypes.c_void_p), 24, MC, 44, 44) == -1 and b"act_feature" in err()
    assert bind(crit.h, ctypes.cast(arr, ctypes.c_void_p), 24, 9, 44, 3) == -1 and b"max_children" in err()
    # mismatched batch structures
    crit.configure([g2], [3])
    assert td(actor.h, crit.h) == -1 and b"different batch structures" in err()
    crit.configure([g7], [3])
    # a max_children mismatch: the structure was built for another width of the children rows than the bound parameters'
    tree = np.asarray([[0, -1, 0, 1, -1], [1, 0, 0, -1, -1]], dtype=np.int32)
    one = np.asarray([2], dtype=np.int32)
    cnt = np.asarray([3], dtype=np.int32)
    npp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L.sgrl_smp_graph(crit.h, 1, npp(one), npp(cnt), 2, npp(tree)) == 0
    assert fq(crit.h) == -1 and b"max_children" in err()
    assert td(actor.h, crit.h) == -1 and b"max_children" in err()
    crit._cfg_key = None
    crit.configure([g7], [3])
    # critic and actor of different per-limb sizes
    other = HipSmpActor(agent.actor)
    other.configure([g7], [3])
    other.sync_weights()
    arr18 = (ctypes.c_void_p * 18)(*[p.data_ptr() for p in other._params()])
    assert L.sgrl_smp_bind_params(other.h, ctypes.cast(arr18, ctypes.c_void_p), 18, MC, 40, 3) == 0
    assert td(other.h, crit.h, old=40 * 7) == -1 and b"feature + out" in err()
    # the td-only mode has no handle
    with pytest.raises(_lib.SgrlError, match="td and bu"):
        HipSmpCritic(_critic(3, td=True, bu=False).to("cuda:0"))
    torch.cuda.synchronize()
    assert bool((q1 == 7).all()) and bool((q2 == 7).all())       # none of the refused calls wrote anything
    # and the well-formed calls go through
    assert fq(crit.h) == 0 and fq(crit.h, o2=null) == 0 and td(actor.h, crit.h) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(q1).all()) and bool(torch.isfinite(q2).all()) and not bool((q2 == 7).any())
