"""Batched HIP SMP actor forward (csrc/smp_actor.hip through sgrl_amd/smp_hip.py) on the MI355X: against the fixtures of the
executed reference, against a float64 copy of the PyTorch module on full-size mixed batches, with live weights, under graph
capture, and inside DeviceTrainer's loop.

Launches of one forward: 6 * D, D = tree levels of the deepest morphology of the batch (1 embedding + 2 D bottom-up + 4 (D - 1)
top-down + 3 action launches), whatever the number of morphologies, environments or limbs.

Tolerance: 2e-5 absolute on actions (|action| <= max_action = 1), the figure tests/test_set_gpu.py and tests/test_swat_hip_gpu.py
allow a HIP actor.  Largest errors measured on one MI355X (every test prints its figure before it asserts); `torch f32` is the
float32 PyTorch module on the same batch against the same float64 copy:
    fixtures (five morphologies, alone and in one batch)   2.4e-7 against the stored f32 actions of the reference
    config 3 (8 walkers x 1024), three initialisations     2.7e-8      torch f32 3.0e-8
    config-5 share (23 morphologies, 8188 envs), three     3.1e-8      torch f32 3.1e-8
    live weights (worst: after the Adam step)              9.9e-8      torch f32 9.3e-8
    DeviceTrainer, after a round of updates                2.0e-8      torch f32 3.2e-8

The fixtures' weights: oracle.formula keys a value on the parameter's state_dict NAME, and the one shared module of SMP is listed
once per limb (`sNet.<i>.`), so the last listing wins and the weights behind a stored action are those written with THAT
morphology's listing (tests/test_smp_policy.py applies the formula after change_morphology for the same reason).  One batch of
all five morphologies can therefore match the stored action of one of them at a time: the batch test runs the five-morphology
batch once per morphology's weights and compares that morphology's rows.
"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
TOL = 2e-5
WALKERS = sorted(["3d_walker_2_right_leg_left_knee", "3d_walker_3_left_leg_right_foot", "3d_walker_3_left_knee_right_knee",
                  "3d_walker_4_right_knee_left_foot", "3d_walker_5_foot", "3d_walker_5_left_knee",
                  "3d_walker_6_right_foot", "3d_walker_7_full"])
HELD = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
        "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}


def _policy(mc=5, seed=None, td=True, bu=True):
    """seed None: torch's default initialisation from the generator as it stands."""
    import torch
    from sgrl_amd.smp_policy import ActorGraphPolicy
    if seed is not None:
        torch.manual_seed(seed)
    return ActorGraphPolicy(41, 3, 32, 1, 1.0, mc, True, td, bu, None).eval()


def _graphs(names):
    import torch
    from sgrl_amd import graph as G, mjcf
    return [G.getGraphDict(mjcf.load_asset(n).parents, TRAV, [], device=torch.device("cuda:0")) for n in names]


def _torch_forward(pol, graphs, counts, obs, act_ld, dtype):
    """ActorGraphPolicy.forward per morphology (change_morphology + forward under no_grad) on a copy of the module in `dtype`."""
    import torch
    pol.clear_buffer()                # the last forward's output (a non-leaf tensor) cannot be deep-copied
    p = copy.deepcopy(pol).to(dtype)
    out = torch.zeros((obs.shape[0], act_ld), dtype=dtype, device=obs.device)
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        p.change_morphology(g)
        with torch.no_grad():
            out[row:row + c, :3 * L] = p(obs[row:row + c, :41 * L].to(dtype))
        row += c
    return out


def _reference(pol, graphs, counts, obs, act_ld):
    import torch
    return _torch_forward(pol, graphs, counts, obs, act_ld, torch.float64)


def _errors(what, got, pol, graphs, counts, obs):
    """max |HIP - float64|, printed with the float32 PyTorch module's error against the same float64 copy."""
    import torch
    ref = _reference(pol, graphs, counts, obs, got.shape[1])
    err = float((got.double() - ref).abs().max())
    f32 = float((_torch_forward(pol, graphs, counts, obs, got.shape[1], torch.float32).double() - ref).abs().max())
    print("%s: max |HIP - float64| = %.3g, torch f32 against float64 = %.3g" % (what, err, f32))
    return err


def _obs(counts, graphs, seed=1):
    import torch
    Lmax = max(len(g["parents"]) for g in graphs)
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    obs = torch.zeros((int(sum(counts)), 41 * Lmax), dtype=torch.float32, device="cuda:0")
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        obs[row:row + c, :41 * L] = torch.randn((c, 41 * L), device="cuda:0", generator=gen)
        row += c
    return obs


def _padding_is_zero(act, graphs, counts):
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        if act.shape[1] > 3 * L:
            assert bool((act[row:row + c, 3 * L:] == 0).all())
        row += c


def _config5_share():
    from sgrl_amd import mjcf
    names = sorted(n for n in mjcf.list_assets() if n not in HELD)
    assert len(names) == 23
    return names, [8188 // len(names)] * len(names)


def test_fixture_morphologies_alone_and_in_one_batch(golden_dir):
    import torch
    from oracle.formula import apply_formula_
    from sgrl_amd.smp_hip import HipSmpActor
    z = np.load(os.path.join(golden_dir, "smp_forward.npz"))
    with open(os.path.join(golden_dir, "smp_state_dict_keys.json")) as f:
        mc = json.load(f)["max_children"]
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("td1_bu1/")})
    assert len(names) == 5
    graphs = _graphs(names)
    pol = _policy(mc).to("cuda:0")
    actor = HipSmpActor(pol)
    Lmax = max(len(g["parents"]) for g in graphs)
    obs_all = torch.zeros((4 * len(names), 41 * Lmax), dtype=torch.float32)
    for k, name in enumerate(names):
        o = z["td1_bu1/%s/obs" % name]
        obs_all[4 * k:4 * k + 4, :o.shape[1]] = torch.from_numpy(o)
    obs_all = obs_all.cuda()
    worst_alone = worst_batch = 0.0
    for k, (name, g) in enumerate(zip(names, graphs)):
        pol.change_morphology(g)          # this morphology's listing of the shared module: see the header
        apply_formula_(pol)
        want = z["td1_bu1/%s/action" % name]
        obs = torch.from_numpy(z["td1_bu1/%s/obs" % name]).cuda()
        actor.configure([g], [obs.shape[0]])
        a = actor.forward_batch(obs).cpu().numpy()
        assert a.shape == want.shape
        worst_alone = max(worst_alone, float(np.abs(a - want).max()))
        actor.configure(graphs, [4] * len(names))
        got = actor.forward_batch(obs_all)
        _padding_is_zero(got, graphs, [4] * len(names))
        b = got[4 * k:4 * k + 4, :want.shape[1]].cpu().numpy()
        worst_batch = max(worst_batch, float(np.abs(b - want).max()))
        assert np.array_equal(a, b)       # the rows of a morphology do not depend on what else is in the batch
    print("fixtures: max |HIP - stored action| alone = %.3g, in one batch = %.3g" % (worst_alone, worst_batch))
    assert worst_alone < TOL and worst_batch < TOL, (worst_alone, worst_batch)


@pytest.mark.parametrize("seed", [None, 5, 6])
@pytest.mark.parametrize("workload", ["config3", "config5_share"])
def test_full_size_mixed_batches_against_float64(workload, seed):
    import torch
    from sgrl_amd.smp_hip import HipSmpActor
    if workload == "config3":
        names, counts = WALKERS, [1024] * len(WALKERS)
    else:
        names, counts = _config5_share()
    graphs = _graphs(names)
    pol = _policy(5, seed=seed).to("cuda:0")
    actor = HipSmpActor(pol)
    actor.configure(graphs, counts)
    obs = _obs(counts, graphs)
    act_ld = 3 * actor.max_limbs + 5            # wider than needed: the extra slots are padding too
    out = torch.full((obs.shape[0], act_ld), float("nan"), device="cuda:0")
    actor.forward_batch(obs, out=out, act_ld=act_ld)
    err = _errors("%s seed %s" % (workload, seed), out, pol, graphs, counts, obs)
    assert err < TOL, err
    _padding_is_zero(out, graphs, counts)
    assert float(out.abs().max()) > 1e-3                        # a non-trivial output


def test_launch_count_depends_on_the_deepest_tree_only():
    from sgrl_amd.smp_hip import HipSmpActor
    pol = _policy(5, seed=2).to("cuda:0")
    actor = HipSmpActor(pol)

    def launches(names, counts):
        actor.configure(_graphs(names), counts)
        assert actor.launches() == 6 * actor.num_levels
        return actor.launches(), actor.num_levels

    assert launches(["3d_walker_7_full"], [3]) == (24, 4)
    assert launches(WALKERS, [1024] * len(WALKERS)) == (24, 4)
    assert launches(["3d_hopper_5_full"], [7]) == (30, 5)
    assert launches(*_config5_share()) == (30, 5)
    assert launches(["3d_walker_2_right_leg_left_knee"], [4]) == (12, 2)


def test_bad_structures_narrow_rows_and_the_td_only_mode_are_rejected():
    import torch
    from sgrl_amd import _lib
    from sgrl_amd.smp_hip import HipSmpActor
    pol = _policy(3).to("cuda:0")
    actor = HipSmpActor(pol)
    with pytest.raises(_lib.SgrlError, match="16"):
        actor.configure([{"parents": list(range(-1, 16))}], [2])             # 17 limbs
    cheetah = _graphs(["3d_cheetah_14_full"])[0]
    with pytest.raises(_lib.SgrlError, match="max_children"):
        actor.configure([cheetah], [2])                                      # a limb with more than 3 children
    g = _graphs(["3d_walker_7_full"])[0]
    actor.configure([g], [3])
    actor.sync_weights()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    obs = torch.zeros((3, 41 * 7), device="cuda:0")
    out = torch.zeros((3, 3 * 7), device="cuda:0")
    rc = actor.L.sgrl_smp_forward(actor.h, ctypes.c_void_p(obs.data_ptr()), 41 * 7, ctypes.c_void_p(out.data_ptr()), 3 * 7 - 1,
                                  ctypes.c_float(1.0), stream)
    assert rc == -1 and b"act_ld" in actor.L.sgrl_smp_last_error()
    rc = actor.L.sgrl_smp_forward(actor.h, ctypes.c_void_p(obs.data_ptr()), 41 * 7 - 1, ctypes.c_void_p(out.data_ptr()), 3 * 7,
                                  ctypes.c_float(1.0), stream)
    assert rc == -1 and b"obs_ld" in actor.L.sgrl_smp_last_error()
    # a batch structure for another max_children than the bound parameters'
    sch_tree = np.asarray([[0, -1, 0, 1, -1], [1, 0, 0, -1, -1]], dtype=np.int32)
    one = np.asarray([2], dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert actor.L.sgrl_smp_graph(actor.h, 1, vp(one), vp(one), 2, vp(sch_tree)) == 0
    rc = actor.L.sgrl_smp_forward(actor.h, ctypes.c_void_p(obs.data_ptr()), 41 * 7, ctypes.c_void_p(out.data_ptr()), 3 * 7,
                                  ctypes.c_float(1.0), stream)
    assert rc == -1 and b"max_children" in actor.L.sgrl_smp_last_error()
    # rows that are no forest: a child listed by a limb that is not its parent
    bad = np.asarray([[0, -1, 0, 1, -1], [1, 0, 0, 0, -1]], dtype=np.int32)
    assert actor.L.sgrl_smp_graph(actor.h, 1, vp(one), vp(one), 2, vp(bad)) == -1
    with pytest.raises(_lib.SgrlError, match="td and bu"):
        HipSmpActor(_policy(3, td=True, bu=False).to("cuda:0"))


def test_live_weights_are_read_on_every_forward():
    import torch
    from sgrl_amd.smp_hip import HipSmpActor
    names = ["3d_hopper_3_shin", "3d_walker_7_full", "3d_humanoid_9_full"]
    counts = [5, 7, 3]
    graphs = _graphs(names)
    pol = _policy(4, seed=11).to("cuda:0")
    actor = HipSmpActor(pol)
    actor.configure(graphs, counts)
    obs = _obs(counts, graphs, seed=4)

    def check(what):
        got = actor.forward_batch(obs)
        err = _errors("live weights, " + what, got, pol, graphs, counts, obs)
        assert err < TOL, (what, err)
        return got.clone()

    a0 = check("initial")
    # an in-place change of one tensor in the middle of the top-down chain
    with torch.no_grad():
        pol.actor[0].msg_base.l2.weight.mul_(1.5)
    a1 = check("msg_base.l2.weight *= 1.5")
    assert float((a1 - a0).abs().max()) > 1e-5
    # an Adam step through the PyTorch module (rows of one morphology)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-2)
    pol.change_morphology(graphs[1])
    pol(obs[5:12, :41 * 7]).square().sum().backward()
    opt.step()
    a2 = check("adam")
    assert float((a2 - a1).abs().max()) > 1e-4
    # load_state_dict from another network (same morphology listing, so the keys agree)
    other = _policy(4, seed=12).to("cuda:0")
    other.change_morphology(graphs[1])
    pol.load_state_dict(other.state_dict())
    a3 = check("load_state_dict")
    assert float((a3 - a2).abs().max()) > 1e-4
    # an in-place soft update (reference common/functional.py:7-10)
    src = _policy(4, seed=13).to("cuda:0")
    with torch.no_grad():
        for p, q in zip(pol.parameters(), src.parameters()):
            p.data.copy_(0.5 * p.data + 0.5 * q.data)
    a4 = check("soft update")
    assert float((a4 - a3).abs().max()) > 1e-4
    # .to() round trip: the storage moves, the next forward re-binds by itself
    pol.clear_buffer()
    pol.cpu()
    pol.to("cuda:0")
    a5 = check(".to() round trip")
    assert torch.equal(a5, a4)


def test_graph_capture_replays_the_eager_result_bit_for_bit():
    import torch
    from sgrl_amd.smp_hip import HipSmpActor
    names = WALKERS
    counts = [64] * len(names)
    graphs = _graphs(names)
    pol = _policy(5, seed=21).to("cuda:0")
    actor = HipSmpActor(pol)
    actor.configure(graphs, counts)
    obs = _obs(counts, graphs, seed=6)
    eager = actor.forward_batch(obs).clone()
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        actor.forward_batch(obs, out=out)
    torch.cuda.current_stream().wait_stream(s)
    gen = actor.generation()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        actor.forward_batch(obs, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # new observations in the captured buffer are picked up by a replay
    obs.copy_(_obs(counts, graphs, seed=7))
    g.replay()
    torch.cuda.synchronize()
    fresh = actor.forward_batch(obs).clone()
    assert torch.equal(out, fresh) and not torch.equal(out, eager)
    # the captured forward reads the parameters too: a change shows up in the next replay
    with torch.no_grad():
        pol.actor[0].action_base.l3.bias.add_(0.25)
        pol.sNet[0].fc2.weight.mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, actor.forward_batch(obs))
    assert not torch.equal(out, fresh)
    assert actor.generation() == gen                            # nothing the graph points into was freed


def test_device_trainer_trains_smp():
    import torch
    from sgrl_amd.smp_policy import ActorGraphPolicy
    from sgrl_amd.smp_hip import HipSmpActor
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_walker_2_right_leg_left_knee", "3d_hopper_3_shin", "3d_humanoid_9_full"]
    args = default_train_args(actor_type="smp", critic_type="smp", td=True, bu=True, max_children=4, max_episode_steps=40)
    tr = DeviceTrainer(names, 32, args=args, seed=3, device="cuda:0", max_buffer_size=4096, batch_size=32)
    assert isinstance(tr.agent.actor, ActorGraphPolicy) and isinstance(tr.ro.actor, HipSmpActor)
    tr.warmup(60)
    assert all(b.max_sample_size >= 32 for b in tr.buffers)
    obs = tr.ro.env.obs.clone()
    before = [p.detach().clone() for p in tr.agent.actor.parameters()]
    a0 = tr.ro.policy_forward(obs).clone()
    out = tr.train_round(max_steps=200, max_iters=2)
    assert out["per_morph_iter"] >= 1
    for name in names:
        loss = tr.last_losses[name]
        assert all(np.isfinite(float(v)) for v in loss.values()), loss
    moved = max(float((p - q).abs().max()) for p, q in zip(tr.agent.actor.parameters(), before))
    assert moved > 0
    a1 = tr.ro.policy_forward(obs).clone()
    assert float((a1 - a0).abs().max()) > 0
    env = tr.ro.env
    err = _errors("DeviceTrainer, after training", a1, tr.agent.actor, tr.graph_dicts, env.counts, obs)
    assert err < TOL, err
