"""Batched HIP SWAT actor forward (csrc/swat_actor.hip through sgrl_amd/swat_hip.py) on the MI355X: against the fixtures of the
executed reference, against a float64 copy of the PyTorch module on full-size mixed batches, with live weights, under graph
capture, and inside DeviceTrainer's loop."""
import copy
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


def _policy(cond=0, tnorm=1, seed=0):
    import torch
    from sgrl_amd.set_policy import default_args
    from sgrl_amd.swat_policy import StructurePolicy
    torch.manual_seed(seed)
    return StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False,
                           default_args(condition_decoder_on_features=cond, transformer_norm=tnorm)).eval()


def _graphs(names):
    import torch
    from sgrl_amd import graph as G, mjcf
    return [G.getGraphDict(mjcf.load_asset(n).parents, TRAV, [], device=torch.device("cuda:0")) for n in names]


def _reference(pol, graphs, counts, obs, act_ld):
    """StructurePolicy.forward per morphology on a float64 copy of the module (graph tensors cast too)."""
    import torch
    pol.clear_buffer()                # the last forward's output (a non-leaf tensor) cannot be deep-copied
    p64 = copy.deepcopy(pol).double()
    out = torch.zeros((obs.shape[0], act_ld), dtype=torch.float64, device=obs.device)
    row = 0
    for g, c in zip(graphs, counts):
        L = len(g["parents"])
        g64 = dict(g)
        g64["relation"] = g["relation"].double()
        p64.change_morphology(g64)
        with torch.no_grad():
            out[row:row + c, :3 * L] = p64(obs[row:row + c, :41 * L].double())
        row += c
    return out


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


@pytest.mark.parametrize("cond", [0, 1])
def test_fixture_morphologies_alone_and_in_one_batch(cond, golden_dir):
    import torch
    from oracle.formula import apply_formula_
    from sgrl_amd.swat_hip import HipSwatActor
    z = np.load(os.path.join(golden_dir, "swat_forward.npz"))
    pol = _policy(cond)
    apply_formula_(pol)
    pol.to("cuda:0")
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("cond%d/" % cond)})
    assert len(names) == 5
    graphs = _graphs(names)
    actor = HipSwatActor(pol)
    for name, g in zip(names, graphs):
        tag = "cond%d/%s/" % (cond, name)
        obs = torch.from_numpy(z[tag + "obs"]).cuda()
        actor.configure([g], [obs.shape[0]])
        a = actor.forward_batch(obs).cpu().numpy()
        assert a.shape == z[tag + "action"].shape
        np.testing.assert_allclose(a, z[tag + "action"], atol=2e-5, rtol=0)
    Lmax = max(len(g["parents"]) for g in graphs)
    obs = torch.zeros((4 * len(names), 41 * Lmax), dtype=torch.float32)
    want = np.zeros((4 * len(names), 3 * Lmax), dtype=np.float32)
    for k, name in enumerate(names):
        tag = "cond%d/%s/" % (cond, name)
        o, a = z[tag + "obs"], z[tag + "action"]
        obs[4 * k:4 * k + 4, :o.shape[1]] = torch.from_numpy(o)
        want[4 * k:4 * k + 4, :a.shape[1]] = a
    actor.configure(graphs, [4] * len(names))
    got = actor.forward_batch(obs.cuda()).cpu().numpy()
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=0)       # padding slots included: exact zeros there


@pytest.mark.parametrize("tnorm", [1, 0])
@pytest.mark.parametrize("workload", ["config3", "config5_share"])
def test_full_size_mixed_batches_against_float64(workload, tnorm):
    import torch
    from sgrl_amd import mjcf
    from sgrl_amd.swat_hip import HipSwatActor
    if workload == "config3":
        names, counts = WALKERS, [1024] * len(WALKERS)
    else:
        names = sorted(n for n in mjcf.list_assets() if n not in HELD)
        assert len(names) == 23
        counts = [8188 // len(names)] * len(names)
    graphs = _graphs(names)
    pol = _policy(tnorm=tnorm, seed=5).to("cuda:0")
    actor = HipSwatActor(pol)
    actor.configure(graphs, counts)
    obs = _obs(counts, graphs)
    act_ld = 3 * actor.max_limbs + 5            # wider than needed: the extra slots are padding too
    out = torch.full((obs.shape[0], act_ld), float("nan"), device="cuda:0")
    actor.forward_batch(obs, out=out, act_ld=act_ld)
    ref = _reference(pol, graphs, counts, obs, act_ld)
    err = float((out.double() - ref).abs().max())
    assert err < 2e-5, err
    _padding_is_zero(out, graphs, counts)
    assert float(out.abs().max()) > 1e-3                        # a non-trivial output


def test_too_many_limbs_and_narrow_rows_are_rejected():
    import torch
    from sgrl_amd import _lib
    from sgrl_amd.swat_hip import HipSwatActor
    pol = _policy().to("cuda:0")
    actor = HipSwatActor(pol)
    g = _graphs(["3d_walker_7_full"])[0]
    big = {"parents": list(range(-1, 15)), "traversals": [torch.zeros(16, dtype=torch.int64)] * 3,
           "relation": torch.zeros((16, 16, 3))}
    with pytest.raises(_lib.SgrlError, match="15"):
        actor.configure([big], [2])
    actor.configure([g], [3])
    actor.sync_weights()
    obs = torch.zeros((3, 41 * 7), device="cuda:0")
    out = torch.zeros((3, 3 * 7 - 1), device="cuda:0")
    import ctypes
    rc = actor.L.sgrl_swat_forward(actor.h, ctypes.c_void_p(obs.data_ptr()), 41 * 7, ctypes.c_void_p(out.data_ptr()), 3 * 7 - 1,
                                   ctypes.c_float(1.0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b"act_ld" in actor.L.sgrl_swat_last_error()


def test_live_weights_are_read_on_every_forward():
    import torch
    from sgrl_amd.swat_hip import HipSwatActor
    names = ["3d_hopper_3_shin", "3d_walker_7_full", "3d_humanoid_9_full"]
    counts = [5, 7, 3]
    graphs = _graphs(names)
    pol = _policy(seed=11).to("cuda:0")
    actor = HipSwatActor(pol)
    actor.configure(graphs, counts)
    obs = _obs(counts, graphs, seed=4)

    def check(what):
        got = actor.forward_batch(obs)
        ref = _reference(pol, graphs, counts, obs, got.shape[1])
        err = float((got.double() - ref).abs().max())
        assert err < 2e-5, (what, err)
        return got.clone()

    a0 = check("initial")
    # an Adam step through the PyTorch module (rows of one morphology)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-2)
    pol.change_morphology(graphs[1])
    pol(obs[5:12, :41 * 7]).square().sum().backward()
    opt.step()
    a1 = check("adam")
    assert float((a1 - a0).abs().max()) > 1e-4
    # load_state_dict from another network
    other = _policy(seed=12).to("cuda:0")
    pol.load_state_dict(other.state_dict())
    a2 = check("load_state_dict")
    assert float((a2 - a1).abs().max()) > 1e-4
    # an in-place soft update (reference common/functional.py:7-10)
    src = _policy(seed=13).to("cuda:0")
    with torch.no_grad():
        for p, q in zip(pol.parameters(), src.parameters()):
            p.data.copy_(0.5 * p.data + 0.5 * q.data)
    a3 = check("soft update")
    assert float((a3 - a2).abs().max()) > 1e-4
    # .to() round trip: the storage moves, the next forward re-binds by itself
    pol.cpu()
    pol.to("cuda:0")
    a4 = check(".to() round trip")
    assert torch.equal(a4, a3)


def test_graph_capture_replays_the_eager_result_bit_for_bit():
    import torch
    from sgrl_amd.swat_hip import HipSwatActor
    names = WALKERS
    counts = [64] * len(names)
    graphs = _graphs(names)
    pol = _policy(seed=21).to("cuda:0")
    actor = HipSwatActor(pol)
    actor.configure(graphs, counts)
    obs = _obs(counts, graphs, seed=6)
    eager = actor.forward_batch(obs).clone()
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        actor.forward_batch(obs, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        actor.forward_batch(obs, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # the captured forward reads the parameters too: a change shows up in the next replay
    with torch.no_grad():
        pol.actor.decoder.bias.add_(0.25)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, actor.forward_batch(obs))
    assert not torch.equal(out, eager)


def test_device_trainer_trains_swat():
    import torch
    from sgrl_amd.swat_policy import StructurePolicy
    from sgrl_amd.swat_hip import HipSwatActor
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_walker_2_right_leg_left_knee", "3d_hopper_3_shin", "3d_humanoid_9_full"]
    args = default_train_args(actor_type="swat", critic_type="swat", max_episode_steps=40)
    tr = DeviceTrainer(names, 32, args=args, seed=3, device="cuda:0", max_buffer_size=4096, batch_size=32)
    assert isinstance(tr.agent.actor, StructurePolicy) and isinstance(tr.ro.actor, HipSwatActor)
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
    ref = _reference(tr.agent.actor, tr.graph_dicts, env.counts, obs, a1.shape[1])
    err = float((a1.double() - ref).abs().max())
    assert err < 2e-5, err
