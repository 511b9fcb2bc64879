"""The fused HIP forward of the monolithic MLP actor (csrc/mlp_actor.hip through sgrl_amd/mlp_hip.py) on the MI355X: against the
reference's own numbers (tests/golden/mlp_forward.npz), against a float64 copy of the module with full-rank random weights at every
path of the kernel (ragged row tiles, widths that are no multiple of a tile, 1 .. 4 hidden layers, the 2- and 4-chunk variants),
padding slots, live / held weights, one launch and graph capture, the device trainer end to end, argument errors.

Bar of the float64 comparisons: max |HIP - float64| < 2e-5 with outputs bounded by max_action = 1 (the bar of the SWAT and SMP
forwards, tests/test_swat_hip_gpu.py).  Measured on the MI355X: 3.8e-7 at the worst case (walker_7, hidden [1, 7]; [256, 256]: 1.2e-7 .. 2.4e-7)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mlp_restate import apply_seeded_, forward64, module_linears

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
MORPHS = {"hopper_3": "3d_hopper_3_shin", "walker_7": "3d_walker_7_full", "cheetah_14": "3d_cheetah_14_full"}
TILE = 32
COUNTS = (1, TILE - 1, TILE + 1, 2 * TILE + 2)      # one ragged tile, both sides of a tile edge, two and a bit tiles


def _graph(name):
    from sgrl_amd import graph as G, mjcf
    return G.getGraphDict(mjcf.load_asset(name).parents, TRAV, [], device=torch.device("cuda:0"))


def _policy(L, hidden=(256, 256), seed=5):
    from sgrl_amd.mlp_policy import MlpPolicy
    from sgrl_amd.td3 import default_train_args
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L)
    args.agent.policy_network = {"hidden_dims": list(hidden)}
    pol = MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, args).eval()
    return apply_seeded_(pol, seed).to("cuda:0")


def _obs(n, width, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, width), generator=g, dtype=torch.float32).cuda()


@pytest.mark.parametrize("name", ["3d_hopper_3_shin", "3d_walker_7_full"])
def test_forward_matches_the_reference_fixture(golden_dir, name):
    from sgrl_amd.mlp_hip import HipMlpActor
    z = np.load(os.path.join(golden_dir, "mlp_forward.npz"))
    obs, want = z[name + "/obs"], z[name + "/action"]
    pol = _policy(obs.shape[1] // 41, seed=int(z["seed"]))
    actor = HipMlpActor(pol)
    actor.configure([_graph(name)], [obs.shape[0]])
    got = actor.forward_batch(torch.from_numpy(obs).cuda()).cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=0)


NETS = [(m, h) for m in ("hopper_3", "walker_7", "cheetah_14") for h in ((256, 256), (40, 72))]
NETS += [("walker_7", (256,)), ("walker_7", (64, 48, 80, 33)), ("walker_7", (1, 7)), ("hopper_3", (300, 512)), ("cheetah_14", (1024, 1000))]


@pytest.mark.parametrize("morph,hidden", NETS, ids=["%s-%s" % (m, "x".join(str(x) for x in h)) for m, h in NETS])
def test_forward_against_float64(morph, hidden):
    from sgrl_amd.mlp_hip import HipMlpActor
    g = _graph(MORPHS[morph])
    L = len(g["parents"])
    pol = _policy(L, hidden)
    actor = HipMlpActor(pol)
    lin = module_linears(pol.actor)
    worst, biggest = 0.0, 0.0
    for n in COUNTS:
        obs = _obs(n, 41 * L, seed=n)
        actor.configure([g], [n])
        got = actor.forward_batch(obs).double().cpu().numpy()
        ref = forward64(lin, obs.double().cpu().numpy(), max_action=1.0)
        assert got.shape == ref.shape == (n, 3 * L)
        worst = max(worst, float(np.abs(got - ref).max()))
        biggest = max(biggest, float(np.abs(ref).max()))
    print("max |HIP - float64| = %.3e (largest |action| %.3f)" % (worst, biggest))
    assert worst < 2e-5, worst
    assert biggest > 1e-3                                   # a non-trivial output


def test_padding_slots_are_exact_zeros_and_nothing_else_is_touched():
    from sgrl_amd.mlp_hip import HipMlpActor
    g = _graph(MORPHS["walker_7"])
    pol = _policy(7)
    actor = HipMlpActor(pol)
    n, act_ld, guard, sentinel = 37, 21 + 70, 64, 12345.0          # more padding than a wave's 64 lanes cover in one pass
    actor.configure([g], [n])
    obs_wide = torch.full((n, 287 + 13), float("nan"), device="cuda:0")      # a leading dimension beyond 41 L: never read
    obs_wide[:, :287] = _obs(n, 287)
    flat = torch.full((guard + n * act_ld + guard,), sentinel, device="cuda:0")
    out = flat[guard:guard + n * act_ld].view(n, act_ld)
    actor.forward_batch(obs_wide, out=out, act_ld=act_ld)
    ref = forward64(module_linears(pol.actor), obs_wide[:, :287].double().cpu().numpy(), max_action=1.0)
    assert float(np.abs(out[:, :21].double().cpu().numpy() - ref).max()) < 2e-5
    assert torch.equal(out[:, 21:], torch.zeros_like(out[:, 21:]))
    assert bool((flat[:guard] == sentinel).all()) and bool((flat[guard + n * act_ld:] == sentinel).all())


def test_live_weights_hold_and_weights_changed():
    from sgrl_amd.mlp_hip import HipMlpActor
    g = _graph(MORPHS["hopper_3"])
    pol = _policy(3)
    actor = HipMlpActor(pol)
    n = 40
    actor.configure([g], [n])
    obs = _obs(n, 123)
    f64 = lambda: forward64(module_linears(pol.actor), obs.double().cpu().numpy(), max_action=1.0)

    def step():                                             # an in-place optimizer-style update
        with torch.no_grad():
            for i, p in enumerate(pol.parameters()):
                p.add_(0.05 * torch.sin(torch.arange(p.numel(), device=p.device, dtype=torch.float32) + i).view_as(p))

    a0 = actor.forward_batch(obs).clone()
    ref0 = f64()
    step()
    ref1 = f64()
    assert np.abs(ref1 - ref0).max() > 1e-2
    a1 = actor.forward_batch(obs).clone()                   # not holding: follows the live parameters
    assert np.abs(a1.double().cpu().numpy() - ref1).max() < 2e-5
    actor.hold_weights(True)
    a1h = actor.forward_batch(obs).clone()                  # the first forward of a hold packs
    assert torch.equal(a1h, a1)
    step()
    ref2 = f64()
    assert np.abs(ref2 - ref1).max() > 1e-2
    a_held = actor.forward_batch(obs).clone()               # holding, nobody said the weights changed: the packed copy
    assert torch.equal(a_held, a1)
    actor.weights_changed()
    a2 = actor.forward_batch(obs).clone()
    assert np.abs(a2.double().cpu().numpy() - ref2).max() < 2e-5
    actor.hold_weights(False)
    step()
    assert np.abs(actor.forward_batch(obs).double().cpu().numpy() - f64()).max() < 2e-5
    assert np.abs(a0.double().cpu().numpy() - ref0).max() < 2e-5


def test_rollout_holds_and_repacks():
    """The rollout's own protocol: hold_weights=True packs once per round, weights_changed() after the updates."""
    from sgrl_amd.rollout import Rollout
    pol = _policy(3)
    ro = Rollout(["3d_hopper_3_shin"], 5, policy=pol, seed=1, device="cuda:0", hold_weights=True)
    ro.reset()
    obs = ro.env.obs.clone()
    a0 = ro.policy_forward(obs).clone()
    assert a0.shape == (5, ro.env.action_max_len)
    ref0 = forward64(module_linears(pol.actor), obs[:, :123].double().cpu().numpy(), max_action=1.0)
    assert np.abs(a0[:, :9].double().cpu().numpy() - ref0).max() < 2e-5
    with torch.no_grad():
        pol.actor.networks[4].bias.add_(0.3)                # PyTorch sees it (version counter): the rollout repacks by itself
    a1 = ro.policy_forward(obs).clone()
    ref1 = forward64(module_linears(pol.actor), obs[:, :123].double().cpu().numpy(), max_action=1.0)
    assert np.abs(a1[:, :9].double().cpu().numpy() - ref1).max() < 2e-5 and np.abs(ref1 - ref0).max() > 1e-2


def test_one_launch_and_graph_capture():
    from sgrl_amd.mlp_hip import HipMlpActor
    g = _graph(MORPHS["walker_7"])
    pol = _policy(7)
    actor = HipMlpActor(pol)
    assert actor.launches() == 1 and int(actor.L.sgrl_mlp_forward_launches()) == 1 and actor.pack_launches() == 1
    n = 70
    actor.configure([g], [n])
    obs = _obs(n, 287, seed=1)
    out = torch.zeros((n, 21), device="cuda:0")
    actor.forward_batch(obs, out=out)                       # eager first
    torch.cuda.synchronize()
    lin = module_linears(pol.actor)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):             # single stream, no parallel branches
            actor.forward_batch(obs, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for seed in (2, 3):
        obs.copy_(_obs(n, 287, seed=seed))
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        ref = forward64(lin, obs.double().cpu().numpy(), max_action=1.0)
        assert np.abs(out.double().cpu().numpy() - ref).max() < 2e-5


@pytest.mark.parametrize("on_device", [True, False], ids=["device_noise_and_sampler", "torch_noise_and_sampler"])
def test_device_trainer_trains_an_mlp_agent(on_device):
    from sgrl_amd.mlp_hip import HipMlpActor
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    args = default_train_args(actor_type="mlp", critic_type="mlp")
    tr = DeviceTrainer(["3d_hopper_3_shin"], 4, args=args, seed=2, device="cuda:0", max_buffer_size=4096, batch_size=64,
                       device_noise=on_device, device_sampler=on_device)
    assert isinstance(tr.ro.actor, HipMlpActor) and tr.agent.actor.mlp_num_limbs == 3
    before = [p.detach().clone() for p in tr.agent.actor.parameters()]
    tr.warmup(8)
    s = tr.train_round(max_steps=40, max_iters=2)
    assert s["per_morph_iter"] == 2
    losses = tr.last_losses["3d_hopper_3_shin"]
    assert all(np.isfinite(float(v)) for v in losses.values())
    assert any(not torch.equal(p, q) for p, q in zip(tr.agent.actor.parameters(), before))
    ev = tr.evaluate(num_eval_trajectories=2, max_trajectory_length=20)
    # (20 steps rarely end a hopper's episode: the means are NaN when no trajectory completed, as in the reference)
    assert set(ev) >= {"performance/eval_return", "performance/eval_length", "performance/eval_return/3d_hopper_3_shin"}
    ev_ro, evaluator = tr.eval_rollouts[("3d_hopper_3_shin",)][1:]
    assert isinstance(ev_ro.actor, HipMlpActor) and 1 <= evaluator.last_steps <= 20
    assert bool(torch.isfinite(evaluator.ep_reward).all()) and int(evaluator.ep_steps.max()) >= 1
    with pytest.raises(ValueError, match="3d_walker_7_full"):          # zero-shot names with another limb count
        tr.evaluate(num_eval_trajectories=2, max_trajectory_length=20, env_names=["3d_walker_7_full"])


def test_argument_errors_come_before_any_launch():
    """Only arguments the library rejects on the host."""
    from sgrl_amd import _lib
    from sgrl_amd.mlp_hip import HipMlpActor, _bind
    L = _lib.lib()
    _bind(L)
    ERR_ARG = -1
    vp = ctypes.c_void_p
    g = _graph(MORPHS["walker_7"])
    pol = _policy(7)
    actor = HipMlpActor(pol)
    actor.configure([g], [4])
    obs, out = _obs(4, 287), torch.zeros((4, 21), device="cuda:0")
    stream = vp(torch.cuda.current_stream().cuda_stream)
    fwd = lambda h, o, old, a, ald: L.sgrl_mlp_forward(h, o, old, a, ald, ctypes.c_float(1.0), stream)
    assert fwd(None, vp(obs.data_ptr()), 287, vp(out.data_ptr()), 21) == ERR_ARG
    assert fwd(actor.h, None, 287, vp(out.data_ptr()), 21) == ERR_ARG
    assert fwd(actor.h, vp(obs.data_ptr()), 287, None, 21) == ERR_ARG
    assert fwd(actor.h, vp(obs.data_ptr()), 286, vp(out.data_ptr()), 21) == ERR_ARG        # below 41 L
    assert fwd(actor.h, vp(obs.data_ptr()), 287, vp(out.data_ptr()), 20) == ERR_ARG        # below 3 L
    assert b"rows too narrow" in L.sgrl_mlp_last_error()
    # widths and depths the kernel is not built for, on a fresh handle
    h = vp()
    assert L.sgrl_mlp_create(ctypes.byref(h)) == 0
    try:
        assert fwd(h, vp(obs.data_ptr()), 287, vp(out.data_ptr()), 21) == ERR_ARG          # nothing bound yet
        w = torch.zeros(1025 * 1025, device="cuda:0")
        for dims in ([287, 1025, 21], [287, 21], [287, 8, 8, 8, 8, 8, 21]):
            d = np.asarray(dims, dtype=np.int32)
            ptrs = (vp * (2 * (len(dims) - 1)))(*([w.data_ptr()] * (2 * (len(dims) - 1))))
            assert L.sgrl_mlp_set_params(h, ctypes.cast(ptrs, vp), len(ptrs), vp(d.ctypes.data), len(d)) == ERR_ARG, dims
        d = np.asarray([287, 256, 256, 21], dtype=np.int32)
        ptrs = (vp * 6)(*([w.data_ptr()] * 5 + [0]))
        assert L.sgrl_mlp_set_params(h, ctypes.cast(ptrs, vp), 6, vp(d.ctypes.data), 4) == ERR_ARG          # a null parameter
        assert L.sgrl_mlp_set_params(h, None, 6, vp(d.ctypes.data), 4) == ERR_ARG
        ptrs = (vp * 6)(*([w.data_ptr()] * 6))
        assert L.sgrl_mlp_set_params(h, ctypes.cast(ptrs, vp), 5, vp(d.ctypes.data), 4) == ERR_ARG          # wrong count
        assert L.sgrl_mlp_set_params(h, ctypes.cast(ptrs, vp), 6, vp(d.ctypes.data), 4) == 0
        la, ca = np.asarray([3], dtype=np.int32), np.asarray([4], dtype=np.int32)
        assert L.sgrl_mlp_configure(h, 1, vp(la.ctypes.data), vp(ca.ctypes.data), 41, 3) == ERR_ARG         # 3 limbs on a 7-limb network
        assert L.sgrl_mlp_configure(h, 1, None, vp(ca.ctypes.data), 41, 3) == ERR_ARG
    finally:
        L.sgrl_mlp_destroy(h)
    with pytest.raises(ValueError):
        actor.configure([_graph(MORPHS["hopper_3"])], [4])
    # the handle still works after all the refusals
    got = actor.forward_batch(obs).double().cpu().numpy()
    assert np.abs(got - forward64(module_linears(pol.actor), obs.double().cpu().numpy(), max_action=1.0)).max() < 2e-5
