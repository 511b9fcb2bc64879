"""The gradient half of the MLP agent's TD3 update on HIP (csrc/mlp_train.hip over include/sgrl_mlp.h, mlp_hip.HipMlpGrads,
td3.Agent(mlp_hip_grads=True)) on the MI355X.

1  per-tensor gradients and losses of both steps against float64 autograd through double copies of the same modules, per tensor
   ||g - g64|| <= 1e-3 ||g64|| + 10 ||g_torch32 - g64|| in the 2-norm and the max-norm (the formula of test_td3_update_init.py /
   test_mlp_policy.py; g_torch32 = float32 PyTorch autograd on the same inputs), losses 1e-4 relative (+ 2e-6 for the actor's)
2  tests/golden/td3_update_mlp.npz (the executed reference's Agent.update) through a CUDA agent on the new path, the assertions
   and tolerances of test_mlp_policy.test_update_matches_the_reference_on_cpu
3  repeatability: bit-identical gradients and losses from the same state; the same action bits from the forward, the gradient half
   and the target chain (one panel product under all three)
4  .grad handling: None, replaced, garbage, the critic's after an actor step
5  argument errors before any launch
6  DeviceTrainer with the path on; twenty updates against the PyTorch gradient half
7  launch counts

Measured on the MI355X (the printed lines of a run): per tensor, |HIP - float64| is beside the float32 PyTorch autograd's own
|torch32 - float64| in both norms (e.g. L3 [256, 256] B = 1, critic1 layer 0 weight: 4.21e-07 against 4.23e-07 at |g64| = 2.23); the
worst error / bar over the four row counts is 4.6e-4 ... 1.1e-3 for the [256, 256], [40, 72] and [64, 48, 80, 33] nets of 3 and 7
limbs, 2.6e-3 ... 8.1e-3 for [1, 7], 3.2e-3 for L14 [64, 48, 80, 33] and 0.10 for L14 [512, 500]; losses within 1.9e-7 relative.  At
PyTorch's default initialisation (actor gradients 1e-4 ... 3e-2 in the 2-norm at these widths) the same picture: errors 2e-10 ...
2e-7, each beside torch32's.  The reference replay: critic loss 2.52044296 / 1.08880043 against 2.52044344 / 1.08880043, actor loss
-0.0656907186 against -0.0656907633, gradient norms within 1.1e-4 of their tolerance.  Twenty updates against the PyTorch gradient
half: per-tensor differences 0 ... 3.3e-7 under tolerances of 7e-7 ... 1.3e-3.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mlp_restate import apply_seeded_

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
MORPHS = {3: "3d_hopper_3_shin", 7: "3d_walker_7_full", 14: "3d_cheetah_14_full"}
ROWS = (1, 31, 33, 66)          # one ragged tile, a tile edge from both sides, three tiles (the cross-tile reductions)
HIDDEN = [(256, 256), (40, 72), (1, 7), (64, 48, 80, 33), (512, 500)]      # the last: the widest the path serves
NETS = [(L, h) for L in (3, 7, 14) for h in HIDDEN]
NET_IDS = ["L%d-%s" % (L, "x".join(str(x) for x in h)) for L, h in NETS]
NS = 8


def _graph(L, device="cuda:0"):
    from sgrl_amd import graph as G, mjcf
    return G.getGraphDict(mjcf.load_asset(MORPHS[L]).parents, TRAV, [], device=torch.device(device))


def _args(L, hidden=(256, 256), **over):
    from sgrl_amd.td3 import default_train_args
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L, **over)
    args.agent.policy_network = {"hidden_dims": list(hidden)}
    args.agent.q_network = {"hidden_dims": list(hidden)}
    return args


def _pair(L, hidden=(256, 256), seed=5, seeded=True):
    from sgrl_amd.mlp_policy import MlpCritic, MlpPolicy
    torch.manual_seed(seed)
    pol = MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, _args(L, hidden))
    crit = MlpCritic(41, 3, 32, 100, 3, True, False, False, _args(L, hidden))
    if seeded:
        apply_seeded_(pol, seed)
        apply_seeded_(crit, seed + 1)
    return pol.to("cuda:0").train(), crit.to("cuda:0").train()


def _batch(L, n, seed):
    g = torch.Generator().manual_seed(2000 + seed)
    b = {"obs": torch.randn((n, 41 * L), generator=g), "action": torch.rand((n, 3 * L), generator=g) * 2 - 1,
         "target": torch.randn((n, 1), generator=g)}
    return {k: v.cuda() for k, v in b.items()}


def _critic_loss(crit, b):
    q1, q2 = crit(b["obs"], b["action"])
    return F.mse_loss(q1, b["target"]) + F.mse_loss(q2, b["target"])


def _actor_loss(pol, crit, b):
    return -crit.Q1(b["obs"], pol(b["obs"])).mean()


def _autograd(mods, wrt, loss_fn, b, dtype):
    """Gradients of loss_fn over copies of the modules in dtype -> (loss, [per-parameter float64 numpy])."""
    mods = [copy.deepcopy(m).to(dtype) for m in mods]
    for m in mods:
        m._mlp_hip = None
        m.zero_grad()
    bb = {k: v.to(dtype) for k, v in b.items()}
    loss = loss_fn(*mods, bb)
    loss.backward()
    return float(loss.detach()), [p.grad.double().cpu().numpy() for p in mods[wrt].parameters()]


def _check_grads(what, module, g64, g32):
    """The bar, per tensor, in the 2-norm and the max-norm; returns the worst ratio error / bar."""
    worst = 0.0
    for (name, p), r64, r32 in zip(module.named_parameters(), g64, g32):
        got = p.grad.double().cpu().numpy()
        assert got.shape == r64.shape
        for norm, nm in ((lambda x: float(np.sqrt((x * x).sum())), "2"), (lambda x: float(np.abs(x).max()), "max")):
            err, e32, ref = norm(got - r64), norm(r32 - r64), norm(r64)
            bar = 1e-3 * ref + 10.0 * e32
            print("%s %s %s-norm: |g64| %.3g  |HIP - g64| %.3g  |torch32 - g64| %.3g  bar %.3g" % (what, name, nm, ref, err, e32, bar))
            assert err <= bar, (what, name, nm, err, bar)
            assert np.isfinite(got).all()
            if bar > 0:
                worst = max(worst, err / bar)
    return worst


def _both_steps(what, pol, crit, grads, b):
    l64, g64 = _autograd([crit], 0, _critic_loss, b, torch.float64)
    _, g32 = _autograd([crit], 0, _critic_loss, b, torch.float32)
    loss = float(grads.critic_step(b["obs"], b["action"], b["target"]))
    print("%s critic loss: HIP %.9g  float64 %.9g  relative %.3g" % (what, loss, l64, abs(loss - l64) / abs(l64)))
    assert abs(loss - l64) < 1e-4 * abs(l64)
    w = _check_grads(what + " critic", crit, g64, g32)
    l64, g64 = _autograd([pol, crit], 0, _actor_loss, b, torch.float64)
    _, g32 = _autograd([pol, crit], 0, _actor_loss, b, torch.float32)
    act = torch.full((b["obs"].shape[0], grads.actor.dims[-1] + 2), 7.0, device="cuda:0")
    loss = float(grads.actor_step(b["obs"], action_out=act))
    print("%s actor loss: HIP %.9g  float64 %.9g  difference %.3g" % (what, loss, l64, abs(loss - l64)))
    assert abs(loss - l64) < 1e-4 * abs(l64) + 2e-6
    with torch.no_grad():
        a32 = pol(b["obs"])
    assert float((act[:, :-2] - a32).abs().max()) < 2e-5 and bool((act[:, -2:] == 7).all())
    return max(w, _check_grads(what + " actor", pol, g64, g32))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hidden", NETS, ids=NET_IDS)
def test_gradients_against_float64(L, hidden):
    from sgrl_amd.mlp_hip import HipMlpGrads
    pol, crit = _pair(L, hidden)
    grads = HipMlpGrads(pol, crit)
    worst = 0.0
    for n in ROWS:
        worst = max(worst, _both_steps("L%d %s B%d" % (L, hidden, n), pol, crit, grads, _batch(L, n, seed=n)))
    print("L%d %s: worst error / bar %.3g" % (L, hidden, worst))


def test_gradients_at_the_default_initialisation():
    """PyTorch's default initialisation: the actor's gradients are ~1e-11 and less, an absolute bar would pass anything."""
    from sgrl_amd.mlp_hip import HipMlpGrads
    pol, crit = _pair(7, seed=11, seeded=False)
    grads = HipMlpGrads(pol, crit)
    for n in (33, 66):
        _both_steps("default init B%d" % n, pol, crit, grads, _batch(7, n, seed=90 + n))


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def _sample_idx(numel):
    return np.unique(np.linspace(0, numel - 1, NS).astype(np.int64)) if numel >= NS else np.arange(numel)


def _grad_record(module):
    norms, samples = [], []
    for _, p in module.named_parameters():
        g = p.grad.detach().double().reshape(-1).cpu()
        norms.append(float(g.norm()))
        s = g[torch.from_numpy(_sample_idx(g.numel()))].numpy()
        samples.append(np.pad(s, (0, NS - s.size), constant_values=np.nan))
    return np.array(norms), np.stack(samples)


def test_hip_gradient_path_replays_the_reference_update(golden_dir):
    from sgrl_amd import td3
    from sgrl_amd.mlp_hip import HipMlpGrads
    from sgrl_amd.td3 import Agent, default_train_args
    z = np.load(os.path.join(golden_dir, "td3_update_mlp.npz"))
    hyper = dict(zip([str(k) for k in z["hyper_keys"]], z["hyper_vals"]))
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=7, lr=hyper["lr"], policy_noise=hyper["policy_noise"],
                              noise_clip=hyper["noise_clip"], discount=hyper["discount"], policy_freq=int(hyper["policy_freq"]),
                              grad_clipping_value=hyper["grad_clipping_value"], max_action=hyper["max_action"])
    args.agent.target_smoothing_tau, args.agent.reward_scale = hyper["target_smoothing_tau"], hyper["reward_scale"]
    agent = Agent(args, device=torch.device("cuda:0"), mlp_hip_grads=True)
    assert agent.use_mlp_hip_grads
    assert [n for n, _ in agent.actor.named_parameters()] == [str(s) for s in z["actor_param_names"]]
    assert [n for n, _ in agent.critic.named_parameters()] == [str(s) for s in z["critic_param_names"]]
    apply_seeded_(agent.actor, int(z["seed"]))
    apply_seeded_(agent.critic, int(z["seed"]))
    with torch.no_grad():
        for tgt, src in ((agent.actor_target, agent.actor), (agent.critic_target, agent.critic)):
            for tp, sp in zip(tgt.parameters(), src.parameters()):
                tp.copy_(0.97 * sp)
    agent.change_morphology(_graph(7))
    agent.models2train()
    grabbed = {}
    real = td3.clip_and_step

    def spy(opt, max_norm):
        which = "critic" if opt is agent.critic_optimizer else "actor"
        grabbed[which] = _grad_record(getattr(agent, which))
        return real(opt, max_norm)

    td3.clip_and_step = spy
    try:
        for it in range(2):
            tag = "it%d/" % it
            batch = {k: torch.from_numpy(z[tag + k]).cuda() for k in ("obs", "action", "next_obs", "reward", "done")}
            before = {nm: [p.detach().double().clone() for p in getattr(agent, nm).parameters()] for nm in ("actor", "critic")}
            grabbed.clear()
            loss = agent.update(batch, it, noise=torch.from_numpy(z[tag + "noise"]).cuda())
            ref_cl = float(z[tag + "critic_loss"])
            print("reference update %d: critic_loss %.9g  reference %.9g" % (it, float(loss["loss/critic_loss"]), ref_cl))
            assert abs(float(loss["loss/critic_loss"]) - ref_cl) < 1e-4 * abs(ref_cl), it
            ref_al = float(z[tag + "actor_loss"])
            assert np.isnan(ref_al) == ("loss/actor_loss" not in loss)
            if not np.isnan(ref_al):
                print("reference update %d: actor_loss %.9g  reference %.9g" % (it, float(loss["loss/actor_loss"]), ref_al))
                assert abs(float(loss["loss/actor_loss"]) - ref_al) < 1e-4 * abs(ref_al) + 2e-6
            assert abs(loss["misc/train_reward_mean"] - float(z[tag + "train_reward_mean"])) < 1e-6
            for nm in ("critic", "actor"):
                k = tag + nm + "_grad_norms"
                if k not in z.files:
                    assert nm not in grabbed, "policy_freq: actor stepped at the wrong iteration"
                else:
                    n32, n64 = z[k], z[k + "_f64"]
                    s32, s64 = z[tag + nm + "_grad_samples"], z[tag + nm + "_grad_samples_f64"]
                    got_n, got_s = grabbed[nm]
                    tol_n = 1e-3 * n64 + 10.0 * np.abs(n32 - n64)
                    tol_s = 1e-3 * n64 + 10.0 * np.nanmax(np.abs(s32 - s64), axis=1)
                    names = z[nm + "_param_names"]
                    print("reference update %d %s: |norm - f64| / tol %s" % (it, nm, np.array2string(np.abs(got_n - n64) / tol_n, precision=3)))
                    assert (np.abs(got_n - n64) <= tol_n).all(), (it, nm, [str(names[i]) for i in np.nonzero(np.abs(got_n - n64) > tol_n)[0]])
                    assert (np.nanmax(np.abs(got_s - s64), axis=1) <= tol_s).all(), (it, nm)
                st = np.array([float((p.detach().double() - q).norm()) for p, q in zip(getattr(agent, nm).parameters(), before[nm])])
                st64 = z[tag + nm + "_step_norms_f64"]
                ulp_floor = np.sqrt(z[nm + "_numel"]) * np.array([float(q.abs().max()) for q in before[nm]]) * 1.2e-7
                assert (np.abs(st - st64) <= 2e-3 * st64 + ulp_floor).all(), (it, nm)
                if k not in z.files:
                    assert st.max() == 0.0
            for nm in ("actor", "critic", "actor_target", "critic_target"):
                got = np.array([float(p.detach().double().sum()) for p in getattr(agent, nm).parameters()])
                ref = z[tag + nm + "_param_sums"]
                numel = np.array([p.numel() for p in getattr(agent, nm).parameters()])
                assert (np.abs(got - ref) <= 2e-3 * hyper["lr"] * numel + 1e-6 * np.abs(ref) + 1e-7).all(), (it, nm)
    finally:
        td3.clip_and_step = real
    assert isinstance(agent._mlp_grads, HipMlpGrads) and agent.critic._mlp_hip is None and agent.actor._mlp_hip is None


# ---- 3, 4 ------------------------------------------------------------------------------------------------------------------
def _grad_bits(module):
    return [p.grad.clone() for p in module.parameters()]


def test_repeatable_bit_for_bit():
    from sgrl_amd.mlp_hip import HipMlpGrads
    pol, crit = _pair(7, (300, 64), seed=21)
    grads = HipMlpGrads(pol, crit)
    b = _batch(7, 66, seed=3)
    runs = []
    for _ in range(2):
        for m in (pol, crit):
            for p in m.parameters():
                if p.grad is not None:
                    p.grad.normal_()                 # whatever was there does not matter
        lc = grads.critic_step(b["obs"], b["action"], b["target"]).clone()
        gc = _grad_bits(crit)
        la = grads.actor_step(b["obs"]).clone()
        runs.append((lc, la, gc, _grad_bits(pol)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in (2, 3):
        for x, y in zip(runs[0][k], runs[1][k]):
            assert torch.equal(x, y)
    assert all(float(g.abs().max()) > 0 for g in runs[0][2][:2])


@pytest.mark.parametrize("hidden", [(256, 256), (40, 72), (512, 500)], ids=lambda h: "x".join(str(x) for x in h))
@pytest.mark.parametrize("L", (3, 7))
def test_the_three_actor_walks_give_the_same_bits(L, hidden):
    """The forward, the gradient half and the target chain walk the actor with one panel product: the same action bits from all
    three (the chain with zero noise; max_action is 1, so its clamp changes nothing).  The pairing of k values inside a matrix
    instruction depends on the panel depth, so the three plans must have chosen the same `bk` (16 at these widths) first."""
    from sgrl_amd import mlp_hip
    pol, crit = _pair(L, hidden, seed=41)
    n = 33
    b = _batch(L, n, seed=33)
    grads = mlp_hip.HipMlpGrads(pol, crit)
    targets = mlp_hip.HipMlpTargets(pol, crit)
    bks = (mlp_hip.plan(targets.actor.dims)["bk"], targets.plan()["bk"], grads.plan(n)["bk"])
    assert bks == (16, 16, 16), bks
    g = _graph(L)
    targets.configure([g], [n])
    forward = targets.actor.forward_batch(b["obs"])
    from_grads = torch.full((n, 3 * L), 7.0, device="cuda:0")
    grads.actor_step(b["obs"], action_out=from_grads)
    from_chain = torch.full((n, 3 * L), 7.0, device="cuda:0")
    zeros = torch.zeros((n, 3 * L), device="cuda:0")
    targets.target_q(b["obs"], zeros, b["target"], torch.zeros((n, 1), device="cuda:0"), g, 0.5, 0.99, action_out=from_chain)
    assert float(forward.abs().max()) > 0
    assert torch.equal(forward, from_grads) and torch.equal(forward, from_chain)


def test_grad_tensors_none_replaced_garbage_and_stale():
    from sgrl_amd import td3
    from sgrl_amd.mlp_hip import HipMlpGrads
    pol, crit = _pair(3, (40, 72), seed=31)
    grads = HipMlpGrads(pol, crit)
    b = _batch(3, 33, seed=4)
    assert all(p.grad is None for m in (pol, crit) for p in m.parameters())
    # None: created, persistent
    grads.critic_step(b["obs"], b["action"], b["target"])
    grads.actor_step(b["obs"])
    ref_c, ref_a = _grad_bits(crit), _grad_bits(pol)
    ptrs = [p.grad.data_ptr() for m in (pol, crit) for p in m.parameters()]
    assert all(p.grad is not None and p.grad.is_contiguous() and p.grad.dtype == torch.float32 for m in (pol, crit) for p in m.parameters())
    # garbage: overwritten, not accumulated; the same tensors
    for m in (pol, crit):
        for p in m.parameters():
            p.grad.fill_(1e6)
    grads.critic_step(b["obs"], b["action"], b["target"])
    grads.actor_step(b["obs"])
    assert ptrs == [p.grad.data_ptr() for m in (pol, crit) for p in m.parameters()]
    for x, y in zip(_grad_bits(crit) + _grad_bits(pol), ref_c + ref_a):
        assert torch.equal(x, y)
    # replaced / set to None by the caller: bound again
    first = next(crit.parameters())
    first.grad = torch.full_like(first, 3.0)
    list(crit.parameters())[3].grad = None
    list(pol.parameters())[0].grad = torch.full_like(list(pol.parameters())[0], 3.0)
    kept = first.grad
    grads.critic_step(b["obs"], b["action"], b["target"])
    grads.actor_step(b["obs"])
    assert first.grad is kept
    for x, y in zip(_grad_bits(crit) + _grad_bits(pol), ref_c + ref_a):
        assert torch.equal(x, y)
    # after an actor step the critic's .grad is what the critic step and the clipping left
    opt = torch.optim.Adam(crit.parameters(), lr=0.0)
    grads.critic_step(b["obs"], b["action"], b["target"])
    td3.clip_and_step(opt, 0.1)
    left = _grad_bits(crit)
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in left)))
    assert total <= 0.1 * (1 + 1e-5) and any(not torch.equal(x, y) for x, y in zip(left, ref_c))      # the clipping bit
    grads.actor_step(b["obs"])
    for x, y in zip(_grad_bits(crit), left):
        assert torch.equal(x, y)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_returned_before_any_launch():
    from sgrl_amd import _lib
    from sgrl_amd.mlp_hip import HipMlpActor, HipMlpCritic, HipMlpGrads
    L7, n = 7, 5
    pol, crit = _pair(L7, seed=7)
    gr = HipMlpGrads(pol, crit)
    b = _batch(L7, n, seed=5)
    gr.critic_step(b["obs"], b["action"], b["target"])
    gr.actor_step(b["obs"])
    torch.cuda.synchronize()
    for m in (pol, crit):
        for p in m.parameters():
            p.grad.fill_(7.0)
    actor, c, L = gr.actor, gr.critic, gr.L
    loss = torch.full((1,), 7.0, device="cuda:0")
    aout = torch.full((n, 21), 7.0, device="cuda:0")
    tq = b["target"].reshape(-1).contiguous()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(None)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = lambda: L.sgrl_mlp_last_error()
    cs = lambda h, o=vp(b["obs"]), old=287, a=vp(b["action"]), ald=21, t=vp(tq), lo=vp(loss): L.sgrl_mlp_critic_step_grads(h, o, old, a, ald, t, lo, st)
    as_ = lambda a, cc, o=vp(b["obs"]), old=287, lo=vp(loss), ao=vp(aout), ald=21: \
        L.sgrl_mlp_actor_step_grads(a, cc, o, old, ctypes.c_float(1.0), lo, ao, ald, st)
    ERR = -1
    # handles of the wrong kind
    assert cs(actor.h) == ERR and b"not bound as a critic" in err()
    assert as_(c.h, c.h) == ERR and b"not bound as an actor" in err()
    assert as_(actor.h, actor.h) == ERR and b"not bound as a critic" in err()
    # rows too narrow
    assert cs(c.h, old=286) == ERR and b"narrow" in err()
    assert cs(c.h, ald=20) == ERR and b"narrow" in err()
    assert as_(actor.h, c.h, old=286) == ERR and b"narrow" in err()
    assert as_(actor.h, c.h, ald=20) == ERR and b"narrow" in err()
    # null pointers (a null action_out is allowed)
    assert cs(null) == ERR and b"null" in err()
    for kw in ("o", "a", "t", "lo"):
        assert cs(c.h, **{kw: null}) == ERR and b"null" in err(), kw
    assert as_(null, c.h) == ERR and as_(actor.h, null) == ERR and b"null" in err()
    for kw in ("o", "lo"):
        assert as_(actor.h, c.h, **{kw: null}) == ERR and b"null" in err(), kw
    # gradients not bound, wrong count, null address; not configured; different batch structures
    other_c, other_a = HipMlpCritic(crit), HipMlpActor(pol)
    g7 = _graph(L7)
    other_c.sync_weights()
    other_a.sync_weights()
    assert cs(other_c.h) == ERR and b"batch structure" in err()
    other_c.configure([g7], [n])
    other_a.configure([g7], [n])
    assert cs(other_c.h) == ERR and b"gradients not bound" in err()
    assert as_(other_a.h, c.h) == ERR and b"gradients not bound" in err()
    arr = (ctypes.c_void_p * 12)(*[p.grad.data_ptr() for p in c._params()])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert L.sgrl_mlp_bind_grads(other_c.h, cast(arr), 6) == ERR and b"expected 12" in err()
    assert L.sgrl_mlp_bind_grads(other_c.h, null, 12) == ERR and b"null" in err()
    bad = (ctypes.c_void_p * 12)(*([p.grad.data_ptr() for p in c._params()][:11] + [None]))
    assert L.sgrl_mlp_bind_grads(other_c.h, cast(bad), 12) == ERR and b"null" in err()
    h = ctypes.c_void_p()
    assert L.sgrl_mlp_create(ctypes.byref(h)) == 0
    try:
        assert L.sgrl_mlp_bind_grads(h, cast(arr), 12) == ERR and b"parameters not set" in err()
        assert cs(h) == ERR and b"not bound as a critic" in err()
    finally:
        L.sgrl_mlp_destroy(h)
    other_c.configure([g7], [n + 1])
    assert as_(actor.h, other_c.h) == ERR and b"different batch structures" in err()
    # a critic that does not read the actor's input + output
    _, crit3 = _pair(3, seed=9)
    c3 = HipMlpCritic(crit3)
    c3.configure([_graph(3)], [n])
    assert as_(actor.h, c3.h) == ERR and b"input + output" in err()
    with pytest.raises(_lib.SgrlError, match="input \\+ output"):
        HipMlpGrads(pol, crit3)
    # widths the path does not serve: refused by the plan, by the class, and the agent keeps the PyTorch gradient half
    polw, critw = _pair(3, (1024, 1000), seed=9)
    with pytest.raises(_lib.SgrlError, match="widths up to 512"):
        HipMlpGrads(polw, critw)
    torch.cuda.synchronize()
    assert bool((loss == 7).all()) and bool((aout == 7).all())
    assert all(bool((p.grad == 7).all()) for m in (pol, crit) for p in m.parameters())      # none of the refused calls wrote anything
    # and the well-formed calls go through, on the same handles
    assert cs(c.h) == 0 and as_(actor.h, c.h) == 0 and as_(actor.h, c.h, ao=null, ald=0) == 0
    torch.cuda.synchronize()
    assert not bool((loss == 7).any()) and not bool((aout == 7).any())
    assert all(not bool((p.grad == 7).all()) for m in (pol, crit) for p in m.parameters())
    _both_steps("after the refusals", pol, crit, gr, b)


def test_agent_keeps_the_pytorch_gradient_half_for_unserved_widths():
    from sgrl_amd.td3 import Agent
    torch.manual_seed(1)
    agent = Agent(_args(3, (1024, 1000)), device=torch.device("cuda:0"), mlp_hip_grads=True)
    agent.change_morphology(_graph(3))
    agent.models2train()
    g = torch.Generator().manual_seed(5)
    n = 9
    batch = {"obs": torch.randn((n, 123), generator=g), "next_obs": torch.randn((n, 123), generator=g), "action": torch.rand((n, 9), generator=g) * 2 - 1,
             "reward": torch.randn((n, 1), generator=g), "done": torch.zeros((n, 1))}
    batch = {k: v.cuda() for k, v in batch.items()}
    out = agent.update(batch, 0)
    assert all(np.isfinite(float(v)) for v in out.values()) and "loss/actor_loss" in out
    assert not agent.use_mlp_hip_grads and agent._mlp_grads is None and "widths up to 512" in agent.mlp_hip_grads_refusal
    assert agent._targets is not None                     # the target chain serves these widths


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_device_trainer_trains_on_the_gradient_path():
    from sgrl_amd.mlp_hip import HipMlpGrads
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_hip_grads=True)
    tr = DeviceTrainer(["3d_hopper_3_shin"], 4, args=args, seed=2, device="cuda:0", max_buffer_size=4096, batch_size=64)
    assert tr.agent.use_mlp_hip_grads and tr.agent._mlp_grads is None
    tr.warmup(8)
    s = tr.train_round(max_steps=40, max_iters=2)
    assert s["per_morph_iter"] == 2
    assert isinstance(tr.agent._mlp_grads, HipMlpGrads) and tr.agent._mlp_grads.critic.n_env > 0
    losses = tr.last_losses["3d_hopper_3_shin"]
    assert all(np.isfinite(float(v)) for v in losses.values())


def test_twenty_updates_against_the_pytorch_gradient_half():
    """From one seeded state, twenty updates (ten with the actor step) on the new path and with the gradient half on PyTorch: every
    parameter tensor of the four networks within the step-norm tolerance of the reference replay (2e-3 of the step's norm plus the
    float32 floor sqrt(numel) * max|p| * 1.2e-7), accumulated over the updates."""
    from sgrl_amd.td3 import Agent
    torch.manual_seed(3)
    hip = Agent(_args(7), device=torch.device("cuda:0"), mlp_hip_grads=True)
    for mod, seed in ((hip.actor, 3), (hip.critic, 4), (hip.actor_target, 5), (hip.critic_target, 6)):
        apply_seeded_(mod, seed)
    pt = Agent(_args(7), device=torch.device("cuda:0"), mlp_hip_grads=False)
    pt.load_state_dict(hip.state_dict())
    g7 = _graph(7)
    for a in (hip, pt):
        a.change_morphology(g7)
        a.models2train()
    nets = ("actor", "critic", "actor_target", "critic_target")
    tol = {nm: [0.0] * len(list(getattr(pt, nm).parameters())) for nm in nets}
    g = torch.Generator().manual_seed(77)
    for it in range(20):
        n = 64
        batch = {"obs": torch.randn((n, 287), generator=g), "next_obs": torch.randn((n, 287), generator=g),
                 "action": torch.rand((n, 21), generator=g) * 2 - 1, "reward": torch.randn((n, 1), generator=g),
                 "done": (torch.rand((n, 1), generator=g) < 0.2).float()}
        batch = {k: v.cuda() for k, v in batch.items()}
        noise = (torch.randn((n, 21), generator=g) * 0.2).cuda()
        before = {nm: [p.detach().double().clone() for p in getattr(pt, nm).parameters()] for nm in nets}
        la, lb = hip.update(batch, it, noise=noise), pt.update(batch, it, noise=noise)
        assert sorted(la) == sorted(lb) and all(np.isfinite(float(v)) for v in la.values())
        for nm in nets:
            for i, (p, q) in enumerate(zip(getattr(pt, nm).parameters(), before[nm])):
                tol[nm][i] += 2e-3 * float((p.detach().double() - q).norm()) + np.sqrt(p.numel()) * float(q.abs().max()) * 1.2e-7
    assert hip._mlp_grads is not None and pt._mlp_grads is None
    for nm in nets:
        for i, ((name, p), q) in enumerate(zip(getattr(hip, nm).named_parameters(), getattr(pt, nm).parameters())):
            d = float((p.detach().double() - q.detach().double()).norm())
            print("20 updates %s %s: |hip - pytorch| %.3g  tolerance %.3g" % (nm, name, d, tol[nm][i]))
            assert d <= tol[nm][i], (nm, name, d, tol[nm][i])


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_launch_counts():
    from sgrl_amd import _lib, mlp_hip
    L = _lib.lib()
    mlp_hip._bind(L)
    assert L.sgrl_mlp_critic_step_launches() == 3 and L.sgrl_mlp_actor_step_launches() == 4
    pol, crit = _pair(3, (40, 72), seed=2)
    gr = mlp_hip.HipMlpGrads(pol, crit)
    assert gr.critic_launches() == 3 and gr.actor_launches() == 4
    b = _batch(3, 33, seed=1)
    gr.critic_step(b["obs"], b["action"], b["target"])
    gr.actor_step(b["obs"])
    gen = (gr.actor.generation(), gr.critic.generation())
    gr.critic_step(b["obs"], b["action"], b["target"])        # the same batch size again: nothing grows
    gr.actor_step(b["obs"])
    assert gen == (gr.actor.generation(), gr.critic.generation())
    b = _batch(3, 66, seed=1)
    gr.critic_step(b["obs"], b["action"], b["target"])        # a larger batch: the workspace grows, the generation says so
    assert gr.critic.generation() == gen[1] + 1
