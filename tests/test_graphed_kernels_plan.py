"""Host side of the graphed SWAT / SMP updates on the HIP kernels (td3.GraphedUpdates(hip_kernels=True), td3.Agent(loss_kernels=...),
train_ops.twin_mse / neg_mean over include/sgrl_train.h sgrl_td3_*; no GPU needed): the float64 restatement of the loss head
(tests/td3_loss_restate.py) against float64 PyTorch, the fallbacks of the two train_ops entries, the argument errors of the C ABI,
the stamp -- what a captured graph has baked of the target handles -- over stub objects, and the refusals."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import td3_loss_restate as R
from sgrl_amd import td3, train_ops

TRAV = ["pre", "inlcrs", "postlcrs"]
NS = [1, 63, 64, 65, 255, 256, 257, 36, 84, 15 * 257, 100003]


def _inputs(n, seed):
    rs = np.random.RandomState(seed)
    return [(0.6 * rs.standard_normal(n)).astype(np.float32) for _ in range(3)]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("g", [1.0, -0.37])
def test_restatement_against_float64_pytorch(n, g):
    q1, q2, t = _inputs(n, n)
    a, b = (torch.from_numpy(x).double().requires_grad_() for x in (q1, q2))
    loss = F.mse_loss(a, torch.from_numpy(t).double()) + F.mse_loss(b, torch.from_numpy(t).double())
    (loss * g).backward()
    assert _rel(R.twin_mse_forward(q1, q2, t), loss.item()) <= 1e-14
    d1, d2 = R.twin_mse_backward(q1, q2, t, g)
    assert _rel(d1, a.grad.numpy()) <= 1e-14 and _rel(d2, b.grad.numpy()) <= 1e-14
    c = torch.from_numpy(q1).double().requires_grad_()
    nm = -c.mean()
    (nm * g).backward()
    assert _rel(R.neg_mean_forward(q1), nm.item()) <= 1e-14
    assert _rel(R.neg_mean_backward(n, g), c.grad.numpy()) <= 1e-14


# ---- the fallbacks of train_ops.twin_mse / neg_mean -------------------------------------------------------------------------
def _bits_equal(a, b):
    raw = lambda t: t.detach().contiguous().reshape(-1).numpy().view(np.uint8)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_tensors_take_the_pytorch_expressions_to_the_bit(dtype):
    q1, q2, t = (torch.from_numpy(x).to(dtype).reshape(12, 7) for x in _inputs(84, 5))
    runs = []
    for fn_twin, fn_neg in ((train_ops.twin_mse, train_ops.neg_mean),
                            (lambda a, b, c: F.mse_loss(a, c) + F.mse_loss(b, c), lambda a: -a.mean())):
        a, b = q1.clone().requires_grad_(), q2.clone().requires_grad_()
        loss = fn_twin(a, b, t)
        (loss * -0.37).backward()
        c = q1.clone().requires_grad_()
        nm = fn_neg(c)
        (nm * -0.37).backward()
        runs.append((loss, a.grad, b.grad, nm, c.grad))
    for x, y in zip(*runs):
        assert _bits_equal(x, y)
    assert type(runs[0][0].grad_fn).__name__ == "AddBackward0" and type(runs[0][3].grad_fn).__name__ == "NegBackward0"
    with torch.no_grad():
        assert _bits_equal(train_ops.twin_mse(q1, q2, t), F.mse_loss(q1, t) + F.mse_loss(q2, t))
        assert _bits_equal(train_ops.neg_mean(q1), -q1.mean())
    # a target of another shape broadcasts as F.mse_loss does (the same warning included); non-contiguous inputs
    a = q1.t().clone().requires_grad_()
    assert _bits_equal(train_ops.neg_mean(a.t()), -a.t().mean())
    assert _bits_equal(train_ops.twin_mse(a.t(), q2, t), F.mse_loss(a.t(), t) + F.mse_loss(q2, t))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_launch_count_need_no_device():
    L = train_ops._L()
    assert L.sgrl_td3_loss_launches() == 1
    ERR_ARG = -1
    buf = np.zeros((6, 64), dtype=np.float32)
    p = [ctypes.c_void_p(buf[i].ctypes.data) for i in range(6)]
    inside = ctypes.c_void_p(buf[2].ctypes.data + 4 * 4)                # with n = 8: shares four elements with the target's first eight
    null, n = ctypes.c_void_p(None), 64
    q1, q2, t, g, d1, d2 = p
    err = lambda: L.sgrl_train_last_error()
    for a in ((null, q2, t, n, g, null), (q1, null, t, n, g, null), (q1, q2, null, n, g, null), (q1, q2, t, n, null, null),
              (q1, q2, t, 0, g, null), (q1, q2, t, -5, g, null), (t, q2, t, n, g, null), (q1, t, t, n, g, null), (q1, inside, t, 8, g, null)):
        assert L.sgrl_td3_twin_mse_forward(*a) == ERR_ARG and b"sgrl_td3_twin_mse_forward" in err(), a
    for a in ((null, q2, t, n, g, d1, d2, null), (q1, null, t, n, g, d1, d2, null), (q1, q2, null, n, g, d1, d2, null),
              (q1, q2, t, n, null, d1, d2, null), (q1, q2, t, n, g, null, d2, null), (q1, q2, t, n, g, d1, null, null),
              (q1, q2, t, 0, g, d1, d2, null), (q1, q2, t, -1, g, d1, d2, null), (t, q2, t, n, g, d1, d2, null), (q1, t, t, n, g, d1, d2, null),
              (q1, q2, t, n, g, t, d2, null), (q1, q2, t, n, g, d1, t, null), (q1, q2, t, 8, g, d1, inside, null)):
        assert L.sgrl_td3_twin_mse_backward(*a) == ERR_ARG and b"sgrl_td3_twin_mse_backward" in err(), a
    for a in ((null, n, g, null), (q1, n, null, null), (q1, 0, g, null), (q1, -2, g, null)):
        assert L.sgrl_td3_neg_mean_forward(*a) == ERR_ARG and b"sgrl_td3_neg_mean_forward" in err(), a
    for a in ((n, null, d1, null), (n, g, null, null), (0, g, d1, null), (-2, g, d1, null)):
        assert L.sgrl_td3_neg_mean_backward(*a) == ERR_ARG and b"sgrl_td3_neg_mean_backward" in err(), a
    assert not buf.any()                                                 # nothing was written


# ---- the stamp over stub handles -----------------------------------------------------------------------------------------------
class _Handle(object):
    def __init__(self, gen, bound):
        self.gen, self._bound = gen, bound

    def generation(self):
        return self.gen


def _stub_updates(targets):
    """A GraphedUpdates over stubs with one 'captured graph' per flag on slot 0: the stamp logic touches no device."""
    gu = td3.GraphedUpdates.__new__(td3.GraphedUpdates)
    args = types.SimpleNamespace(policy_freq=2)
    holder = types.SimpleNamespace(targets=targets)
    gu.agent = types.SimpleNamespace(args=args, actor_target=object(), critic_target=object(), _hip_targets=lambda next_obs: holder.targets)
    gu.hip_kernels, gu.split, gu.B = True, False, 12
    gu.warmed, gu.captures = {0}, {}
    sl = {"graph": None, "batch": {"next_obs": None}, "graphs": {}, "stamp": {}, "out": {}, "targets": targets}
    gu.slots = {0: sl}
    for flag in (0, 1):
        sl["graphs"][flag], sl["stamp"][flag] = object(), gu._stamp(sl)
    return gu, holder


def _swat_targets():
    return types.SimpleNamespace(actor=_Handle(0, (16, 32)), critic=types.SimpleNamespace(q1=_Handle(3, (48, 64)), q2=_Handle(0, (80, 96))))


def test_stamp_follows_generations_and_bound_addresses():
    swat = _swat_targets()
    smp = types.SimpleNamespace(actor=_Handle(1, (16,)), critic=_Handle(2, (32,)))
    assert td3.target_handles(None) == []
    assert td3.target_handles(swat) == [swat.actor, swat.critic.q1, swat.critic.q2]          # three generations for SWAT
    assert td3.target_handles(smp) == [smp.actor, smp.critic]                                 # two for SMP
    assert td3.handles_stamp(td3.target_handles(swat)) == ((0, (16, 32)), (3, (48, 64)), (0, (80, 96)))
    for targets, handles in ((swat, td3.target_handles(swat)), (smp, td3.target_handles(smp))):
        for h in handles:
            gu, _ = _stub_updates(targets)
            assert not gu.stale(0, 0) and not gu.stale(0, 1)                  # unchanged handles
            h.gen += 1                                                        # the library freed something a graph may point into
            assert gu.stale(0, 0) and gu.stale(0, 1)
            h.gen -= 1
            assert not gu.stale(0, 0)
            old, h._bound = h._bound, h._bound[:-1] + (h._bound[-1] + 256,)   # a parameter moved: bound again, nothing freed
            assert gu.stale(0, 0) and gu.stale(0, 1)
            h._bound = old
            assert not gu.stale(0, 0) and not gu.stale(0, 1)
    gu, holder = _stub_updates(swat)
    assert not gu.stale(1, 0) and not gu.stale(0, 2)                          # nothing captured there: nothing to be stale
    holder.targets = _swat_targets()                                          # a re-created target object with fresh handles
    holder.targets.actor._bound = None
    assert gu.stale(0, 0)
    # without hip_kernels the target handles are not followed (the agent's chain is PyTorch then)
    gu, _ = _stub_updates(swat)
    gu.hip_kernels = False
    for flag in (0, 1):
        gu.slots[0]["stamp"][flag] = gu._stamp(gu.slots[0])
    swat.actor.gen += 1
    assert not gu.stale(0, 0)


def test_capture_preconditions_raise_on_the_host():
    swat = _swat_targets()
    gu, holder = _stub_updates(swat)
    sl = gu.slots[0]
    gu._check_capture(sl, 0)                                                   # warmed, same target object: fine
    gu.split = True
    with pytest.raises(RuntimeError, match="three-graph form is not built"):
        gu._check_capture(sl, 0)
    del sl["graphs"][0]                                                        # ... and through the update path, before any capture
    with pytest.raises(RuntimeError, match="three-graph form is not built"):
        gu._replay(sl, 0, None, 0)
    assert gu.captures == {}
    gu.split = False
    with pytest.raises(RuntimeError, match="warm\\(1, ...\\) every morphology"):
        gu._check_capture(sl, 1)
    holder.targets = _swat_targets()                                           # Agent._hip_targets re-created it
    with pytest.raises(RuntimeError, match="warm\\(0, ...\\) again"):
        gu._check_capture(sl, 0)
    with pytest.raises(RuntimeError, match="warm\\(0, ...\\) again"):
        gu._replay(sl, 0, None, 0)
    assert gu.captures == {}


# ---- refusals and the Agent switch -----------------------------------------------------------------------------------------------
def _args(atype, **over):
    a = td3.default_train_args(actor_type=atype, critic_type=atype, **over)
    if atype == "smp":
        a.td = a.bu = True
    if atype == "mlp":
        a.mlp_num_limbs = 3
        a.agent.policy_network = {"hidden_dims": [8, 8]}
        a.agent.q_network = {"hidden_dims": [8, 8]}
    return a


def test_constructor_refusals_are_those_without_the_keyword():
    cpu = torch.device("cpu")
    for atype in ("swat", "smp", "set"):
        agent = td3.Agent(_args(atype), device=cpu)
        with pytest.raises(RuntimeError, match="needs the agent on the GPU") as with_kw:
            td3.GraphedUpdates(agent, 16, hip_kernels=True)
        with pytest.raises(RuntimeError, match="needs the agent on the GPU") as without:
            td3.GraphedUpdates(agent, 16)
        assert str(with_kw.value) == str(without.value)
    mlp = td3.Agent(_args("mlp"), device=cpu)
    with pytest.raises(NotImplementedError, match="GraphedUpdates is not built for 'mlp'"):
        td3.GraphedUpdates(mlp, 16, hip_kernels=True)
    with pytest.raises(NotImplementedError, match="the differentiable passes of those updates on the training kernels"):
        td3.Agent(td3.default_train_args(actor_type="gnn"), device=cpu)


def test_loss_switch_resolution():
    cpu = torch.device("cpu")
    assert td3.LOSS_KERNELS_DEFAULT is False
    assert not td3.Agent(_args("swat"), device=cpu).use_loss_kernels
    assert td3.Agent(_args("swat", loss_kernels=True), device=cpu).use_loss_kernels                     # args.loss_kernels
    assert not td3.Agent(_args("swat", loss_kernels=True), device=cpu, loss_kernels=False).use_loss_kernels
    assert td3.Agent(_args("smp"), device=cpu, loss_kernels=True).use_loss_kernels
    assert not td3.Agent(_args("swat"), device=cpu, use_hip=False, loss_kernels=True).use_loss_kernels  # follows use_hip
    assert not td3.Agent(_args("mlp"), device=cpu, loss_kernels=True).use_loss_kernels                  # mlp agents ignore it


@pytest.mark.parametrize("atype", ["swat", "smp"])
def test_cpu_agent_with_the_loss_switch_is_bit_equal(atype):
    from sgrl_amd import graph as G, mjcf
    cpu = torch.device("cpu")
    g = G.getGraphDict(mjcf.load_asset("3d_hopper_3_shin").parents, TRAV, [], device=cpu)
    L, B = len(g["parents"]), 8
    torch.manual_seed(3)
    on = td3.Agent(_args(atype), device=cpu, loss_kernels=True)
    off = td3.Agent(_args(atype), device=cpu, loss_kernels=False)
    off.load_state_dict(on.state_dict())
    assert on.use_loss_kernels and not off.use_loss_kernels
    before = [p.detach().clone() for p in on.critic.parameters()]
    gen = torch.Generator().manual_seed(11)
    for it in range(3):
        batch = {"obs": torch.randn((B, 41 * L), generator=gen), "next_obs": torch.randn((B, 41 * L), generator=gen),
                 "action": torch.rand((B, 3 * L), generator=gen) * 2 - 1, "reward": torch.rand((B, 1), generator=gen),
                 "done": (torch.rand((B, 1), generator=gen) < 0.3).float()}
        noise = torch.randn((B, 3 * L), generator=gen) * 0.2
        outs = []
        for agent in (on, off):
            agent.change_morphology(g)
            agent.models2train()
            outs.append(agent.update(batch, it, noise=noise))
        assert outs[0].keys() == outs[1].keys() and ("loss/actor_loss" in outs[0]) == (it % 2 == 0)
        for k in outs[0]:
            assert _bits_equal(torch.as_tensor(outs[0][k]), torch.as_tensor(outs[1][k])), (it, k)
    for (n, a), (_, b) in zip(on.state_dict().items(), off.state_dict().items()):
        assert torch.equal(a, b), n
    assert max(float((p.detach() - q).abs().max()) for p, q in zip(on.critic.parameters(), before)) > 0
