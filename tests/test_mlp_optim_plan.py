"""Host side of the optimizer half of the MLP agent's TD3 update (sgrl_amd/mlp_hip.py `optim_plan` over include/sgrl_mlp.h
sgrl_mlp_optim_plan; no GPU needed): the chunk cut against a NumPy restatement (tests/mlp_optim_restate.py), the refusals, the
launch count, the exported symbols, the agent keyword on a CPU agent -- and the float64 restatement of the step itself, the yardstick
of tests/test_mlp_optim_gpu.py, against what the reference executes: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step +
its Polyak loop, in float64 on the CPU."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from mlp_optim_restate import CHUNK, optim_plan_restated, step_restated
from sgrl_amd import _lib, mlp_hip

HIDDEN = [[256, 256], [40, 72], [1, 7], [64, 48, 80, 33], [512, 500]]        # the widths of test_mlp_train_plan.py


def _dims(L, hidden):
    return [41 * L] + list(hidden) + [3 * L], [44 * L] + list(hidden) + [1]


@pytest.mark.parametrize("L", [3, 7, 14])
@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(str(x) for x in h))
def test_optim_plan_matches_the_restatement(L, hidden):
    ad, cd = _dims(L, hidden)
    for dims, stacks in ((ad, 1), (cd, 2), (cd, 1)):
        got = mlp_hip.optim_plan(dims, stacks)
        assert got == optim_plan_restated(dims, stacks), (dims, stacks)
        assert got["tensors"] == 2 * stacks * (len(dims) - 1) and got["chunk"] == CHUNK
        assert 22 + -(-got["chunks"] // 256) <= 128            # the longest chain of additions into the gradient norm (sgrl_mlp.h)


def test_optim_plan_of_the_workload_pair_and_of_the_widest_handle():
    a, c = mlp_hip.optim_plan([287, 256, 256, 21], 1), mlp_hip.optim_plan([308, 256, 256, 1], 2)
    assert a == {"tensors": 6, "elements": 287 * 256 + 256 + 256 * 256 + 256 + 256 * 21 + 21, "chunks": 72 + 1 + 64 + 1 + 6 + 1, "chunk": 1024}
    assert c == {"tensors": 12, "elements": 2 * (308 * 256 + 256 + 256 * 256 + 256 + 256 + 1), "chunks": 2 * (77 + 1 + 64 + 1 + 1 + 1), "chunk": 1024}
    widest = mlp_hip.optim_plan([1024] * 5 + [1], 2)
    assert widest["chunks"] == 2 * (4 * 1025 + 2) and 22 + -(-widest["chunks"] // 256) <= 128
    one = mlp_hip.optim_plan([1, 1, 1], 1)                    # every tensor a single element
    assert one == {"tensors": 4, "elements": 4, "chunks": 4, "chunk": 1024}


@pytest.mark.parametrize("dims,stacks,what", [
    ([287, 256, 256, 21], 0, "n_stacks"),
    ([287, 256, 256, 21], 3, "n_stacks"),
    ([287, 256, 256, 21], 2, "last width must be 1"),
    ([308, 1025, 1], 2, "outside"),
    ([0, 256, 21], 1, "outside"),
    ([287, 21], 1, "hidden"),
    ([287, 8, 8, 8, 8, 8, 21], 1, "hidden"),
])
def test_optim_plan_refuses(dims, stacks, what):
    with pytest.raises(_lib.SgrlError, match=what):
        mlp_hip.optim_plan(dims, stacks)
    if what in ("outside", "hidden"):                          # exactly what sgrl_mlp_plan refuses
        with pytest.raises(_lib.SgrlError, match=what):
            mlp_hip.plan(dims)
    else:
        mlp_hip.plan(dims)


def test_exports_launch_count_and_null_arguments():
    so = ctypes.CDLL(_lib.build())
    for n in ("sgrl_mlp_optim_plan", "sgrl_mlp_bind_optim", "sgrl_mlp_optim_bound", "sgrl_mlp_optim_step", "sgrl_mlp_optim_step_launches"):
        assert hasattr(so, n), n
    assert "mlp_optim.hip" in _lib.SOURCES
    assert not any(n.startswith("sgrl_mlp") for n in _lib.EXPORTS)          # declared in sgrl_mlp.h, not sgrl.h
    L = _lib.lib()
    mlp_hip._bind(L)
    assert L.sgrl_mlp_optim_step_launches() == 2
    null = ctypes.c_void_p(None)
    err = lambda: L.sgrl_mlp_last_error()
    d = np.asarray([287, 256, 21], dtype=np.int32)
    assert L.sgrl_mlp_optim_plan(ctypes.c_void_p(d.ctypes.data), 3, 1, null) == -1 and b"null" in err()
    assert L.sgrl_mlp_optim_plan(null, 3, 1, ctypes.c_void_p(np.zeros(4, dtype=np.int64).ctypes.data)) == -1
    assert L.sgrl_mlp_bind_optim(null, null, null, 0, null, 0, null, 0, null, 0) == -1 and b"null" in err()
    assert L.sgrl_mlp_optim_step(null, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.0, null) == -1 and b"null handle" in err()
    assert L.sgrl_mlp_optim_bound(null) == 0


# ---- the float64 restatement against what the reference executes ------------------------------------------------------------------
def _polyak_reference(source, target, tau):
    for t, s in zip(target, source):                          # reference common/functional.py:7-10
        t.data.copy_(tau * s.data + (1 - tau) * t.data)


@pytest.mark.parametrize("scale", [10.0, 0.5], ids=["clip-active", "clip-inactive"])
def test_restated_step_matches_torch_adam_clip_and_polyak_in_float64(scale):
    max_norm, tau, lr, betas, eps = 0.1, 0.005, 1e-4, (0.9, 0.999), 1e-8
    g = torch.Generator().manual_seed(4)
    shapes = [(7, 5), (7,), (3, 7), (3,), (1, 3), (1,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    target = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps)
    p = [x.detach().numpy().copy() for x in params]
    m, v, t = [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes], 0
    tg = [x.numpy().copy() for x in target]
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    for step in range(3):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
        norm = float(torch.sqrt(sum((x * x).sum() for x in grads)))
        grads = [x * (scale * max_norm / norm) for x in grads]
        for x, gr in zip(params, grads):
            x.grad = gr.clone()
        p, gc, m, v, t, tg = step_restated(p, [x.numpy() for x in grads], m, v, t, lr, betas[0], betas[1], eps, max_norm, tau, tg)
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        _polyak_reference(params, target, tau)
        assert (scale > 1) == (not all(torch.equal(x.grad, gr) for x, gr in zip(params, grads)))       # the clip bit, or not
        for i, x in enumerate(params):
            st = opt.state[x]
            assert float(st["step"]) == t == step + 1
            for what, got, want in (("p", p[i], x.detach().numpy()), ("g", gc[i], x.grad.numpy()), ("m", m[i], st["exp_avg"].numpy()),
                                    ("v", v[i], st["exp_avg_sq"].numpy()), ("target", tg[i], target[i].numpy())):
                assert rel(got, want) <= 1e-12, (step, i, what, rel(got, want))
    # tau = 0 and no clipping leave the target and the gradients as given
    p2, g2, _, _, _, tg2 = step_restated(p, gc, m, v, t, lr, betas[0], betas[1], eps, 0.0, 0.0, tg)
    assert all(np.array_equal(a, b) for a, b in zip(g2, gc)) and all(np.array_equal(a, b) for a, b in zip(tg2, tg))


# ---- the agent keyword ----------------------------------------------------------------------------------------------------------------
def test_the_keyword_follows_the_gradient_half_and_is_off_by_default():
    from sgrl_amd import td3
    from sgrl_amd.td3 import Agent, default_train_args
    assert td3.MLP_HIP_OPTIM_DEFAULT is False
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3)
    assert not Agent(args, device="cpu").use_mlp_hip_optim
    on = Agent(args, device="cpu", mlp_hip_grads=True, mlp_hip_optim=True)
    assert on.use_mlp_hip_optim and on._mlp_optim is None
    assert not Agent(args, device="cpu", mlp_hip_grads=False, mlp_hip_optim=True).use_mlp_hip_optim     # only with the gradient half
    assert not Agent(args, device="cpu", use_hip=False, mlp_hip_optim=True).use_mlp_hip_optim
    assert not Agent(default_train_args(), device="cpu", use_hip=False, mlp_hip_optim=True).use_mlp_hip_optim   # mlp + mlp only
    assert Agent(default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3, mlp_hip_grads=True, mlp_hip_optim=True),
                 device="cpu").use_mlp_hip_optim                                                        # args can carry it
    on._mlp_optim = object()                                  # a stand-in for the live object does not travel with a copy
    twin = copy.deepcopy(on)
    assert twin._mlp_optim is None and twin.use_mlp_hip_optim
    on._mlp_optim = None
    # on the CPU the keyword changes nothing: the same bits as the agent built without it
    off = Agent(args, device="cpu", mlp_hip_grads=True)
    off.load_state_dict(on.state_dict())
    g = torch.Generator().manual_seed(9)
    for a in (on, off):
        a.models2train()
    for it in range(2):
        batch = {"obs": torch.randn((5, 123), generator=g), "next_obs": torch.randn((5, 123), generator=g),
                 "action": torch.rand((5, 9), generator=g) * 2 - 1, "reward": torch.randn((5, 1), generator=g), "done": torch.zeros((5, 1))}
        noise = torch.randn((5, 9), generator=g) * 0.2
        la, lb = on.update(batch, it, noise=noise), off.update(batch, it, noise=noise)
        assert all(float(la[k]) == float(lb[k]) for k in la)
    for (n, p), (_, q) in zip(on.state_dict().items(), off.state_dict().items()):
        assert torch.equal(p, q), n
    assert on._mlp_optim is None


def test_optimizers_the_path_does_not_serve_are_named():
    lin = torch.nn.Linear(3, 2)
    ps = list(lin.parameters())
    ok = torch.optim.Adam(ps, lr=1e-3)
    assert mlp_hip.HipMlpOptim.refusal(ok, ps) is None
    assert mlp_hip.HipMlpOptim.refusal(torch.optim.Adam(ps, lr=1e-3, capturable=True), ps) is None
    for bad in (torch.optim.Adam(ps, lr=1e-3, weight_decay=0.1), torch.optim.Adam(ps, lr=1e-3, amsgrad=True),
                torch.optim.Adam(ps, lr=1e-3, maximize=True), torch.optim.Adam([{"params": ps[:1]}, {"params": ps[1:]}], lr=1e-3),
                torch.optim.SGD(ps, lr=1e-3)):
        assert mlp_hip.HipMlpOptim.refusal(bad, ps)
    assert mlp_hip.HipMlpOptim.refusal(ok, ps[:1])            # not exactly the network's parameters
