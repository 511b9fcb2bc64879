"""Host side of the gradient half of the MLP agent's TD3 update (sgrl_amd/mlp_hip.py `train_plan` over include/sgrl_mlp.h
sgrl_mlp_train_plan; no GPU needed): kernel variant, LDS bytes, workspace floats and weight-gradient tiles against a NumPy
restatement (tests/mlp_train_restate.py), the refusals, the exported symbols, and the agent keyword on a CPU agent (ignored:
the update is bit-identical)."""
import copy
import ctypes

import pytest
import torch

from mlp_restate import apply_seeded_
from mlp_train_restate import train_plan_restated
from sgrl_amd import _lib, mlp_hip
from sgrl_amd.td3 import Agent, default_train_args

HIDDEN = [[256, 256], [40, 72], [1, 7], [64, 48, 80, 33], [512, 500]]        # the last: the widest pair the path serves
BATCHES = [1, 31, 33, 66, 256]


def _dims(L, hidden):
    return [41 * L] + list(hidden) + [3 * L], [44 * L] + list(hidden) + [1]


@pytest.mark.parametrize("L", [3, 7, 14])
@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(str(x) for x in h))
def test_train_plan_matches_the_restatement(L, hidden):
    ad, cd = _dims(L, hidden)
    for B in BATCHES:
        got, want = mlp_hip.train_plan(ad, cd, B), train_plan_restated(ad, cd, B)
        assert got == want, B
        assert got["lds_bytes"] <= 160 * 1024 and got["sx"] % 8 == 4
        pa, pc = mlp_hip.plan(ad), mlp_hip.plan(cd)
        assert got["sx"] >= max(pa["kpad"] + pa["npad"] + pc["kpad"] + pc["npad"]) + 4
        assert all(k % got["bk"] == 0 for k in pa["kpad"] + pc["kpad"] + pa["npad"] + pc["npad"])
        assert got["chunks"] * 256 >= max(pa["npad"] + pc["npad"])


def test_train_plan_of_the_workload_pair():
    p = mlp_hip.train_plan([287, 256, 256, 21], [308, 256, 256, 1], 256)
    assert (p["chunks"], p["bk"], p["sx"], p["lds_bytes"], p["row_tiles"]) == (1, 16, 324, 4 * (32 * 324 + 512 * 20), 8)
    assert p["critic_wgrad_tiles"] == 2 * (8 * 10 + 8 * 8 + 1 * 8) and p["actor_wgrad_tiles"] == 8 * 9 + 8 * 8 + 1 * 8
    assert p["critic_ws_floats"] == 256 * 320 + 2 * 256 * (512 + 544) + 4 * 8
    assert p["actor_ws_floats"] == 256 * 288 + 256 * (512 + 544) + 256 * (32 + 21) + 2 * 8


@pytest.mark.parametrize("actor_dims,critic_dims,batch,what", [
    ([287, 256, 256, 21], [308, 256, 256, 2], 8, "last width must be 1"),
    ([287, 256, 256, 21], [307, 256, 256, 1], 8, "input \\+ output"),
    ([123, 40, 9], [308, 40, 1], 8, "input \\+ output"),
    ([287, 256, 256, 21], [308, 1025, 1], 8, "outside"),
    ([287, 21], [308, 256, 1], 8, "hidden"),
    ([287, 256, 256, 21], [308, 256, 256, 1], 0, "batch"),
    ([287, 256, 256, 21], [308, 256, 256, 1], (1 << 24) + 1, "batch"),
    ([287, 256, 256, 21], [308, 513, 1], 8, "widths up to 512"),
    ([287, 1024, 1000, 21], [308, 256, 256, 1], 8, "widths up to 512"),
    ([41 * 14, 64, 3 * 14], [44 * 14, 64, 1], 8, None),                     # a 616-wide INPUT is served: only layer outputs count
])
def test_train_plan_refuses(actor_dims, critic_dims, batch, what):
    if what is None:
        assert mlp_hip.train_plan(actor_dims, critic_dims, batch)["chunks"] == 1
        return
    with pytest.raises(_lib.SgrlError, match=what):
        mlp_hip.train_plan(actor_dims, critic_dims, batch)


def test_exports_and_launch_counts():
    so = ctypes.CDLL(_lib.build())
    for n in ("sgrl_mlp_train_plan", "sgrl_mlp_bind_grads", "sgrl_mlp_critic_step_grads", "sgrl_mlp_actor_step_grads",
              "sgrl_mlp_critic_step_launches", "sgrl_mlp_actor_step_launches"):
        assert hasattr(so, n), n
    null = ctypes.c_void_p(None)
    so.sgrl_mlp_last_error.restype = ctypes.c_char_p
    assert so.sgrl_mlp_train_plan(null, 4, null, 4, 8, null, null) == -1 and b"null" in so.sgrl_mlp_last_error()
    assert so.sgrl_mlp_bind_grads(null, null, 0) == -1 and b"null" in so.sgrl_mlp_last_error()
    assert so.sgrl_mlp_critic_step_grads(null, null, 0, null, 0, null, null, null) == -1 and b"null" in so.sgrl_mlp_last_error()
    assert so.sgrl_mlp_actor_step_grads(null, null, null, 0, ctypes.c_float(1.0), null, null, 0, null) == -1 and b"null" in so.sgrl_mlp_last_error()


def _batch(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return {"obs": torch.randn((B, 41 * L), generator=g), "next_obs": torch.randn((B, 41 * L), generator=g),
            "action": torch.rand((B, 3 * L), generator=g) * 2 - 1, "reward": torch.randn((B, 1), generator=g),
            "done": (torch.rand((B, 1), generator=g) < 0.3).float()}, torch.randn((B, 3 * L), generator=g) * 0.2


def test_the_keyword_is_ignored_on_a_cpu_agent():
    """mlp_hip_grads=True on a CPU agent: no handle is ever built and three updates (two with the actor step) leave exactly the bits
    of the agent built without the keyword; other agent types never take the keyword's path; args can carry it."""
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3)
    on, off = Agent(args, device="cpu", mlp_hip_grads=True), Agent(args, device="cpu", mlp_hip_grads=False)
    assert on.use_mlp_hip_grads and not off.use_mlp_hip_grads and on._mlp_grads is None
    assert not Agent(args, device="cpu", use_hip=False, mlp_hip_grads=True).use_mlp_hip_grads          # follows use_hip
    assert not Agent(default_train_args(), device="cpu", use_hip=False, mlp_hip_grads=True).use_mlp_hip_grads   # mlp + mlp only
    assert Agent(default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3, mlp_hip_grads=True), device="cpu").use_mlp_hip_grads
    from sgrl_amd import td3
    assert Agent(args, device="cpu").use_mlp_hip_grads == bool(td3.MLP_HIP_GRADS_DEFAULT)
    on._mlp_grads = object()                              # a stand-in for live handles does not travel with a copy
    twin = copy.deepcopy(on)
    assert twin._mlp_grads is None and twin.use_mlp_hip_grads
    on._mlp_grads = None
    for mod, seed in ((on.actor, 3), (on.critic, 4), (on.actor_target, 5), (on.critic_target, 6)):
        apply_seeded_(mod, seed)
    off.load_state_dict(on.state_dict())
    for a in (on, off):
        a.models2train()
    for it in range(3):
        batch, noise = _batch(5, 3, 40 + it)
        la, lb = on.update(batch, it, noise=noise), off.update(batch, it, noise=noise)
        assert sorted(la) == sorted(lb) and ("loss/actor_loss" in la) == (it % 2 == 0)
        for k in la:
            assert float(la[k]) == float(lb[k]), (it, k)
    for (n, p), (_, q) in zip(on.state_dict().items(), off.state_dict().items()):
        assert torch.equal(p, q), n
    for p, q in zip(on.critic.parameters(), off.critic.parameters()):
        assert torch.equal(p.grad, q.grad)
    assert on._mlp_grads is None and on.use_mlp_hip_grads
