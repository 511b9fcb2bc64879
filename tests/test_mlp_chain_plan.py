"""Host side of the MLP twin critic and the fused TD3 target chain (sgrl_amd/mlp_hip.py `chain_plan` over include/sgrl_mlp.h
sgrl_mlp_chain_plan; no GPU needed): the pair's kernel variant, LDS bytes and activation stride against a NumPy restatement
(tests/mlp_chain_restate.py), the pairs the library refuses, an MLP agent on the CPU (never builds a handle, survives deepcopy),
and the exported symbols of include/sgrl_mlp.h."""
import copy
import ctypes
import os
import re

import pytest
import torch

from mlp_chain_restate import chain_plan_restated
from sgrl_amd import _lib, mlp_hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = [([287, 256, 256, 21], [308, 256, 256, 1]),
         ([123, 40, 72, 9], [132, 300, 512, 1]),                       # 1 chunk against 2
         ([574, 1024, 1000, 42], [616, 1024, 1000, 1]),                # panel depth 8
         ([287, 64, 21], [308, 64, 48, 80, 33, 1]),                    # 1 against 4 hidden layers
         ([287, 64, 48, 80, 33, 21], [308, 600, 1]),                   # 4 against 1, 1 chunk against 4
         ([41, 1, 3], [44, 1, 7, 1])]


@pytest.mark.parametrize("actor_dims,critic_dims", PAIRS)
def test_chain_plan_matches_the_restatement(actor_dims, critic_dims):
    got, want = mlp_hip.chain_plan(actor_dims, critic_dims), chain_plan_restated(actor_dims, critic_dims)
    assert got == want
    pa, pc = mlp_hip.plan(actor_dims), mlp_hip.plan(critic_dims)
    assert got["chunks"] == max(pa["chunks"], pc["chunks"]) and got["sx"] == max(pa["sx"], pc["sx"])
    assert got["lds_bytes"] <= 160 * 1024 and got["sx"] % 8 == 4           # row stride 4 x odd: conflict-free 128-bit operand reads
    assert all(k % got["bk"] == 0 for k in pa["kpad"] + pc["kpad"])
    assert got["sx"] >= pc["kpad"][0] + 4 >= actor_dims[0] + actor_dims[-1] + 4   # the action columns fit behind the observation's


def test_chain_plan_of_the_named_pairs():
    assert mlp_hip.chain_plan(*PAIRS[0]) == {"chunks": 1, "bk": 16, "lds_bytes": 4 * (32 * 324 + 512 * 20), "sx": 324, "tile_rows": 32}
    p = mlp_hip.chain_plan(*PAIRS[1])
    assert (p["chunks"], mlp_hip.plan(PAIRS[1][0])["chunks"], mlp_hip.plan(PAIRS[1][1])["chunks"]) == (2, 1, 2)
    p = mlp_hip.chain_plan(*PAIRS[2])
    assert (p["chunks"], p["bk"], p["lds_bytes"], p["sx"]) == (4, 8, 156160, 1028)


@pytest.mark.parametrize("actor_dims,critic_dims,what", [
    ([287, 256, 256, 21], [308, 256, 256, 2], "last width must be 1"),
    ([287, 256, 256, 21], [307, 256, 256, 1], "input \\+ output"),
    ([287, 256, 256, 21], [287, 256, 256, 1], "input \\+ output"),
    ([287, 256, 256, 21], [308, 1025, 1], "outside"),
    ([287, 21], [308, 256, 1], "hidden"),
])
def test_chain_plan_refuses(actor_dims, critic_dims, what):
    with pytest.raises(_lib.SgrlError, match=what):
        mlp_hip.chain_plan(actor_dims, critic_dims)


def test_cpu_mlp_agent_never_builds_a_handle_and_deep_copies():
    from sgrl_amd.mlp_policy import MlpCritic
    from sgrl_amd.td3 import Agent, default_train_args
    agent = Agent(default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3), device="cpu")
    assert agent.use_mlp_hip and agent._targets is None
    assert not Agent(default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3), device="cpu", use_hip=False).use_mlp_hip
    assert not Agent(default_train_args(), device="cpu", use_hip=False).use_mlp_hip
    g = torch.Generator().manual_seed(0)
    B = 5
    batch = {"obs": torch.randn((B, 123), generator=g), "next_obs": torch.randn((B, 123), generator=g),
             "action": torch.rand((B, 9), generator=g) * 2 - 1, "reward": torch.randn((B, 1), generator=g),
             "done": torch.tensor([[0.0], [1.0], [0.0], [0.0], [1.0]])}
    reward, tq = agent.update_targets(batch, torch.randn((B, 9), generator=g) * 0.4)
    assert tq.shape == (B, 1) and bool(torch.isfinite(tq).all())
    assert torch.equal(tq[batch["done"] == 1], reward[batch["done"] == 1])
    assert agent._targets is None and agent.actor_target._mlp_hip is None and agent.critic_target._mlp_hip is None
    assert isinstance(agent.critic_target, MlpCritic) and hasattr(agent.critic_target, "hip_handle")
    twin = copy.deepcopy(agent)
    assert twin._targets is None and twin.critic_target._mlp_hip is None and twin.use_mlp_hip
    _, tq2 = twin.update_targets(batch, torch.zeros((B, 9)))
    _, tq1 = agent.update_targets(batch, torch.zeros((B, 9)))
    assert torch.equal(tq1, tq2)
    # a stand-in for a live handle does not travel with a copy either
    agent._targets = agent.critic_target._mlp_hip = object()
    twin = copy.deepcopy(agent)
    assert twin._targets is None and twin.critic_target._mlp_hip is None
    agent._targets = agent.critic_target._mlp_hip = None


def test_exports_every_symbol_the_header_declares():
    text = open(os.path.join(REPO, "include", "sgrl_mlp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(sgrl_mlp_[a-z0-9_]+)\s*\(", text)))
    assert {"sgrl_mlp_set_critic_params", "sgrl_mlp_critic_forward", "sgrl_mlp_td_target", "sgrl_mlp_chain_plan",
            "sgrl_mlp_td_target_launches", "sgrl_mlp_critic_forward_launches", "sgrl_mlp_forward", "sgrl_mlp_plan"} <= set(names)
    so = ctypes.CDLL(_lib.build())
    for n in names:
        assert hasattr(so, n), n
    assert so.sgrl_mlp_td_target_launches() == 1 and so.sgrl_mlp_critic_forward_launches() == 1
