"""The seven opt-in switches of td3.Agent and its target-chain slot, on the CPU: where each switch's value comes from (constructor
keyword, then args.<name>, then the module's *_DEFAULT constant read when the agent is built), which agent kinds each switch
reaches, that a CPU batch never takes a HIP target chain, and that no per-process device object travels with a copy of the agent."""
import copy

import pytest
import torch

from sgrl_amd import td3
from sgrl_amd.td3 import Agent, default_train_args

CPU = torch.device("cpu")
SLOTS = ("_targets",)                     # where Agent keeps its target-chain object

KINDS = {"set": dict(),
         "swat": dict(actor_type="swat", critic_type="swat"),
         "smp": dict(actor_type="smp", critic_type="smp", td=True, bu=True),
         "smp_td": dict(actor_type="smp", critic_type="smp", td=True, bu=False),
         "mlp": dict(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3),
         "swat_set": dict(actor_type="swat", critic_type="set")}

# switch (constructor keyword = args name; NAME_DEFAULT in td3) -> the public attribute it feeds, the agent kinds it reaches, and
# what else the constructor needs for it to take effect
SWITCHES = {"swat_train_kernels": ("use_swat_train_kernels", {"swat"}, {}),
            "smp_train_kernels": ("use_smp_train_kernels", {"smp"}, {}),
            "mlp_hip_grads": ("use_mlp_hip_grads", {"mlp"}, {}),
            "mlp_hip_optim": ("use_mlp_hip_optim", {"mlp"}, {"mlp_hip_grads": True}),
            "loss_kernels": ("use_loss_kernels", {"set", "swat", "smp", "smp_td", "swat_set"}, {}),
            "set_hip_targets": ("use_set_hip", {"set"}, {}),
            "swat_hip_dropout": ("swat_hip_dropout", {"swat"}, {})}
# the cheapest kind to build that each switch reaches
PRECEDENCE_KIND = {"swat_train_kernels": "swat", "smp_train_kernels": "smp", "mlp_hip_grads": "mlp", "mlp_hip_optim": "mlp",
                   "loss_kernels": "swat", "set_hip_targets": "set", "swat_hip_dropout": "swat"}


def _agent(kind, use_hip=True, args_over=None, **kw):
    return Agent(default_train_args(**dict(KINDS[kind], **(args_over or {}))), device=CPU, use_hip=use_hip, **kw)


class _StubHandle(object):
    """Stands for a device-side object: refuses to be copied or pickled, as a ctypes pointer does."""

    def __reduce_ex__(self, protocol):
        raise TypeError("a device handle must not travel with the agent")


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_keyword_beats_args_beats_the_module_default(name, monkeypatch):
    attr, _, needs = SWITCHES[name]
    kind, const = PRECEDENCE_KIND[name], name.upper() + "_DEFAULT"
    assert isinstance(getattr(td3, const), bool)
    assert not hasattr(default_train_args(**KINDS[kind]), name)        # the lowest level is really reached below
    for want in (True, False):
        # the constant alone, patched after td3 was imported: it is read when the agent is built
        monkeypatch.setattr(td3, const, want)
        assert getattr(_agent(kind, **needs), attr) is want
        # args.<name> beats the constant
        monkeypatch.setattr(td3, const, not want)
        assert getattr(_agent(kind, args_over={name: want}, **needs), attr) is want
        # an args.<name> of None says nothing: the constant again
        assert getattr(_agent(kind, args_over={name: None}, **needs), attr) is (not want)
        # the keyword beats both
        assert getattr(_agent(kind, args_over={name: not want}, **dict(needs, **{name: want})), attr) is want
        monkeypatch.setattr(td3, const, want)
        assert getattr(_agent(kind, args_over={name: not want}, **dict(needs, **{name: want})), attr) is want


@pytest.fixture(scope="module")
def all_on():
    """One agent per kind with every switch given as True, with and without use_hip."""
    kw = {name: True for name in SWITCHES}
    return {(kind, use_hip): _agent(kind, use_hip=use_hip, **kw) for kind in KINDS for use_hip in (True, False)}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_switch_reaches_only_the_kinds_it_applies_to(kind, all_on):
    agent = all_on[(kind, True)]
    for name, (attr, kinds, _) in SWITCHES.items():
        assert getattr(agent, attr) is (kind in kinds), (kind, name)
    assert agent.use_swat_hip is (kind == "swat") and agent.use_smp_hip is (kind == "smp") and agent.use_mlp_hip is (kind == "mlp")
    for net in (agent.actor, agent.critic):
        assert bool(getattr(net, "train_kernels", False)) is (kind in ("swat", "smp"))
    for net in (agent.actor_target, agent.critic_target):
        assert not getattr(net, "train_kernels", False)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_use_hip_false_turns_every_switch_off(kind, all_on):
    agent = all_on[(kind, False)]
    for name, (attr, _, _) in SWITCHES.items():
        assert getattr(agent, attr) is False, (kind, name)
    assert not (agent.use_swat_hip or agent.use_smp_hip or agent.use_mlp_hip or agent.use_set_hip)


def test_args_reach_only_the_kinds_they_apply_to_as_well():
    for kind in KINDS:
        agent = _agent(kind, args_over={name: True for name in SWITCHES})
        for name, (attr, kinds, _) in SWITCHES.items():
            assert getattr(agent, attr) is (kind in kinds), (kind, name)


def test_the_optimizer_half_needs_the_gradient_half():
    assert not _agent("mlp", mlp_hip_grads=False, mlp_hip_optim=True).use_mlp_hip_optim
    assert not _agent("mlp", args_over={"mlp_hip_grads": False, "mlp_hip_optim": True}).use_mlp_hip_optim
    assert _agent("mlp", mlp_hip_grads=True, mlp_hip_optim=True).use_mlp_hip_optim


def test_dropout_rate_is_read_for_swat_networks_only():
    for kind in KINDS:
        agent = _agent(kind, args_over={"dropout_rate": 0.1, "seed": 7})
        assert agent.dropout_rate == (0.1 if "swat" in kind else 0.0) and agent.dropout_seed == 7
    assert _agent("swat").dropout_rate == 0.0 and _agent("swat").dropout_seed == 0


@pytest.mark.parametrize("kind", ["set", "swat", "smp", "mlp"])
def test_a_cpu_batch_takes_no_hip_chain_and_caches_nothing(kind, all_on):
    agent = all_on[(kind, True)]
    assert getattr(agent, {"set": "use_set_hip", "swat": "use_swat_hip", "smp": "use_smp_hip", "mlp": "use_mlp_hip"}[kind])
    for dtype in (torch.float32, torch.float64):
        assert agent._hip_targets(torch.zeros(4, 41 * 3, dtype=dtype)) is None
        for slot in SLOTS:
            assert getattr(agent, slot) is None


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_no_device_object_travels_with_a_copy(kind):
    agent = _agent(kind, **{name: True for name in SWITCHES})
    held = SLOTS + ("_mlp_grads", "_mlp_optim")
    for slot in held:
        assert getattr(agent, slot) is None
        setattr(agent, slot, _StubHandle())
    state = agent.__getstate__()
    twin = copy.deepcopy(agent)
    for slot in held:
        assert state[slot] is None and getattr(twin, slot) is None
        assert isinstance(getattr(agent, slot), _StubHandle)           # the original keeps its own
    assert not any(isinstance(v, _StubHandle) for v in state.values())
    for name, (attr, _, _) in SWITCHES.items():
        assert getattr(twin, attr) is getattr(agent, attr)
    assert list(twin.state_dict().keys()) == list(agent.state_dict().keys())
