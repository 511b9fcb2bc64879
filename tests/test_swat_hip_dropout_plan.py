"""Host side of the SWAT HIP chain's dropout entries (no GPU): `swat_hip.dropout_site_plan()` against the sites the modules really
take, `train_ops.DropoutRng.reserve`, the `swat_hip_dropout` switch of td3.Agent, and the cases GraphedUpdates still refuses."""
import pytest
import torch

from sgrl_amd import graph as G, mjcf, swat_hip, train_ops
from sgrl_amd.set_policy import default_args
from sgrl_amd.swat_policy import _model
from sgrl_amd.td3 import Agent, GraphedUpdates, default_train_args
import sgrl_amd.td3 as td3

TRAV = ["pre", "inlcrs", "postlcrs"]
MORPHS = {3: "3d_walker_3_left_knee_right_knee", 7: "3d_walker_7_full"}


def _graph(L, dtype=torch.float32):
    g = dict(G.getGraphDict(mjcf.load_asset(MORPHS[L]).parents, TRAV, [], device=torch.device("cpu")))
    g["relation"] = g["relation"].to(dtype)
    return g


@pytest.fixture
def recorded(monkeypatch):
    """Every train_ops._counter_dropout call as (site, shape)."""
    calls = []
    inner = train_ops._counter_dropout

    def recording(x, p, rng, site):
        calls.append((site, tuple(x.shape)))
        return inner(x, p, rng, site)

    monkeypatch.setattr(train_ops, "_counter_dropout", recording)
    return calls


def _plan_shapes(B, L):
    return [shape(B, L) for _, _, shape in swat_hip.dropout_site_plan()]


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
def test_plan_is_thirteen_rows_in_the_layers_order():
    plan = swat_hip.dropout_site_plan()
    assert len(plan) == swat_hip.SITES_PER_NET == 13
    assert [(k, l) for k, l, _ in plan] == [("pos", None)] + [(k, l) for l in range(3) for k in ("attn", "dropout1", "dropout", "dropout2")]


@pytest.mark.parametrize("B,L", [(2, 3), (3, 7)])
@pytest.mark.parametrize("feature,out", [(41, 3), (44, 1)])
def test_plan_is_what_a_network_in_training_mode_takes(recorded, B, L, feature, out):
    """A float32 CPU actor net (41 -> 3) and a critic net (44 -> 1) in training mode with dropout 0.1 under dropout_rng: the 13
    recorded (site, shape) rows are the plan's, numbered from the context's running site."""
    torch.manual_seed(L)
    net = _model(feature, out, default_args(dropout_rate=0.1)).train()
    x = torch.randn(B, L, feature)
    with torch.no_grad(), train_ops.dropout_rng(5, torch.tensor([2])) as rng:
        first = rng.reserve(4)                     # the network does not start at 0: it takes the sites that are next
        net(x, _graph(L))
        assert first == 0 and rng.site == 4 + 13
    assert recorded == [(4 + k, shape) for k, shape in enumerate(_plan_shapes(B, L))]


def _cpu_agent(dtype=torch.float32, **kw):
    torch.manual_seed(0)
    agent = Agent(default_train_args(actor_type="swat", critic_type="swat", dropout_rate=0.1, seed=11), device=torch.device("cpu"), **kw)
    if dtype == torch.float64:
        agent.double()
    agent.change_morphology(_graph(3, dtype))
    return agent


def _batch(L, B, dtype):
    gen = torch.Generator().manual_seed(B)
    r = lambda *s: torch.rand(s, generator=gen)
    batch = {"obs": torch.randn((B, 41 * L), generator=gen), "next_obs": torch.randn((B, 41 * L), generator=gen),
             "action": r(B, 3 * L) * 2 - 1, "reward": r(B, 1) * 2 - 1, "done": (r(B, 1) < 0.3).float()}
    return {k: v.to(dtype) for k, v in batch.items()}, (torch.randn((B, 3 * L), generator=gen) * 0.4).to(dtype)


def test_update_targets_takes_39_sites_actor_critic1_critic2(recorded):
    """A full Agent.update_targets on a float64 CPU agent: three networks of 13 sites in the chain's order -- the numbers
    HipSwatTargets.target_q(dropout=(..., site0)) gives its three networks."""
    B, L = 4, 3
    agent = _cpu_agent(torch.float64)
    agent.models2train()
    batch, noise = _batch(L, B, torch.float64)
    seen = []
    for name, net in (("actor", agent.actor_target.actor), ("critic1", agent.critic_target.critic1), ("critic2", agent.critic_target.critic2)):
        net.register_forward_pre_hook(lambda m, a, name=name: seen.append((name, train_ops._rng.site)))
    with train_ops.dropout_rng(5, torch.tensor([2])) as rng:
        agent.update_targets(batch, noise)
        assert rng.site == 39
    assert seen == [("actor", 0), ("critic1", 13), ("critic2", 26)]
    assert recorded == [(13 * n + k, shape) for n in range(3) for k, shape in enumerate(_plan_shapes(B, L))]


# ---- DropoutRng.reserve -------------------------------------------------------------------------------------------------------------
def test_reserve_returns_the_running_site_and_advances():
    rng = train_ops.DropoutRng(3, torch.tensor([0]))
    assert [rng.next_site(), rng.next_site()] == [0, 1]
    assert rng.reserve(39) == 2 and rng.site == 41
    assert rng.reserve(0) == 41 and rng.site == 41
    assert [rng.next_site(), rng.next_site()] == [41, 42]
    with train_ops.dropout_rng(3, torch.tensor([0])) as ctx:
        assert ctx.reserve(13) == 0
        y = train_ops.dropout(torch.ones(8), 0.5)            # the next call numbers itself behind the reserved block
        assert ctx.site == 14
    with train_ops.dropout_rng(3, torch.tensor([0])) as ctx:
        want = train_ops._counter_dropout(torch.ones(8), 0.5, ctx, 13)
    assert torch.equal(y, want)


# ---- the switch ---------------------------------------------------------------------------------------------------------------------
def test_switch_defaults_off_and_follows_argument_then_args():
    assert td3.SWAT_HIP_DROPOUT_DEFAULT is False
    mk = lambda kw=None, **over: Agent(default_train_args(actor_type="swat", critic_type="swat", dropout_rate=0.1, **over),
                                       device=torch.device("cpu"), **(kw or {}))
    assert mk().swat_hip_dropout is False
    assert mk(dict(swat_hip_dropout=True)).swat_hip_dropout is True
    assert mk(swat_hip_dropout=True).swat_hip_dropout is True                      # args.swat_hip_dropout
    assert mk(dict(swat_hip_dropout=False), swat_hip_dropout=True).swat_hip_dropout is False      # the argument wins
    assert mk(dict(swat_hip_dropout=True, use_hip=False)).swat_hip_dropout is False               # follows use_hip


@pytest.mark.parametrize("atype,over", [("set", {}), ("smp", dict(td=True, bu=True)), ("mlp", dict(mlp_num_limbs=3))])
def test_switch_is_ignored_by_the_other_agent_types(atype, over):
    agent = Agent(default_train_args(actor_type=atype, critic_type=atype, dropout_rate=0.1, swat_hip_dropout=True, **over),
                  device=torch.device("cpu"), swat_hip_dropout=True)
    assert agent.swat_hip_dropout is False and not agent.use_swat_hip


def test_cpu_agent_with_the_switch_takes_the_module_path(recorded):
    on, off = _cpu_agent(swat_hip_dropout=True), _cpu_agent()
    assert on.swat_hip_dropout and not off.swat_hip_dropout
    off.load_state_dict(on.state_dict())
    batch, noise = _batch(3, 4, torch.float32)
    outs = []
    for agent in (on, off):
        agent.models2train()
        assert agent._hip_targets(batch["next_obs"]) is None
        del recorded[:]
        with train_ops.dropout_rng(5, torch.tensor([2])):
            outs.append(agent.update_targets(batch, noise)[1])
        assert [s for s, _ in recorded] == list(range(39))
    assert torch.equal(outs[0], outs[1])


# ---- GraphedUpdates ------------------------------------------------------------------------------------------------------------------
def test_graphed_updates_still_refuse_what_they_refused():
    for hip_kernels in (False, True):                          # a dropout agent without the switch: the error naming dropout
        with pytest.raises(NotImplementedError, match="dropout"):
            GraphedUpdates(_cpu_agent(), 6, hip_kernels=hip_kernels)
    with pytest.raises(NotImplementedError, match="dropout"):  # the switch without hip_kernels: the targets would run the modules
        GraphedUpdates(_cpu_agent(swat_hip_dropout=True), 6, hip_kernels=False)
    with pytest.raises(RuntimeError, match="on the GPU"):      # a CPU agent, dropout or not
        GraphedUpdates(_cpu_agent(swat_hip_dropout=True), 6, hip_kernels=True)
    torch.manual_seed(0)
    plain = Agent(default_train_args(actor_type="swat", critic_type="swat"), device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="on the GPU"):
        GraphedUpdates(plain, 6, hip_kernels=True)
