"""dropout_rate on the SWAT networks (sgrl_amd/swat_policy.py, train_ops.dropout / dropout_rng, td3.Agent), the parts that need no
GPU: the modules honour the rate in training mode only, the PyTorch path under a dropout_rng context draws the masks of the
counter-RNG definition (tests/dropout_restate.py) at every site, the keep rate, the executed reference (tests/golden/swat_dropout.npz,
tools/capture_golden_swat_dropout.py), the refusal of graphed updates and the untouched paths of an agent without dropout."""
import os

import numpy as np
import pytest
import torch

import dropout_restate as R
from oracle.formula import apply_formula_
from sgrl_amd import graph as G, mjcf, train_ops
from sgrl_amd.set_policy import default_args
from sgrl_amd.swat_policy import CriticStructurePolicy, StructurePolicy

TRAV = ["pre", "inlcrs", "postlcrs"]
SITES_PER_NET = 1 + 4 * 3            # the position embedding, then four per encoder layer


def _graph(name, dtype=torch.float32):
    g = G.getGraphDict(mjcf.load_asset(name).parents, TRAV, [], device=torch.device("cpu"))
    if dtype == torch.float64:
        g = dict(g)
        g["relation"] = g["relation"].double()
    return g


def _policy(p, name="3d_walker_7_full"):
    pol = StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False, default_args(dropout_rate=p))
    apply_formula_(pol)
    pol.change_morphology(_graph(name))
    return pol


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
def test_policy_honours_dropout_rate_in_training_mode_only():
    pol, plain = _policy(0.5), _policy(0.0)
    assert list(pol.state_dict().keys()) == list(plain.state_dict().keys())            # no parameter, no buffer
    x = torch.randn(4, 41 * 7, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = plain.eval()(x).clone()
        assert torch.equal(plain.train()(x), want)                                     # rate 0: training mode changes nothing
        assert torch.equal(pol.eval()(x), want)                                        # eval: the rate-0 module bit for bit
        torch.manual_seed(2)
        got = pol.train()(x).clone()
    assert float((got - want).abs().max()) > 1e-3
    for kernels in (False, True):                                                      # both paths of the module get the dropouts
        pol.train_kernels = kernels
        with torch.no_grad(), train_ops.dropout_rng(5, torch.tensor([9])):
            a = pol(x).clone()
        assert float((a - want).abs().max()) > 1e-3
    pol.train_kernels = False


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", [("3d_walker_3_left_knee_right_knee", 3), ("3d_walker_7_full", 7)])
def test_fallback_masks_are_the_restatement_at_every_site(monkeypatch, name, L):
    """Every dropout call of a float64 actor and critic network under dropout_rng is recorded (input, output, site) and recomputed
    by the restatement from (seed, step, site) alone: equal bit for bit, at the reference's sites and shapes, in their order."""
    p, seed, step, B = 0.1, 0x1234567890ABCDEF, 3, 5
    calls = []
    inner = train_ops._counter_dropout

    def recording(x, p_, rng, site):
        y = inner(x, p_, rng, site)
        calls.append((site, float(p_), x.detach().clone(), y.detach().clone()))
        return y

    monkeypatch.setattr(train_ops, "_counter_dropout", recording)
    args = default_args(dropout_rate=p)
    pol = StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False, args).double().train()
    crit = CriticStructurePolicy(41, 3, 32, 1, 3, True, False, False, args).double().train()
    g = _graph(name, torch.float64)
    pol.change_morphology(g)
    crit.change_morphology(g)
    gen = torch.Generator().manual_seed(L)
    obs = torch.randn(B, 41 * L, generator=gen, dtype=torch.float64)
    act = torch.rand(B, 3 * L, generator=gen, dtype=torch.float64) * 2 - 1
    before = dict(train_ops.dropout_calls)
    with train_ops.dropout_rng(seed, torch.tensor([step])) as rng:
        out = pol(obs)
        q1 = crit.Q1(obs, act)
        assert rng.site == 2 * SITES_PER_NET
    assert train_ops.dropout_calls["counter"] - before["counter"] == 2 * SITES_PER_NET
    assert train_ops.dropout_calls["torch"] == before["torch"] and train_ops.dropout_calls["kernel"] == before["kernel"]
    shapes = [(L, 128)] + [(B, 2, L, L), (B, L, 128), (B, L, 256), (B, L, 128)] * 3
    assert [c[0] for c in calls] == list(range(2 * SITES_PER_NET))
    assert [tuple(c[2].shape) for c in calls] == shapes * 2
    for site, p_, x, y in calls:
        want = R.dropout(x.numpy(), p_, seed, step, site)
        assert np.array_equal(y.numpy(), want), site
        keep = R.keep_mask(seed, step, site, x.numel(), p_).reshape(x.shape)
        assert np.array_equal(y.numpy() != 0, keep & (x.numpy() != 0)), site
    assert torch.isfinite(out).all() and torch.isfinite(q1).all()
    # another step: other masks; the same (seed, step): the same output
    with train_ops.dropout_rng(seed, torch.tensor([step])):
        again = pol(obs)
    with train_ops.dropout_rng(seed, torch.tensor([step + 1])):
        other = pol(obs)
    assert torch.equal(again, out) and not torch.equal(other, out)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    n, seed, step, site = 2 ** 20, 77, 12, 4
    keep = R.keep_mask(seed, step, site, n, p)
    bound = 5 * np.sqrt(p * (1 - p) / n)
    assert abs(keep.mean() - (1 - p)) <= bound, (keep.mean(), bound)           # the restatement itself, for the seeds used here
    x = torch.ones(n)
    with train_ops.dropout_rng(seed, torch.tensor([step])) as rng:
        rng.site = site
        y = train_ops.dropout(x, p, True)
    assert np.array_equal(y.numpy() != 0, keep)                                # the torch restatement draws the same words
    assert abs(float((y != 0).float().mean()) - (1 - p)) <= bound
    assert np.array_equal(y.numpy(), R.dropout(np.ones(n, dtype=np.float32), p, seed, step, site))


def test_keep_rate_at_the_ends():
    n = 4099
    x = torch.randn(n, generator=torch.Generator().manual_seed(0))
    with train_ops.dropout_rng(1, torch.tensor([1])):
        assert train_ops.dropout(x, 0.0, True) is x                            # p = 0: nothing happens at all
        assert train_ops.dropout(x, 0.3, False) is x
        y1 = train_ops.dropout(x, 1.0, True)
    assert float(y1.abs().max()) == 0.0
    assert R.keep_mask(1, 1, 0, n, 0.0).all() and not R.keep_mask(1, 1, 0, n, 1.0).any()
    assert np.array_equal(R.dropout(x.numpy(), 0.0, 1, 1, 0).view(np.uint32), x.numpy().view(np.uint32))
    assert R.threshold(0.0) == 0 and R.threshold(1.0) == 2 ** 32 and R.threshold(0.5) == 2 ** 31
    # a step beyond 32 bits and a 64-bit seed reach the counter and the key whole
    big = train_ops.counter_words(2 ** 64 - 3, torch.tensor([2 ** 40 + 5]), 0x100 + 7, torch.arange(64))
    assert np.array_equal(big.numpy().astype(np.uint32), R.stream_words(2 ** 64 - 3, 2 ** 40 + 5, 0x100 + 7, 0, 64))


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
def test_switch_off_module_reproduces_the_executed_reference(golden_dir):
    """The reference's StructurePolicy and Q1 of its CriticStructurePolicy in train() with dropout_rate 0.1 on ONE walker_7 row
    (tools/capture_golden_swat_dropout.py): without a dropout_rng context the modules draw from torch's generator through
    F.dropout, and at B = 1 the reference's (N, B, d) layout and this module's [B, L, E] number the elements of every dropped
    tensor alike, so the same torch.manual_seed gives the same masks and the outputs agree to 1e-6.  For B > 1 the masks are drawn
    in THIS module's layout ([B, L, E], weights [B, H, L, L]): the same distribution, not the reference's numbers.

    The fixture is the reference run in float64 (the capture tool asserts that its float32 run draws the same masks), and the 1e-6
    is asserted on the float64 module: there rounding is nine orders below the bound on any host, while one differing mask
    element moves an output by 1e-2 or more.  A float32 run of this network differs from float64 by 3e-7 .. 1.3e-6 depending on
    the host's BLAS blocking (two hosts' float32 eval outputs were 1.25e-6 apart), so 1e-6 says nothing about masks there; the
    float32 module is held to the bars tests/test_swat_policy.py already sets for these outputs in eval mode (2e-6 on the action,
    1e-5 x max(1, |q|) on q)."""
    z = np.load(os.path.join(golden_dir, "swat_dropout.npz"))
    assert z["action"].dtype == np.float64
    args = default_args(dropout_rate=float(z["p"]))
    dev = {}
    for dtype in (torch.float64, torch.float32):
        pol = StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False, args).to(dtype).train()
        crit = CriticStructurePolicy(41, 3, 32, 1, 3, True, False, False, args).to(dtype).train()
        apply_formula_(pol)
        apply_formula_(crit)
        g = _graph("3d_walker_7_full", dtype)
        pol.change_morphology(g)
        crit.change_morphology(g)
        obs, act = torch.from_numpy(z["obs"]).to(dtype), torch.from_numpy(z["act_in"]).to(dtype)
        before = train_ops.dropout_calls["torch"]
        with torch.no_grad():
            torch.manual_seed(int(z["seed_actor"]))
            a = pol(obs).double().numpy()
            torch.manual_seed(int(z["seed_critic"]))
            q1 = crit.Q1(obs, act).double().numpy()
            a_eval, q_eval = pol.eval()(obs).double().numpy(), crit.eval().Q1(obs, act).double().numpy()
        assert train_ops.dropout_calls["torch"] - before == 2 * SITES_PER_NET
        dev[dtype] = [float(np.abs(x - z[k]).max()) for x, k in ((a, "action"), (q1, "q1"), (a_eval, "action_eval"), (q_eval, "q1_eval"))]
        print("%s: |action - ref| %.3g  |q1 - ref| %.3g  (eval: %.3g, %.3g; dropout moved the reference's outputs by %.3g, %.3g)"
              % ((dtype,) + tuple(dev[dtype]) + (np.abs(z["action"] - z["action_eval"]).max(), np.abs(z["q1"] - z["q1_eval"]).max())))
    assert all(d <= 1e-6 for d in dev[torch.float64]), dev[torch.float64]
    q_bar = 1e-5 * max(1.0, float(np.abs(z["q1"]).max()), float(np.abs(z["q1_eval"]).max()))
    d32 = dev[torch.float32]
    assert d32[0] <= 2e-6 and d32[2] <= 2e-6 and d32[1] <= q_bar and d32[3] <= q_bar, (d32, q_bar)


# ---- (e), (f) -----------------------------------------------------------------------------------------------------------------
def _agent(p, **kw):
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(0)
    agent = Agent(default_train_args(actor_type="swat", critic_type="swat", dropout_rate=p, seed=11, **kw), device=torch.device("cpu"))
    agent.change_morphology(_graph("3d_walker_3_left_knee_right_knee"))
    return agent


def _batch(L, B, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(s, generator=gen)
    return {"obs": torch.randn((B, 41 * L), generator=gen), "next_obs": torch.randn((B, 41 * L), generator=gen),
            "action": r(B, 3 * L) * 2 - 1, "reward": r(B, 1) * 2 - 1, "done": (r(B, 1) < 0.3).float()}, torch.randn((B, 3 * L), generator=gen) * 0.4


def test_graphed_updates_refuse_dropout():
    from sgrl_amd.td3 import GraphedUpdates
    with pytest.raises(NotImplementedError, match="dropout"):
        GraphedUpdates(_agent(0.1), 6)
    with pytest.raises(NotImplementedError, match="dropout"):
        GraphedUpdates(_agent(0.1), 6, hip_kernels=True)


def test_agent_without_dropout_enters_no_dropout_path():
    batch, noise = _batch(3, 6, 1)
    agent = _agent(0.0)
    agent.models2train()
    before = dict(train_ops.dropout_calls)
    for it in range(2):
        agent.update(batch, it, noise=noise)
    assert train_ops.dropout_calls == before and agent._dropout_step is None and agent.dropout_rate == 0.0
    # with a rate the same two updates run every site of every pass under the agent's context, and the step moves once per update
    agent = _agent(0.1)
    agent.models2train()
    assert agent.dropout_rate == np.float64(0.1) and agent.dropout_seed == 11
    params = [p.detach().clone() for p in agent.actor.parameters()]
    for it in range(2):
        out = agent.update(batch, it, noise=noise)
        assert all(np.isfinite(float(v)) for v in out.values())
    # it 0: target actor + two target critics + two critics + (actor, Q1); it 1: no policy step
    assert train_ops.dropout_calls["counter"] - before["counter"] == (7 + 5) * SITES_PER_NET
    assert train_ops.dropout_calls["torch"] == before["torch"] and int(agent._dropout_step) == 2 and train_ops._rng is None
    assert max(float((p.detach() - q).abs().max()) for p, q in zip(agent.actor.parameters(), params)) > 0
    # eval mode (collection, evaluation): no dropout whatever the rate
    agent.models2eval()
    mid = dict(train_ops.dropout_calls)
    agent.select_action(batch["obs"][0])
    agent.update(batch, 1, noise=noise)
    assert train_ops.dropout_calls == mid
    # an smp agent never reads the rate
    from sgrl_amd.td3 import Agent, default_train_args
    assert Agent(default_train_args(actor_type="smp", critic_type="smp", td=True, bu=True, dropout_rate=0.3), device=torch.device("cpu")).dropout_rate == 0.0
