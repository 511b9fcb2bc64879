"""The SWAT update on the training kernels, the parts that need no GPU: the NumPy restatement of the attention kernels
(tests/swat_attn_restate.py) against float64 autograd, train_ops.swat_attention's fallback, the `train_kernels` switch of
swat_policy (it changes no bit where the kernels do not run) and td3.Agent's `swat_train_kernels` plumbing."""
import copy
import json
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import swat_attn_restate as R
from oracle.formula import apply_formula_
from sgrl_amd import graph as G, mjcf, td3, train_ops
from sgrl_amd.set_policy import default_args
from sgrl_amd.swat_policy import CriticStructurePolicy, StructurePolicy, _SelfAttention
from sgrl_amd.td3 import Agent, default_train_args

TRAV = ["pre", "inlcrs", "postlcrs"]
SCALE = 64 ** -0.5


def _core(qkv, bias, scale=SCALE, H=2):
    """swat_policy._SelfAttention.forward between in_proj and out_proj, line for line."""
    B, L = qkv.shape[:2]
    E = qkv.shape[-1] // 3
    hd = E // H
    q, k, v = qkv.chunk(3, dim=-1)
    q = (q * scale).view(B, L, H, hd)
    k, v = k.view(B, L, H, hd), v.view(B, L, H, hd)
    s = torch.einsum("bihd,bjhd->bhij", q, k)
    if bias is not None:
        s = s + bias.unsqueeze(0)
    w = F.softmax(s, dim=-1)
    return torch.einsum("bhij,bjhd->bihd", w, v).reshape(B, L, E), w


def test_the_copied_core_is_the_modules():
    torch.manual_seed(0)
    att = _SelfAttention(128, 2)
    with torch.no_grad():
        att.in_proj_bias.normal_()
    x, bias = torch.randn(5, 7, 128), torch.randn(2, 7, 7)
    for bz in (bias, None):
        o, _ = _core(F.linear(x, att.in_proj_weight, att.in_proj_bias), bz, float(64) ** -0.5)
        assert torch.equal(att.out_proj(o), att(x, bz))


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("L", [1, 2, 7, 15])
def test_restatement_against_float64_autograd(L, with_bias):
    torch.manual_seed(10 * L + with_bias)
    B = 23
    qkv = (torch.randn(B, L, 384, dtype=torch.float64) * 0.6).requires_grad_()
    bias = torch.randn(2, L, L, dtype=torch.float64).requires_grad_() if with_bias else None
    d_o = torch.randn(B, L, 128, dtype=torch.float64)
    o, w = _core(qkv, bias)
    w.retain_grad()
    (o * d_o).sum().backward()
    w_r, o_r = R.forward(qkv.detach().numpy(), None if bias is None else bias.detach().numpy(), SCALE)
    dqkv_r, ds_r = R.backward(qkv.detach().numpy(), SCALE, w_r, d_o.numpy())
    assert w_r.shape == (B, 2, L, L) and o_r.shape == (B, L, 128) and dqkv_r.shape == (B, L, 384) and ds_r.shape == (B, 2, L, L)
    assert np.abs(w_r - w.detach().numpy()).max() < 1e-12
    assert np.abs(o_r - o.detach().numpy()).max() < 1e-12
    assert np.abs(dqkv_r - qkv.grad.numpy()).max() < 1e-12
    if with_bias:
        assert np.abs(ds_r.sum(0) - bias.grad.numpy()).max() < 1e-12
    if L == 1:
        assert (w_r == 1).all() and (ds_r == 0).all()
        assert (dqkv_r[..., :256] == 0).all() and np.array_equal(dqkv_r[..., 256:], d_o.numpy())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_swat_attention_on_the_cpu_is_the_modules_code_bit_for_bit(dtype):
    for L, with_bias in ((1, True), (7, True), (7, False), (15, True), (16, True)):
        torch.manual_seed(L)
        qkv0 = torch.randn(9, L, 384, dtype=dtype) * 0.6
        bias0 = torch.randn(2, L, L, dtype=dtype) if with_bias else None
        d_o = torch.randn(9, L, 128, dtype=dtype)
        got = []
        for fn in (lambda q, b: train_ops.swat_attention(q, b, SCALE), lambda q, b: _core(q, b)[0]):
            q = qkv0.clone().requires_grad_()
            b = None if bias0 is None else bias0.clone().requires_grad_()
            o = fn(q, b)
            assert type(o.grad_fn).__name__ != "_SwatAttnFnBackward"
            (o * d_o).sum().backward()
            got.append((o.detach(), q.grad, None if b is None else b.grad))
        for a, c in zip(*got):
            assert (a is None and c is None) or torch.equal(a, c)


def _pair(cond, tnorm, seed=0):
    args = default_args(condition_decoder_on_features=cond, transformer_norm=tnorm)
    torch.manual_seed(seed)
    pol = StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False, args).eval()
    crit = CriticStructurePolicy(41, 3, 32, 1, 3, True, False, False, args).eval()
    return pol, crit


def _graph(name):
    m = mjcf.load_asset(name)
    return m, G.getGraphDict(m.parents, TRAV, [], device=torch.device("cpu"))


def _switch_is_everywhere(mod, on):
    seen = [m.train_kernels for m in mod.modules() if hasattr(type(m), "train_kernels")]
    return len(seen) >= 1 + 1 + 1 + 3 * 2 and all(s is on for s in seen)      # policy, model, encoder, 3 x (layer, attention)


@pytest.mark.parametrize("tnorm", [0, 1])
@pytest.mark.parametrize("cond", [0, 1])
def test_the_switch_changes_no_bit_on_the_cpu(cond, tnorm, golden_dir):
    pol, crit = _pair(cond, tnorm)
    with torch.no_grad():
        for mod in (pol, crit):                   # biases away from their zero initial values
            for n, p in mod.named_parameters():
                if n.endswith("bias"):
                    p.normal_(0, 0.1)
    assert pol.train_kernels is False and crit.train_kernels is False and _switch_is_everywhere(pol, False)
    on_pol, on_crit = copy.deepcopy(pol), copy.deepcopy(crit)
    on_pol.train_kernels = True
    on_crit.train_kernels = True
    assert _switch_is_everywhere(on_pol, True) and _switch_is_everywhere(on_crit, True) and _switch_is_everywhere(pol, False)
    assert on_crit.critic1.train_kernels and on_crit.critic2.transformer_encoder.layers[2].self_attn.train_kernels
    # not a parameter, not in the state_dict, kept by pickle and deepcopy
    for on, off in ((on_pol, pol), (on_crit, crit)):
        assert list(on.state_dict().keys()) == list(off.state_dict().keys())
        assert [n for n, _ in on.named_parameters()] == [n for n, _ in off.named_parameters()]
        assert not any("train_kernels" in k for k in on.state_dict())
        assert _switch_is_everywhere(copy.deepcopy(on), True) and _switch_is_everywhere(pickle.loads(pickle.dumps(on)), True)
        assert _switch_is_everywhere(pickle.loads(pickle.dumps(off)), False)
    if tnorm == 1:                                # the fixtures' setting
        with open(os.path.join(golden_dir, "swat_state_dict_keys.json")) as f:
            keys = json.load(f)
        assert {k: list(v.shape) for k, v in on_pol.state_dict().items()} == keys["actor_cond%d" % cond]
        assert {k: list(v.shape) for k, v in on_crit.state_dict().items()} == keys["critic_cond%d" % cond]
    for name in ("3d_walker_2_right_leg_left_knee", "3d_walker_7_full", "3d_cheetah_14_full"):
        m, gd = _graph(name)
        L = m.num_limbs
        torch.manual_seed(L)
        obs0, act0 = torch.randn(5, 41 * L), torch.rand(5, 3 * L) * 2 - 1
        pa, pq = torch.randn(5, 3 * L), torch.randn(5, L)
        res = []
        for p, c in ((pol, crit), (on_pol, on_crit)):
            p.change_morphology(gd)
            c.change_morphology(gd)
            p.zero_grad()
            c.zero_grad()
            obs, act = obs0.clone().requires_grad_(), act0.clone().requires_grad_()
            a = p(obs)
            q1, q2 = c(obs, act)
            q1b = c.Q1(obs, a)
            ((a * pa).sum() + (q1 * pq).sum() - (q2 * pq).sum() + (q1b * pq).sum()).backward()
            res.append([a.detach(), q1.detach(), q2.detach(), q1b.detach(), obs.grad, act.grad] +
                       [t.grad for t in p.parameters()] + [t.grad for t in c.parameters()])
        assert len(res[0]) == len(res[1]) and all(g is not None for g in res[0])
        for x, y in zip(*res):
            assert torch.equal(x, y)


@pytest.mark.parametrize("cond", [0, 1])
def test_the_reference_fixtures_hold_with_the_switch_on(cond, golden_dir):
    z = np.load(os.path.join(golden_dir, "swat_forward.npz"))
    pol, crit = _pair(cond, 1)
    apply_formula_(pol)
    apply_formula_(crit)
    pol.train_kernels = True
    crit.train_kernels = True
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("cond%d/" % cond)})
    assert len(names) == 5
    for name in names:
        m, gd = _graph(name)
        pol.change_morphology(gd)
        crit.change_morphology(gd)
        tag = "cond%d/%s/" % (cond, name)
        obs, act = torch.from_numpy(z[tag + "obs"]), torch.from_numpy(z[tag + "act_in"])
        a = pol(obs)                              # autograd recording, as in an update
        q1, q2 = crit(obs, act)
        np.testing.assert_allclose(a.detach().numpy(), z[tag + "action"], atol=2e-6)
        scale = max(1.0, np.abs(z[tag + "q1"]).max())
        np.testing.assert_allclose(q1.detach().numpy(), z[tag + "q1"], atol=1e-5 * scale)
        np.testing.assert_allclose(q2.detach().numpy(), z[tag + "q2"], atol=1e-5 * scale)


def _swat_agent(seed=3, **kw):
    torch.manual_seed(seed)
    return Agent(default_train_args(actor_type="swat", critic_type="swat"), **kw)


def _online(agent):
    return agent.actor.train_kernels, agent.critic.train_kernels


def _targets(agent):
    return agent.actor_target.train_kernels, agent.critic_target.train_kernels


def test_agent_plumbing():
    assert td3.SWAT_TRAIN_KERNELS_DEFAULT is False
    a = _swat_agent()
    assert a.use_swat_train_kernels is False and _online(a) == (False, False) and _targets(a) == (False, False)
    a = _swat_agent(swat_train_kernels=True)
    assert a.use_swat_train_kernels is True and _online(a) == (True, True) and _targets(a) == (False, False)
    assert _switch_is_everywhere(a.actor, True) and _switch_is_everywhere(a.critic, True)
    assert _switch_is_everywhere(a.actor_target, False) and _switch_is_everywhere(a.critic_target, False)
    a = Agent(default_train_args(actor_type="swat", critic_type="swat", swat_train_kernels=None), swat_train_kernels=None)
    assert a.use_swat_train_kernels is False               # None in both places: the module default
    a = Agent(default_train_args(actor_type="swat", critic_type="swat", swat_train_kernels=True))
    assert a.use_swat_train_kernels is True and _online(a) == (True, True) and _targets(a) == (False, False)
    a = Agent(default_train_args(actor_type="swat", critic_type="swat", swat_train_kernels=True), swat_train_kernels=False)
    assert a.use_swat_train_kernels is False and _online(a) == (False, False)      # the keyword wins
    a = _swat_agent(swat_train_kernels=True, use_hip=False)
    assert a.use_swat_train_kernels is False and _online(a) == (False, False)      # follows use_hip
    for b in (copy.deepcopy(_swat_agent(swat_train_kernels=True)), pickle.loads(pickle.dumps(_swat_agent(swat_train_kernels=True)))):
        assert b.use_swat_train_kernels is True and _online(b) == (True, True) and _targets(b) == (False, False)
    # the other agent types ignore it
    for over in ({}, {"actor_type": "smp", "critic_type": "smp", "td": True, "bu": True, "max_children": 5},
                 {"actor_type": "mlp", "critic_type": "mlp", "mlp_num_limbs": 7}, {"actor_type": "swat", "critic_type": "set"}):
        b = Agent(default_train_args(swat_train_kernels=True, **over), swat_train_kernels=True)
        assert b.use_swat_train_kernels is False
        assert not any(getattr(m, "train_kernels", False) for net in (b.actor, b.critic, b.actor_target, b.critic_target) for m in net.modules())


@pytest.mark.parametrize("skip", [False, True])
def test_a_cpu_update_with_the_switch_on_equals_the_switch_off(skip):
    from oracle.formula import synth_obs
    m, gd = _graph("3d_walker_5_foot")
    B, L = 6, m.num_limbs
    torch.manual_seed(5)
    batch = {"obs": torch.from_numpy(synth_obs(L, B, 1).astype(np.float32)), "next_obs": torch.from_numpy(synth_obs(L, B, 2).astype(np.float32)),
             "action": torch.rand(B, 3 * L) * 2 - 1, "reward": torch.randn(B, 1), "done": torch.zeros(B, 1)}
    noise = torch.randn(B, 3 * L) * 0.2
    off = _swat_agent(seed=8)
    on = _swat_agent(seed=9, swat_train_kernels=True)
    on.load_state_dict(off.state_dict())
    outs = []
    for agent in (off, on):
        agent.change_morphology(gd)
        agent.models2train()
        outs.append([agent.update(batch, it, noise=noise, skip_unused_critic_grads=skip) for it in range(2)])
    assert _online(on) == (True, True) and _online(off) == (False, False)
    for o_off, o_on in zip(*outs):
        assert o_off.keys() == o_on.keys()
        for k in o_off:
            assert torch.equal(torch.as_tensor(o_off[k]), torch.as_tensor(o_on[k])), k
    assert "loss/actor_loss" in outs[0][0]
    sd_off, sd_on = off.state_dict(), on.state_dict()
    assert sd_off.keys() == sd_on.keys()
    for k in sd_off:
        assert torch.equal(sd_off[k], sd_on[k]), k
