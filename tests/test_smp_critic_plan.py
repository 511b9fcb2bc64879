"""Host side of the HIP SMP critic forward and TD3 target chain (sgrl_amd/smp_hip.py plan_critic_params / HipSmpCritic /
HipSmpTargets, include/sgrl_smp.h): the parameter plan the C ABI binds against the executed reference's key list and against the
header's slot enum, the exported symbols, the refusals on the host, td3.Agent's dispatch, and the MEANING of plan and schedule: a
NumPy float64 evaluation that walks nothing but level_schedule's rows and reads the weights in plan order -- raw (not tanh'd) head
inputs in the column order [up | action | parent message slot], the two 67-wide first layers staged into one zero-padded
[800, 80] matrix as csrc/smp_actor.hip does, the sum over the limbs -- reproduces the q1 / q2 of the executed reference."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from sgrl_amd import _lib, mjcf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QK = 80           # row stride of the staged first layer (csrc/smp_actor.hip)


def _critic(mc=3, td=True, bu=True, state_dim=41, action_dim=3, msg_dim=32):
    from sgrl_amd.smp_policy import CriticGraphPolicy
    return CriticGraphPolicy(state_dim, action_dim, msg_dim, 1, mc, True, td, bu, None)


@pytest.mark.parametrize("mc", [3, 5])
def test_plan_covers_every_critic_parameter_once(mc, golden_dir):
    from sgrl_amd.smp_hip import plan_critic_params
    crit = _critic(mc)
    plan = plan_critic_params(crit)
    names = [n for n, _ in plan]
    assert len(names) == len(set(names)) == 24
    params = dict(crit.named_parameters())
    assert sorted(names) == sorted(params)
    for n, shape in plan:
        assert tuple(params[n].shape) == tuple(shape), n
    with open(os.path.join(golden_dir, "smp_state_dict_keys.json")) as f:
        keys = json.load(f)
    # the executed reference lists the one shared module once per limb (sNet.<i>. / critic.<i>.): map the listing to index 0
    gold = {}
    for k, s in keys["critic_td1_bu1"].items():
        k0 = re.sub(r"^(sNet|critic)\.\d+\.", r"\1.0.", k)
        assert gold.setdefault(k0, s) == s
    gmc = keys["max_children"]
    mcdim = lambda d: {32 * gmc: 32 * mc, 64 + 32 * gmc: 64 + 32 * mc}.get(d, d)
    assert {n: list(s) for n, s in plan} == {k: [mcdim(d) for d in s] for k, s in gold.items()}


def test_plan_order_matches_the_critic_slot_enum_of_the_header():
    from sgrl_amd.smp_hip import plan_critic_params
    text = open(os.path.join(REPO, "include", "sgrl_smp.h")).read()
    enum = re.search(r"enum \{\s*SGRL_SMPQ_FC1_W = 0,(.*?)SGRL_SMPQ_NW", text, re.S).group(0)
    names = re.findall(r"/\* ([A-Za-z_.0-9]+) \[", enum)
    assert len(names) == 24
    assert [n for n, _ in plan_critic_params(_critic(5))] == names
    # the actor's enum is still there, with its own count
    assert re.search(r"enum \{\s*SGRL_SMP_FC1_W = 0,(.*?)SGRL_SMP_NW\s*\};", text, re.S)


def test_library_exports_every_new_symbol():
    so = ctypes.CDLL(_lib.build())
    text = open(os.path.join(REPO, "include", "sgrl_smp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sgrl_[a-z0-9_]+)\s*\(", text))
    new = {"sgrl_smp_bind_critic_params", "sgrl_smp_forward_q", "sgrl_smp_td_target", "sgrl_smp_forward_q_launches",
           "sgrl_smp_td_target_launches"}
    assert new <= declared
    for n in new:
        assert hasattr(so, n), n


def test_td_only_mode_and_other_sizes_are_refused_on_the_host():
    from sgrl_amd.smp_hip import plan_critic_params
    with pytest.raises(_lib.SgrlError, match="td and bu"):
        plan_critic_params(_critic(3, td=True, bu=False))
    with pytest.raises(_lib.SgrlError, match="32 and hidden sizes 64 / 400 / 300"):
        plan_critic_params(_critic(3, msg_dim=16))
    crit = _critic(3)
    crit.critic[0].baseQ1.l2 = torch.nn.Linear(400, 256)
    with pytest.raises(_lib.SgrlError, match="400 / 300"):
        plan_critic_params(crit)
    with pytest.raises(_lib.SgrlError, match="max_children"):
        plan_critic_params(_critic(9))
    with pytest.raises(_lib.SgrlError, match="inputs per limb"):
        plan_critic_params(_critic(3, state_dim=62, action_dim=3))
    plan_critic_params(_critic(8))


def test_agent_picks_the_chain_for_smp_and_smp_with_td_and_bu_only():
    from sgrl_amd.td3 import Agent, default_train_args

    def flags(use_hip=True, **over):
        a = Agent(default_train_args(**over), use_hip=use_hip)
        assert a._targets is None
        return a.use_smp_hip, a.use_swat_hip, a

    smp = dict(actor_type="smp", critic_type="smp")
    on, swat, agent = flags(td=True, bu=True, **smp)
    assert on and not swat
    assert flags(td=True, bu=False, **smp)[:2] == (False, False)                    # the td-only mode
    assert flags(use_hip=False, td=True, bu=True, **smp)[:2] == (False, False)
    assert flags(actor_type="smp", critic_type="swat", td=True, bu=True)[:2] == (False, False)
    assert flags(actor_type="swat", critic_type="smp", td=True, bu=True)[:2] == (False, False)
    assert flags(actor_type="swat", critic_type="swat")[:2] == (False, True)
    assert flags()[:2] == (False, False)                                            # SET
    # a CPU batch never reaches a handle, whatever the flag says; cached handles are not part of a pickled / copied agent
    assert agent._hip_targets(torch.zeros((2, 41))) is None
    agent._targets = object()
    assert agent.__getstate__()["_targets"] is None
    agent.actor_target._smp_hip = object()
    assert agent.actor_target.__getstate__()["_smp_hip"] is None
    agent.actor_target._smp_hip = agent._targets = None


# ---- the meaning of plan + schedule ---------------------------------------------------------------------------------------
def _normalize(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12)


def _eval_critic(rows, plan, w, obs, act, mc):
    """CriticGraphPolicy.forward in float64 from the rows of level_schedule (level | parent | slot | children) and the tensors
    `w` in PLAN order (a list, indexed like the C ABI's slots): obs [B, 41 L], act [B, 3 L] -> q1, q2 [B, 1]."""
    slot_of = {n: i for i, (n, _) in enumerate(plan)}
    W = lambda name: w[slot_of[name]]
    lin = lambda name, x: x @ W(name + ".weight").T + W(name + ".bias")
    mlp = lambda base, x: lin(base + ".l3", np.maximum(lin(base + ".l2", np.maximum(lin(base + ".l1", x), 0)), 0))
    L, B = len(rows), obs.shape[0]
    level, par, slot, ch = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:]
    x, u = obs.reshape(B, L, 41), act.reshape(B, L, 3)
    up = np.zeros((L, B, 32))
    for d in range(level.max(), -1, -1):
        for i in np.nonzero(level == d)[0]:
            m = np.concatenate([up[c] if c >= 0 else np.zeros((B, 32)) for c in ch[i]], axis=-1)
            xu = np.concatenate([x[:, i], u[:, i]], axis=-1)                               # fc1 over [obs 41 | action 3]
            h = np.tanh(np.concatenate([_normalize(lin("sNet.0.fc1", xu)), m], axis=-1))
            up[i] = _normalize(lin("sNet.0.fc3", np.tanh(lin("sNet.0.fc2", h))))
    # the two 67-wide first layers as ONE zero-padded [800, 80] matrix, the head inputs as zero-padded 80-wide rows
    wq = np.zeros((800, QK))
    wq[:400, :67], wq[400:, :67] = W("critic.0.baseQ1.l1.weight"), W("critic.0.baseQ2.l1.weight")
    bq = np.concatenate([W("critic.0.baseQ1.l1.bias"), W("critic.0.baseQ2.l1.bias")])
    down = np.zeros((L, B, 32 * mc))
    q = np.zeros((2, B))
    for d in range(level.max() + 1):
        for i in np.nonzero(level == d)[0]:
            dm = down[par[i]][:, 32 * slot[i]:32 * slot[i] + 32] if par[i] >= 0 else np.zeros((B, 32))
            down[i] = _normalize(mlp("critic.0.msg_base", np.tanh(np.concatenate([up[i], dm], axis=-1))))
            xq = np.zeros((B, QK))
            xq[:, 0:32], xq[:, 32:35], xq[:, 35:67] = up[i], u[:, i], dm                  # RAW values, no tanh
            h1 = np.maximum(xq @ wq.T + bq, 0)                                              # [B, 800]
            for k, head in enumerate(("critic.0.baseQ1", "critic.0.baseQ2")):
                h2 = np.maximum(lin(head + ".l2", h1[:, 400 * k:400 * k + 400]), 0)
                q[k] += lin(head + ".l3", h2)[:, 0]                                          # limbs in order 0 .. L - 1
    return q[0][:, None], q[1][:, None]


def test_plan_and_schedule_rows_alone_reproduce_the_reference_q_values(golden_dir):
    from oracle.formula import apply_formula_
    from sgrl_amd.smp_hip import level_schedule, plan_critic_params
    with open(os.path.join(golden_dir, "smp_state_dict_keys.json")) as f:
        mc = json.load(f)["max_children"]
    z = np.load(os.path.join(golden_dir, "smp_forward.npz"))
    names = sorted({k.split("/")[1] for k in z.files if k.startswith("td1_bu1/")})
    assert len(names) == 5
    crit = _critic(mc)
    plan = plan_critic_params(crit)
    sch = level_schedule([mjcf.load_asset(n).parents for n in names], mc)
    for k, name in enumerate(names):
        # the formula keys a value on the parameter's state_dict name and the shared module is listed once per limb: the weights
        # behind a stored value are those written with THIS morphology's listing (see the header of tests/test_smp_hip_gpu.py)
        crit.change_morphology({"parents": list(mjcf.load_asset(name).parents)})
        apply_formula_(crit)
        sd = crit.state_dict()
        w = [sd[n].double().numpy() for n, _ in plan]
        rows = sch["tree"][sch["offset"][k]:sch["offset"][k] + sch["L"][k]]
        tag = "td1_bu1/%s/" % name
        got = _eval_critic(rows, plan, w, z[tag + "obs"].astype(np.float64), z[tag + "act_in"].astype(np.float64), mc)
        for g, key in zip(got, ("q1", "q2")):
            want = z[tag + key]
            bound = 1e-5 * max(1.0, float(np.abs(want).max()))
            err = float(np.abs(g - want).max())
            print("%s %s: max|q| %.3g, |plan + schedule float64 - reference f32| = %.3g (bound %.3g)"
                  % (name, key, float(np.abs(want).max()), err, bound))
            assert g.shape == want.shape and err <= bound, (name, key, err, bound)
