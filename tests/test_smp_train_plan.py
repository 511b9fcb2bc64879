"""The SMP update on the training kernels, the parts that need no GPU: the NumPy restatements of the three kernel pairs
(tests/smp_train_restate.py) against float64 autograd through the module's own lines, the gather tables smp_policy builds from its
_Tree, the CPU fallbacks of train_ops.smp_gather / smp_up_tail / normalize_rows, the `train_kernels` switch of smp_policy (it changes
no bit where the kernels do not run) and td3.Agent's `smp_train_kernels` plumbing."""
import copy
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import smp_train_restate as R
from sgrl_amd import mjcf, td3, train_ops
from sgrl_amd.smp_policy import ActorGraphPolicy, ActorUp, CriticGraphPolicy, _LevelPlan, _Tree, _up_message
from sgrl_amd.td3 import Agent, default_train_args

ASSETS = ["3d_walker_7_full", "3d_humanoid_9_full", "3d_cheetah_14_full"]
FLIPPED = [-2, 0, 1, 1, 0, 4]           # a flipped structure: the message order is mirrored at the root (_Tree.slot)


def _parents(name):
    if name == "one":
        return [-1]
    if name == "chain3":
        return [-1, 0, 1]
    if name == "flipped":
        return list(FLIPPED)
    return [int(p) for p in mjcf.load_asset(name).parents]


MORPHS = ["one", "chain3", "flipped"] + ASSETS


def _mc(parents, mc):
    """max_children for a test case: the humanoid's torso has four children, so it runs at 4 where 3 is asked for."""
    return max(mc, max(parents.count(i) for i in range(len(parents))))


def _n(t):
    return t.detach().numpy()


# ---- restatements against float64 autograd -----------------------------------------------------------------------------------------
def _module_up_input(h, ups_next, children_rows, B):
    """The fc2 input of _up_message as smp_policy builds it: _bottom_up's zeros / cat / stack, then normalise, cat, tanh."""
    zero = torch.zeros((B, 32), dtype=h.dtype)
    m = torch.stack([torch.cat([ups_next[c] if c >= 0 else zero for c in row], dim=-1) for row in children_rows])
    return torch.tanh(torch.cat([F.normalize(h, dim=-1), m], dim=-1))


@pytest.mark.parametrize("mc", [1, 3, 5, 8])
def test_gather_restatement_bottom_up(mc):
    torch.manual_seed(mc)
    B, n, n_src = 5, 3, 4
    rows = [[-1] * mc, [1] + [-1] * (mc - 1), ([3, 0, 2] + [-1] * mc)[:mc]]          # all children missing / one / several
    tab = train_ops.SmpTable(rows, [[0] * mc] * n)
    h = torch.randn(n, B, 64, dtype=torch.float64).requires_grad_()
    with torch.no_grad():
        h[0, 0] = 0                                                                   # an all-zero row through the normalise
    src = torch.randn(n_src, B, 32, dtype=torch.float64).requires_grad_()
    d_out = torch.randn(n, B, 64 + 32 * mc, dtype=torch.float64)
    for s in (src, None):                                                             # None: the deepest level (null src)
        want = _module_up_input(h, s if s is not None else [None] * n_src, rows if s is not None else [[-1] * mc] * n, B)
        h.grad = None
        src.grad = None
        (want * d_out).sum().backward()
        out, inv = R.gather_forward(_n(h), None if s is None else _n(s), tab.node, tab.off, True, True)
        d_own, d_src = R.gather_backward(_n(d_out), out, _n(h), inv, None if s is None else tuple(s.shape), tab.node, tab.off, True, True)
        assert np.abs(out - _n(want)).max() < 1e-12 and np.abs(d_own[1:] - _n(h.grad)[1:]).max() < 1e-12
        assert np.abs(d_own[0, 1:] - _n(h.grad)[0, 1:]).max() < 1e-12
        assert np.abs(d_own[0, 0] - _n(h.grad)[0, 0]).max() <= 1e-12 * max(1.0, np.abs(_n(h.grad)[0, 0]).max())     # dy / 1e-12
        if s is not None:
            assert np.abs(d_src - _n(src.grad)).max() < 1e-12
            read = {c for row in rows for c in row if c >= 0}
            assert all((d_src[k] == 0).all() for k in range(n_src) if k not in read)


@pytest.mark.parametrize("mc", [1, 3, 5, 8])
def test_gather_restatement_top_down(mc):
    """tanh(cat([x, m])) of the down modules and the critic's raw m, m = the parent's slot of the previous level's messages."""
    torch.manual_seed(10 + mc)
    B, n, n_src = 4, 3, 2
    node = [[1], [-1], [0]]
    off = [[32 * (mc - 1)], [0], [0]]
    tab = train_ops.SmpTable(node, off)
    x = torch.randn(n, B, 32, dtype=torch.float64).requires_grad_()
    src = torch.randn(n_src, B, 32 * mc, dtype=torch.float64).requires_grad_()
    zero = torch.zeros((B, 32 * mc), dtype=torch.float64)
    for s in (src, None):
        ms = torch.stack([(s[a[0]] if (a[0] >= 0 and s is not None) else zero)[:, o[0]:o[0] + 32] for a, o in zip(node, off)])
        for own, act in ((x, True), (None, False)):
            want = torch.tanh(torch.cat([x, ms], dim=-1)) if own is not None else ms
            d_out = torch.randn(want.shape, dtype=torch.float64)
            x.grad = None
            src.grad = None
            if want.requires_grad:
                (want * d_out).sum().backward()
            out, _ = R.gather_forward(None if own is None else _n(x), None if s is None else _n(s), tab.node, tab.off, False, act, B=B)
            d_own, d_src = R.gather_backward(_n(d_out), out, None if own is None else _n(x), None, None if s is None else tuple(s.shape),
                                             tab.node, tab.off, False, act)
            assert np.abs(out - _n(want)).max() < 1e-12
            if own is not None:
                assert np.abs(d_own - _n(x.grad)).max() < 1e-12
            if s is not None:
                assert np.abs(d_src - _n(src.grad)).max() < 1e-12
                if mc > 1:
                    assert (d_src[0, :, 32:] == 0).all() and (d_src[1, :, :32 * (mc - 1)] == 0).all()      # columns nobody read


def test_up_tail_and_normalize_restatements():
    torch.manual_seed(3)
    mod = ActorUp(41, 32, 3).double()
    with torch.no_grad():
        mod.fc3.bias.normal_()
    R_ = 23
    a = (torch.randn(R_, 64, dtype=torch.float64) * 1.5).requires_grad_()
    du = torch.randn(R_, 32, dtype=torch.float64)
    want = F.normalize(mod.fc3(torch.tanh(a)), dim=-1)              # the last two lines of _up_message behind fc2
    (want * du).sum().backward()
    t, u, inv = R.up_tail_forward(_n(a), _n(mod.fc3.weight), _n(mod.fc3.bias))
    dz, da, dw, db = R.up_tail_backward(_n(du), u, inv, t, _n(mod.fc3.weight))
    assert np.abs(u - _n(want)).max() < 1e-12 and np.abs(da - _n(a.grad)).max() < 1e-12
    assert np.abs(dw - _n(mod.fc3.weight.grad)).max() < 1e-12 and np.abs(db - _n(mod.fc3.bias.grad)).max() < 1e-12
    # and the whole of _up_message through gather + fc2 + tail
    x, m = torch.randn(2, 5, 41, dtype=torch.float64), torch.randn(2, 5, 96, dtype=torch.float64)
    full = _up_message(mod, x, m)
    g = torch.tanh(torch.cat([F.normalize(mod.fc1(x), dim=-1), m], dim=-1))
    _, u2, _ = R.up_tail_forward(_n(mod.fc2(g)).reshape(-1, 64), _n(mod.fc3.weight), _n(mod.fc3.bias))
    assert np.abs(u2.reshape(2, 5, 32) - _n(full)).max() < 1e-12
    for W in (32, 96, 160, 256):
        xw = torch.randn(7, W, dtype=torch.float64)
        xw[2] = 0                                                   # one all-zero row
        xw.requires_grad_()
        dy = torch.randn(7, W, dtype=torch.float64)
        y = F.normalize(xw, dim=-1)
        (y * dy).sum().backward()
        y2, inv2 = R.normalize_forward(_n(xw))
        dx = R.normalize_backward(_n(dy), y2, inv2)
        assert np.abs(y2 - _n(y)).max() < 1e-12 and (y2[2] == 0).all()
        keep = [0, 1, 3, 4, 5, 6]
        assert np.abs(dx[keep] - _n(xw.grad)[keep]).max() < 1e-12
        assert np.abs(dx[2] - _n(xw.grad)[2]).max() <= 1e-12 * np.abs(_n(xw.grad)[2]).max()           # dy / 1e-12


# ---- tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MORPHS)
@pytest.mark.parametrize("mc", [3, 5])
def test_tables_follow_the_tree(name, mc):
    parents = _parents(name)
    mc = _mc(parents, mc)
    tree = _Tree(parents, mc)
    plan = _LevelPlan(tree, 32, mc)
    assert plan.fits and sorted(plan.perm) == list(range(tree.L)) and [plan.perm[k] for k in plan.inv] == list(range(tree.L))
    assert plan.sizes == [len(lv) for lv in tree.levels]
    read_up = []
    for d, lv in enumerate(tree.levels):
        up, down = plan.up[d], plan.down[d]
        assert up.node.shape == (len(lv), mc) and down.node.shape == (len(lv), 1) and up.node.dtype == np.int32
        for j, i in enumerate(lv):
            for s in range(mc):
                c = tree.children[i][s]
                assert (up.node[j, s] == -1) == (c == -1)                          # every -1 where _Tree.children has -1
                if c >= 0:
                    assert tree.levels[d + 1][up.node[j, s]] == c and up.off[j, s] == 0
                    read_up.append(c)
            p = tree.parents[i]
            if p >= 0:
                assert tree.levels[d - 1][down.node[j, 0]] == p and down.off[j, 0] == 32 * tree.slot[i]
            else:
                assert down.node[j, 0] == -1
    non_root = [i for i in range(tree.L) if tree.parents[i] >= 0]
    assert sorted(read_up) == non_root                                              # each read exactly once by its parent
    if name == "flipped":
        assert tree.slot[1] == mc - 1


# ---- train_ops fallbacks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_fallbacks_are_the_modules_code(dtype):
    torch.manual_seed(7)
    mc, B = 3, 6
    tree = _Tree(_parents("3d_walker_7_full"), mc)
    plan = _LevelPlan(tree, 32, mc)
    d = 1
    n, n_src = plan.sizes[d], plan.sizes[d + 1]
    mod = ActorUp(41, 32, mc).to(dtype)

    def run(fn):
        h = torch.randn(n, B, 64, dtype=dtype, generator=torch.Generator().manual_seed(1)).requires_grad_()
        src = torch.randn(n_src, B, 32, dtype=dtype, generator=torch.Generator().manual_seed(2)).requires_grad_()
        mod.zero_grad()
        out = fn(h, src)
        out.square().sum().backward()
        return out, [out.detach(), h.grad, src.grad, mod.fc2.weight.grad.clone(), mod.fc3.weight.grad.clone(), mod.fc3.bias.grad.clone()]

    def module_code(h, src):
        rows = [tree.children[i] for i in tree.levels[d]]
        ups_next = {c: src[k] for k, c in enumerate(tree.levels[d + 1])}
        zero = torch.zeros((B, 32), dtype=dtype)
        m = torch.stack([torch.cat([ups_next[c] if c >= 0 else zero for c in row], dim=-1) for row in rows])
        g = torch.tanh(torch.cat([F.normalize(h, dim=-1), m], dim=-1))
        return F.normalize(mod.fc3(torch.tanh(mod.fc2(g))), dim=-1)

    def ops_code(h, src):
        g = train_ops.smp_gather(h, src, plan.up[d], normalize=True, act_tanh=True)
        return train_ops.smp_up_tail(train_ops.linear(g, mod.fc2.weight, mod.fc2.bias), mod.fc3.weight, mod.fc3.bias)
    (o1, r1), (o2, r2) = run(module_code), run(ops_code)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))
    names = ("_SmpGatherFnBackward", "_SmpUpTailFnBackward", "_NormalizeRowsFnBackward")
    assert type(o2.grad_fn).__name__ not in names
    # top-down input and the row normalisation
    x = torch.randn(n_src, B, 32, dtype=dtype).requires_grad_()
    prev = torch.randn(n, B, 32 * mc, dtype=dtype).requires_grad_()
    lv = tree.levels[d + 1]
    zero = torch.zeros((B, 32 * mc), dtype=dtype)
    res = []
    for use_ops in (False, True):
        x.grad = prev.grad = None
        if use_ops:
            xm = train_ops.smp_gather(x, prev, plan.down[d + 1], normalize=False, act_tanh=True)
            m = train_ops.smp_gather(None, prev, plan.down[d + 1])
            y = train_ops.normalize_rows(prev)
        else:
            ms = torch.stack([prev[tree.levels[d].index(tree.parents[i])][:, tree.slot[i] * 32:(tree.slot[i] + 1) * 32] for i in lv])
            xm, m, y = torch.tanh(torch.cat([x, ms], dim=-1)), ms, F.normalize(prev, dim=-1)
        assert type(xm.grad_fn).__name__ not in names and type(m.grad_fn).__name__ not in names and type(y.grad_fn).__name__ not in names
        row = [xm.detach(), m.detach(), y.detach()]
        for loss in (xm.square().sum(), (m * m).sum(), (y * y * y).sum()):      # one consumer of `prev` at a time: no order of additions
            x.grad = prev.grad = None
            loss.backward()
            row += [prev.grad.clone()] + ([x.grad.clone()] if x.grad is not None else [])
        res.append(row)
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ---- the switch ----------------------------------------------------------------------------------------------------------------------
def _pair(td, bu, mc, seed=0):
    torch.manual_seed(seed)
    pol = ActorGraphPolicy(41, 3, 32, 1, 1.0, mc, True, td, bu)
    crit = CriticGraphPolicy(41, 3, 32, 1, mc, True, td, bu)
    return pol, crit


def test_switch_is_a_plain_attribute():
    pol, crit = _pair(True, True, 3)
    for net in (pol, crit):
        assert net.train_kernels is False
        keys = set(net.state_dict().keys())
        net.train_kernels = True
        assert net.train_kernels is True and set(net.state_dict().keys()) == keys
        assert not any("train_kernels" in k for k in keys)
        for clone in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
            assert clone.train_kernels is True
        net.train_kernels = False
        assert net.train_kernels is False


@pytest.mark.parametrize("td,bu", [(True, True), (True, False)])
@pytest.mark.parametrize("name", MORPHS)
def test_switch_on_equals_switch_off_on_the_cpu(name, td, bu):
    parents = _parents(name)
    L, B = len(parents), 4
    nets = []
    for on in (False, True):
        pol, crit = _pair(td, bu, _mc(parents, 3), seed=11)
        pol.train_kernels = crit.train_kernels = on
        pol.change_morphology({"parents": parents})
        crit.change_morphology({"parents": parents})
        nets.append((pol, crit))
    gen = torch.Generator().manual_seed(L)
    obs0, act0 = torch.randn(B, 41 * L, generator=gen), torch.rand(B, 3 * L, generator=gen) * 2 - 1
    pa, pq = torch.randn(B, 3 * L, generator=gen), torch.randn(B, 1, generator=gen)
    res = []
    for pol, crit in nets:
        obs, act = obs0.clone().requires_grad_(), act0.clone().requires_grad_()
        a = pol(obs)
        q1, q2 = crit(obs, act)
        q1b = crit.Q1(obs, a)
        ((a * pa).sum() + (q1 * pq).sum() - (q2 * pq).sum() + (q1b * pq).sum()).backward()
        res.append([a.detach(), q1.detach(), q2.detach(), q1b.detach(), obs.grad, act.grad] +
                   [t.grad for t in pol.parameters()] + [t.grad for t in crit.parameters()])
    # (a gradient is None where nothing reads the parameter: msg_base in a tree of one level)
    assert len(res[0]) == len(res[1]) and sum(g is not None for g in res[0]) >= 24
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(*res))


# ---- the agent -------------------------------------------------------------------------------------------------------------------------
SMP = dict(actor_type="smp", critic_type="smp", td=True, bu=True)


def _smp_agent(seed=3, over=None, **kw):
    torch.manual_seed(seed)
    return Agent(default_train_args(**dict(SMP, **(over or {}))), **kw)


def _online(agent):
    return getattr(agent.actor, "train_kernels", False), getattr(agent.critic, "train_kernels", False)


def _targets(agent):
    return getattr(agent.actor_target, "train_kernels", False), getattr(agent.critic_target, "train_kernels", False)


def test_agent_plumbing():
    assert td3.SMP_TRAIN_KERNELS_DEFAULT is False
    a = _smp_agent()
    assert a.use_smp_train_kernels is False and _online(a) == (False, False) and _targets(a) == (False, False)
    a = _smp_agent(smp_train_kernels=True)
    assert a.use_smp_hip and a.use_smp_train_kernels is True and _online(a) == (True, True) and _targets(a) == (False, False)
    a = _smp_agent(over={"smp_train_kernels": None}, smp_train_kernels=None)
    assert a.use_smp_train_kernels is False                                            # None in both places: the module default
    a = _smp_agent(over={"smp_train_kernels": True})
    assert a.use_smp_train_kernels is True and _online(a) == (True, True) and _targets(a) == (False, False)
    a = _smp_agent(over={"smp_train_kernels": True}, smp_train_kernels=False)
    assert a.use_smp_train_kernels is False and _online(a) == (False, False)          # the keyword wins
    a = _smp_agent(smp_train_kernels=True, use_hip=False)
    assert a.use_smp_train_kernels is False and _online(a) == (False, False)          # follows use_hip
    a = _smp_agent(over={"bu": False}, smp_train_kernels=True)
    assert not a.use_smp_hip and a.use_smp_train_kernels is False and _online(a) == (False, False)     # the td-only mode
    a = _smp_agent(smp_train_kernels=True, swat_train_kernels=True)
    assert a.use_swat_train_kernels is False and a.use_smp_train_kernels is True and _online(a) == (True, True)
    a.set_smp_train_kernels(False)
    assert a.use_smp_train_kernels is False and _online(a) == (False, False)
    a.set_smp_train_kernels(True)
    assert a.use_smp_train_kernels is True and _online(a) == (True, True) and _targets(a) == (False, False)
    for b in (copy.deepcopy(_smp_agent(smp_train_kernels=True)), pickle.loads(pickle.dumps(_smp_agent(smp_train_kernels=True)))):
        assert b.use_smp_train_kernels is True and _online(b) == (True, True) and _targets(b) == (False, False)
    # the other agent types ignore it
    for over in ({"actor_type": "set", "critic_type": "set", "td": False, "bu": False}, {"actor_type": "swat", "critic_type": "swat"},
                 {"actor_type": "mlp", "critic_type": "mlp", "mlp_num_limbs": 7}, {"actor_type": "smp", "critic_type": "swat", "td": True, "bu": True}):
        b = Agent(default_train_args(smp_train_kernels=True, **over), smp_train_kernels=True)
        assert b.use_smp_train_kernels is False
        assert not any(getattr(m, "train_kernels", False) for net in (b.actor, b.critic, b.actor_target, b.critic_target) for m in net.modules())


@pytest.mark.parametrize("skip", [False, True])
def test_a_cpu_update_with_the_switch_on_equals_the_switch_off(skip):
    from oracle.formula import synth_obs
    parents = _parents("3d_walker_7_full")
    B, L = 6, len(parents)
    torch.manual_seed(5)
    batch = {"obs": torch.from_numpy(synth_obs(L, B, 1).astype(np.float32)), "next_obs": torch.from_numpy(synth_obs(L, B, 2).astype(np.float32)),
             "action": torch.rand(B, 3 * L) * 2 - 1, "reward": torch.randn(B, 1), "done": torch.zeros(B, 1)}
    noise = torch.randn(B, 3 * L) * 0.2
    off = _smp_agent(seed=8)
    on = _smp_agent(seed=9, smp_train_kernels=True)
    on.load_state_dict(off.state_dict())
    outs = []
    for agent in (off, on):
        agent.change_morphology({"parents": parents})
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
