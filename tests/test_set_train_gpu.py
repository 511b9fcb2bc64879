"""The differentiable passes of a SET update on the training kernels (csrc/train_gemm.hip through sgrl_amd/train_ops.py: k_sgemm* and
the grouped weight gradients, k_gram_tri_*, k_fold_sym / k_unfold_sym, k_attn_*, k_zmat_*, k_add_ln_*, k_embed3_*) on the MI355X, at
full-rank weights, against float64 copies of the PyTorch modules: whole networks -- the actor net, one critic net, the twin critics
walked at once -- and three Agent.update iterations.  The bar is per tensor (tests/set_train_ref.py compare); tests/test_set_train.py
qualifies it and the inputs on the CPU."""
import copy

import numpy as np
import pytest

import set_full_rank_ref as R
import set_train_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (morphology, batch): 2, 7, 9 and 14 limbs at B = 5, and the smallest batch at which the 64 x 64 weight-gradient tile cuts its
# contraction into two pieces (sgrl_linear_wgrad_group: kt64 / 7 >= 2 from 896 node rows on; 2 688 vector-channel rows)
CASES = [("3d_walker_2_right_leg_left_knee", 5), ("3d_walker_7_full", 5), ("3d_humanoid_9_full", 5), ("3d_cheetah_14_full", 5),
         ("3d_cheetah_14_full", 64)]
KINDS = ["actor", "critic1", "twin"]
_nets, _refs = {}, {}


def _models(kind):
    """(float32 model(s) on the device, their float64 copies), full-rank weights; one TransformerModel or the pair of critic nets."""
    import torch
    if kind not in _nets:
        from sgrl_amd.set_policy import make_critic, make_policy
        torch.manual_seed(0)
        if kind == "actor":
            m = T.full_rank(make_policy(device=DEV, use_hip=False)).actor
            _nets[kind] = (m, copy.deepcopy(m).double())
        else:
            if "critic" not in _nets:
                c = T.full_rank(make_critic(device=DEV, use_hip=False))
                _nets["critic"] = (c, copy.deepcopy(c).double())
            c, c64 = _nets["critic"]
            _nets[kind] = (c.critic1, c64.critic1) if kind == "critic1" else ((c.critic1, c.critic2), (c64.critic1, c64.critic2))
    return _nets[kind]


def _switched_off(fn):
    from sgrl_amd import train_ops
    enabled, train_ops.ENABLED = train_ops.ENABLED, False
    try:
        return fn()
    finally:
        train_ops.ENABLED = enabled


def _inputs(kind, name, B):
    L = R.num_limbs(name)
    x = T.net_input("actor" if kind == "actor" else "critic", L, B, DEV)
    shape = (B, L, 3) if kind == "actor" else ((2, B, L, 1) if kind == "twin" else (B, L, 1))
    return x, T.projection(shape, 11 * L + B + KINDS.index(kind), DEV)


def _reference(kind, name, B):
    """(names, float32 PyTorch pass with the switch off, float64 pass): computed once per case, shared and left unchanged."""
    import torch
    key = (kind, name, B)
    if key not in _refs:
        net, n64 = _models(kind)
        x, proj = _inputs(kind, name, B)
        fns = set()
        off = _switched_off(lambda: T.net_pass(net, R.graph_dict(name, DEV), x, proj, torch.float32, twin=(kind == "twin"), fns=fns))
        assert not any(f.startswith(k) for f in fns for k in T.KERNEL_FNS + ("_LinearFn", "_Linear2Fn")), fns
        ref = T.net_pass(n64, R.graph_dict(name, DEV, f64=True), x, proj, torch.float64)      # the twin's: the two nets one after the other
        _refs[key] = (T.pass_names(net), off, ref)
    return _refs[key]


def _on(kind, name, B, deferred, fns=None):
    import torch
    net, _ = _models(kind)
    x, proj = _inputs(kind, name, B)
    return T.net_pass(net, R.graph_dict(name, DEV), x, proj, torch.float32, twin=(kind == "twin"), deferred=deferred, fns=fns)


@pytest.mark.parametrize("deferred", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("name,B", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_network_pass_matches_float64(kind, name, B, deferred):
    from sgrl_amd import train_ops
    assert train_ops.ENABLED
    names, off, ref = _reference(kind, name, B)
    fns = set()
    on = _on(kind, name, B, deferred, fns)
    want = T.KERNEL_FNS + (("_Linear2Fn",) if kind == "twin" else ("_LinearFn",))
    missing = [k for k in want if not any(f.startswith(k) for f in fns)]
    assert not missing, (missing, sorted(fns))          # the kernels did run
    assert "_FoldFnBackward" in fns                     # ... on folded triangular weights
    assert not all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(on, off))          # and are another path than the switch-off pass
    worst = T.compare(names, on, off, ref, what="%s %s B %d %s" % (kind, name, B, "deferred" if deferred else "immediate"))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("kind", KINDS)
def test_split_contractions_are_reproducible(kind):
    """The B = 64 pass twice, weight gradients immediate and deferred: every tensor bit-equal (the split contractions of the 64 x 64
    weight-gradient tile reduce in a fixed order)."""
    name, B = CASES[-1]
    for deferred in (False, True):
        first = _on(kind, name, B, deferred)
        second = _on(kind, name, B, deferred)
        names = T.pass_names(_models(kind)[0])
        differ = [n for n, a, b in zip(names, first, second) if not np.array_equal(a.numpy(), b.numpy())]
        assert not differ, (deferred, differ)


def _agent(**kw):
    import torch
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(0)
    return Agent(default_train_args(), device=torch.device(DEV), **kw)


@pytest.mark.parametrize("skip", [False, True])
def test_three_updates_stay_on_float64(skip):
    """Three Agent.update iterations (two policy steps) of a default SET agent from one state_dict, the same batches and noise: the
    training kernels (on), float32 PyTorch with train_ops.ENABLED = False (off; both with the HIP target chain) and float64 PyTorch
    (use_hip=False).  The raw gradients of the first iteration (through the three-part API, since update() clips in place) at the
    per-tensor bar, critic and actor network each by itself; every loss of the on agent within max(4 x the off agent's relative
    deviation, 1e-5) of float64."""
    import torch
    from sgrl_amd import train_ops
    name, L, B = "3d_walker_7_full", 7, 33
    on, off, f64 = _agent(), _agent(), _agent(use_hip=False)
    T.full_rank(on.actor)
    T.full_rank(on.critic)
    on.actor_target.load_state_dict(on.actor.state_dict())
    on.critic_target.load_state_dict(on.critic.state_dict())
    with torch.no_grad():            # targets away from the online networks, as in the middle of a run
        gen = torch.Generator(device=DEV).manual_seed(33)
        for mod in (on.actor_target, on.critic_target):
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device=DEV, generator=gen) * 0.02)
    off.load_state_dict(on.state_dict())
    f64.load_state_dict(on.state_dict())
    f64.double()
    assert on.actor.use_hip and on.critic_target.use_hip and off.actor_target.use_hip and not f64.actor_target.use_hip
    g, g64 = R.graph_dict(name, DEV), R.graph_dict(name, DEV, f64=True)
    agents = (("on", on, g), ("off", off, g), ("float64", f64, g64))
    for _, agent, gd in agents:
        agent.change_morphology(gd)
        agent.models2train()
    data = [T.update_batch(L, B, it, DEV) for it in range(3)]
    cast = lambda tag, b, n: T.cast_batch(b, n, torch.float64 if tag == "float64" else torch.float32)
    run = lambda tag, fn: _switched_off(fn) if tag == "off" else fn()
    assert train_ops.ENABLED
    raw = {tag: run(tag, lambda: T.raw_gradients(agent, *cast(tag, *data[0]), skip)) for tag, agent, _ in agents}
    cn, an = [n for n, _ in T.used_parameters(on.critic, "critic.")], [n for n, _ in T.used_parameters(on.actor, "actor.")]
    assert len(cn) > 200 and len(an) > 100
    worst_c = T.compare(cn, raw["on"][2], raw["off"][2], raw["float64"][2], what="skip %d critic gradients" % skip)
    worst_a = T.compare(an, raw["on"][3], raw["off"][3], raw["float64"][3], what="skip %d actor gradients" % skip)
    assert not all(torch.equal(a, b) for a, b in zip(raw["on"][2], raw["off"][2]))
    assert worst_c <= 1.0 and worst_a <= 1.0, (worst_c, worst_a)
    for k in (0, 1):
        ref = raw["float64"][k]
        d_on, d_off = abs(raw["on"][k] - ref) / abs(ref), abs(raw["off"][k] - ref) / abs(ref)
        print("skip %d raw %s loss: float64 %.9g  off rel dev %.3g  on rel dev %.3g" % (skip, ("critic", "actor")[k], ref, d_off, d_on))
        assert d_on <= max(4 * d_off, 1e-5), (k, d_on, d_off)
    losses = {tag: [] for tag, _, _ in agents}
    for it in range(3):
        for tag, agent, _ in agents:
            b, n = cast(tag, *data[it])
            out = run(tag, lambda: agent.update(b, it, noise=n, skip_unused_critic_grads=skip))
            assert ("loss/actor_loss" in out) == (it % 2 == 0)
            losses[tag].append({k: float(torch.as_tensor(v).double()) for k, v in out.items() if k.startswith("loss/")})
    for it in range(3):
        for k, ref in losses["float64"][it].items():
            d_on, d_off = abs(losses["on"][it][k] - ref) / abs(ref), abs(losses["off"][it][k] - ref) / abs(ref)
            print("skip %d it %d %s: float64 %.9g  off rel dev %.3g  on rel dev %.3g" % (skip, it, k, ref, d_off, d_on))
            assert np.isfinite(losses["on"][it][k]) and d_on <= max(4 * d_off, 1e-5), (it, k, d_on, d_off)
