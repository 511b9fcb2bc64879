"""Qualifies the inputs and the bar of tests/test_set_train_gpu.py on the CPU, in float64 and float32, before any device is involved
(as tests/test_set_full_rank.py does for the forward side).

The bar (tests/set_train_ref.py compare) is per tensor: max(4 x float32 PyTorch's deviation from float64, 1e-5 x the tensor's own
largest float64 magnitude).  Conditions, asserted here so that a change to the generators or the modules that loses them fails on the
CPU and not silently on the device: every tensor that is held to its own magnitude has one above float32 rounding of the whole
network; float32 PyTorch alone stays inside every bar; an exchange of two columns in any weight gradient is flagged; the update's
losses, which the relative loss bars divide by, are not degenerate."""
import pytest
import torch

import set_full_rank_ref as R
import set_train_ref as T
from oracle.formula import apply_formula_
from sgrl_amd.td3 import Agent, default_train_args

NAME, L, B = "3d_walker_7_full", 7, 6
OWN_FLOOR = 1e-7            # own max of every non-exempt gradient tensor, as a fraction of the network's largest gradient
KINDS = ["actor", "critic1", "critic2"]


def _net(kind, apply, dtype):
    m = R.cpu_modules("actor" if kind == "actor" else "critic", apply, dtype)
    return m.actor if kind == "actor" else getattr(m, kind)


_cache = {}


def _passes(kind, weights="full_rank"):
    """(names, float64 pass, float32 pass) of one network on the CPU; computed once per (kind, weights) and never modified."""
    key = (kind, weights)
    if key not in _cache:
        apply = T.full_rank if weights == "full_rank" else apply_formula_
        x = T.net_input(kind, L, B)
        proj = T.projection((B, L, 3 if kind == "actor" else 1), 7 + KINDS.index(kind))
        n64, n32 = _net(kind, apply, torch.float64), _net(kind, apply, torch.float32)
        ref = T.net_pass(n64, R.graph_dict(NAME, f64=True), x, proj, torch.float64)
        f32 = T.net_pass(n32, R.graph_dict(NAME), x, proj, torch.float32)
        _cache[key] = (T.pass_names(n64), ref, f32)
    return _cache[key]


@pytest.mark.parametrize("kind", KINDS)
def test_every_tensor_held_to_its_own_magnitude_has_one(kind):
    """net_pass itself asserts that every parameter the forward uses received a gradient (and the inherited, unused ones none)."""
    names, ref, _ = _passes(kind)
    assert len(names) == len(ref) and len(names) > 100
    scale = max(float(r.abs().max()) for n, r in zip(names, ref) if n not in T.OUTPUTS)
    small = [(n, float(r.abs().max()) / scale) for n, r in zip(names, ref)
             if n not in T.OUTPUTS and not T.is_exempt(n) and float(r.abs().max()) < OWN_FLOOR * scale]
    assert not small, small
    lowest = min((float(r.abs().max()) / scale, n) for n, r in zip(names, ref) if n not in T.OUTPUTS and not T.is_exempt(n))
    below = sum(float(r.abs().max()) < 1e-4 * scale for n, r in zip(names, ref) if n not in T.OUTPUTS)
    print("%s: %d gradient tensors, largest %.3g; %d lie wholly below 1e-4 x that (a group floor's blind spot); smallest own max of a "
          "non-exempt tensor %.3g x (%s)" % (kind, len(names) - len(T.OUTPUTS), scale, below, lowest[0], lowest[1]))
    for n, r in zip(names, ref):          # the outputs are held to their own magnitude too
        if n in T.OUTPUTS:
            assert float(r.abs().max()) > 1e-6, n


@pytest.mark.parametrize("kind", KINDS)
def test_float32_pytorch_alone_stays_inside_the_bar(kind):
    names, ref, f32 = _passes(kind)
    margin = T.compare(names, f32, f32, ref, what="%s, float32 CPU module as both sides" % kind)
    assert margin <= 1.0 / T.FACTOR + 1e-12          # by construction: d_on = d_off
    # without the 4 x d_off term: at most the exempt tensors exceed 1e-5 x their own magnitude
    over = [n for n, a, r in zip(names, f32, ref) if float((a - r).abs().max()) > T.FLOOR * float(r.abs().max())]
    print("%s: float32 exceeds 1e-5 x own max on %d of %d tensors: %s" % (kind, len(over), len(names), over))
    assert all(T.is_exempt(n) for n in over), [n for n in over if not T.is_exempt(n)]
    # and with the exempt tensors on the group floor, the floor term alone holds float32 PyTorch: the reference is inside the bar
    floor_only = T.compare(names, f32, ref, ref, what="%s, float32 CPU module against the floor terms alone" % kind)
    print("%s: float32 margin against the floor terms alone %.3g" % (kind, floor_only))
    assert floor_only <= 1.0


def _exchange(t, c0, c1):
    t = t.clone()
    t[:, [c0, c1]] = t[:, [c1, c0]]
    return t


def _sites(names, ref):
    """Every 2-D parameter gradient with at least 16 columns that is not exempt: columns 3 <-> 11 and 5 <-> 5 + 8 (K // 16), the
    exchanges of set_full_rank_ref.swap_sites.  In the invariant layers' 1 024 columns a MIRROR exchange a * 32 + b <-> b * 32 + a is
    no error at all -- Z'Z is symmetric, the two columns are equal in exact arithmetic -- and would not count as a miss; neither
    exchange here is one (3 <-> 11 is (0, 3) <-> (0, 11), 5 <-> 517 is (0, 5) <-> (16, 5))."""
    out = []
    for i, (n, r) in enumerate(zip(names, ref)):
        if n in T.OUTPUTS or T.is_exempt(n) or r.dim() != 2 or r.shape[1] < 16:
            continue
        K = r.shape[1]
        for c0, c1 in ((3, 11), (5, 5 + 8 * (K // 16))):
            assert not (K == 1024 and (c0 // 32, c0 % 32) == (c1 % 32, c1 // 32))
            out.append((i, c0, c1))
    return out


def _flagged(names, ref, f32):
    """(live exchanges, how many of them compare() flags, the missed ones, the dead ones) with the float64 gradient carrying the
    exchange as the side under test.  Dead: the two columns are EQUAL in float64, bit for bit, so the exchange changes nothing and is
    no error (both hidden units behind a ReLU are off on every row of the batch: two all-zero gradient columns) -- the forward
    census (set_full_rank_ref.census) leaves out its dead exchanges in the same way."""
    base = T.bars(names, f32, ref)
    live, hit, missed, dead = [], 0, [], []
    for i, c0, c1 in _sites(names, ref):
        label = "%s[:, %d<->%d]" % (names[i], c0, c1)
        d_on = float((_exchange(ref[i], c0, c1) - ref[i]).abs().max())
        if d_on == 0.0:
            assert torch.equal(ref[i][:, c0], ref[i][:, c1])
            dead.append(label)
            continue
        live.append((i, c0, c1))
        if d_on > base[i][2]:
            hit += 1
        else:
            missed.append((label, d_on, base[i][2]))
    return live, hit, missed, dead


@pytest.mark.parametrize("kind", KINDS)
def test_every_column_exchange_in_a_weight_gradient_is_flagged(kind):
    names, ref, f32 = _passes(kind)
    sites, hit, missed, dead = _flagged(names, ref, f32)
    fnames, fref, f32f = _passes(kind, "formula")
    fsites, fhit, _, fdead = _flagged(fnames, fref, f32f)
    print("%s: %d live exchanges (%d dead: %s), %d flagged at full rank; at the formula weights %d of %d live ones would pass (%d dead)"
          % (kind, len(sites), len(dead), dead, hit, len(fsites) - fhit, len(fsites), len(fdead)))
    assert len(sites) >= 120 and len(dead) <= 6 and not missed, missed
    # the same through compare() itself, on the weakest site and one other: the worst ratio is the exchanged tensor's
    for i, c0, c1 in (sites[0], sites[len(sites) // 2]):
        on = list(ref)
        on[i] = _exchange(ref[i], c0, c1)
        assert T.compare(names, on, f32, ref, what="%s with %s[:, %d<->%d]" % (kind, names[i], c0, c1)) > 1.0


def test_compare_keeps_its_exemptions_to_the_three_bias_names():
    names, ref, f32 = _passes("actor")
    with pytest.raises(AssertionError):
        T.compare(names, f32, f32, ref, exempt=T.EXEMPT + ("linear1.weight",))
    # fewer exemptions are allowed and are stricter
    assert T.compare(names, f32, f32, ref, exempt=()) <= 1.0 / T.FACTOR + 1e-12
    # a tensor that is not finite is never within its bar
    bad = list(f32)
    bad[5] = bad[5].clone()
    bad[5].view(-1)[0] = float("nan")
    assert T.compare(names, bad, f32, ref) == float("inf")


def test_the_update_losses_are_not_degenerate():
    """The relative loss bars of the device test divide by these: the batch of its first iteration (B = 33), float64, CPU."""
    torch.manual_seed(0)
    agent = Agent(default_train_args(), device=torch.device("cpu"), use_hip=False)
    T.full_rank(agent.actor)
    T.full_rank(agent.critic)
    agent.actor_target.load_state_dict(agent.actor.state_dict())
    agent.critic_target.load_state_dict(agent.critic.state_dict())
    agent.double()
    agent.change_morphology(R.graph_dict(NAME, f64=True))
    agent.models2train()
    batch, noise = T.update_batch(L, 33, 0)
    closs, aloss, gc, ga = T.raw_gradients(agent, batch, noise, False)
    print("critic loss %.6g, actor loss %.6g, %d critic and %d actor gradient tensors" % (closs, aloss, len(gc), len(ga)))
    assert abs(closs) >= 1e-6 and abs(aloss) >= 1e-6
    assert len(gc) == len(T.used_parameters(agent.critic)) > 200 and len(ga) == len(T.used_parameters(agent.actor)) > 100
