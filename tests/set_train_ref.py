"""Shared by tests/test_set_train.py (CPU) and tests/test_set_train_gpu.py: one differentiable pass of a SET TransformerModel (or of
the twin critics), the raw gradients of a TD3 update, and the bar both files hold them to.

Weights: oracle.formula.apply_full_rank_(module, SEED); observations synth_obs(L, B, OBS_SEED); actions
set_full_rank_ref.critic_actions(L, B, ACT_SEED) -- the seeds tests/test_set_full_rank.py qualified for the forward side.  The float64
reference is the same module built with use_hip=False and cast with .double(), on the graph whose `relation` is double.

The bar is PER TENSOR: max(FACTOR x the deviation of float32 PyTorch from float64, FLOOR x the tensor's own largest float64 magnitude).
A floor taken from the largest gradient of the whole network (tests/test_swat_train_gpu.py) would hide whole tensors here: with these
weights a quarter of a SET network's gradient tensors lie entirely below 1e-4 of that scale (layer 0's q / k / v projections and its
feed-forward pair among them).  Only the three bias vectors of EXEMPT -- zero or cancelling sums in exact arithmetic -- take it."""
import numpy as np
import torch
import torch.nn.functional as F

import set_full_rank_ref as R
from oracle.formula import apply_full_rank_, synth_obs
from sgrl_amd import set_policy, train_ops

SEED, OBS_SEED, ACT_SEED = 8, 108, 208
FACTOR, FLOOR = 4.0, 1e-5          # the project's own: tests/test_swat_train_gpu.py _check_against_float64
# rel_encoder.bias: zero in exact arithmetic (softmax is shift invariant); q_proj.bias / k_proj.bias: cancelling sums for the same
# reason (k_proj.bias shifts every score of a row alike, q_proj.bias meets sum_j dS_ij k_j with sum_j dS_ij = 0).  A cap: no other
# name may be exempted, and no weight matrix.
EXEMPT = ("rel_encoder.bias", "k_proj.bias", "q_proj.bias")
OUTPUTS = ("out", "x.grad")        # compared at their own largest magnitude, like every weight gradient
# what the kernels of a pass leave in the autograd graph (train_ops): one network / the twin critics
KERNEL_FNS = ("_AttnFn", "_GramTriFn", "_ZmatFn", "_AddLNFn", "_Embed3Fn")


def full_rank(module):
    return apply_full_rank_(module, SEED)


def unused(name):
    """The parameters MyMultiheadAttention inherits without using them (reference SEActor.py:34-46): they exist for the state_dict
    and receive no gradient."""
    return ".self_attn.in_proj_" in name or ".self_attn.out_proj." in name


def used_parameters(module, prefix=""):
    return [(prefix + n, p) for n, p in module.named_parameters() if not unused(n)]


def _grads(module, prefix=""):
    """float64 CPU copies of the gradients of every parameter the forward uses; each must have one, the unused ones none."""
    out = []
    for n, p in module.named_parameters():
        if unused(n):
            assert p.grad is None, prefix + n
        else:
            assert p.grad is not None, "no gradient for " + prefix + n
            out.append(p.grad.detach().double().cpu().clone())
    return out


def net_input(kind, L, B, device="cpu"):
    """x [B, L, 41] (actor) or [B, L, 44] (a critic: the action columns appended), float64."""
    x = synth_obs(L, B, OBS_SEED).reshape(B, L, 41)
    if kind != "actor":
        x = np.concatenate([x, R.critic_actions(L, B, ACT_SEED).reshape(B, L, 3)], axis=-1)
    return torch.from_numpy(x).to(device)


def projection(shape, seed, device="cpu"):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(size=tuple(shape))).to(device)


def pass_names(model):
    nets = model if isinstance(model, (tuple, list)) else (model,)
    names = list(OUTPUTS)
    for i, m in enumerate(nets):
        names += [n for n, _ in used_parameters(m, "net%d." % i if len(nets) == 2 else "")]
    return names


def graph_fns(out):
    """Names of the autograd functions reachable from `out`."""
    seen, names, todo = set(), set(), [out.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo += [g for g, _ in f.next_functions]
    return names


def net_pass(model, graph, x0, proj, dtype, twin=False, deferred=False, fns=None):
    """One differentiable pass: loss = a fixed projection of the output -> [output, input gradient, parameter gradients...] as float64
    CPU tensors, in the order of pass_names(model).  model: a TransformerModel (the actor net or one critic net; a critic's x0 holds
    the action columns), or the pair of critic nets -- walked at once by set_policy.twin_forward if `twin`, one after the other and
    stacked otherwise.  deferred: the backward pass inside train_ops.deferred_wgrads.  fns: a set that receives graph_fns(output)."""
    nets = model if isinstance(model, (tuple, list)) else (model,)
    for m in nets:
        m.zero_grad()
    x = x0.detach().to(dtype, copy=True).requires_grad_()
    if len(nets) == 2:
        out = set_policy.twin_forward(nets[0], nets[1], x, graph) if twin else torch.stack([m(x, graph) for m in nets])
    else:
        out = nets[0](x, graph)
    if fns is not None:
        fns.update(graph_fns(out))
    with train_ops.deferred_wgrads(enabled=deferred):
        (out * proj.to(dtype)).sum().backward()
    res = [out.detach().double().cpu(), x.grad.double().cpu()]
    for i, m in enumerate(nets):
        res += _grads(m, "net%d." % i if len(nets) == 2 else "")
    for m in nets:
        m.zero_grad()
    return res


def update_batch(L, B, it, device="cpu"):
    """(batch, policy noise) of update iteration `it`, float64: the qualified observation / action generators at seeds moved by `it`."""
    rng = np.random.RandomState(1000 + it)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
    batch = {"obs": t(synth_obs(L, B, OBS_SEED + 2 * it)), "next_obs": t(synth_obs(L, B, OBS_SEED + 2 * it + 1)),
             "action": t(R.critic_actions(L, B, ACT_SEED + it)), "reward": t(rng.normal(1.0, 0.5, size=(B, 1))),
             "done": t(rng.uniform(size=(B, 1)) < 0.3)}
    return batch, t(rng.normal(0.0, 0.2, size=(B, 3 * L)))


def cast_batch(batch, noise, dtype):
    return {k: v.to(dtype) for k, v in batch.items()}, noise.to(dtype)


def raw_gradients(agent, batch, noise, skip):
    """The two backward passes of Agent.update through its three-part API, without clipping or stepping -> (critic loss, actor loss,
    critic gradients, actor gradients); the gradients as float64 CPU tensors of the parameters the forward uses, in
    used_parameters() order."""
    _, target_q = agent.update_targets(batch, noise)
    q1, q2 = agent.update_critic_forward(batch)
    critic_loss = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
    agent.critic.zero_grad()
    with train_ops.deferred_wgrads(enabled=skip):
        critic_loss.backward()
    gc = _grads(agent.critic, "critic.")
    frozen = list(agent.critic.parameters()) if skip else []
    for p in frozen:
        p.requires_grad_(False)
    try:
        actor_loss = -agent.critic.Q1(batch["obs"], agent.actor(batch["obs"])).mean()
        agent.actor.zero_grad()
        with train_ops.deferred_wgrads(enabled=skip):
            actor_loss.backward()
    finally:
        for p in frozen:
            p.requires_grad_(True)
    ga = _grads(agent.actor, "actor.")
    agent.critic.zero_grad()
    agent.actor.zero_grad()
    return float(critic_loss.detach().double()), float(actor_loss.detach().double()), gc, ga


def is_exempt(name, exempt=EXEMPT):
    return name.endswith(tuple(exempt)) if exempt else False


def bars(names, off, ref, exempt=EXEMPT, factor=FACTOR):
    """[(own, d_off, bar)] per tensor: bar = max(factor x d_off, FLOOR x own), own = the tensor's largest float64 magnitude -- for
    the exempt bias vectors the largest float64 parameter gradient of the network instead."""
    assert set(exempt) <= set(EXEMPT), "only %r may take the group floor" % (EXEMPT,)
    net = lambda n: n.split(".")[0] if n.startswith(("net0.", "net1.")) else ""          # the twin pass holds two networks
    group = {}
    for n, r in zip(names, ref):
        if n not in OUTPUTS:
            group[net(n)] = max(group.get(net(n), 0.0), float(r.abs().max()))
    out = []
    for name, b, r in zip(names, off, ref):
        own = float(r.abs().max())
        scale = own
        if name not in OUTPUTS and is_exempt(name, exempt):
            assert r.dim() == 1 and name.endswith(".bias"), "no weight matrix may take the group floor: " + name
            scale = group[net(name)]
        d_off = float((b - r).abs().max())
        out.append((own, d_off, max(factor * d_off, FLOOR * scale)))
    return out


def compare(names, on, off, ref, exempt=EXEMPT, what="", factor=FACTOR):
    """on / off / ref: the tensors of one pass (or the parameter gradients of one network) under test, from float32 PyTorch with
    train_ops.ENABLED = False, and in float64.  Returns the worst d_on / bar over the tensors (<= 1: every tensor within its bar;
    inf for a tensor that is not finite) and prints it with the tensor's name."""
    assert len(names) == len(on) == len(off) == len(ref), (len(names), len(on), len(off), len(ref))
    worst, at = 0.0, None
    for name, a, r, (own, d_off, bar) in zip(names, on, ref, bars(names, off, ref, exempt, factor)):
        assert a.shape == r.shape, (what, name, tuple(a.shape), tuple(r.shape))
        d_on = float((a - r).abs().max())
        if not np.isfinite(d_on):
            ratio = float("inf")
        elif bar > 0.0:
            ratio = d_on / bar
        else:
            ratio = 0.0 if d_on == 0.0 else float("inf")
        if at is None or ratio > worst:
            worst, at = ratio, (name, d_on, d_off, own, bar)
    print("%s: %d tensors, worst deviation / bar = %.3g at %s (deviation %.3g, float32 PyTorch's %.3g, own max %.3g, bar %.3g)"
          % ((what, len(names), worst) + at))
    return worst
