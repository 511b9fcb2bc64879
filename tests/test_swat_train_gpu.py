"""The differentiable passes of a SWAT update on the training kernels, on the MI355X: the attention kernel pair
(csrc/train_gemm.hip k_swat_attn_fwd / k_swat_attn_bwd through train_ops.swat_attention) against float64, its input handling and
the argument errors of its C ABI; whole networks with swat_policy's `train_kernels` switch, three Agent.update iterations and a
DeviceTrainer round with `swat_train_kernels=True`, each against float64 copies of the PyTorch modules."""
import copy
import ctypes

import numpy as np
import pytest

import swat_attn_restate as R

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
SCALE = 64 ** -0.5
MORPHS = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full", "3d_cheetah_14_full"]      # 2, 7 and 14 limbs


def _attn_inputs(B, L, with_bias, seed, qk_gain=1.0):
    import torch
    torch.manual_seed(seed)
    qkv = torch.randn(B, L, 384) * 0.6
    qkv[..., :256] *= qk_gain
    bias = torch.randn(2, L, L) if with_bias else None
    return qkv, bias, torch.randn(B, L, 128)


def _attn_ref(qkv, bias, d_o):
    """float64 restatement -> (o, dqkv, dbias or None)."""
    w, o = R.forward(qkv.numpy(), None if bias is None else bias.numpy(), SCALE)
    dqkv, ds = R.backward(qkv.numpy(), SCALE, w, d_o.numpy())
    return o, dqkv, (None if bias is None else ds.sum(0))


def _attn_run(qkv, bias, d_o, fn=None):
    """train_ops.swat_attention (or `fn`) on the GPU in float32 -> (o, dqkv, dbias or None) as float64 arrays, and the output tensor."""
    from sgrl_amd import train_ops
    q = qkv.cuda().requires_grad_()
    b = None if bias is None else bias.cuda().requires_grad_()
    o = (fn or train_ops.swat_attention)(q, b, SCALE)
    (o * d_o.cuda()).sum().backward()
    f = lambda t: None if t is None else t.detach().double().cpu().numpy()
    return (f(o), f(q.grad), None if b is None else f(b.grad)), o


def _torch_core(qkv, bias, scale):
    """The module's einsum code (the fallback of train_ops.swat_attention), forced."""
    from sgrl_amd import train_ops
    enabled, train_ops.ENABLED = train_ops.ENABLED, False
    try:
        return train_ops.swat_attention(qkv, bias, scale)
    finally:
        train_ops.ENABLED = enabled


def _dev(got, ref):
    return [None if r is None else float(np.abs(g - r).max()) for g, r in zip(got, ref)]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,with_bias", [(23, 1, True), (23, 2, True), (23, 7, True), (23, 9, False), (23, 15, True), (23, 15, False),
                                           (1, 15, True), (130, 15, True)])
def test_kernel_matches_float64(B, L, with_bias):
    qkv, bias, d_o = _attn_inputs(B, L, with_bias, seed=100 * L + B)
    ref = _attn_ref(qkv, bias, d_o)
    got, o = _attn_run(qkv, bias, d_o)
    assert type(o.grad_fn).__name__ == "_SwatAttnFnBackward"
    assert got[0].shape == (B, L, 128) and got[1].shape == (B, L, 384) and (not with_bias or got[2].shape == (2, L, L))
    dev = _dev(got, ref)
    print("B %d L %d bias %d: |o - o64| %.3g  |dqkv - ref| %.3g (max|ref| %.3g)  |dbias - ref| %s"
          % (B, L, with_bias, dev[0], dev[1], np.abs(ref[1]).max(), dev[2]))
    assert dev[0] < 1e-5
    assert dev[1] < 2e-5 * (float(np.abs(ref[1]).max()) + 1)
    if with_bias:
        assert dev[2] < 2e-5 * (float(np.abs(ref[2]).max()) + 1)
    if L == 1:                                    # a softmax over one entry: w = 1 exactly, so ds, dq and dk vanish and dv = d_o
        assert (got[1][..., :256] == 0).all() and np.array_equal(got[1][..., 256:], d_o.double().numpy()) and (got[2] == 0).all()
        assert np.array_equal(got[0], qkv[..., 256:].double().numpy())


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
def test_kernel_with_large_scores(with_bias):
    """q and k six times larger: q . k of several hundred, a saturated softmax.  The absolute bars of test 1 do not hold here even
    for float32 PyTorch, so the kernel may deviate from float64 by at most max(4 x float32 PyTorch's own deviation on the same
    inputs, the bars of test 1)."""
    B, L = 23, 15
    qkv, bias, d_o = _attn_inputs(B, L, with_bias, seed=7, qk_gain=6.0)
    ref = _attn_ref(qkv, bias, d_o)
    got, o = _attn_run(qkv, bias, d_o)
    pt, _ = _attn_run(qkv, bias, d_o, fn=_torch_core)
    assert type(o.grad_fn).__name__ == "_SwatAttnFnBackward"
    assert all(g is None or np.isfinite(g).all() for g in got)
    dots = np.einsum("bihd,bjhd->bhij", qkv[..., :128].double().numpy().reshape(B, L, 2, 64), qkv[..., 128:256].double().numpy().reshape(B, L, 2, 64))
    w64 = R.forward(qkv.numpy(), None if bias is None else bias.numpy(), SCALE)[0]
    assert np.abs(dots).max() > 200 and np.median(w64.max(-1)) > 0.9          # q . k of several hundred, most rows all but one-hot
    dev, dev_pt = _dev(got, ref), _dev(pt, ref)
    floors = [1e-5, 2e-5 * (float(np.abs(ref[1]).max()) + 1), None if ref[2] is None else 2e-5 * (float(np.abs(ref[2]).max()) + 1)]
    for name, d, p, fl in zip(("o", "dqkv", "dbias"), dev, dev_pt, floors):
        if d is None:
            continue
        print("large scores, bias %d, %s: kernel %.3g  float32 PyTorch %.3g  floor %.3g" % (with_bias, name, d, p, fl))
        assert d <= max(4 * p, fl), (name, d, p, fl)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_input_handling():
    import torch
    from sgrl_amd import train_ops
    B, L = 23, 7
    qkv, bias, d_o = _attn_inputs(B, L, True, seed=3)
    ref = _attn_ref(qkv, bias, d_o)
    # qkv a strided slice of a wider tensor, the incoming gradient an expanded one
    wide = torch.zeros(B, L, 500, device="cuda:0")
    wide[..., 50:434] = qkv.cuda()
    wide.requires_grad_()
    b = bias.cuda().requires_grad_()
    view = wide[..., 50:434]
    assert not view.is_contiguous()
    o = train_ops.swat_attention(view, b, SCALE)
    assert type(o.grad_fn).__name__ == "_SwatAttnFnBackward"
    row = torch.randn(128)
    go = row.cuda().expand(B, L, 128)
    assert not go.is_contiguous()
    o.backward(go)
    ref_e = R.backward(qkv.numpy(), SCALE, R.forward(qkv.numpy(), bias.numpy(), SCALE)[0], row.double().numpy()[None, None].repeat(B, 0).repeat(L, 1))
    assert float(np.abs(o.detach().double().cpu().numpy() - ref[0]).max()) < 1e-5
    g = wide.grad.double().cpu().numpy()
    assert (g[..., :50] == 0).all() and (g[..., 434:] == 0).all()
    assert float(np.abs(g[..., 50:434] - ref_e[0]).max()) < 2e-5 * (float(np.abs(ref_e[0]).max()) + 1)
    assert float(np.abs(b.grad.double().cpu().numpy() - ref_e[1].sum(0)).max()) < 2e-5 * (float(np.abs(ref_e[1].sum(0)).max()) + 1)
    # a frozen bias: no gradient for it (and no ds.sum)
    q = qkv.cuda().requires_grad_()
    bf = bias.cuda()
    o = train_ops.swat_attention(q, bf, SCALE)
    assert type(o.grad_fn).__name__ == "_SwatAttnFnBackward"
    (o * d_o.cuda()).sum().backward()
    assert bf.grad is None and float(np.abs(q.grad.double().cpu().numpy() - ref[1]).max()) < 2e-5 * (float(np.abs(ref[1]).max()) + 1)
    # torch.no_grad(): the module's operations, no graph
    with torch.no_grad():
        o_ng = train_ops.swat_attention(q, b, SCALE)
    assert o_ng.grad_fn is None and not o_ng.requires_grad
    assert float(np.abs(o_ng.double().cpu().numpy() - ref[0]).max()) < 1e-5
    # 16 limbs: more than the kernels hold -- the module's operations, differentiable
    q16, b16, d16 = _attn_inputs(5, 16, True, seed=16)
    got16, o16 = _attn_run(q16, b16, d16)
    assert type(o16.grad_fn).__name__ != "_SwatAttnFnBackward"
    ref16 = _attn_ref(q16, b16, d16)
    assert float(np.abs(got16[0] - ref16[0]).max()) < 1e-5 and float(np.abs(got16[1] - ref16[1]).max()) < 2e-5 * (float(np.abs(ref16[1]).max()) + 1)
    # the same input twice: the same bits
    q15, b15, d15 = _attn_inputs(130, 15, True, seed=15)
    first, _ = _attn_run(q15, b15, d15)
    second, _ = _attn_run(q15, b15, d15)
    assert all(np.array_equal(x, y) for x, y in zip(first, second))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_returned_not_faults():
    import torch
    from sgrl_amd import train_ops
    lib = train_ops._L()
    B, L = 4, 15
    qkv, bias, d_o = _attn_inputs(B, L, True, seed=4)
    q, b, g = qkv.cuda(), bias.cuda(), d_o.cuda()
    w, o = torch.zeros(B, 2, L, L, device="cuda:0"), torch.zeros(B, L, 128, device="cuda:0")
    dqkv, ds = torch.zeros_like(q), torch.zeros_like(w)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc = ctypes.c_float(SCALE)
    fwd = lambda q_, b_, w_, o_, B_, L_: lib.sgrl_swat_attention_forward(p(q_), p(b_), sc, p(w_), p(o_), B_, L_, st)
    bwd = lambda q_, w_, g_, dq_, ds_, B_, L_: lib.sgrl_swat_attention_backward(p(q_), sc, p(w_), p(g_), p(dq_), p(ds_), B_, L_, st)
    ERR_ARG = -1
    bad_f = [(q, b, w, o, B, 0), (q, b, w, o, B, 16), (q, b, w, o, 0, L), (q, b, w, o, -3, L), (None, b, w, o, B, L), (q, b, None, o, B, L),
             (q, b, w, None, B, L)]
    for a in bad_f:
        assert fwd(*a) == ERR_ARG and b"sgrl_swat_attention_forward" in lib.sgrl_train_last_error()
    bad_b = [(q, w, g, dqkv, ds, B, 0), (q, w, g, dqkv, ds, B, 16), (q, w, g, dqkv, ds, 0, L), (None, w, g, dqkv, ds, B, L),
             (q, None, g, dqkv, ds, B, L), (q, w, None, dqkv, ds, B, L), (q, w, g, None, ds, B, L), (q, w, g, dqkv, None, B, L)]
    for a in bad_b:
        assert bwd(*a) == ERR_ARG and b"sgrl_swat_attention_backward" in lib.sgrl_train_last_error()
    torch.cuda.synchronize()
    assert float(w.abs().max()) == 0 and float(o.abs().max()) == 0 and float(dqkv.abs().max()) == 0       # nothing was launched
    # the well-formed calls go through (a null bias is one of them) and are correct
    assert fwd(q, b, w, o, B, L) == 0 and bwd(q, w, g, dqkv, ds, B, L) == 0
    torch.cuda.synchronize()
    ref = _attn_ref(qkv, bias, d_o)
    assert float(np.abs(o.double().cpu().numpy() - ref[0]).max()) < 1e-5
    assert float(np.abs(dqkv.double().cpu().numpy() - ref[1]).max()) < 2e-5 * (float(np.abs(ref[1]).max()) + 1)
    assert float(np.abs(ds.sum(0).double().cpu().numpy() - ref[2]).max()) < 2e-5 * (float(np.abs(ref[2]).max()) + 1)
    assert fwd(q, None, w, o, B, L) == 0
    torch.cuda.synchronize()
    assert float(np.abs(o.double().cpu().numpy() - _attn_ref(qkv, None, d_o)[0]).max()) < 1e-5


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def _graphs(names):
    import torch
    from sgrl_amd import graph as G, mjcf
    return [G.getGraphDict(mjcf.load_asset(n).parents, TRAV, [], device=torch.device("cuda:0")) for n in names]


def _g64(g):
    g64 = dict(g)
    g64["relation"] = g["relation"].double()
    return g64


def _net_pass(model, graph, x0, proj, dtype):
    """One differentiable pass of a TransformerModel: loss = a fixed projection of the output -> [output, input gradient,
    parameter gradients...] as float64 CPU tensors."""
    model.zero_grad()
    x = x0.detach().to(dtype, copy=True).requires_grad_()
    out = model(x, graph)
    (out * proj.to(dtype)).sum().backward()
    return [out.detach().double().cpu(), x.grad.double().cpu()] + [p.grad.double().cpu() for p in model.parameters()]


def _check_against_float64(names, on, off, ref, what):
    """on / off / ref: the tensors of one pass with the switch on, with the switch off and in float64 (outputs first, then the
    gradients from "x.grad" on).  Every tensor of `on` lies within max(4 x the switch-off float32 PyTorch deviation, 1e-5 x the
    largest float64 magnitude among the outputs, resp. among the gradients).  The floor is NOT scaled by the tensor's own norm:
    some gradients are zero in exact arithmetic (the k-third of in_proj_bias and rel_encoder.bias -- softmax is shift invariant)
    and hold rounding only."""
    n_out = names.index("x.grad")
    groups = [max(float(r.abs().max()) for r in ref[:n_out])] * n_out
    groups += [max(float(r.abs().max()) for r in ref[n_out:])] * (len(ref) - n_out)
    worst = 0.0
    for name, a, b, r, scale in zip(names, on, off, ref, groups):
        assert a.shape == r.shape, (what, name)
        d_on, d_off = float((a - r).abs().max()), float((b - r).abs().max())
        bar = max(4 * d_off, 1e-5 * scale)
        worst = max(worst, d_on / bar)
        assert np.isfinite(d_on) and d_on <= bar, (what, name, d_on, d_off, bar)
    print("%s: %d tensors, worst deviation / bar = %.3g" % (what, len(ref), worst))


@pytest.mark.parametrize("cond", [0, 1])
@pytest.mark.parametrize("feature,out", [(41, 3), (44, 1)])
def test_networks_match_float64(feature, out, cond):
    import torch
    from sgrl_amd.set_policy import default_args
    from sgrl_amd.swat_policy import _model
    torch.manual_seed(10 * feature + cond)
    net = _model(feature, out, default_args(condition_decoder_on_features=cond)).to("cuda:0")
    with torch.no_grad():
        for n, p in net.named_parameters():       # biases (and the norms' gains) away from their initial values
            if n.endswith("bias") or "norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
    on = copy.deepcopy(net)
    on.train_kernels = True
    n64 = copy.deepcopy(net).double()
    names = ["out", "x.grad"] + [n for n, _ in net.named_parameters()]
    B = 33
    for name, g in zip(MORPHS, _graphs(MORPHS)):
        L = len(g["parents"])
        gen = torch.Generator(device="cuda:0").manual_seed(L)
        x = torch.randn((B, L, feature), device="cuda:0", generator=gen)
        proj = torch.randn((B, L, out), device="cuda:0", generator=gen)
        ref = _net_pass(n64, _g64(g), x, proj, torch.float64)
        r_off = _net_pass(net, g, x, proj, torch.float32)
        r_on = _net_pass(on, g, x, proj, torch.float32)
        _check_against_float64(names, r_on, r_off, ref, "feature %d cond %d %s" % (feature, cond, name))
        assert not all(torch.equal(a, b) for a, b in zip(r_on, r_off))          # the switch did take another path


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def _agent(seed=0, **kw):
    import torch
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(seed)
    return Agent(default_train_args(actor_type="swat", critic_type="swat"), device=torch.device("cuda:0"), **kw)


def _batch(L, B, seed):
    import torch
    gen = torch.Generator(device="cuda:0").manual_seed(seed)
    r = lambda *s: torch.rand(s, device="cuda:0", generator=gen)
    batch = {"obs": torch.randn((B, 41 * L), device="cuda:0", generator=gen), "next_obs": torch.randn((B, 41 * L), device="cuda:0", generator=gen),
             "action": r(B, 3 * L) * 2 - 1, "reward": r(B, 1) * 2 - 1, "done": (r(B, 1) < 0.3).float()}
    return batch, torch.randn((B, 3 * L), device="cuda:0", generator=gen) * 0.4


def _raw_gradients(agent, batch, noise, skip):
    """The two backward passes of Agent.update through its three-part API, without clipping or stepping -> (critic loss, actor
    loss, critic gradients, actor gradients)."""
    import torch
    import torch.nn.functional as F
    from sgrl_amd import train_ops
    _, target_q = agent.update_targets(batch, noise)
    q1, q2 = agent.update_critic_forward(batch)
    critic_loss = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
    agent.critic.zero_grad()
    with train_ops.deferred_wgrads(enabled=skip):
        critic_loss.backward()
    gc = [p.grad.detach().double().cpu().clone() for p in agent.critic.parameters()]
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
    ga = [p.grad.detach().double().cpu().clone() for p in agent.actor.parameters()]
    agent.critic.zero_grad()
    agent.actor.zero_grad()
    return float(critic_loss.detach().double()), float(actor_loss.detach().double()), gc, ga


@pytest.mark.parametrize("skip", [False, True])
def test_three_updates_stay_on_float64(skip):
    """Three Agent.update iterations (two policy steps) from one state_dict, the same batches and noise: switch on, switch off
    (float32 PyTorch with the HIP target chain, as today) and float64 PyTorch.  Every loss of the switch-on agent within max(4 x
    the switch-off agent's relative deviation, 1e-5) of float64; the raw gradients of the first iteration (taken through the
    three-part API, since update() clips in place) at the per-tensor bar of the network test."""
    g = _graphs(["3d_walker_7_full"])[0]
    on = _agent(seed=30, swat_train_kernels=True)
    off = _agent(seed=31)
    f64 = _agent(seed=32, use_hip=False)
    import torch
    with torch.no_grad():            # targets away from the online networks, as in the middle of a run
        gen = torch.Generator(device="cuda:0").manual_seed(33)
        for mod in (on.actor_target, on.critic_target):
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.02)
    off.load_state_dict(on.state_dict())
    f64.load_state_dict(on.state_dict())
    f64.double()
    assert on.use_swat_train_kernels and on.actor.train_kernels and on.critic.train_kernels
    assert not on.actor_target.train_kernels and not on.critic_target.train_kernels
    assert off.use_swat_hip and not off.use_swat_train_kernels and not off.actor.train_kernels and not f64.use_swat_hip
    agents = (("on", on, g), ("off", off, g), ("float64", f64, _g64(g)))
    for _, agent, gd in agents:
        agent.change_morphology(gd)
        agent.models2train()
    data = [_batch(7, 33, seed=40 + it) for it in range(3)]
    cast = lambda tag, b, n: ({k: v.double() for k, v in b.items()}, n.double()) if tag == "float64" else (b, n)
    raw = {tag: _raw_gradients(agent, *cast(tag, *data[0]), skip) for tag, agent, _ in agents}
    names = ["critic." + n for n, _ in on.critic.named_parameters()] + ["actor." + n for n, _ in on.actor.named_parameters()]
    flat = {tag: r[2] + r[3] for tag, r in raw.items()}
    scale = max(float(t.abs().max()) for t in flat["float64"])
    worst = 0.0
    for name, a, b, r in zip(names, flat["on"], flat["off"], flat["float64"]):
        d_on, d_off = float((a - r).abs().max()), float((b - r).abs().max())
        bar = max(4 * d_off, 1e-5 * scale)
        worst = max(worst, d_on / bar)
        assert np.isfinite(d_on) and d_on <= bar, (name, d_on, d_off, bar)
    print("skip %d raw gradients: %d tensors, largest |g64| %.3g, worst deviation / bar %.3g" % (skip, len(names), scale, worst))
    for k in (0, 1):
        ref = raw["float64"][k]
        d_on, d_off = abs(raw["on"][k] - ref) / abs(ref), abs(raw["off"][k] - ref) / abs(ref)
        assert d_on <= max(4 * d_off, 1e-5), (k, d_on, d_off)
    losses = {tag: [] for tag, _, _ in agents}
    for it in range(3):
        for tag, agent, _ in agents:
            b, n = cast(tag, *data[it])
            out = agent.update(b, it, noise=n, skip_unused_critic_grads=skip)
            assert ("loss/actor_loss" in out) == (it % 2 == 0)
            losses[tag].append({k: float(torch.as_tensor(v).double()) for k, v in out.items() if k.startswith("loss/")})
    for it in range(3):
        for k, ref in losses["float64"][it].items():
            d_on, d_off = abs(losses["on"][it][k] - ref) / abs(ref), abs(losses["off"][it][k] - ref) / abs(ref)
            print("skip %d it %d %s: float64 %.9g  switch off rel dev %.3g  switch on rel dev %.3g" % (skip, it, k, ref, d_off, d_on))
            assert np.isfinite(losses["on"][it][k]) and d_on <= max(4 * d_off, 1e-5), (it, k, d_on, d_off)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_device_trainer_trains_with_the_switch_on():
    import torch
    from sgrl_amd.swat_hip import HipSwatActor
    from sgrl_amd.swat_policy import StructurePolicy
    from sgrl_amd.td3 import GraphedUpdates, default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full"]
    args = default_train_args(actor_type="swat", critic_type="swat", swat_train_kernels=True, max_episode_steps=40)
    tr = DeviceTrainer(names, 4, args=args, seed=3, device="cuda:0", max_buffer_size=1024, batch_size=16)
    agent = tr.agent
    assert isinstance(agent.actor, StructurePolicy) and isinstance(tr.ro.actor, HipSwatActor)
    assert agent.use_swat_train_kernels and agent.actor.train_kernels and agent.critic.train_kernels
    assert not agent.actor_target.train_kernels and not agent.critic_target.train_kernels
    tr.warmup(30)
    assert all(b.max_sample_size >= 16 for b in tr.buffers)
    obs = tr.ro.env.obs.clone()
    before = [p.detach().clone() for p in agent.actor.parameters()]
    out = tr.train_round(max_steps=60, max_iters=2)
    assert out["per_morph_iter"] >= 1
    for name in names:
        loss = tr.last_losses[name]
        assert all(np.isfinite(float(v)) for v in loss.values()), loss
    assert max(float((p.detach() - q).abs().max()) for p, q in zip(agent.actor.parameters(), before)) > 0
    # the rollout's HIP forward reads the live weights: it equals the module's forward on the same observations
    a1 = tr.ro.policy_forward(obs).clone()
    env, row = tr.ro.env, 0
    for gd, c in zip(tr.graph_dicts, env.counts):
        L = len(gd["parents"])
        agent.actor.change_morphology(gd)
        with torch.no_grad():
            want = agent.actor(obs[row:row + c, :41 * L])
        assert float((a1[row:row + c, :3 * L] - want).abs().max()) < 1e-5
        row += c
    # graphed updates keep today's behaviour: the switch is turned off with the HIP target chain
    fresh = _agent(seed=5, swat_train_kernels=True)
    assert fresh.use_swat_train_kernels and fresh.actor.train_kernels
    GraphedUpdates(fresh, 16)
    assert not fresh.use_swat_train_kernels and not fresh.use_swat_hip
    assert not any(getattr(m, "train_kernels", False) for net in (fresh.actor, fresh.critic) for m in net.modules())
