"""Counter-RNG dropout of the SWAT networks on the MI355X: the element-wise kernel pair (csrc/dropout.hip) bit for bit against the
restatement (tests/dropout_restate.py), the attention pair with dropped softmax weights (csrc/train_gemm.hip k_swat_attn_*_drop)
against its float64 restatement, whole networks with `train_kernels`, three Agent.update iterations and a two-round DeviceTrainer
with dropout_rate 0.1, each against float64 copies of the PyTorch modules under the same dropout_rng."""
import copy
import ctypes

import numpy as np
import pytest

import dropout_restate as R
import test_swat_train_gpu as T

pytestmark = pytest.mark.gpu

SCALE = 64 ** -0.5
SEED = 0xC0FFEE1234567
ERR_ARG = -1
SITES_PER_NET = 13


def _lib_and_helpers():
    import torch
    from sgrl_amd import train_ops
    lib = train_ops._L()
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib, p, st


def _step(value):
    import torch
    return torch.tensor([value], dtype=torch.int64, device="cuda:0")


# ---- 1: the element-wise pair ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 1023, 4 * 15 * 128 + 3])
def test_elementwise_pair_is_the_restatement_bit_for_bit(n):
    """Aligned and unaligned (offset by one float) base pointers, input and output independently; forward and backward entry; every
    p; two values of the device step.  The floats around the output keep their sentinel: nothing is written out of bounds."""
    import torch
    lib, p_, st = _lib_and_helpers()
    x_host = torch.randn(n + 8, generator=torch.Generator().manual_seed(n))
    x_host[0] = -0.0
    xbuf = x_host.cuda()
    step = _step(0)
    site = n % 11
    for step_value in (5, 2 ** 33 + 1):
        step.fill_(step_value)
        for p in (0.0, 0.1, 0.5, 1.0):
            for xo, yo, fn in ((0, 0, lib.sgrl_dropout_forward), (1, 1, lib.sgrl_dropout_forward), (1, 0, lib.sgrl_dropout_backward),
                               (0, 1, lib.sgrl_dropout_backward)):
                ybuf = torch.full((n + 8,), 7.5, device="cuda:0")
                x, y = xbuf[xo:xo + n], ybuf[4 + yo:4 + yo + n]
                assert x.data_ptr() % 16 == 4 * xo and y.data_ptr() % 16 == 4 * yo
                assert fn(p_(x), p_(y), n, ctypes.c_float(p), ctypes.c_uint64(SEED), p_(step), site, st) == 0
                torch.cuda.synchronize()
                got = ybuf.cpu().numpy()
                want = R.dropout(x_host[xo:xo + n].numpy(), p, SEED, step_value, site)
                assert np.array_equal(got[4 + yo:4 + yo + n].view(np.uint32), want.view(np.uint32)), (p, xo, yo, step_value)
                assert (got[:4 + yo] == 7.5).all() and (got[4 + yo + n:] == 7.5).all()
                if p == 0.0:
                    assert np.array_equal(want.view(np.uint32), x_host[xo:xo + n].numpy().view(np.uint32))       # a bit copy
                if p == 1.0:
                    assert not want.any()


def test_elementwise_argument_errors_launch_nothing():
    import torch
    lib, p_, st = _lib_and_helpers()
    n = 64
    x, y, step = torch.randn(n, device="cuda:0"), torch.full((n,), 7.5, device="cuda:0"), _step(1)
    f32, u64 = ctypes.c_float, ctypes.c_uint64
    for name in ("sgrl_dropout_forward", "sgrl_dropout_backward"):
        fn = getattr(lib, name)
        bad = [(None, y, n, 0.1, step, 0), (x, None, n, 0.1, step, 0), (x, y, n, 0.1, None, 0), (x, y, 0, 0.1, step, 0), (x, y, -5, 0.1, step, 0),
               (x, y, n, -0.01, step, 0), (x, y, n, 1.01, step, 0), (x, y, n, float("nan"), step, 0), (x, y, n, 0.1, step, -1),
               (x, y, n, 0.1, step, 1 << 24), (x, x, n, 0.1, step, 0)]
        for a, b, n_, p, s, site in bad:
            assert fn(p_(a), p_(b), n_, f32(p), u64(SEED), p_(s), site, st) == ERR_ARG
            assert name.encode() in lib.sgrl_train_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.5).all())
    assert lib.sgrl_dropout_forward(p_(x), p_(y), n, f32(1.0), u64(SEED), p_(step), (1 << 24) - 1, st) == 0       # the ends are valid
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0


# ---- 2: the attention pair -------------------------------------------------------------------------------------------------------
def _attn_call(qkv, bias, d_o, p, step, site):
    """Both entry points through ctypes -> (w, o, dqkv, ds) as float64 arrays."""
    import torch
    lib, p_, st = _lib_and_helpers()
    B, L = qkv.shape[:2]
    q, b, g = qkv.cuda(), None if bias is None else bias.cuda(), d_o.cuda()
    w, o = torch.full((B, 2, L, L), 9.0, device="cuda:0"), torch.full((B, L, 128), 9.0, device="cuda:0")
    dqkv, ds = torch.full_like(q, 9.0), torch.full_like(w, 9.0)
    sc, pf, sd = ctypes.c_float(SCALE), ctypes.c_float(p), ctypes.c_uint64(SEED)
    assert lib.sgrl_swat_attention_forward_dropout(p_(q), p_(b), sc, p_(w), p_(o), B, L, pf, sd, p_(step), site, st) == 0
    assert lib.sgrl_swat_attention_backward_dropout(p_(q), sc, p_(w), p_(g), p_(dqkv), p_(ds), B, L, pf, sd, p_(step), site, st) == 0
    torch.cuda.synchronize()
    return tuple(t.double().cpu().numpy() for t in (w, o, dqkv, ds))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,L", [(1, 1), (3, 2), (5, 7), (4, 15)])
def test_attention_pair_matches_float64(B, L, with_bias, p):
    qkv, bias, d_o = T._attn_inputs(B, L, with_bias, seed=100 * L + B)
    step_value, site = 3 + L, B
    step = _step(step_value)
    bz = None if bias is None else bias.numpy()
    w64, o64, keep = R.attn_forward(qkv.numpy(), bz, SCALE, p, SEED, step_value, site)
    dqkv64, ds64 = R.attn_backward(qkv.numpy(), SCALE, w64, d_o.numpy(), p, SEED, step_value, site)
    w, o, dqkv, ds = _attn_call(qkv, bias, d_o, p, step, site)
    dev = [float(np.abs(a - b).max()) for a, b in ((w, w64), (o, o64), (dqkv, dqkv64), (ds.sum(0), ds64.sum(0)))]
    print("B %d L %d bias %d p %g: |w - w64| %.3g  |o - o64| %.3g  |dqkv - ref| %.3g (max %.3g)  |dbias - ref| %.3g (max %.3g)  kept %.3f"
          % (B, L, with_bias, p, dev[0], dev[1], dev[2], np.abs(dqkv64).max(), dev[3], np.abs(ds64.sum(0)).max(), keep.mean()))
    assert dev[0] < 1e-5                                            # w is stored undropped
    assert dev[1] < 1e-5
    assert dev[2] < 2e-5 * (float(np.abs(dqkv64).max()) + 1)
    assert dev[3] < 2e-5 * (float(np.abs(ds64.sum(0)).max()) + 1)
    dead = ~keep.any(axis=-1)                                       # [B, 2, L]: rows whose weights were all dropped
    o_heads = o.reshape(B, L, 2, 64).transpose(0, 2, 1, 3)
    assert (o_heads[dead] == 0).all()
    # the same (seed, step, site) again: the same bits
    again = _attn_call(qkv, bias, d_o, p, step, site)
    assert all(np.array_equal(a, b) for a, b in zip((w, o, dqkv, ds), again))
    # the step changes ON THE DEVICE, no host argument does: another mask, the restatement's for the new step
    step.add_(1)
    w2, o2, dqkv2, _ = _attn_call(qkv, bias, d_o, p, step, site)
    _, o64b, keep2 = R.attn_forward(qkv.numpy(), bz, SCALE, p, SEED, step_value + 1, site)
    assert np.array_equal(w2, w) and float(np.abs(o2 - o64b).max()) < 1e-5
    if not np.array_equal(keep2, keep):
        assert not np.array_equal(o2, o)


def test_attention_rows_with_every_weight_dropped_are_exact_zeros():
    """L = 1 and L = 2 at p = 0.5: a half resp. a quarter of the rows lose every weight (the restatement says which)."""
    for B, L in ((8, 1), (64, 2)):
        qkv, bias, d_o = T._attn_inputs(B, L, True, seed=B)
        step = _step(21)
        _, o64, keep = R.attn_forward(qkv.numpy(), bias.numpy(), SCALE, 0.5, SEED, 21, 0)
        dead = ~keep.any(axis=-1)
        assert dead.any() and not dead.all()
        w, o, dqkv, ds = _attn_call(qkv, bias, d_o, 0.5, step, 0)
        o_heads = o.reshape(B, L, 2, 64).transpose(0, 2, 1, 3)
        assert (o_heads[dead] == 0).all() and (o_heads[~dead] != 0).any()
        assert float(np.abs(o - o64).max()) < 1e-5
        assert (ds[dead] == 0).all()                                   # dw = 0 on such a row, so ds = w (0 - 0)


def test_attention_argument_errors_launch_nothing():
    import torch
    lib, p_, st = _lib_and_helpers()
    B, L = 4, 15
    qkv, bias, d_o = T._attn_inputs(B, L, True, seed=4)
    q, b, g, step = qkv.cuda(), bias.cuda(), d_o.cuda(), _step(1)
    w, o = torch.zeros(B, 2, L, L, device="cuda:0"), torch.zeros(B, L, 128, device="cuda:0")
    dqkv, ds = torch.zeros_like(q), torch.zeros_like(w)
    sc, sd = ctypes.c_float(SCALE), ctypes.c_uint64(SEED)
    fwd = lambda q_, w_, o_, B_, L_, p, s_, site: lib.sgrl_swat_attention_forward_dropout(p_(q_), p_(b), sc, p_(w_), p_(o_), B_, L_, ctypes.c_float(p),
                                                                                         sd, p_(s_), site, st)
    bwd = lambda q_, w_, g_, dq_, ds_, B_, L_, p, s_, site: lib.sgrl_swat_attention_backward_dropout(p_(q_), sc, p_(w_), p_(g_), p_(dq_), p_(ds_), B_, L_,
                                                                                                     ctypes.c_float(p), sd, p_(s_), site, st)
    for a in [(q, w, o, B, 0, .1, step, 0), (q, w, o, B, 16, .1, step, 0), (q, w, o, 0, L, .1, step, 0), (None, w, o, B, L, .1, step, 0),
              (q, None, o, B, L, .1, step, 0), (q, w, None, B, L, .1, step, 0), (q, w, o, B, L, .1, None, 0), (q, w, o, B, L, -.1, step, 0),
              (q, w, o, B, L, 1.5, step, 0), (q, w, o, B, L, .1, step, -1)]:
        assert fwd(*a) == ERR_ARG and b"sgrl_swat_attention_forward_dropout" in lib.sgrl_train_last_error()
    for a in [(q, w, g, dqkv, ds, B, 0, .1, step, 0), (q, w, g, dqkv, ds, B, 16, .1, step, 0), (q, w, g, dqkv, ds, 0, L, .1, step, 0),
              (None, w, g, dqkv, ds, B, L, .1, step, 0), (q, None, g, dqkv, ds, B, L, .1, step, 0), (q, w, None, dqkv, ds, B, L, .1, step, 0),
              (q, w, g, None, ds, B, L, .1, step, 0), (q, w, g, dqkv, None, B, L, .1, step, 0), (q, w, g, dqkv, ds, B, L, .1, None, 0),
              (q, w, g, dqkv, ds, B, L, 2.0, step, 0), (q, w, g, dqkv, ds, B, L, .1, step, 1 << 24)]:
        assert bwd(*a) == ERR_ARG and b"sgrl_swat_attention_backward_dropout" in lib.sgrl_train_last_error()
    torch.cuda.synchronize()
    assert float(w.abs().max()) == 0 and float(o.abs().max()) == 0 and float(dqkv.abs().max()) == 0 and float(ds.abs().max()) == 0


def test_train_ops_picks_the_dropout_pair_only_when_asked():
    """p > 0 and training under a dropout_rng: the dropout pair; p = 0 or not training: today's function, bit for bit today's result."""
    import torch
    from sgrl_amd import train_ops
    qkv, bias, d_o = T._attn_inputs(5, 7, True, seed=9)
    plain, o_plain = T._attn_run(qkv, bias, d_o)
    before = dict(train_ops.dropout_calls)
    with train_ops.dropout_rng(SEED, _step(4)) as rng:
        for kw in (dict(dropout_p=0.0, training=True), dict(dropout_p=0.3, training=False)):
            got, o = T._attn_run(qkv, bias, d_o, fn=lambda q, b, s: train_ops.swat_attention(q, b, s, **kw))
            assert type(o.grad_fn).__name__ == "_SwatAttnFnBackward" and all(np.array_equal(a, b) for a, b in zip(got, plain))
        assert rng.site == 0 and train_ops.dropout_calls == before
        got, o = T._attn_run(qkv, bias, d_o, fn=lambda q, b, s: train_ops.swat_attention(q, b, s, dropout_p=0.3, training=True))
        assert type(o.grad_fn).__name__ == "_SwatAttnDropFnBackward" and rng.site == 1
    w64, o64, _ = R.attn_forward(qkv.numpy(), bias.numpy(), SCALE, 0.3, SEED, 4, 0)
    dqkv64, ds64 = R.attn_backward(qkv.numpy(), SCALE, w64, d_o.numpy(), 0.3, SEED, 4, 0)
    assert float(np.abs(got[0] - o64).max()) < 1e-5 and float(np.abs(got[1] - dqkv64).max()) < 2e-5 * (float(np.abs(dqkv64).max()) + 1)
    assert float(np.abs(got[2] - ds64.sum(0)).max()) < 2e-5 * (float(np.abs(ds64.sum(0)).max()) + 1)
    # the element-wise function: kernels with autograd on the GPU, the torch restatement under no_grad -- the same bits
    x = torch.randn(5, 7, 128, device="cuda:0", requires_grad=True)
    with train_ops.dropout_rng(SEED, _step(4)):
        y = train_ops.dropout(x, 0.1, True)
    assert type(y.grad_fn).__name__ == "_DropoutFnBackward"
    y.backward(torch.ones_like(y))
    with torch.no_grad(), train_ops.dropout_rng(SEED, _step(4)):
        y_ng = train_ops.dropout(x, 0.1, True)
    want = R.dropout(x.detach().cpu().numpy(), 0.1, SEED, 4, 0)
    assert np.array_equal(y.detach().cpu().numpy(), want) and np.array_equal(y_ng.cpu().numpy(), want)
    assert np.array_equal(x.grad.cpu().numpy(), R.dropout(np.ones((5, 7, 128), dtype=np.float32), 0.1, SEED, 4, 0))


# ---- 3: networks -----------------------------------------------------------------------------------------------------------------
NET_MORPHS = ["3d_walker_3_left_knee_right_knee", "3d_walker_7_full"]


@pytest.mark.parametrize("feature,out", [(41, 3), (44, 1)])
def test_networks_with_dropout_match_float64(feature, out):
    """Actor (41 -> 3) and one critic network (44 -> 1) in training mode with dropout 0.1: switch on, switch off (float32 PyTorch
    operations, the same masks) and float64, every pass under dropout_rng with the same (seed, step).  The bar is that of
    test_swat_train_gpu.test_networks_match_float64: max(4 x the switch-off deviation, 1e-5 x scale), outputs and every gradient."""
    import torch
    from sgrl_amd import train_ops
    from sgrl_amd.set_policy import default_args
    from sgrl_amd.swat_policy import _model
    torch.manual_seed(feature)
    net = _model(feature, out, default_args(dropout_rate=0.1)).to("cuda:0").train()
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("bias") or "norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
    on = copy.deepcopy(net)
    on.train_kernels = True
    n64 = copy.deepcopy(net).double()
    assert on.training and n64.training and on.dropout == 0.1 and on.transformer_encoder.layers[2].self_attn.dropout == 0.1
    names = ["out", "x.grad"] + [n for n, _ in net.named_parameters()]
    B = 5
    for k, (name, g) in enumerate(zip(NET_MORPHS, T._graphs(NET_MORPHS))):
        L = len(g["parents"])
        gen = torch.Generator(device="cuda:0").manual_seed(L)
        x = torch.randn((B, L, feature), device="cuda:0", generator=gen)
        proj = torch.randn((B, L, out), device="cuda:0", generator=gen)
        step = _step(100 + k)
        res = {}
        for tag, model, gd, dt in (("f64", n64, T._g64(g), torch.float64), ("off", net, g, torch.float32), ("on", on, g, torch.float32)):
            before = dict(train_ops.dropout_calls)
            with train_ops.dropout_rng(SEED, step) as rng:
                res[tag] = T._net_pass(model, gd, x, proj, dt)
                assert rng.site == SITES_PER_NET
            used = {key: train_ops.dropout_calls[key] - before[key] for key in before}
            assert used == {"f64": dict(kernel=0, attention_kernel=0, counter=13, torch=0), "off": dict(kernel=13, attention_kernel=0, counter=0, torch=0),
                            "on": dict(kernel=10, attention_kernel=3, counter=0, torch=0)}[tag], (tag, used)
        T._check_against_float64(names, res["on"], res["off"], res["f64"], "dropout feature %d %s" % (feature, name))
        # dropout did act, and the step decides the masks
        n64.eval()
        plain = T._net_pass(n64, T._g64(g), x, proj, torch.float64)
        n64.train()
        assert float((plain[0] - res["f64"][0]).abs().max()) > 1e-3
        with train_ops.dropout_rng(SEED, _step(100 + k)):
            again = T._net_pass(on, g, x, proj, torch.float32)
        assert all(torch.equal(a, b) for a, b in zip(again, res["on"]))


# ---- 4: three updates -------------------------------------------------------------------------------------------------------------
def _agent(seed, **kw):
    import torch
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(seed)
    return Agent(default_train_args(actor_type="swat", critic_type="swat", dropout_rate=0.1, seed=77), device=torch.device("cuda:0"), **kw)


def test_three_updates_with_dropout_stay_on_float64(monkeypatch):
    """Three Agent.update iterations (two policy steps) of walker_3 at batch 6 with dropout_rate 0.1: training kernels on, off, and
    float64 PyTorch, one state_dict, the same batches, noise and dropout seed.  The bar of test_swat_train_gpu.
    test_three_updates_stay_on_float64: every loss within max(4 x the switch-off agent's relative deviation, 1e-5) of float64; the
    parameters after the three updates per tensor within max(4 x the switch-off deviation, 1e-5 x the largest float64 parameter)."""
    import torch
    from sgrl_amd import swat_hip, train_ops
    name = "3d_walker_3_left_knee_right_knee"
    g = T._graphs([name])[0]
    on, off, f64 = _agent(30, swat_train_kernels=True), _agent(31), _agent(32, use_hip=False)
    with torch.no_grad():
        gen = torch.Generator(device="cuda:0").manual_seed(33)
        for mod in (on.actor_target, on.critic_target):
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.02)
    off.load_state_dict(on.state_dict())
    f64.load_state_dict(on.state_dict())
    f64.double()
    assert on.use_swat_train_kernels and on.use_swat_hip and off.use_swat_hip and not off.use_swat_train_kernels and not f64.use_swat_hip
    assert on.dropout_rate == off.dropout_rate == f64.dropout_rate == np.float64(0.1) and on.dropout_seed == 77
    agents = (("on", on, g), ("off", off, g), ("float64", f64, T._g64(g)))
    for _, agent, gd in agents:
        agent.change_morphology(gd)
        agent.models2train()
    # the HIP target chain has no dropout: with the targets in training mode it must not run
    chain_calls = []
    monkeypatch.setattr(swat_hip.HipSwatTargets, "target_q", lambda self, *a, **k: chain_calls.append(1) or (_ for _ in ()).throw(AssertionError("HIP chain")))
    assert on._hip_targets(torch.zeros(6, 41 * 3, device="cuda:0")) is None
    # the masks the no-grad target passes of the switch-on agent draw, by (step, site)
    seen = {}
    inner = train_ops._counter_dropout

    def recording(x, p, rng, site):
        y = inner(x, p, rng, site)
        if recording.tag == "on" and site == 0:
            seen[int(rng.step)] = (y != 0).cpu().numpy()
        return y

    monkeypatch.setattr(train_ops, "_counter_dropout", recording)
    data = [T._batch(3, 6, seed=40 + it) for it in range(3)]
    cast = lambda tag, b, n: ({k: v.double() for k, v in b.items()}, n.double()) if tag == "float64" else (b, n)
    losses = {tag: [] for tag, _, _ in agents}
    for it in range(3):
        for tag, agent, _ in agents:
            recording.tag = tag
            b, n = cast(tag, *data[it])
            before = dict(train_ops.dropout_calls)
            out = agent.update(b, it, noise=n)
            used = {key: train_ops.dropout_calls[key] - before[key] for key in before}
            passes = 7 if it % 2 == 0 else 5          # target actor, two target critics, two critics (+ actor and Q1 on a policy step)
            assert sum(used.values()) == passes * SITES_PER_NET and used["torch"] == 0, (tag, it, used)
            if tag == "on":                            # the three target networks ran the MODULES (no-grad: the torch restatement)
                assert used["counter"] == 3 * SITES_PER_NET and used["attention_kernel"] == 3 * (passes - 3)
            assert int(agent._dropout_step) == it + 1
            assert ("loss/actor_loss" in out) == (it % 2 == 0)
            losses[tag].append({k: float(torch.as_tensor(v).double()) for k, v in out.items() if k.startswith("loss/")})
    assert not chain_calls
    assert sorted(seen) == [1, 2, 3] and not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[2], seen[3])
    assert np.array_equal(seen[2], R.keep_mask(77, 2, 0, 3 * 128, 0.1).reshape(3, 128))       # x: embedding rows, never exactly zero
    for it in range(3):
        for k, ref in losses["float64"][it].items():
            d_on, d_off = abs(losses["on"][it][k] - ref) / abs(ref), abs(losses["off"][it][k] - ref) / abs(ref)
            print("it %d %s: float64 %.9g  switch off rel dev %.3g  switch on rel dev %.3g" % (it, k, ref, d_off, d_on))
            assert np.isfinite(losses["on"][it][k]) and d_on <= max(4 * d_off, 1e-5), (it, k, d_on, d_off)
    named = lambda a: [("actor." + n, p) for n, p in a.actor.named_parameters()] + [("critic." + n, p) for n, p in a.critic.named_parameters()]
    ref = [p.detach().double().cpu() for _, p in named(f64)]
    scale = max(float(r.abs().max()) for r in ref)
    worst, failed = 0.0, []
    for (pname, a), (_, b), r in zip(named(on), named(off), ref):
        d_on, d_off = float((a.detach().double().cpu() - r).abs().max()), float((b.detach().double().cpu() - r).abs().max())
        bar = max(4 * d_off, 1e-5 * scale)
        worst = max(worst, d_on / bar)
        if not (np.isfinite(d_on) and d_on <= bar):
            failed.append((pname, d_on, d_off, bar))
    print("parameters after three updates: %d tensors, largest |p64| %.3g, worst deviation / bar %.3g" % (len(ref), scale, worst))
    assert not failed, failed


# ---- 5: the trainer ---------------------------------------------------------------------------------------------------------------
def test_device_trainer_trains_with_dropout():
    import torch
    from sgrl_amd import train_ops
    from sgrl_amd.swat_hip import HipSwatActor
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full"]
    args = default_train_args(actor_type="swat", critic_type="swat", swat_train_kernels=True, dropout_rate=0.1, max_episode_steps=40)
    tr = DeviceTrainer(names, 2, args=args, seed=3, device="cuda:0", max_buffer_size=1024, batch_size=16)
    agent = tr.agent
    assert isinstance(tr.ro.actor, HipSwatActor) and agent.use_swat_train_kernels and agent.dropout_rate == np.float64(0.1) and agent.dropout_seed == 3
    with pytest.raises(NotImplementedError, match="dropout"):
        DeviceTrainer(names, 2, args=args, seed=3, device="cuda:0", max_buffer_size=1024, batch_size=16, graph_updates=True)
    tr.warmup(30)
    before = [p.detach().clone() for p in agent.actor.parameters()]
    calls = dict(train_ops.dropout_calls)
    updates = 0
    for _ in range(2):
        out = tr.train_round(max_steps=60, max_iters=2)
        assert out["per_morph_iter"] >= 1
        updates += out["per_morph_iter"] * len(names)
        for name in names:
            assert all(np.isfinite(float(v)) for v in tr.last_losses[name].values()), tr.last_losses[name]
        assert not agent.actor.training and not agent.critic_target.training           # collection runs in eval mode
    assert int(agent._dropout_step) == updates
    assert train_ops.dropout_calls["attention_kernel"] > calls["attention_kernel"] and train_ops.dropout_calls["kernel"] > calls["kernel"]
    assert train_ops.dropout_calls["torch"] == calls["torch"]
    assert max(float((p.detach() - q).abs().max()) for p, q in zip(agent.actor.parameters(), before)) > 0
    # collection: the dropout-free HIP forward -- it equals the module's eval-mode forward on the same observations
    mid = dict(train_ops.dropout_calls)
    obs = tr.ro.env.obs.clone()
    a1 = tr.ro.policy_forward(obs).clone()
    env, row = tr.ro.env, 0
    for gd, c in zip(tr.graph_dicts, env.counts):
        L = len(gd["parents"])
        agent.actor.change_morphology(gd)
        with torch.no_grad():
            want = agent.actor(obs[row:row + c, :41 * L])
        assert float((a1[row:row + c, :3 * L] - want).abs().max()) < 1e-5
        row += c
    assert train_ops.dropout_calls == mid
    # a module in training mode with dropout is refused by the dropout-free HIP forward
    from sgrl_amd import _lib
    agent.actor.train()
    with pytest.raises(_lib.SgrlError, match="dropout"):
        tr.ro.policy_forward(obs)
    agent.actor.eval()
