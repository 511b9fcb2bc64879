"""The differentiable passes of an SMP update on the training kernels, on the MI355X: the three kernel pairs of csrc/smp_train.hip
(through train_ops.smp_gather / smp_up_tail / normalize_rows) against their float64 restatements, their input handling and the
argument errors of their C ABI; whole networks with smp_policy's `train_kernels` switch, three Agent.update iterations and a
DeviceTrainer round with `smp_train_kernels=True`, each against float64 copies of the PyTorch modules."""
import copy
import ctypes

import numpy as np
import pytest

import smp_train_restate as R

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
MORPHS = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full", "3d_humanoid_9_full", "3d_cheetah_14_full"]
FN_NAMES = ("_SmpGatherFnBackward", "_SmpUpTailFnBackward", "_NormalizeRowsFnBackward")


def _f(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _grad_bar(ref):
    return 2e-5 * (float(np.abs(ref).max()) + 1)


def _torch_only(fn, *a, **k):
    """The fallback of a train_ops entry (the module's own operations), forced."""
    from sgrl_amd import train_ops
    enabled, train_ops.ENABLED = train_ops.ENABLED, False
    try:
        return fn(*a, **k)
    finally:
        train_ops.ENABLED = enabled


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def _up_table(n, mc, rng):
    """Children table [n, mc] over a source of n_src nodes: row 0 has no children (n > 1), one source node is read by nobody."""
    from sgrl_amd import train_ops
    pos = [(j, s) for j in range(1 if n > 1 else 0, n) for s in range(mc)]
    n_src = min(16, len(pos) + 1)
    node = -np.ones((n, mc), dtype=np.int32)
    nodes = rng.permutation(n_src)[:n_src - 1]
    for k, p in enumerate(rng.permutation(len(pos))[:len(nodes)]):
        node[pos[p]] = nodes[k]
    return train_ops.SmpTable(node, np.zeros((n, mc), dtype=np.int32)), n_src


def _down_table(n, mc, rng):
    """Parent table [n, 1]: limb 0 is a root (n > 1), every (parent, slot) is read at most once, at least one slot by nobody."""
    from sgrl_amd import train_ops
    count = n - (1 if n > 1 else 0)
    n_src = min(16, count + 1)
    pairs = rng.permutation(n_src * mc)[:count]
    node, off = -np.ones((n, 1), dtype=np.int32), np.zeros((n, 1), dtype=np.int32)
    for k, pr in enumerate(pairs):
        node[n - count + k, 0], off[n - count + k, 0] = pr // mc, 32 * (pr % mc)
    return train_ops.SmpTable(node, off), n_src


def _gather_case(kind, n, B, mc, seed, gain=1.0, zero_row=False):
    """-> (own, src, tab, normalize, act) as float32 CPU tensors."""
    import torch
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    if kind == "up":
        tab, n_src = _up_table(n, mc, rng)
        own, src = torch.randn(n, B, 64) * gain, torch.randn(n_src, B, 32) * gain
        if zero_row:
            own[0, 0] = 0
        return own, src, tab, True, True
    tab, n_src = _down_table(n, mc, rng)
    src = torch.randn(n_src, B, 32 * mc) * gain
    if kind == "down":
        return torch.randn(n, B, 32) * gain, src, tab, False, True
    return None, src, tab, False, False                    # "raw": the critic's parent message, W0 = 0


def _gather_ref(own, src, tab, normalize, act, d_out, B):
    o64 = None if own is None else own.double().numpy()
    s64 = None if src is None else src.double().numpy()
    out, inv = R.gather_forward(o64, s64, tab.node, tab.off, normalize, act, B=B)
    d_own, d_src = R.gather_backward(d_out.double().numpy(), out, o64, inv, None if src is None else tuple(src.shape), tab.node, tab.off,
                                     normalize, act)
    return out, d_own, d_src


def _gather_run(own, src, tab, normalize, act, d_out, B, torch_only=False):
    from sgrl_amd import train_ops
    o = None if own is None else own.cuda().requires_grad_()
    s = None if src is None else src.cuda().requires_grad_()
    call = lambda: train_ops.smp_gather(o, s, tab, normalize=normalize, act_tanh=act, batch=B)
    out = _torch_only(call) if torch_only else call()
    (out * d_out.cuda()).sum().backward()
    return (_f(out), None if o is None else _f(o.grad), None if s is None else _f(s.grad)), out


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mc", [1, 3, 5, 8])
@pytest.mark.parametrize("n,B", [(1, 1), (1, 23), (4, 23), (16, 23), (3, 130)])
def test_gather_matches_float64(n, B, mc):
    import torch
    for kind in ("up", "down", "raw"):
        for with_src in (True, False):
            if kind == "raw" and not with_src:
                continue                               # neither an own part nor a source: nothing to differentiate
            own, src, tab, normalize, act = _gather_case(kind, n, B, mc, seed=1000 * n + 10 * B + mc)
            src = src if with_src else None
            W0 = 0 if own is None else own.shape[-1]
            d_out = torch.randn(n, B, W0 + 32 * tab.S)
            ref = _gather_ref(own, src, tab, normalize, act, d_out, B)
            got, out = _gather_run(own, src, tab, normalize, act, d_out, B)
            assert type(out.grad_fn).__name__ == "_SmpGatherFnBackward"
            assert got[0].shape == ref[0].shape
            dev = [None if r is None else float(np.abs(g - r).max()) for g, r in zip(got, ref)]
            print("gather %s n %d B %d mc %d src %d: |out - ref| %.3g  |d_own - ref| %s  |d_src - ref| %s" % (kind, n, B, mc, with_src, dev[0], dev[1], dev[2]))
            assert dev[0] < 1e-5
            if own is not None:
                assert dev[1] < _grad_bar(ref[1])
            if src is not None:
                assert dev[2] < _grad_bar(ref[2])
                unread = ref[2] == 0                   # rows with all children missing read nothing; columns nobody reads come back exactly 0
                assert unread.any() and (got[2][unread] == 0).all()
                missing = tab.node < 0
                for j, s in zip(*np.nonzero(missing)):
                    assert (got[0][j, :, W0 + 32 * s:W0 + 32 * (s + 1)] == 0).all()
            else:
                assert (got[0][..., W0:] == 0).all()


@pytest.mark.parametrize("R_", [1, 23, 2080])
def test_up_tail_matches_float64(R_):
    import torch
    from sgrl_amd import train_ops
    torch.manual_seed(R_)
    a, w3, b3, du = torch.randn(R_, 64) * 1.5, torch.randn(32, 64) / 8, torch.randn(32) * 0.3, torch.randn(R_, 32)
    t, u, inv = R.up_tail_forward(a.numpy(), w3.numpy(), b3.numpy())
    dz, da, dw, db = R.up_tail_backward(du.numpy(), u, inv, t, w3.numpy())
    ag, wg, bg = a.cuda().requires_grad_(), w3.cuda().requires_grad_(), b3.cuda().requires_grad_()
    out = train_ops.smp_up_tail(ag, wg, bg)
    assert type(out.grad_fn).__name__ == "_SmpUpTailFnBackward" and out.shape == (R_, 32)
    (out * du.cuda()).sum().backward()
    dev = [float(np.abs(_f(x) - r).max()) for x, r in ((out, u), (ag.grad, da), (wg.grad, dw), (bg.grad, db))]
    print("up tail R %d: |u| %.3g |da| %.3g |dw| %.3g |db| %.3g" % (R_, *dev))
    assert dev[0] < 1e-5 and dev[1] < _grad_bar(da) and dev[2] < _grad_bar(dw) and dev[3] < _grad_bar(db)


@pytest.mark.parametrize("R_,W", [(1, 32), (23, 96), (23, 160), (2080, 256)])
def test_normalize_rows_matches_float64(R_, W):
    import torch
    from sgrl_amd import train_ops
    torch.manual_seed(R_ + W)
    x, dy = torch.randn(R_, W), torch.randn(R_, W)
    y, inv = R.normalize_forward(x.numpy())
    dx = R.normalize_backward(dy.numpy(), y, inv)
    xg = x.cuda().requires_grad_()
    out = train_ops.normalize_rows(xg)
    assert type(out.grad_fn).__name__ == "_NormalizeRowsFnBackward"
    (out * dy.cuda()).sum().backward()
    d0, d1 = float(np.abs(_f(out) - y).max()), float(np.abs(_f(xg.grad) - dx).max())
    print("normalize R %d W %d: |y| %.3g |dx| %.3g" % (R_, W, d0, d1))
    assert d0 < 1e-5 and d1 < _grad_bar(dx)


def _held(name, d, p, floor):
    print("%s: kernel %.3g  float32 PyTorch %.3g  floor %.3g" % (name, d, p, floor))
    assert np.isfinite(d) and d <= max(4 * p, floor), (name, d, p, floor)


def test_saturated_inputs():
    """Inputs six times larger: tanh saturates and 1 - t^2 is a difference of nearly equal numbers.  The kernels may deviate from
    float64 by at most max(4 x float32 PyTorch's own deviation on the same inputs, the bars of the tests above)."""
    import torch
    from sgrl_amd import train_ops
    n, B, mc = 4, 23, 3
    for kind in ("up", "down"):
        own, src, tab, normalize, act = _gather_case(kind, n, B, mc, seed=77, gain=6.0)
        d_out = torch.randn(n, B, own.shape[-1] + 32 * tab.S)
        ref = _gather_ref(own, src, tab, normalize, act, d_out, B)
        got, out = _gather_run(own, src, tab, normalize, act, d_out, B)
        pt, out_pt = _gather_run(own, src, tab, normalize, act, d_out, B, torch_only=True)
        assert type(out.grad_fn).__name__ == "_SmpGatherFnBackward" and type(out_pt.grad_fn).__name__ not in FN_NAMES
        assert float(np.median(np.abs(ref[0][..., own.shape[-1]:][ref[0][..., own.shape[-1]:] != 0]))) > 0.99      # saturated
        for name, g, p, r, fl in zip(("out", "d_own", "d_src"), got, pt, ref, (1e-5, _grad_bar(ref[1]), _grad_bar(ref[2]))):
            _held("saturated gather %s %s" % (kind, name), float(np.abs(g - r).max()), float(np.abs(p - r).max()), fl)
    torch.manual_seed(78)
    R_ = 23
    a, w3, b3, du = torch.randn(R_, 64) * 6, torch.randn(32, 64) / 8, torch.randn(32) * 0.3, torch.randn(R_, 32)
    t, u, inv = R.up_tail_forward(a.numpy(), w3.numpy(), b3.numpy())
    dz, da, dw, db = R.up_tail_backward(du.numpy(), u, inv, t, w3.numpy())
    res = []
    for torch_only in (False, True):
        ag, wg, bg = a.cuda().requires_grad_(), w3.cuda().requires_grad_(), b3.cuda().requires_grad_()
        out = _torch_only(train_ops.smp_up_tail, ag, wg, bg) if torch_only else train_ops.smp_up_tail(ag, wg, bg)
        assert (type(out.grad_fn).__name__ == "_SmpUpTailFnBackward") != torch_only
        (out * du.cuda()).sum().backward()
        res.append([_f(out), _f(ag.grad), _f(wg.grad), _f(bg.grad)])
    for name, g, p, r, fl in zip(("u", "da", "dw", "db"), res[0], res[1], (u, da, dw, db), (1e-5, _grad_bar(da), _grad_bar(dw), _grad_bar(db))):
        _held("saturated up tail %s" % name, float(np.abs(g - r).max()), float(np.abs(p - r).max()), fl)


def test_zero_norm_rows():
    """A row of zeros is divided by 1e-12 and its gradient is dy / 1e-12 (1e12 times the incoming gradient): held at max(4 x float32
    PyTorch's own deviation, the bars above); the other rows at the bars above, on their own scale."""
    import torch
    from sgrl_amd import train_ops
    torch.manual_seed(5)
    x, dy = torch.randn(23, 96), torch.randn(23, 96)
    x[7] = 0
    y, inv = R.normalize_forward(x.numpy())
    dx = R.normalize_backward(dy.numpy(), y, inv)
    res = []
    for torch_only in (False, True):
        xg = x.cuda().requires_grad_()
        out = _torch_only(train_ops.normalize_rows, xg) if torch_only else train_ops.normalize_rows(xg)
        assert (type(out.grad_fn).__name__ == "_NormalizeRowsFnBackward") != torch_only
        (out * dy.cuda()).sum().backward()
        res.append([_f(out), _f(xg.grad)])
    keep = [r for r in range(23) if r != 7]
    assert (res[0][0][7] == 0).all() and float(np.abs(res[0][0] - y).max()) < 1e-5
    assert float(np.abs(res[0][1][keep] - dx[keep]).max()) < _grad_bar(dx[keep])
    _held("zero row normalize dx", float(np.abs(res[0][1][7] - dx[7]).max()), float(np.abs(res[1][1][7] - dx[7]).max()), _grad_bar(dx[7]))
    own, src, tab, normalize, act = _gather_case("up", 4, 23, 3, seed=9, zero_row=True)
    d_out = torch.randn(4, 23, 64 + 96)
    ref = _gather_ref(own, src, tab, normalize, act, d_out, 23)
    got, out = _gather_run(own, src, tab, normalize, act, d_out, 23)
    pt, _ = _gather_run(own, src, tab, normalize, act, d_out, 23, torch_only=True)
    assert type(out.grad_fn).__name__ == "_SmpGatherFnBackward" and float(np.abs(got[0] - ref[0]).max()) < 1e-5
    mask = np.ones((4, 23), dtype=bool)
    mask[0, 0] = False
    assert float(np.abs(got[1][mask] - ref[1][mask]).max()) < _grad_bar(ref[1][mask])
    _held("zero row gather d_own", float(np.abs(got[1][0, 0] - ref[1][0, 0]).max()), float(np.abs(pt[1][0, 0] - ref[1][0, 0]).max()),
          _grad_bar(ref[1][0, 0]))


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
def test_input_handling():
    import torch
    from sgrl_amd import train_ops
    n, B, mc = 4, 23, 3
    own, src, tab, normalize, act = _gather_case("up", n, B, mc, seed=21)
    # a strided own (a slice of a wider tensor), an expanded incoming gradient
    wide = torch.zeros(n, B, 100, device="cuda:0")
    wide[..., 20:84] = own.cuda()
    wide.requires_grad_()
    s = src.cuda().requires_grad_()
    view = wide[..., 20:84]
    assert not view.is_contiguous()
    out = train_ops.smp_gather(view, s, tab, normalize=True, act_tanh=True)
    assert type(out.grad_fn).__name__ == "_SmpGatherFnBackward"
    row = torch.randn(64 + 32 * mc)
    go = row.cuda().expand(n, B, 64 + 32 * mc)
    assert not go.is_contiguous()
    out.backward(go)
    ref = _gather_ref(own, src, tab, True, True, row.expand(n, B, -1), B)
    g = _f(wide.grad)
    assert float(np.abs(_f(out) - ref[0]).max()) < 1e-5 and (g[..., :20] == 0).all() and (g[..., 84:] == 0).all()
    assert float(np.abs(g[..., 20:84] - ref[1]).max()) < _grad_bar(ref[1]) and float(np.abs(_f(s.grad) - ref[2]).max()) < _grad_bar(ref[2])
    # a frozen W3: no weight gradient, da still right; under deferred_wgrads fc3.weight.grad equals the immediate one
    torch.manual_seed(22)
    fc3 = torch.nn.Linear(64, 32).cuda()
    a, du = torch.randn(n, B, 64), torch.randn(n, B, 32)
    t, u, inv = R.up_tail_forward(a.reshape(-1, 64).numpy(), _f(fc3.weight), _f(fc3.bias))
    dz, da, dw, db = R.up_tail_backward(du.reshape(-1, 32).numpy(), u, inv, t, _f(fc3.weight))
    grads = {}
    for mode in ("immediate", "deferred", "frozen"):
        fc3.zero_grad()
        fc3.weight.requires_grad_(mode != "frozen")
        ag = a.cuda().requires_grad_()
        out = train_ops.smp_up_tail(ag, fc3.weight, fc3.bias)
        assert type(out.grad_fn).__name__ == "_SmpUpTailFnBackward" and out.shape == (n, B, 32)
        with train_ops.deferred_wgrads(enabled=mode == "deferred"):
            (out * du.cuda()).sum().backward()
            if mode == "deferred":
                assert fc3.weight.grad is None          # postponed to the end of the context
        assert float(np.abs(_f(ag.grad).reshape(-1, 64) - da).max()) < _grad_bar(da)
        grads[mode] = (fc3.weight.grad, fc3.bias.grad.clone())
    fc3.weight.requires_grad_(True)
    assert grads["frozen"][0] is None and torch.equal(grads["frozen"][1], grads["immediate"][1])
    assert torch.equal(grads["immediate"][0], grads["deferred"][0]) and torch.equal(grads["immediate"][1], grads["deferred"][1])
    assert float(np.abs(_f(grads["immediate"][0]) - dw).max()) < _grad_bar(dw) and float(np.abs(_f(grads["immediate"][1]) - db).max()) < _grad_bar(db)
    # torch.no_grad(): the module's operations, no graph
    with torch.no_grad():
        o_ng = train_ops.smp_gather(own.cuda().requires_grad_(), s, tab, normalize=True, act_tanh=True)
        n_ng = train_ops.normalize_rows(s)
        u_ng = train_ops.smp_up_tail(a.cuda(), fc3.weight, fc3.bias)
    assert all(o.grad_fn is None and not o.requires_grad for o in (o_ng, n_ng, u_ng))
    assert float(np.abs(_f(o_ng) - ref[0]).max()) < 1e-5 and float(np.abs(_f(u_ng).reshape(-1, 32) - u).max()) < 1e-5
    # 17 nodes, or 257 columns: more than the kernels hold -- the module's operations, differentiable
    tab17 = train_ops.SmpTable(-np.ones((17, mc), dtype=np.int32), np.zeros((17, mc), dtype=np.int32))
    tab17.node[5, 1] = 2
    tab17 = train_ops.SmpTable(tab17.node, tab17.off)
    own17, src17, d17 = torch.randn(17, 5, 64), torch.randn(3, 5, 32), torch.randn(17, 5, 64 + 32 * mc)
    got17, out17 = _gather_run(own17, src17, tab17, True, True, d17, 5)
    ref17 = _gather_ref(own17, src17, tab17, True, True, d17, 5)
    assert type(out17.grad_fn).__name__ not in FN_NAMES
    assert float(np.abs(got17[0] - ref17[0]).max()) < 1e-5 and float(np.abs(got17[1] - ref17[1]).max()) < _grad_bar(ref17[1])
    assert float(np.abs(got17[2] - ref17[2]).max()) < _grad_bar(ref17[2])
    x257 = torch.randn(9, 257).cuda().requires_grad_()
    y257 = train_ops.normalize_rows(x257)
    assert type(y257.grad_fn).__name__ not in FN_NAMES
    y257.square().sum().backward()
    assert float(np.abs(_f(y257) - R.normalize_forward(_f(x257))[0]).max()) < 1e-5 and x257.grad is not None
    # the same input twice: the same bits
    own2, src2, tab2, _, _ = _gather_case("up", 16, 130, 8, seed=31)
    d2 = torch.randn(16, 130, 64 + 256)
    first, _ = _gather_run(own2, src2, tab2, True, True, d2, 130)
    second, _ = _gather_run(own2, src2, tab2, True, True, d2, 130)
    assert all(np.array_equal(x, y) for x, y in zip(first, second))
    runs = []
    for _ in range(2):
        ag = torch.randn(2080, 64, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_()
        fc3.zero_grad()
        out = train_ops.normalize_rows(train_ops.smp_up_tail(ag, fc3.weight, fc3.bias))
        out[:, :7].sum().backward()
        runs.append([out.detach().clone(), ag.grad.clone(), fc3.weight.grad.clone(), fc3.bias.grad.clone()])
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_returned_not_faults():
    import torch
    from sgrl_amd import train_ops
    lib = train_ops._L()
    ERR_ARG, SENT = -1, 12345.0
    n, B, mc = 4, 6, 3
    own, src, tab, _, _ = _gather_case("up", n, B, mc, seed=41)
    n_src = src.shape[0]
    o, s = own.cuda(), src.cuda()
    sent = lambda *shape: torch.full(shape, SENT, device="cuda:0")
    out, inv, d_own, d_src = sent(n, B, 64 + 32 * mc), sent(n, B), sent(n, B, 64), sent(n_src, B, 32)
    d_out = torch.randn(n, B, 64 + 32 * mc).cuda()
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    hp = lambda a: ctypes.c_void_p(0 if a is None else a.ctypes.data)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    node, off = tab.node, tab.off

    def fwd(own_=o, W0=64, norm=1, src_=s, n_src_=n_src, Wsrc=32, node_=node, off_=off, S=mc, out_=out, inv_=inv, n_=n, B_=B):
        return lib.sgrl_smp_gather_forward(p(own_), W0, norm, p(src_), n_src_, Wsrc, hp(node_), hp(off_), S, 1, p(out_), p(inv_), n_, B_, st)

    def bwd(d_out_=d_out, out_=out, own_=o, inv_=inv, W0=64, n_src_=n_src, Wsrc=32, node_=node, off_=off, S=mc, d_own_=d_own, d_src_=d_src, n_=n, B_=B):
        return lib.sgrl_smp_gather_backward(p(d_out_), p(out_), p(own_), p(inv_), W0, 1, n_src_, Wsrc, hp(node_), hp(off_), S, 1, p(d_own_),
                                            p(d_src_), n_, B_, st)
    far, low, odd, late = node.copy(), node.copy(), off.copy(), off.copy()
    j, k = [int(v[0]) for v in np.nonzero(node >= 0)]
    far[j, k], low[j, k], odd[j, k], late[j, k] = n_src, -2, 16, 32
    twice = node.copy()
    twice[0, 0] = node[j, k]                               # row 0 has no children: now two entries read one node
    bad = [dict(own_=None), dict(out_=None), dict(inv_=None), dict(node_=None), dict(off_=None), dict(B_=0), dict(B_=-2), dict(n_=0), dict(n_=17),
           dict(S=0), dict(S=9), dict(W0=16), dict(W0=96), dict(Wsrc=48), dict(Wsrc=288), dict(Wsrc=0), dict(n_src_=0), dict(n_src_=17),
           dict(node_=far), dict(node_=low), dict(off_=odd), dict(off_=late)]
    for kw in bad:
        assert fwd(**kw) == ERR_ARG and b"sgrl_smp_gather_forward" in lib.sgrl_train_last_error(), kw
    bad_b = [dict(d_out_=None), dict(out_=None), dict(own_=None), dict(inv_=None), dict(d_own_=None, d_src_=None), dict(node_=None), dict(B_=0),
             dict(n_=0), dict(n_=17), dict(S=0), dict(S=9), dict(W0=16), dict(Wsrc=48), dict(Wsrc=288), dict(n_src_=0), dict(n_src_=17),
             dict(node_=far), dict(off_=odd), dict(off_=late), dict(node_=twice), dict(W0=0)]
    for kw in bad_b:
        assert bwd(**kw) == ERR_ARG and b"sgrl_smp_gather_backward" in lib.sgrl_train_last_error(), kw
    a, w3, b3 = torch.randn(B, 64).cuda(), torch.randn(32, 64).cuda() / 8, torch.randn(32).cuda()
    t, u, iv, dz, da = sent(B, 64), sent(B, 32), sent(B), sent(B, 32), sent(B, 64)
    du = torch.randn(B, 32).cuda()
    ut_f = lambda a_=a, w_=w3, b_=b3, t_=t, u_=u, i_=iv, R_=B: lib.sgrl_smp_up_tail_forward(p(a_), p(w_), p(b_), p(t_), p(u_), p(i_), R_, st)
    ut_b = lambda du_=du, u_=u, i_=iv, t_=t, w_=w3, dz_=dz, da_=da, R_=B: lib.sgrl_smp_up_tail_backward(p(du_), p(u_), p(i_), p(t_), p(w_), p(dz_), p(da_), R_, st)
    for kw in [dict(a_=None), dict(w_=None), dict(b_=None), dict(t_=None), dict(u_=None), dict(i_=None), dict(R_=0), dict(R_=-1)]:
        assert ut_f(**kw) == ERR_ARG and b"sgrl_smp_up_tail_forward" in lib.sgrl_train_last_error(), kw
    for kw in [dict(du_=None), dict(u_=None), dict(i_=None), dict(t_=None), dict(w_=None), dict(dz_=None), dict(da_=None), dict(R_=0)]:
        assert ut_b(**kw) == ERR_ARG and b"sgrl_smp_up_tail_backward" in lib.sgrl_train_last_error(), kw
    x = torch.randn(B, 96).cuda()
    y, ni, dx = sent(B, 96), sent(B), sent(B, 96)
    nf = lambda x_=x, y_=y, i_=ni, R_=B, W=96: lib.sgrl_row_normalize_forward(p(x_), p(y_), p(i_), R_, W, st)
    nb = lambda d_=x, y_=y, i_=ni, dx_=dx, R_=B, W=96: lib.sgrl_row_normalize_backward(p(d_), p(y_), p(i_), p(dx_), R_, W, st)
    for kw in [dict(x_=None), dict(y_=None), dict(i_=None), dict(R_=0), dict(W=0), dict(W=257)]:
        assert nf(**kw) == ERR_ARG and b"sgrl_row_normalize_forward" in lib.sgrl_train_last_error(), kw
    for kw in [dict(d_=None), dict(y_=None), dict(i_=None), dict(dx_=None), dict(R_=0), dict(W=0), dict(W=257)]:
        assert nb(**kw) == ERR_ARG and b"sgrl_row_normalize_backward" in lib.sgrl_train_last_error(), kw
    torch.cuda.synchronize()
    for buf in (out, inv, d_own, d_src, t, u, iv, dz, da, y, ni, dx):
        assert bool((buf == SENT).all())                   # nothing was launched
    # the well-formed calls go through and are correct
    assert fwd() == 0 and bwd() == 0 and ut_f() == 0 and ut_b() == 0 and nf() == 0
    torch.cuda.synchronize()
    ref = _gather_ref(own, src, tab, True, True, d_out.cpu(), B)
    assert float(np.abs(_f(out) - ref[0]).max()) < 1e-5 and float(np.abs(_f(d_own) - ref[1]).max()) < _grad_bar(ref[1])
    assert float(np.abs(_f(d_src) - ref[2]).max()) < _grad_bar(ref[2])
    t64, u64, i64 = R.up_tail_forward(_f(a), _f(w3), _f(b3))
    dz64, da64, _, _ = R.up_tail_backward(_f(du), u64, i64, t64, _f(w3))
    assert float(np.abs(_f(u) - u64).max()) < 1e-5 and float(np.abs(_f(t) - t64).max()) < 1e-5
    assert float(np.abs(_f(dz) - dz64).max()) < _grad_bar(dz64) and float(np.abs(_f(da) - da64).max()) < _grad_bar(da64)
    y64, ni64 = R.normalize_forward(_f(x))
    assert float(np.abs(_f(y) - y64).max()) < 1e-5 and float(np.abs(_f(ni) * ni64 ** -1 - 1).max()) < 1e-5
    assert nb() == 0
    torch.cuda.synchronize()
    assert float(np.abs(_f(dx) - R.normalize_backward(_f(x), y64, ni64)).max()) < _grad_bar(_f(x))
    assert fwd(src_=None, n_src_=0, Wsrc=0) == 0           # a null source is well formed: all segments zero
    torch.cuda.synchronize()
    assert bool((out[..., 64:] == 0).all())


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------
def _graphs(names):
    import torch
    from sgrl_amd import graph as G, mjcf
    return [G.getGraphDict(mjcf.load_asset(n).parents, TRAV, [], device=torch.device("cuda:0")) for n in names]


def _widest(parents):
    parents = [int(p) for p in parents]
    return max(parents.count(i) for i in range(len(parents)))


def _check_against_float64(names, on, off, ref, what):
    """on / off / ref: the tensors of one pass with the switch on, with the switch off and in float64 (outputs first, then the
    gradients from "x.grad" on).  Every tensor of `on` lies within max(4 x the switch-off float32 PyTorch deviation, 1e-5 x the
    largest float64 magnitude among the outputs, resp. among the gradients): the bar of tests/test_swat_train_gpu.py."""
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
    return worst


def _pass(net, kind, obs0, act0, proj, dtype):
    """One differentiable pass -> [outputs..., input gradients..., parameter gradients...] as float64 CPU tensors."""
    import torch
    net.zero_grad()
    obs = obs0.detach().to(dtype, copy=True).requires_grad_()
    if kind == "actor":
        outs, ins = [net(obs)], [obs]
    else:
        act = act0.detach().to(dtype, copy=True).requires_grad_()
        outs, ins = (list(net(obs, act)) if kind == "forward" else [net.Q1(obs, act)]), [obs, act]
    sum((o * pr.to(dtype)).sum() * (k + 1) for k, (o, pr) in enumerate(zip(outs, proj))).backward()
    zero = lambda p: torch.zeros(p.shape, dtype=torch.float64)
    return [o.detach().double().cpu() for o in outs] + [i.grad.double().cpu() for i in ins] + \
        [zero(p) if p.grad is None else p.grad.double().cpu() for p in net.parameters()]


@pytest.mark.parametrize("mc", [3, 5])
@pytest.mark.parametrize("kind", ["actor", "forward", "Q1"])
def test_networks_match_float64(kind, mc):
    """(the humanoid's torso has four children: it runs at max_children 4 where 3 is asked for)"""
    import torch
    from sgrl_amd.smp_policy import ActorGraphPolicy, CriticGraphPolicy
    B = 33
    for name, g in zip(MORPHS, _graphs(MORPHS)):
        m = max(mc, _widest(g["parents"]))
        torch.manual_seed(100 * mc + len(name))
        net = (ActorGraphPolicy(41, 3, 32, 1, 1.0, m, True, True, True) if kind == "actor" else
               CriticGraphPolicy(41, 3, 32, 1, m, True, True, True)).to("cuda:0")
        with torch.no_grad():
            for n_, p in net.named_parameters():       # biases away from their initial values
                if n_.endswith("bias"):
                    p.add_(torch.randn_like(p) * 0.1)
        on = copy.deepcopy(net)
        on.train_kernels = True
        n64 = copy.deepcopy(net).double()
        for x in (net, on, n64):
            x.change_morphology(g)
        L = len(g["parents"])
        gen = torch.Generator(device="cuda:0").manual_seed(L)
        obs = torch.randn((B, 41 * L), device="cuda:0", generator=gen)
        act = torch.rand((B, 3 * L), device="cuda:0", generator=gen) * 2 - 1
        proj = [torch.randn((B, 3 * L if kind == "actor" else 1), device="cuda:0", generator=gen) for _ in range(2)]
        n_in = 1 if kind == "actor" else 2
        n_o = 2 if kind == "forward" else 1
        names = ["out%d" % k for k in range(n_o)] + ["x.grad"] + ["u.grad"] * (n_in - 1) + [n_ for n_, _ in net.named_parameters()]
        ref = _pass(n64, kind, obs, act, proj, torch.float64)
        r_off = _pass(net, kind, obs, act, proj, torch.float32)
        r_on = _pass(on, kind, obs, act, proj, torch.float32)
        _check_against_float64(names, r_on, r_off, ref, "%s mc %d %s" % (kind, m, name))
        assert not all(torch.equal(a, b) for a, b in zip(r_on, r_off))          # the switch did take another path


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------
def _agent(seed=0, **kw):
    import torch
    from sgrl_amd.td3 import Agent, default_train_args
    torch.manual_seed(seed)
    return Agent(default_train_args(actor_type="smp", critic_type="smp", td=True, bu=True), device=torch.device("cuda:0"), **kw)


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
    import torch
    g = _graphs(["3d_walker_7_full"])[0]
    on = _agent(seed=30, smp_train_kernels=True)
    off = _agent(seed=31)
    f64 = _agent(seed=32, use_hip=False)
    with torch.no_grad():            # targets away from the online networks, as in the middle of a run
        gen = torch.Generator(device="cuda:0").manual_seed(33)
        for mod in (on.actor_target, on.critic_target):
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, device="cuda:0", generator=gen) * 0.02)
    off.load_state_dict(on.state_dict())
    f64.load_state_dict(on.state_dict())
    f64.double()
    assert on.use_smp_train_kernels and on.actor.train_kernels and on.critic.train_kernels
    assert not on.actor_target.train_kernels and not on.critic_target.train_kernels
    assert off.use_smp_hip and not off.use_smp_train_kernels and not off.actor.train_kernels and not f64.use_smp_hip
    agents = (("on", on), ("off", off), ("float64", f64))
    for _, agent in agents:
        agent.change_morphology(g)
        agent.models2train()
    data = [_batch(7, 33, seed=40 + it) for it in range(3)]
    cast = lambda tag, b, n: ({k: v.double() for k, v in b.items()}, n.double()) if tag == "float64" else (b, n)
    raw = {tag: _raw_gradients(agent, *cast(tag, *data[0]), skip) for tag, agent in agents}
    names = ["critic." + n for n, _ in on.critic.named_parameters()] + ["actor." + n for n, _ in on.actor.named_parameters()]
    flat = {tag: r[2] + r[3] for tag, r in raw.items()}
    scale = max(float(t.abs().max()) for t in flat["float64"])
    worst = 0.0
    for name, a, b, r in zip(names, flat["on"], flat["off"], flat["float64"]):
        d_on, d_off = float((a - r).abs().max()), float((b - r).abs().max())
        bar = max(4 * d_off, 1e-5 * scale)
        worst = max(worst, d_on / bar)
        assert np.isfinite(d_on) and d_on <= bar, (name, d_on, d_off, bar)
    assert not all(torch.equal(a, b) for a, b in zip(flat["on"], flat["off"]))
    print("skip %d raw gradients: %d tensors, largest |g64| %.3g, worst deviation / bar %.3g" % (skip, len(names), scale, worst))
    for k in (0, 1):
        ref = raw["float64"][k]
        d_on, d_off = abs(raw["on"][k] - ref) / abs(ref), abs(raw["off"][k] - ref) / abs(ref)
        assert d_on <= max(4 * d_off, 1e-5), (k, d_on, d_off)
    losses = {tag: [] for tag, _ in agents}
    for it in range(3):
        for tag, agent in agents:
            b, n = cast(tag, *data[it])
            out = agent.update(b, it, noise=n, skip_unused_critic_grads=skip)
            assert ("loss/actor_loss" in out) == (it % 2 == 0)
            losses[tag].append({k: float(torch.as_tensor(v).double()) for k, v in out.items() if k.startswith("loss/")})
    for it in range(3):
        for k, ref in losses["float64"][it].items():
            d_on, d_off = abs(losses["on"][it][k] - ref) / abs(ref), abs(losses["off"][it][k] - ref) / abs(ref)
            print("skip %d it %d %s: float64 %.9g  switch off rel dev %.3g  switch on rel dev %.3g" % (skip, it, k, ref, d_off, d_on))
            assert np.isfinite(losses["on"][it][k]) and d_on <= max(4 * d_off, 1e-5), (it, k, d_on, d_off)


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
def test_device_trainer_trains_with_the_switch_on():
    import torch
    from sgrl_amd.smp_hip import HipSmpActor
    from sgrl_amd.smp_policy import ActorGraphPolicy
    from sgrl_amd.td3 import GraphedUpdates, default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_walker_2_right_leg_left_knee", "3d_walker_7_full"]
    args = default_train_args(actor_type="smp", critic_type="smp", td=True, bu=True, smp_train_kernels=True, max_episode_steps=40)
    tr = DeviceTrainer(names, 4, args=args, seed=3, device="cuda:0", max_buffer_size=1024, batch_size=16)
    agent = tr.agent
    assert isinstance(agent.actor, ActorGraphPolicy) and isinstance(tr.ro.actor, HipSmpActor)
    assert agent.use_smp_train_kernels and agent.actor.train_kernels and agent.critic.train_kernels
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
    fresh = _agent(seed=5, smp_train_kernels=True)
    assert fresh.use_smp_train_kernels and fresh.actor.train_kernels
    GraphedUpdates(fresh, 16)
    assert not fresh.use_smp_train_kernels and not fresh.use_smp_hip
    assert not any(getattr(m, "train_kernels", False) for net in (fresh.actor, fresh.critic) for m in net.modules())
