"""The SET-only operators of sgrl_amd/train_ops.py (csrc/train_gemm.hip k_attn_*, k_gram_*, k_gram_tri_*, k_zmat_*, k_fold_sym /
k_unfold_sym) at their edges, each against float64 on the CPU with the tolerances tests/test_train_ops_gpu.py uses for the same
operator: one limb, one environment, saturated scores, one-sided upstream gradients, a frozen bias, strided inputs, the sizes at which
the kernels are not taken, one node, an odd node count, a zero node; and the argument errors of their C ABI, which are returned, not
faults."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 128 ** -0.5
ERR_ARG = -1


def _t(a):
    return a.detach().double().cpu()


# ---- set_attention ---------------------------------------------------------------------------------------------------------
def _scores(qkv):
    B, L = qkv.shape[:2]
    return torch.einsum("bihd,bjhd->bhij", qkv[..., :256].double().view(B, L, 2, 128), qkv[..., 256:512].double().view(B, L, 2, 128)) * SCALE


def _attn_inputs(B, L, with_bias, seed, max_score=None):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, L, 768, generator=g) * 0.6
    vgp, gdir = torch.randn(B, L, 3, 252, generator=g), torch.randn(B, L, 3, 2, generator=g)
    bias = torch.randn(2, L, L, generator=g) if with_bias else None
    if max_score is not None:
        # per (environment, head): the query row and the key row of the largest |scale q . k| scaled so that it becomes max_score -- that
        # row of scores is all but one-hot (or, at -max_score, loses an entry), the key's column spreads to a dozen.  Scaling ALL of q
        # and k instead puts hundreds of unsaturated entries at 40 .. 80, where a float32 score carries 4e-6 of rounding however it is
        # summed: float32 PyTorch then deviates from float64 by 1.07e-5 in og, above this file's 1e-5 (the kernel: 2.1e-5; measured
        # on the MI355X, 23 x 14 limbs) -- no float32 evaluation could be held to the bar on such inputs.
        s = _scores(qkv)
        for b in range(B):
            for h in range(2):
                e = int(s[b, h].abs().argmax())
                i, j = e // L, e % L
                gain = float(np.sqrt(max_score / float(s[b, h, i, j].abs())))
                qkv[b, i, 128 * h:128 * h + 128] *= gain
                qkv[b, j, 256 + 128 * h:256 + 128 * h + 128] *= gain
    return qkv, vgp, gdir, bias, torch.randn(B, L, 256, generator=g), torch.randn(B, L, 3, 256, generator=g)


def _attn_ref(qkv, vgp, gdir, bias, d_o, d_og):
    """The einsum formulation of train_ops.set_attention in float64 on the CPU -> (o, og, [dqkv, dvgp, dgdir, dbias or None])."""
    from sgrl_amd import train_ops
    leaves = [t.double().requires_grad_() for t in (qkv, vgp, gdir)] + [None if bias is None else bias.double().requires_grad_()]
    enabled, train_ops.ENABLED = train_ops.ENABLED, False
    try:
        o, og = train_ops.set_attention(*leaves, SCALE)
    finally:
        train_ops.ENABLED = enabled
    loss = 0.0
    if d_o is not None:
        loss = loss + (o * d_o.double()).sum()
    if d_og is not None:
        loss = loss + (og * d_og.double()).sum()
    loss.backward()
    return o.detach(), og.detach(), [None if t is None else t.grad for t in leaves]


def _attn_run(qkv, vgp, gdir, bias, d_o, d_og, bias_grad=True, wrap=None):
    from sgrl_amd import train_ops
    leaves = [t.cuda().requires_grad_() for t in (qkv, vgp, gdir)]
    b = None if bias is None else (bias.cuda().requires_grad_() if bias_grad else bias.cuda())
    ins = leaves if wrap is None else wrap(leaves)
    o, og = train_ops.set_attention(ins[0], ins[1], ins[2], b, SCALE)
    loss = 0.0
    if d_o is not None:
        loss = loss + (o * d_o.cuda()).sum()
    if d_og is not None:
        loss = loss + (og * d_og.cuda()).sum()
    loss.backward()
    return o, og, [t.grad for t in leaves] + [None if b is None else b.grad]


def _attn_check(got, ref, what):
    o, og, grads = got
    o_r, og_r, grads_r = ref
    d_o, d_og = float((_t(o) - o_r).abs().max()), float((_t(og) - og_r).abs().max())
    print("%s: |o - o64| %.3g  |og - og64| %.3g" % (what, d_o, d_og))
    assert torch.isfinite(o).all() and torch.isfinite(og).all()
    assert d_o < 1e-5 and d_og < 1e-5, (what, d_o, d_og)
    for g, r, name in zip(grads, grads_r, "qkv vgp gdir bias".split()):
        if r is None:          # nothing reaches this input in float64: no gradient here either, or one that is zero
            assert g is None or float(g.abs().max()) == 0.0, name
            continue
        assert g is not None and g.shape == r.shape, name
        d = float((_t(g) - r).abs().max())
        print("%s: |d%s - ref| %.3g (max |ref| %.3g)" % (what, name, d, float(r.abs().max())))
        assert torch.isfinite(g).all() and d < 2e-5 * (float(r.abs().max()) + 1), (what, name, d)


@pytest.mark.parametrize("B,L,with_bias", [(1, 1, True), (3, 1, False), (1, 14, True), (5, 13, True)])
def test_attention_at_the_smallest_and_largest_sizes(B, L, with_bias):
    ins = _attn_inputs(B, L, with_bias, seed=10 * L + B)
    got = _attn_run(*ins)
    assert type(got[0].grad_fn).__name__.startswith("_AttnFn")
    _attn_check(got, _attn_ref(*ins), "B %d L %d bias %d" % (B, L, with_bias))
    if L == 1:          # a softmax over one entry: w = 1 exactly -- the values pass through, q and k receive nothing
        qkv, vgp, gdir = ins[:3]
        assert torch.equal(got[0].cpu(), qkv[..., 512:])
        assert torch.equal(got[1].cpu().view(B, 1, 3, 2, 128)[..., :126], vgp.view(B, 1, 3, 2, 126))
        assert float(got[2][0][..., :512].abs().max()) == 0.0 and torch.equal(got[2][0][..., 512:].cpu(), ins[4])
        if with_bias:
            assert float(got[2][3].abs().max()) == 0.0


@pytest.mark.parametrize("with_bias", [True, False])
def test_attention_with_large_scores(with_bias):
    """|scale q . k| of 80 in every (environment, head): e^80 = 5.5e34 is within a factor of 1e4 of float32's largest number, the other
    entries of such a row underflow against it -- the kernel subtracts the row maximum.  Finite, and on float64 at the usual bars."""
    B, L = 23, 14
    ins = _attn_inputs(B, L, with_bias, seed=7, max_score=80.0)
    s = _scores(ins[0])
    assert 79.9 < float(s.abs().max()) < 80.1 and float(s.abs().flatten(1).max(1)[0].min()) > 79.9          # reached in every environment
    assert float(s.max()) > 79.9 and float(s.min()) < -79.9          # on both sides
    got = _attn_run(*ins)
    assert type(got[0].grad_fn).__name__.startswith("_AttnFn")
    _attn_check(got, _attn_ref(*ins), "large scores, bias %d" % with_bias)


@pytest.mark.parametrize("side", ["o", "og"])
def test_attention_with_a_one_sided_upstream_gradient(side):
    ins = list(_attn_inputs(6, 9, True, seed=21))
    ins[4 if side == "og" else 5] = None          # the loss reads one output only
    got = _attn_run(*ins)
    assert type(got[0].grad_fn).__name__.startswith("_AttnFn")
    _attn_check(got, _attn_ref(*ins), "upstream gradient on %s only" % side)
    if side == "o":             # nothing reaches the vector values
        assert float(got[2][1].abs().max()) == 0.0 and float(got[2][2].abs().max()) == 0.0


def test_attention_input_handling():
    from sgrl_amd import train_ops
    ins = _attn_inputs(4, 7, True, seed=3)
    ref = _attn_ref(*ins)
    # a bias that does not require a gradient
    got = _attn_run(*ins, bias_grad=False)
    assert type(got[0].grad_fn).__name__.startswith("_AttnFn") and got[2][3] is None
    _attn_check((got[0], got[1], got[2][:3] + [None]), (ref[0], ref[1], ref[2][:3] + [None]), "frozen bias")
    # qkv a slice of a wider tensor
    def wrap(leaves):
        wide = torch.zeros(4, 7, 900, device="cuda")
        wide[..., 100:868] = leaves[0]
        view = wide[..., 100:868]
        assert not view.is_contiguous()
        return [view, leaves[1], leaves[2]]
    got = _attn_run(*ins, wrap=wrap)
    assert type(got[0].grad_fn).__name__.startswith("_AttnFn")
    _attn_check(got, ref, "strided qkv")
    # 15 limbs: more than the kernels hold -- the einsum formulation, differentiable, no kernel in the graph
    ins15 = _attn_inputs(3, 15, True, seed=15)
    got = _attn_run(*ins15)
    assert got[0].grad_fn is not None and "_AttnFn" not in type(got[0].grad_fn).__name__ and "_AttnFn" not in type(got[1].grad_fn).__name__
    _attn_check(got, _attn_ref(*ins15), "L 15")
    # torch.no_grad(): no graph
    with torch.no_grad():
        o, og = train_ops.set_attention(ins[0].cuda(), ins[1].cuda(), ins[2].cuda(), ins[3].cuda(), SCALE)
    assert o.grad_fn is None and float((_t(o) - ref[0]).abs().max()) < 1e-5 and float((_t(og) - ref[1]).abs().max()) < 1e-5


# ---- gram_fn / gram_tri_fn ---------------------------------------------------------------------------------------------------
_TRI = torch.tril_indices(32, 32)          # row-major over the lower triangle: entry k = a (a + 1) / 2 + b is (a, b)


def _gram_ref(z, dgram, dfn, tri):
    """float64: vec(Z'Z) [M, 1024] (tri: its lower triangle packed [M, 528]), ||Z'Z||_F + 1 from the FULL symmetric matrix, and dz
    for loss = <gram, dgram> + <fn, dfn> (a part that is None is left out; no norm term at a zero node)."""
    zr = z.double().requires_grad_()
    full = torch.einsum("msa,msc->mac", zr, zr)
    gram = full[:, _TRI[0], _TRI[1]] if tri else full.flatten(-2)
    nrm = full.flatten(-2).norm(dim=-1, keepdim=True)
    fn = nrm + 1.0
    dz = torch.zeros_like(zr)
    if dgram is not None:
        dz = dz + torch.autograd.grad((gram * dgram.double()).sum(), zr, retain_graph=True)[0]
    if dfn is not None:
        dz = dz + torch.nan_to_num(torch.autograd.grad((fn * dfn.double()).sum(), zr)[0])
    return gram.detach(), fn.detach(), dz


@pytest.mark.parametrize("use", ["both", "gram", "fn"])
@pytest.mark.parametrize("M", [1, 2, 257])
@pytest.mark.parametrize("tri", [False, True], ids=["full", "tri"])
def test_gram_invariants_match_float64(tri, M, use):
    from sgrl_amd import train_ops
    g = torch.Generator().manual_seed(100 * M + tri)
    z = torch.randn(M, 3, 32, generator=g) * 0.7
    if M > 1:
        z[M // 2] = 0.0                                      # a node whose Gram matrix vanishes: no norm term, no NaN
    width = 528 if tri else 1024
    dgram = torch.randn(M, width, generator=g) if use in ("both", "gram") else None
    dfn = torch.randn(M, 1, generator=g) if use in ("both", "fn") else None
    gr, fr, dzr = _gram_ref(z, dgram, dfn, tri)
    zd = z.cuda().requires_grad_()
    gram, fn = (train_ops.gram_tri_fn if tri else train_ops.gram_fn)(zd)
    assert type(gram.grad_fn).__name__.startswith("_GramTriFn" if tri else "_GramFn")
    assert gram.shape == (M, width) and fn.shape == (M, 1)
    loss = 0.0
    if dgram is not None:
        loss = loss + (gram * dgram.cuda()).sum()
    if dfn is not None:
        loss = loss + (fn * dfn.cuda()).sum()
    loss.backward()
    d = (float((_t(gram) - gr).abs().max()), float((_t(fn) - fr).abs().max()), float((_t(zd.grad) - dzr).abs().max()))
    print("tri %d M %d %s: |gram - ref| %.3g  |fn - ref| %.3g (max %.3g)  |dz - ref| %.3g (max %.3g)" % (tri, M, use, d[0], d[1], float(fr.max()), d[2], float(dzr.abs().max())))
    assert torch.isfinite(zd.grad).all()
    assert d[0] < 1e-5 and d[1] < 1e-5 * float(fr.max()) and d[2] < 2e-5 * (float(dzr.abs().max()) + 1)
    if M > 1:
        assert float(fn.detach()[M // 2]) == 1.0 and float(gram.detach()[M // 2].abs().max()) == 0.0
        if use == "fn":
            assert float(zd.grad[M // 2].abs().max()) == 0.0


@pytest.mark.parametrize("tri", [False, True], ids=["full", "tri"])
def test_gram_backward_with_one_null_upstream_at_the_abi(tri):
    """The C ABI takes a null dgram (dtri) OR a null dfn -- autograd always hands over both, zero filled --: each against float64."""
    from sgrl_amd import train_ops
    lib = train_ops._L()
    M, width = 5, 528 if tri else 1024
    g = torch.Generator().manual_seed(31 + tri)
    z = torch.randn(M, 3, 32, generator=g) * 0.7
    z[2] = 0.0
    dgram, dfn = torch.randn(M, width, generator=g), torch.randn(M, 1, generator=g)
    zd, gd, fd = z.cuda().reshape(M, 96), dgram.cuda(), dfn.cuda().reshape(M)
    gram, fn = torch.empty(M, width, device="cuda"), torch.empty(M, device="cuda")
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fwd, bwd = (lib.sgrl_gram_tri_forward, lib.sgrl_gram_tri_backward) if tri else (lib.sgrl_gram_forward, lib.sgrl_gram_backward)
    assert fwd(p(zd), p(gram), p(fn), M, st) == 0
    for a, b, what in ((gd, None, "gram"), (None, fd, "fn")):
        dz = torch.full((M, 96), 7.0, device="cuda")
        assert bwd(p(zd), p(a), p(b), p(fn), p(dz), M, st) == 0
        torch.cuda.synchronize()
        ref = _gram_ref(z, dgram if a is not None else None, dfn if b is not None else None, tri)[2]
        dev = float((_t(dz).view(M, 3, 32) - ref).abs().max())
        print("tri %d, upstream on %s only: |dz - ref| %.3g (max %.3g)" % (tri, what, dev, float(ref.abs().max())))
        assert dev < 2e-5 * (float(ref.abs().max()) + 1)


# ---- zmat --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3])
def test_zmat_with_few_nodes(M):
    """Two nodes per workgroup: an odd count leaves half a workgroup without one."""
    from sgrl_amd import train_ops
    g = torch.Generator().manual_seed(40 + M)
    z, mat, dt = torch.randn(M, 3, 32, generator=g), torch.randn(M, 32, 32, generator=g) * 0.2, torch.randn(M, 3, 32, generator=g)
    zr, mr = z.double().requires_grad_(), mat.double().requires_grad_()
    tr = torch.einsum("msa,mac->msc", zr, mr)
    tr.backward(dt.double())
    zd, md = z.cuda().requires_grad_(), mat.cuda().requires_grad_()
    t = train_ops.zmat(zd, md)
    assert type(t.grad_fn).__name__.startswith("_ZmatFn") and t.shape == (M, 3, 32)
    t.backward(dt.cuda())
    assert float((_t(t) - tr.detach()).abs().max()) < 1e-5
    assert float((_t(zd.grad) - zr.grad).abs().max()) < 1e-5
    assert float((_t(md.grad) - mr.grad).abs().max()) < 1e-5


# ---- tri_weights -------------------------------------------------------------------------------------------------------------
def _fold64(w):
    a, b = _TRI[0], _TRI[1]
    return torch.where(a == b, w[:, a * 33], w[:, a * 32 + b] + w[:, b * 32 + a])


def test_tri_weights_fold_and_unfold_sixteen_matrices():
    from sgrl_amd import train_ops
    rows = [1, 30, 128, 256, 2, 3, 64, 17, 255, 5, 100, 31, 33, 7, 129, 9]
    g = torch.Generator().manual_seed(16)
    ws = [torch.randn(r, 1024, generator=g) for r in rows]
    ds = [torch.randn(r, 528, generator=g) for r in rows]
    like = torch.zeros(1, device="cuda")
    wd = [torch.nn.Parameter(w.cuda()) for w in ws]
    out = train_ops.tri_weights(wd, like)
    assert out is not None and len(out) == 16
    sum((o * d.cuda()).sum() for o, d in zip(out, ds)).backward()
    for r, w, d, o, p in zip(rows, ws, ds, out, wd):
        assert o.shape == (r, 528) and type(o.grad_fn).__name__.startswith("_FoldFn")
        wr = w.double().requires_grad_()
        fr = _fold64(wr)
        (fr * d.double()).sum().backward()
        # one float32 addition per folded entry: half an ulp of the result
        assert float(((_t(o) - fr.detach()).abs() - 2.0 ** -24 * fr.detach().abs()).max()) <= 0.0, r
        assert torch.equal(_t(p.grad), wr.grad), r          # the unfold copies: both mirror columns receive the folded entry's gradient
    # 17 matrices: more than one launch takes -- None, and the callers keep the unfolded weights with gram_fn
    assert train_ops.tri_weights(wd + [torch.nn.Parameter(ws[0].cuda())], like) is None
    # nothing differentiated, or another width: None as well
    assert train_ops.tri_weights([w.cuda() for w in ws[:2]], like) is None
    assert train_ops.tri_weights([torch.nn.Parameter(torch.randn(4, 528).cuda())], like) is None


# ---- argument errors of the C ABI ------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_returned_not_faults():
    """Only what the entry points reject on the host: nothing here reaches a kernel."""
    from sgrl_amd import train_ops
    lib = train_ops._L()
    B, L, M = 3, 7, 4
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc = ctypes.c_float(SCALE)
    new = lambda *s: torch.full(s, 7.0, device="cuda")          # the sentinel
    outs = []

    def bad(rc, name):
        assert rc == ERR_ARG, (name, rc)
        assert name.encode() in lib.sgrl_train_last_error(), (name, lib.sgrl_train_last_error())

    # attention
    qkv, vgp, gdir, bias = new(B, 14, 768), new(B, 14, 3, 252), new(B, 14, 3, 2), new(2, 14, 14)
    w, o, og = new(B, 2, 14, 14), new(B, 14, 256), new(B, 14, 3, 256)
    d_o, d_og, dqkv, dvgp, dgdh, ds = new(B, 14, 256), new(B, 14, 3, 256), new(B, 14, 768), new(B, 14, 3, 252), new(B, 14, 3, 2, 2), new(B, 2, 14, 14)
    outs += [w, o, og, dqkv, dvgp, dgdh, ds]
    fwd = lambda q_, v_, g_, w_, o_, og_, B_, L_: lib.sgrl_attention_forward(p(q_), p(v_), p(g_), p(bias), sc, p(w_), p(o_), p(og_), B_, L_, st)
    for a in [(qkv, vgp, gdir, w, o, og, B, 0), (qkv, vgp, gdir, w, o, og, B, 15), (qkv, vgp, gdir, w, o, og, 0, L), (qkv, vgp, gdir, w, o, og, -2, L),
              (None, vgp, gdir, w, o, og, B, L), (qkv, None, gdir, w, o, og, B, L), (qkv, vgp, None, w, o, og, B, L), (qkv, vgp, gdir, None, o, og, B, L),
              (qkv, vgp, gdir, w, None, og, B, L), (qkv, vgp, gdir, w, o, None, B, L)]:
        bad(fwd(*a), "sgrl_attention_forward")
    full = [qkv, vgp, gdir, w, d_o, d_og, dqkv, dvgp, dgdh, ds]
    bwd = lambda t, B_, L_: lib.sgrl_attention_backward(p(t[0]), p(t[1]), p(t[2]), sc, p(t[3]), p(t[4]), p(t[5]), p(t[6]), p(t[7]), p(t[8]), p(t[9]), B_, L_, st)
    for B_, L_ in ((B, 0), (B, 15), (0, L)):
        bad(bwd(full, B_, L_), "sgrl_attention_backward")
    for k in range(len(full)):
        bad(bwd(full[:k] + [None] + full[k + 1:], B, L), "sgrl_attention_backward")
    # Gram invariants, full and triangular
    z, fn, dz, dfn = new(M, 96), new(M), new(M, 96), new(M)
    for width, f, b in ((1024, "sgrl_gram_forward", "sgrl_gram_backward"), (528, "sgrl_gram_tri_forward", "sgrl_gram_tri_backward")):
        gram, dgram = new(M, width), new(M, width)
        outs += [gram]
        ff, bf = getattr(lib, f), getattr(lib, b)
        for a in [(z, gram, fn, 0), (z, gram, fn, -1), (None, gram, fn, M), (z, None, fn, M), (z, gram, None, M)]:
            bad(ff(p(a[0]), p(a[1]), p(a[2]), a[3], st), f)
        for a in [(z, dgram, dfn, fn, dz, 0), (None, dgram, dfn, fn, dz, M), (z, dgram, dfn, None, dz, M), (z, dgram, dfn, fn, None, M),
                  (z, None, None, fn, dz, M)]:          # neither upstream gradient: nothing to do is an error
            bad(bf(p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), a[5], st), b)
    outs += [fn, dz]
    # zmat
    mat, t, dt, dzz, dmat = new(M, 1024), new(M, 96), new(M, 96), new(M, 96), new(M, 1024)
    outs += [t, dzz, dmat]
    for a in [(z, mat, t, 0), (None, mat, t, M), (z, None, t, M), (z, mat, None, M)]:
        bad(lib.sgrl_zmat_forward(p(a[0]), p(a[1]), p(a[2]), a[3], st), "sgrl_zmat_forward")
    for a in [(z, mat, dt, dzz, dmat, 0), (None, mat, dt, dzz, dmat, M), (z, None, dt, dzz, dmat, M), (z, mat, None, dzz, dmat, M),
              (z, mat, dt, None, dmat, M), (z, mat, dt, dzz, None, M)]:
        bad(lib.sgrl_zmat_backward(p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), a[5], st), "sgrl_zmat_backward")
    # fold / unfold
    full_w, tri_w = [new(2, 1024) for _ in range(17)], [new(2, 528) for _ in range(17)]
    outs += tri_w + full_w

    def fold(n, rows, unfold, null_at=None):
        pw = (ctypes.c_void_p * 17)(*[0 if i == null_at else t.data_ptr() for i, t in enumerate(full_w)])
        pt = (ctypes.c_void_p * 17)(*[t.data_ptr() for t in tri_w])
        return lib.sgrl_sym_fold(n, pw, pt, (ctypes.c_int * 17)(*rows), unfold, st)
    for unfold in (0, 1):
        bad(fold(0, [2] * 17, unfold), "sgrl_sym_fold")
        bad(fold(17, [2] * 17, unfold), "sgrl_sym_fold")
        bad(fold(3, [2, 0, 2] + [2] * 14, unfold), "sgrl_sym_fold")
        bad(fold(3, [2, 2, -1] + [2] * 14, unfold), "sgrl_sym_fold")
        bad(fold(3, [2] * 17, unfold, null_at=1), "sgrl_sym_fold")
    bad(lib.sgrl_sym_fold(2, None, None, None, 0, st), "sgrl_sym_fold")
    # residual + LayerNorm
    R_ = 6
    x, lw, lb, y, xhat, rstd = new(3 * R_, 128), new(128), new(128), new(3 * R_, 128), new(3 * R_, 128), new(3 * R_)
    dx, dw0, db0 = new(3 * R_, 128), new(128), new(128)
    outs += [y, xhat, rstd, dx, dw0, db0]
    eps = ctypes.c_float(1e-5)
    lnf = lambda x_, w0, b0, w1, b1, y_, xh, rs, rows, nets: lib.sgrl_add_ln_forward(p(x_), p(None), p(w0), p(b0), p(w1), p(b1), p(y_), p(xh), p(rs), rows, nets, eps, st)
    for a in [(x, lw, lb, lw, lb, y, xhat, rstd, R_, 3), (x, lw, lb, None, None, y, xhat, rstd, R_, 0), (x, lw, lb, None, None, y, xhat, None, R_, 1),
              (x, lw, lb, None, None, y, None, rstd, R_, 1), (x, lw, lb, None, lb, y, xhat, rstd, R_, 2), (x, lw, lb, lw, None, y, xhat, rstd, R_, 2),
              (x, lw, lb, None, None, y, xhat, rstd, 0, 1), (None, lw, lb, None, None, y, xhat, rstd, R_, 1), (x, None, lb, None, None, y, xhat, rstd, R_, 1),
              (x, lw, None, None, None, y, xhat, rstd, R_, 1), (x, lw, lb, None, None, None, xhat, rstd, R_, 1)]:
        bad(lnf(*a), "sgrl_add_ln_forward")
    lnb = lambda dy, xh, rs, w0, w1, dx_, rows, nets: lib.sgrl_add_ln_backward(p(dy), p(xh), p(rs), p(w0), p(w1), p(dx_), p(dw0), p(db0), p(None), p(None), rows, nets, st)
    for a in [(x, xhat, rstd, lw, lw, dx, R_, 3), (x, xhat, rstd, lw, None, dx, R_, 2), (x, xhat, rstd, lw, None, dx, 0, 1), (None, xhat, rstd, lw, None, dx, R_, 1),
              (x, None, rstd, lw, None, dx, R_, 1), (x, xhat, None, lw, None, dx, R_, 1), (x, xhat, rstd, None, None, dx, R_, 1), (x, xhat, rstd, lw, None, None, R_, 1)]:
        bad(lnb(*a), "sgrl_add_ln_backward")
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)          # nothing was launched: every output still holds the sentinel
