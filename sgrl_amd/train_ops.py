"""Differentiable linear layers of the TD3 update on the HIP kernels of csrc/train_gemm.hip (C ABI: include/sgrl_train.h).

`linear(x, weight, bias, relu)` is `torch.nn.functional.linear` (+ ReLU) as a `torch.autograd.Function` whose forward,
input gradient and weight / bias gradient run on this library's own small-product kernels instead of the vendor GEMMs
(which pick single-workgroup 256 x 256 tilings for the update's 700-row problems: DESIGN.md section 5).  Used by the SET
modules (set_policy.py) whenever autograd is recording on the GPU -- i.e. inside `Agent.update` (reference agent.py:117-183);
the no-grad rollout path is the fused forward of csrc/set_actor.hip.  No CPU fallback: on the CPU the modules use
`F.linear`; on the GPU a missing extension raises.
"""
import contextlib
import ctypes
import os

import numpy as np

import torch
import torch.nn.functional as F

from . import _lib

_bound = False
_fns = {}              # name -> the bound entry point (_L)
_ws = {}
ENABLED = os.environ.get("SGRL_TRAIN_GEMM", "1") != "0"      # 0: vendor GEMMs (A/B comparisons)

# Every prototype of include/sgrl_train.h: name -> (return type, argument types), one letter per type -- p: any pointer, i: int,
# f: float, d: double, l: int64_t, u: uint64_t, s: const char*.  tests/test_train_ops_abi.py holds each entry to the header.
_KIND = {"p": ctypes.c_void_p, "i": ctypes.c_int, "f": ctypes.c_float, "d": ctypes.c_double, "l": ctypes.c_int64, "u": ctypes.c_uint64,
         "s": ctypes.c_char_p}
_ABI = {
    "sgrl_train_ws_floats": ("l", ""),
    "sgrl_linear_forward": ("i", "pipipppiiiiip"),
    "sgrl_linear_forward_fused": ("i", "pipipppipipiiiiip"),
    "sgrl_linear_forward_twin_fused": ("i", "ppippippppppippippiiiiip"),
    "sgrl_linear_backward": ("i", "pipiippipipipippiiipp"),
    "sgrl_linear_backward_xrelu": ("i", "pipiippipipipippiiiipp"),
    "sgrl_linear_backward_acc": ("i", "pipiippipipipippiiiiipp"),
    "sgrl_linear_wgrad_group": ("i", "ippp"),
    "sgrl_linear_forward_twin": ("i", "ppippippppppiiiiip"),
    "sgrl_linear_dgrad_twin": ("i", "ppippiippppippippiiip"),
    "sgrl_linear_dgrad_twin_xrelu": ("i", "ppippiippppippippppiiiip"),
    "sgrl_linear_dgrad_twin_acc": ("i", "ppippiippppippippppiiiiip"),
    "sgrl_gram_forward": ("i", "pppip"),
    "sgrl_gram_backward": ("i", "pppppip"),
    "sgrl_gram_tri_forward": ("i", "pppip"),
    "sgrl_gram_tri_backward": ("i", "pppppip"),
    "sgrl_sym_fold": ("i", "ipppip"),
    "sgrl_zmat_forward": ("i", "pppip"),
    "sgrl_zmat_backward": ("i", "pppppip"),
    "sgrl_add_ln_forward": ("i", "pppppppppiifp"),
    "sgrl_add_ln_backward": ("i", "ppppppppppiip"),
    "sgrl_embed3_forward": ("i", "ppppiiipip"),
    "sgrl_embed3_backward": ("i", "pppppiiiiip"),
    "sgrl_optim_chunk": ("i", ""),
    "sgrl_optim_clip_adam": ("i", "pipiddddfpp"),
    "sgrl_optim_lerp": ("i", "ppifp"),
    "sgrl_attention_forward": ("i", "ppppfpppiip"),
    "sgrl_attention_backward": ("i", "pppfpppppppiip"),
    "sgrl_swat_attention_forward": ("i", "ppfppiip"),
    "sgrl_swat_attention_backward": ("i", "pfppppiip"),
    "sgrl_dropout_forward": ("i", "pplfupip"),
    "sgrl_dropout_backward": ("i", "pplfupip"),
    "sgrl_swat_attention_forward_dropout": ("i", "ppfppiifupip"),
    "sgrl_swat_attention_backward_dropout": ("i", "pfppppiifupip"),
    "sgrl_smp_gather_forward": ("i", "piipiippiippiip"),
    "sgrl_smp_gather_backward": ("i", "ppppiiiippiippiip"),
    "sgrl_smp_up_tail_forward": ("i", "ppppppip"),
    "sgrl_smp_up_tail_backward": ("i", "pppppppip"),
    "sgrl_row_normalize_forward": ("i", "pppiip"),
    "sgrl_row_normalize_backward": ("i", "ppppiip"),
    "sgrl_td3_twin_mse_forward": ("i", "ppplpp"),
    "sgrl_td3_twin_mse_backward": ("i", "ppplpppp"),
    "sgrl_td3_neg_mean_forward": ("i", "plpp"),
    "sgrl_td3_neg_mean_backward": ("i", "lppp"),
    "sgrl_td3_loss_launches": ("i", ""),
    "sgrl_train_last_error": ("s", ""),
}


def _L():
    global _bound
    L = _lib.lib()
    if not _bound:
        for name, (res, args) in _ABI.items():
            fn = _fns[name] = getattr(L, name)
            fn.restype = _KIND[res]
            fn.argtypes = [_KIND[k] for k in args]
        _bound = True
    return L


def _check(L, rc, what):
    if rc != 0:
        raise _lib.SgrlError("%s failed (%d): %s" % (what, rc, L.sgrl_train_last_error().decode()))


def _call(name, *args):
    """The entry point `name` of the library; a non-zero return code raises SgrlError with the library's message."""
    if not _bound:
        _L()
    rc = _fns[name](*args)
    if rc != 0:
        _check(_L(), rc, name)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st(device):
    """The current stream of `device` as the ABI's `void* stream`."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _f32(device, *shape):
    return torch.empty(shape, dtype=torch.float32, device=device)


def _c(t):
    """None, or t itself if contiguous, or a contiguous copy."""
    return t if (t is None or t.is_contiguous()) else t.contiguous()


def _rows(t, width):
    """t [rows, >= width] or stacked [2, rows, >= width] as the product kernels read it: a row-strided view (one part of a
    concatenation, a slice of a wider tensor) is read as is -- last stride 1, rows at least `width` apart, the stacked pair not
    reversed --, anything else is copied."""
    if t.stride(-1) != 1 or t.stride(-2) < width or (t.dim() == 3 and t.stride(0) < 0):
        return t.contiguous()
    return t


def _scratch(device):
    """Scratch of the split weight-gradient contractions (zero filled once; every call leaves its counters zero): one buffer
    per (device, stream) -- calls on one stream run in order (include/sgrl_train.h)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _ws.get(key)
    if ws is None:
        ws = torch.zeros(int(_L().sgrl_train_ws_floats()), dtype=torch.float32, device=device)
        _ws[key] = ws
    return ws


# struct sgrl_wgrad_desc (include/sgrl_train.h)
_DESC = np.dtype([("dy", "<u8"), ("y", "<u8"), ("rowdiv", "<u8"), ("x", "<u8"), ("dw", "<u8"), ("db", "<u8"), ("lddy", "<i4"),
                  ("ldy", "<i4"), ("ldx", "<i4"), ("lddw", "<i4"), ("M", "<i4"), ("N", "<i4"), ("K", "<i4"), ("relu", "<i4")])
assert _DESC.itemsize == 80
_pending = None        # None: weight gradients are computed inside backward(); a list: they are postponed (deferred_wgrads)


@contextlib.contextmanager
def deferred_wgrads(enabled=True):
    """Inside this context the backward() of a linear layer whose weight (and bias) are leaf parameters launches only the
    INPUT-gradient product; its weight / bias gradients -- which nothing needs before the optimizer steps -- are collected and
    issued together (12 layers per launch) when the context exits, and only then stored into (or added to) the parameters'
    `.grad`: autograd itself never sees a gradient tensor that has not been computed yet."""
    global _pending
    if not enabled or _pending is not None:
        yield
        return
    _pending = []
    try:
        yield
    finally:
        todo, _pending = _pending, None
        flush_wgrads(todo)


def _leaf_targets(weight, bias):
    """Where deferred_wgrads may store a layer's postponed gradients: (the weight if it is a leaf, else None; the leaf behind a
    FOLDED weight (tri_weights), else None; the bias) -- or None where they may not be postponed: the weight neither a leaf nor a
    folded tensor whose leaf is known, or the bias not a leaf.  Kept by reference so that `.grad` can be set at the flush."""
    if bias is not None and not bias.is_leaf:
        return None
    if weight.is_leaf:
        return weight, None, bias
    fold_leaf = getattr(weight, "_sgrl_fold_leaf", None)
    return None if fold_leaf is None else (None, fold_leaf, bias)


class _Wgrad(object):
    """One layer's weight (+ bias) gradient as sgrl_linear_wgrad_group takes it: dw [N, K] = g^T x and db [N] = the column sums of
    g, g = dy [M, N] masked by y > 0 (relu; y's rows ldy apart) or divided row-wise by rowdiv.  dw is allocated here, and db if the
    bias wants a gradient (it rides on the weight's launch, so dw exists even for a frozen weight).  `targets`: _leaf_targets() of
    the layer; w_param / fold_param / b_param are the tensors whose `.grad` flush_wgrads stores into if the record is POSTPONED
    (_settle) -- only those among the targets that want a gradient; a folded weight's dw is unfolded into fold_param's.  st: the
    stream of the backward() call, _st(dev)."""
    __slots__ = ("dy", "y", "rowdiv", "x", "dw", "db", "ldy", "relu", "dev", "stream", "want_w", "postponable",
                 "w_param", "fold_param", "b_param")

    def __init__(self, dy, y, rowdiv, x, ldy, relu, targets, want_w, want_b, st):
        dev = dy.device
        self.dy, self.y, self.rowdiv, self.x, self.ldy, self.relu = dy, y, rowdiv, x, ldy, relu
        self.dw = _f32(dev, dy.shape[1], x.shape[1])
        self.db = _f32(dev, dy.shape[1]) if want_b else None
        self.dev, self.stream = dev, st
        self.want_w, self.postponable = want_w, targets is not None
        w_leaf, fold_leaf, b_leaf = targets or (None, None, None)
        self.w_param, self.fold_param = (w_leaf if want_w else None), (fold_leaf if want_w else None)
        self.b_param = b_leaf if want_b else None


def _settle(recs):
    """The fate of the weight-gradient records of one backward() call -> (what autograd gets back for each, [(dw, db)]; the records
    the caller has to issue NOW, together).  Under deferred_wgrads a record whose targets are known is postponed: autograd sees
    (None, None), the flush stores into `.grad`.  The others are returned, dw only if the weight itself wanted it."""
    out, now = [], []
    for r in recs:
        if _pending is not None and r.postponable:
            _pending.append(r)
            out.append((None, None))
        else:
            r.w_param = r.fold_param = r.b_param = None         # nothing is stored: autograd takes the gradients
            now.append(r)
            out.append((r.dw if r.want_w else None, r.db))
    return out, now


def flush_wgrads(todo):
    if not todo:
        return
    by_stream = {}
    for r in todo:
        by_stream.setdefault((r.dev, r.stream.value), []).append(r)
    for (dev, _), recs in by_stream.items():
        d = np.zeros(len(recs), dtype=_DESC)
        for i, r in enumerate(recs):
            (M, N), K = r.dy.shape, r.x.shape[1]
            d[i] = (r.dy.data_ptr(), 0 if r.y is None else r.y.data_ptr(), 0 if r.rowdiv is None else r.rowdiv.data_ptr(),
                    r.x.data_ptr(), r.dw.data_ptr(), 0 if r.db is None else r.db.data_ptr(), r.dy.stride(0), r.ldy, r.x.stride(0), K, M, N, K,
                    1 if r.relu else 0)
        _call("sgrl_linear_wgrad_group", len(recs), ctypes.c_void_p(d.ctypes.data), _p(_scratch(dev)), recs[0].stream)
        with torch.no_grad():
            # gradients of FOLDED weights (tri_weights): spread onto both mirror columns of their leaf parameters, one launch for all
            folded = [r for r in recs if r.fold_param is not None]
            for i0 in range(0, len(folded), 16):
                part = folded[i0:i0 + 16]
                full = [torch.empty_like(r.fold_param) for r in part]
                _sym_fold_call(full, [r.dw for r in part], True, dev)
                for r, f in zip(part, full):
                    r.w_param, r.dw = r.fold_param, f
            for r in recs:
                for prm, g in ((r.w_param, r.dw), (r.b_param, r.db)):
                    if prm is None:
                        continue
                    g = g.view_as(prm)
                    if prm.grad is None:
                        prm.grad = g
                    else:
                        prm.grad.add_(g)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu, rowdiv, addend=None, tail=None, x_relu=False, premasked=False, slot=None):
        # slot: x is one output of fan_out() -- this layer's input gradient is written into / accumulated onto the fan-out's shared
        # buffer (sgrl_linear_backward_acc) instead of travelling through autograd's own additions.
        # x_relu: x is the output of a ReLU layer whose backward is told `premasked` -- this layer's input gradient comes out masked
        # by x > 0 (the dgrad kernel's epilogue), and THAT layer's two backward products read no mask (include/sgrl_train.h
        # sgrl_linear_backward_xrelu).  Valid when nothing else consumes the ReLU layer's output (the SET feed-forward pairs).
        N, K = weight.shape
        assert not premasked or relu
        x2 = _rows(x.reshape(-1, K), K)
        w = _c(weight)
        M = x2.shape[0]
        rd = None
        if rowdiv is not None:
            rd = _c(rowdiv.reshape(-1))
            assert rd.shape[0] == M and not relu
        # fused followers (include/sgrl_train.h sgrl_linear_forward_fused): a residual added to the result, columns appended to it
        nt = 0 if tail is None else tail.shape[-1]
        ad2 = tl2 = None
        if addend is not None:
            assert not relu and rd is None and tail is None
            ad2 = _rows(addend.reshape(M, N), N)
        if tail is not None:
            tl2 = _c(tail.reshape(M, nt))
        dev = x.device
        y = _f32(dev, M, N + nt)
        if ad2 is None and tl2 is None:
            _call("sgrl_linear_forward", _p(x2), x2.stride(0), _p(w), K, _p(bias), _p(rd), _p(y), N, M, N, K, 1 if relu else 0, _st(dev))
        else:
            _call("sgrl_linear_forward_fused", _p(x2), x2.stride(0), _p(w), K, _p(bias), _p(rd), _p(ad2), 0 if ad2 is None else ad2.stride(0),
                  _p(tl2), nt, _p(y), N + nt, M, N, K, 1 if relu else 0, _st(dev))
        ctx.ntail = nt
        ctx.ad_shape = None if addend is None else addend.shape
        ctx.tail_shape = None if tail is None else tail.shape
        ctx.save_for_backward(x2, w, y if (relu or rd is not None) else None, rd)
        ctx.has_bias, ctx.relu = bias is not None, bool(relu)
        ctx.x_relu, ctx.mask = bool(x_relu), bool(relu) and not premasked       # mask: dy still has to be masked by y > 0 here
        ctx.targets = _leaf_targets(weight, bias)                               # what deferred_wgrads may postpone
        ctx.x_shape = x.shape
        ctx.rd_shape = None if rowdiv is None else rowdiv.shape
        ctx.slot = slot
        return y.view(*x.shape[:-1], N + nt)

    @staticmethod
    def backward(ctx, dy):
        x2, w, yo, rd = ctx.saved_tensors
        N, K = w.shape
        M = x2.shape[0]
        nt = ctx.ntail
        dev = dy.device
        dyf = _rows(dy.reshape(M, N + nt), N + nt)
        dy2 = dyf[:, :N] if nt else dyf             # the product's own columns: a row-strided view, read as is
        ldyo = N + nt                               # row stride of the saved output (ReLU mask / row-divisor gradient)
        need = ctx.needs_input_grad
        need_x, need_b = need[0], ctx.has_bias and need[2]
        need_rd = rd is not None and need[4]
        acc_dx = False
        slot = ctx.slot if need_x else None
        if slot is not None and slot.buf is not None:          # a sibling consumer was here first: add onto its gradient
            dx, acc_dx = slot.buf.view(M, K), True
        else:
            dx = _f32(dev, M, K) if need_x else None
            if slot is not None:
                slot.buf = dx
        # the bias gradient rides on the weight-gradient kernel, so a record exists for either
        st = _st(dev)
        recs = [_Wgrad(dy2, yo if ctx.mask else None, rd, x2, ldyo, ctx.mask, ctx.targets, need[1], need_b, st)] if (need[1] or need_b) else []
        drd = _f32(dev, M) if need_rd else None
        grads, now = _settle(recs)
        gw, gb = grads[0] if grads else (None, None)
        now_w, now_b = (now[0].dw, now[0].db) if now else (None, None)     # not postponed: the launch below computes them with dx
        if dx is not None or now_w is not None or drd is not None:
            _call("sgrl_linear_backward_acc", _p(dy2), dy2.stride(0), _p(yo), ldyo, 1 if ctx.mask else 0, _p(rd), _p(x2), x2.stride(0),
                  _p(w), K, _p(dx), K, _p(now_w), K, _p(now_b), _p(drd), M, N, K, 1 if ctx.x_relu else 0, 1 if acc_dx else 0,
                  _p(_scratch(dev)), st)
        dadd = dy.reshape(ctx.ad_shape) if (ctx.ad_shape is not None and need[5]) else None
        dtail = dyf[:, N:].reshape(ctx.tail_shape) if (nt and need[6]) else None
        # (a slot consumer hands its gradient to the fan-out through the slot: the first one also returns it so that the fan-out's
        # backward is certain to run; the others return nothing)
        return (dx.view(ctx.x_shape) if (need_x and not acc_dx) else None), gw, gb, None, (drd.view(ctx.rd_shape) if need_rd else None), \
            dadd, dtail, None, None, None


class _Linear2Fn(torch.autograd.Function):
    """The same layer of two networks of identical shape in one launch (csrc/train_gemm.hip k_sgemm_twin; include/sgrl_train.h):
    x is either ONE input both share, [..., K], or their two inputs stacked, [2, ..., K]; the result is stacked, [2, ..., N]."""

    @staticmethod
    def forward(ctx, x, w0, w1, b0, b1, relu, rowdiv, shared, addend=None, tail=None, x_relu=False, premasked=False, slot=None):
        assert slot is None or not shared
        N, K = w0.shape
        assert w1.shape == w0.shape and (b0 is None) == (b1 is None)
        assert (not premasked or relu) and not (x_relu and shared)        # x_relu / premasked: see _LinearFn
        lead = x.shape[:-1] if shared else x.shape[1:-1]
        xs = _rows(x.reshape(-1, K) if shared else x.reshape(2, -1, K), K)
        M = xs.shape[-2]
        x0, x1 = (xs, xs) if shared else (xs[0], xs[1])
        # the tensors autograd knows (leaf parameters, or e.g. a concatenation of some): what deferred_wgrads may postpone
        ctx.targets = [_leaf_targets(w0, b0), _leaf_targets(w1, b1)]
        w0, w1 = _c(w0), _c(w1)
        rd = None
        if rowdiv is not None:
            rd = _c(rowdiv.reshape(2, -1))
            assert rd.shape[1] == M and not relu
        rd0, rd1 = (None, None) if rd is None else (rd[0], rd[1])
        # fused followers: addend [2, ..., N] (a residual per network), tail [..., nt] or [2, ..., nt] (columns appended to each result)
        nt = 0 if tail is None else tail.shape[-1]
        ad2 = tl = None
        if addend is not None:
            assert not relu and rd is None and tail is None
            ad2 = _c(addend.reshape(2, M, N))
        if tail is not None:
            tl = _c(tail.reshape(-1, M, nt))         # one tail both networks share, or one each
            tl = (tl[0], tl[0]) if tl.shape[0] == 1 else (tl[0], tl[1])
        dev = x.device
        y = _f32(dev, 2, M, N + nt)
        if ad2 is None and tl is None:
            _call("sgrl_linear_forward_twin", _p(x0), _p(x1), xs.stride(-2), _p(w0), _p(w1), K, _p(b0), _p(b1), _p(rd0), _p(rd1),
                  _p(y[0]), _p(y[1]), N, M, N, K, 1 if relu else 0, _st(dev))
        else:
            _call("sgrl_linear_forward_twin_fused", _p(x0), _p(x1), xs.stride(-2), _p(w0), _p(w1), K, _p(b0), _p(b1), _p(rd0), _p(rd1),
                  _p(None if ad2 is None else ad2[0]), _p(None if ad2 is None else ad2[1]), N,
                  _p(None if tl is None else tl[0]), _p(None if tl is None else tl[1]), nt,
                  _p(y[0]), _p(y[1]), N + nt, M, N, K, 1 if relu else 0, _st(dev))
        ctx.ntail = nt
        ctx.ad_shape = None if addend is None else addend.shape
        ctx.tail_shape = None if tail is None else tail.shape
        ctx.save_for_backward(xs, w0, w1, y if (relu or rd is not None) else None, rd)
        ctx.has_bias, ctx.relu, ctx.shared = b0 is not None, bool(relu), bool(shared)
        ctx.x_relu, ctx.mask = bool(x_relu), bool(relu) and not premasked
        ctx.x_shape = x.shape
        ctx.rd_shape = None if rowdiv is None else rowdiv.shape
        ctx.slot = slot
        return y.view(2, *lead, N + nt)

    @staticmethod
    def backward(ctx, dy):
        xs, w0, w1, yo, rd = ctx.saved_tensors
        N, K = w0.shape
        M = xs.shape[-2]
        nt = ctx.ntail
        dyf = _rows(dy.reshape(2, M, N + nt), N + nt)      # a row-strided view (the gradient of one part of a concatenation) is read as is
        dy2 = dyf[:, :, :N] if nt else dyf
        lddy = dy2.stride(1)
        ldyo = N + nt
        need = ctx.needs_input_grad
        need_x = need[0]
        need_w = [need[1], need[2]]
        need_b = [ctx.has_bias and need[3], ctx.has_bias and need[4]]
        need_rd = rd is not None and need[6]
        dev = dy.device
        st = _st(dev)
        acc_dx = False
        slot = ctx.slot if need_x else None
        if slot is not None and slot.buf is not None:
            dx, acc_dx = slot.buf.view(2, M, K), True
        else:
            dx = _f32(dev, 2, M, K) if need_x else None
            if slot is not None:
                slot.buf = dx
        drd = _f32(dev, 2, M) if need_rd else None
        if need_x:
            xm = (xs[0], xs[1]) if ctx.x_relu else (None, None)
            _call("sgrl_linear_dgrad_twin_acc", _p(dy2[0]), _p(dy2[1]), lddy, _p(None if yo is None else yo[0]),
                  _p(None if yo is None else yo[1]), ldyo, 1 if ctx.mask else 0,
                  _p(None if rd is None else rd[0]), _p(None if rd is None else rd[1]),
                  _p(w0), _p(w1), K, _p(dx[0]), _p(dx[1]), K, _p(None if drd is None else drd[0]),
                  _p(None if drd is None else drd[1]), _p(xm[0]), _p(xm[1]), xs.stride(-2), M, N, K,
                  1 if acc_dx else 0, st)
        elif need_rd:                               # the row divisor's gradient without an input gradient: the single-network kernel twice
            for i in range(2):
                _call("sgrl_linear_backward", _p(dy2[i]), lddy, _p(yo[i]), ldyo, 0, _p(rd[i]), _p(None), 0, _p(None), 0, _p(None), 0,
                      _p(None), 0, _p(None), _p(drd[i]), M, N, K, _p(_scratch(dev)), st)
        # weight / bias gradients: one record per network -- postponed (deferred_wgrads) or issued together now
        nets = [i for i in range(2) if need_w[i] or need_b[i]]
        recs = [_Wgrad(dy2[i], yo[i] if ctx.mask else None, None if rd is None else rd[i], xs if ctx.shared else xs[i], ldyo, ctx.mask,
                       ctx.targets[i], need_w[i], need_b[i], st) for i in nets]
        grads, now = _settle(recs)
        flush_wgrads(now)
        grads_w, grads_b = [None, None], [None, None]
        for i, (gw, gb) in zip(nets, grads):
            grads_w[i], grads_b[i] = gw, gb
        dx_out = None
        if need_x and not acc_dx:
            dx_out = (dx[0] + dx[1]).view(ctx.x_shape) if ctx.shared else dx.view(ctx.x_shape)
        dadd = dy.reshape(ctx.ad_shape) if (ctx.ad_shape is not None and need[8]) else None
        dtail = None
        if nt and need[9]:
            dtail = dyf[:, :, N:].reshape(2, *ctx.x_shape[(0 if ctx.shared else 1):-1], nt).sum_to_size(ctx.tail_shape)
        return dx_out, grads_w[0], grads_w[1], grads_b[0], grads_b[1], None, (drd.view(ctx.rd_shape) if need_rd else None), None, dadd, dtail, \
            None, None, None


TRI = 528      # lower triangle of a symmetric 32 x 32 matrix, packed k = a (a + 1) / 2 + b (include/sgrl_train.h)


def _gram_forward(ctx, name, width, z):
    z2 = _c(z.reshape(-1, 96))
    M = z2.shape[0]
    gram = _f32(z.device, M, width)
    fn = _f32(z.device, M)
    _call(name, _p(z2), _p(gram), _p(fn), M, _st(z.device))
    ctx.save_for_backward(z2, fn)
    ctx.z_shape = z.shape
    lead = z.shape[:-2]
    return gram.view(*lead, width), fn.view(*lead, 1)


def _gram_backward(ctx, name, width, dgram, dfn):
    z2, fn = ctx.saved_tensors
    M = z2.shape[0]
    dg = None if dgram is None else _c(dgram.reshape(M, width))
    df = None if dfn is None else _c(dfn.reshape(M))
    dz = _f32(z2.device, M, 96)
    _call(name, _p(z2), _p(dg), _p(df), _p(fn), _p(dz), M, _st(z2.device))
    return dz.view(ctx.z_shape)


class _GramFn(torch.autograd.Function):
    """z [..., 3, 32] -> (vec(Z'Z) [..., 1024], ||Z'Z||_F + 1 [..., 1])."""

    @staticmethod
    def forward(ctx, z):
        return _gram_forward(ctx, "sgrl_gram_forward", 1024, z)

    @staticmethod
    def backward(ctx, dgram, dfn):
        return _gram_backward(ctx, "sgrl_gram_backward", 1024, dgram, dfn)


class _GramTriFn(torch.autograd.Function):
    """z [..., 3, 32] -> (tri(Z'Z) [..., 528], ||Z'Z||_F + 1 [..., 1]): the invariants without their mirror copies."""

    @staticmethod
    def forward(ctx, z):
        return _gram_forward(ctx, "sgrl_gram_tri_forward", TRI, z)

    @staticmethod
    def backward(ctx, dtri, dfn):
        return _gram_backward(ctx, "sgrl_gram_tri_backward", TRI, dtri, dfn)


def _sym_fold_call(full, tri, unfold, device):
    n = len(full)
    pw = (ctypes.c_void_p * n)(*[t.data_ptr() for t in full])
    pt = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tri])
    rows = (ctypes.c_int * n)(*[t.shape[0] for t in full])
    _call("sgrl_sym_fold", n, pw, pt, rows, 1 if unfold else 0, _st(device))


class _FoldFn(torch.autograd.Function):
    """Weights [rows, 1024] acting on vec(G), G symmetric -> [rows, 528] acting on tri(G) (mirror columns added), up to 16 matrices in
    one launch; the backward spreads a folded gradient onto both mirror columns, one launch too."""

    @staticmethod
    def forward(ctx, *ws):
        ctx.set_materialize_grads(False)       # a folded weight whose gradient was postponed (deferred_wgrads) gets None here, not zeros to unfold
        ws = [_c(w) for w in ws]
        out = [_f32(w.device, w.shape[0], TRI) for w in ws]
        _sym_fold_call(ws, out, False, ws[0].device)
        ctx.shapes = [w.shape for w in ws]
        return tuple(out)

    @staticmethod
    def backward(ctx, *ds):
        idx = [i for i, d in enumerate(ds) if d is not None and ctx.needs_input_grad[i]]
        res = [None] * len(ds)
        if idx:
            src = [_c(ds[i]) for i in idx]
            full = [_f32(src[0].device, *ctx.shapes[i]) for i in idx]
            _sym_fold_call(full, src, True, src[0].device)
            for i, f in zip(idx, full):
                res[i] = f
        return tuple(res)


class _ZmatFn(torch.autograd.Function):
    """z [..., 3, 32], mat [..., 32, 32] -> z . mat [..., 3, 32] per node."""

    @staticmethod
    def forward(ctx, z, mat):
        z2, m2 = _c(z.reshape(-1, 96)), _c(mat.reshape(-1, 1024))
        M = z2.shape[0]
        t = _f32(z.device, M, 96)
        _call("sgrl_zmat_forward", _p(z2), _p(m2), _p(t), M, _st(z.device))
        ctx.save_for_backward(z2, m2)
        ctx.shapes = (z.shape, mat.shape)
        return t.view(z.shape)

    @staticmethod
    def backward(ctx, dt):
        z2, m2 = ctx.saved_tensors
        M = z2.shape[0]
        d = _c(dt.reshape(M, 96))
        dz, dm = torch.empty_like(z2), torch.empty_like(m2)
        _call("sgrl_zmat_backward", _p(z2), _p(m2), _p(d), _p(dz), _p(dm), M, _st(z2.device))
        return dz.view(ctx.shapes[0]), dm.view(ctx.shapes[1])


class _AttnFn(torch.autograd.Function):
    """qkv [B, L, 768], vgp [B, L, 3, 252], gdir [B, L, 3, 2], bias [2, L, L] or None -> (o [B, L, 256], og [B, L, 3, 256])."""

    @staticmethod
    def forward(ctx, qkv, vgp, gdir, bias, scale):
        B, Ln = qkv.shape[0], qkv.shape[1]
        qkv, vgp, gdir, bz = _c(qkv), _c(vgp), _c(gdir), _c(bias)
        dev = qkv.device
        w = _f32(dev, B, 2, Ln, Ln)
        o = _f32(dev, B, Ln, 256)
        og = _f32(dev, B, Ln, 3, 256)
        _call("sgrl_attention_forward", _p(qkv), _p(vgp), _p(gdir), _p(bz), ctypes.c_float(scale), _p(w), _p(o), _p(og), B, Ln, _st(dev))
        ctx.save_for_backward(qkv, vgp, gdir, w)
        ctx.has_bias, ctx.scale = bias is not None, float(scale)
        return o, og

    @staticmethod
    def backward(ctx, d_o, d_og):
        qkv, vgp, gdir, w = ctx.saved_tensors
        B, Ln = qkv.shape[0], qkv.shape[1]
        dev = qkv.device
        d_o = torch.zeros((B, Ln, 256), dtype=torch.float32, device=dev) if d_o is None else _c(d_o)
        d_og = torch.zeros((B, Ln, 3, 256), dtype=torch.float32, device=dev) if d_og is None else _c(d_og)
        dqkv, dvgp, ds = torch.empty_like(qkv), torch.empty_like(vgp), torch.empty_like(w)
        dgdh = _f32(dev, B, Ln, 3, 2, 2)
        _call("sgrl_attention_backward", _p(qkv), _p(vgp), _p(gdir), ctypes.c_float(ctx.scale), _p(w), _p(d_o), _p(d_og), _p(dqkv),
              _p(dvgp), _p(dgdh), _p(ds), B, Ln, _st(dev))
        dgdir = dgdh.sum(3) if ctx.needs_input_grad[2] else None
        dbias = ds.sum(0) if (ctx.has_bias and ctx.needs_input_grad[3]) else None
        return dqkv, dvgp, dgdir, dbias, None


def _drop_args(call):
    """The ABI arguments of a counter-RNG dropout call (p, seed, step tensor, site); none for an empty call."""
    if not call:
        return ()
    p, seed, step, site = call
    return ctypes.c_float(p), ctypes.c_uint64(seed), _p(step), site


def _swat_attn_forward(ctx, name, qkv, bias, scale, *call):
    B, Ln = qkv.shape[0], qkv.shape[1]
    qkv, bz = _c(qkv), _c(bias)
    dev = qkv.device
    w = _f32(dev, B, 2, Ln, Ln)
    o = _f32(dev, B, Ln, 128)
    _call(name, _p(qkv), _p(bz), ctypes.c_float(scale), _p(w), _p(o), B, Ln, *_drop_args(call), _st(dev))
    ctx.save_for_backward(qkv, w)
    ctx.has_bias, ctx.scale, ctx.call = bias is not None, float(scale), call
    return o


def _swat_attn_backward(ctx, name, d_o):
    qkv, w = ctx.saved_tensors
    B, Ln = qkv.shape[0], qkv.shape[1]
    d_o = _c(d_o)
    dqkv, ds = torch.empty_like(qkv), torch.empty_like(w)
    _call(name, _p(qkv), ctypes.c_float(ctx.scale), _p(w), _p(d_o), _p(dqkv), _p(ds), B, Ln, *_drop_args(ctx.call), _st(qkv.device))
    dbias = ds.sum(0) if (ctx.has_bias and ctx.needs_input_grad[1]) else None
    return ((dqkv if ctx.needs_input_grad[0] else None), dbias, None) + (None,) * len(ctx.call)


class _SwatAttnFn(torch.autograd.Function):
    """qkv [B, L, 384], bias [2, L, L] or None -> o [B, L, 128]: the SWAT networks' attention, 2 heads x 64 channels, L <= 15
    (csrc/train_gemm.hip k_swat_attn_fwd / k_swat_attn_bwd), one launch forward and one backward."""

    @staticmethod
    def forward(ctx, qkv, bias, scale):
        return _swat_attn_forward(ctx, "sgrl_swat_attention_forward", qkv, bias, scale)

    @staticmethod
    def backward(ctx, d_o):
        return _swat_attn_backward(ctx, "sgrl_swat_attention_backward", d_o)


class _AddLNFn(torch.autograd.Function):
    """y = LayerNorm(x + res) * w + b over 128 columns, one launch forward and one backward (csrc/train_gemm.hip k_add_ln_*);
    w1 / b1 given: x stacks TWO networks along dim 0, each with its own affine pair."""

    @staticmethod
    def forward(ctx, x, res, w0, b0, w1, b1, eps):
        nets = 2 if w1 is not None else 1
        x2 = _c(x.reshape(-1, 128))
        r2 = None if res is None else _c(res.expand_as(x).reshape(-1, 128))
        total = x2.shape[0]
        assert total % nets == 0
        y = torch.empty_like(x2)
        xhat = torch.empty_like(x2)
        rstd = _f32(x.device, total)
        _call("sgrl_add_ln_forward", _p(x2), _p(r2), _p(w0), _p(b0), _p(w1), _p(b1), _p(y), _p(xhat), _p(rstd), total // nets, nets,
              ctypes.c_float(eps), _st(x.device))
        ctx.save_for_backward(xhat, rstd, w0, w1)
        ctx.nets, ctx.x_shape, ctx.res_shape = nets, x.shape, None if res is None else res.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        xhat, rstd, w0, w1 = ctx.saved_tensors
        total, nets = xhat.shape[0], ctx.nets
        dy2 = _c(dy.reshape(total, 128))
        need = ctx.needs_input_grad
        dx = torch.empty_like(xhat)
        new = lambda want: _f32(dy.device, 128) if want else None
        dw0, db0 = new(need[2]), new(need[3])
        dw1, db1 = new(nets == 2 and need[4]), new(nets == 2 and need[5])
        _call("sgrl_add_ln_backward", _p(dy2), _p(xhat), _p(rstd), _p(w0), _p(w1), _p(dx), _p(dw0), _p(db0), _p(dw1), _p(db1),
              total // nets, nets, _st(dy.device))
        dxv = dx.view(ctx.x_shape)
        dres = None
        if ctx.res_shape is not None and need[1]:
            dres = dxv if tuple(ctx.res_shape) == tuple(ctx.x_shape) else dxv.sum_to_size(ctx.res_shape)
        return (dxv if need[0] else None), dres, dw0, db0, dw1, db1, None


class _Embed3Fn(torch.autograd.Function):
    """cat([w0[idx[0]], w1[idx[1]], w2[idx[2]]], dim=1) -- the three traversal embeddings -- one launch forward, one backward."""

    @staticmethod
    def forward(ctx, idx, w0, w1, w2):
        n = (w0.shape[1], w1.shape[1], w2.shape[1])
        ws = [_c(w) for w in (w0, w1, w2)]
        Ln = idx.shape[1]
        out = _f32(w0.device, Ln, sum(n))
        _call("sgrl_embed3_forward", _p(idx), _p(ws[0]), _p(ws[1]), _p(ws[2]), n[0], n[1], n[2], _p(out), Ln, _st(w0.device))
        ctx.save_for_backward(idx)
        ctx.n, ctx.rows = n, w0.shape[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        d = _c(dout)
        n, rows = ctx.n, ctx.rows
        dws = [_f32(dout.device, rows, n[t]) if ctx.needs_input_grad[1 + t] else None for t in range(3)]
        _call("sgrl_embed3_backward", _p(idx), _p(d), _p(dws[0]), _p(dws[1]), _p(dws[2]), n[0], n[1], n[2], idx.shape[1], rows, _st(dout.device))
        return None, dws[0], dws[1], dws[2]


_NO_GRAD_KERNELS = False      # no_grad_kernels(): the own kernels also where nothing is differentiated


@contextlib.contextmanager
def no_grad_kernels(enabled=True):
    """Inside this context (meant for torch.no_grad() passes) the operations of this module launch their own kernels although nothing
    requires a gradient -- the twin target critics of a TD3 update walk both networks in one pass that way (set_policy.SECritic)."""
    global _NO_GRAD_KERNELS
    old, _NO_GRAD_KERNELS = _NO_GRAD_KERNELS, bool(enabled) or _NO_GRAD_KERNELS
    try:
        yield
    finally:
        _NO_GRAD_KERNELS = old


def _on_device_with_grad(*ts):
    if not (ENABLED and ts[0].is_cuda and ts[0].dtype == torch.float32):
        return False
    if _NO_GRAD_KERNELS and not torch.is_grad_enabled():
        return True
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


class _Slot(object):
    """What the consumers of one fan_out() share during a backward pass: the buffer their input gradients are summed in."""
    __slots__ = ("buf",)

    def __init__(self):
        self.buf = None


class _FanOutFn(torch.autograd.Function):
    """x -> n aliases of x, one per consumer.  Consumers that are this module's linear layers are handed the slot and sum their
    input gradients IN the slot's buffer, product by product (the input-gradient kernel's accumulate epilogue); whatever the other
    consumers return is added here.  Without it autograd launches one element-wise addition per extra consumer: eight per SET layer
    and pass (the vector stream feeds two projections and the residual, the invariant features two feed-forward pairs, ...)."""

    @staticmethod
    def forward(ctx, x, slot, n):
        ctx.slot, ctx.x_shape = slot, x.shape
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        slot = ctx.slot
        buf, slot.buf = slot.buf, None
        total, owned = buf, buf is not None          # the slot's buffer is ours to add onto; a consumer's own gradient is not
        for g in gs:
            if g is None or (buf is not None and g.data_ptr() == buf.data_ptr() and g.numel() == buf.numel()):
                continue                    # nothing, or the slot's own buffer as returned by its first consumer
            g = g.reshape(ctx.x_shape)
            if total is None:
                total = g
            elif owned:
                total = total.view(ctx.x_shape).add_(g)
            else:
                total, owned = total + g, True
        return (None if total is None else total.view(ctx.x_shape)), None, None


_FAN_OUT = True      # False (tests, A/B): every consumer's input gradient through autograd's own additions


def fan_out(x, n):
    """(slot, [n aliases of x]) where the own kernels differentiate x on the GPU, (None, [x] * n) otherwise.  Pass the slot to the
    linear layers among x's consumers (linear / linear2 `slot=`), each with its OWN alias; any other consumer takes an alias too."""
    if n > 1 and _FAN_OUT and _on_device_with_grad(x) and x.requires_grad:
        slot = _Slot()
        return slot, list(_FanOutFn.apply(x, slot, n))
    return None, [x] * n


def linear(x, weight, bias=None, relu=False, rowdiv=None, addend=None, tail=None, x_relu=False, premasked=False, slot=None):
    """act(x @ weight.T + bias) / rowdiv, differentiable in x, weight, bias and rowdiv (act = ReLU if relu; rowdiv: one value
    per row, broadcast over the output features -- the `/ F_norm` of the reference's SET layers).  Two followers can ride on
    the product's launch: `addend` (same shape as the result) is added to it -- a residual --, `tail` [..., t] is appended to it
    along the last dimension (torch.cat([result, tail], -1)).  x_relu / premasked: a ReLU layer feeding ONLY this one -- the pair
    linear(linear(x, w1, relu=True, premasked=True), w2, x_relu=True) applies the ReLU's mask once, in the epilogue of the second
    layer's input gradient (_LinearFn); they change nothing in the forward and nothing outside the HIP path."""
    if _on_device_with_grad(x, weight, bias, rowdiv, addend, tail):
        if addend is None or (not relu and rowdiv is None and tail is None):
            return _LinearFn.apply(x, weight, bias, bool(relu), rowdiv, addend, tail, bool(x_relu), bool(premasked), slot)
        y = _LinearFn.apply(x, weight, bias, bool(relu), rowdiv, None, None, bool(x_relu), bool(premasked), slot)     # a follower the kernel does not take: own launches
    else:
        y = F.linear(x, weight, bias)
        y = F.relu(y) if relu else y
        y = y if rowdiv is None else y / rowdiv
    y = y if addend is None else addend + y
    return y if tail is None else torch.cat([y, tail], dim=-1)


class _Adjacent3Fn(torch.autograd.Function):
    """Three parameters that lie back to back in one allocation, seen as the one stacked tensor they already are: no launch in
    the forward, views of the incoming gradient in the backward (what `torch.cat` + its backward produce with two copies)."""

    @staticmethod
    def forward(ctx, a, b, c):
        ctx.n = a.shape[0]
        return a.detach().as_strided((3 * a.shape[0],) + tuple(a.shape[1:]), a.stride(), a.storage_offset())

    @staticmethod
    def backward(ctx, d):
        n = ctx.n
        return d[:n], d[n:2 * n], d[2 * n:]


def adjacent3(a, b, c):
    """True if b starts where a ends and c where b ends (same shape, dtype, contiguous): SubequivariantAttention lays its q / k / v
    projections out that way (set_policy.py `_adjoin`)."""
    if not (a.shape == b.shape == c.shape and a.dtype == b.dtype == c.dtype and a.is_contiguous() and b.is_contiguous()
            and c.is_contiguous() and a.device == b.device == c.device):
        return False
    step = a.numel() * a.element_size()
    return b.data_ptr() == a.data_ptr() + step and c.data_ptr() == b.data_ptr() + step and \
        a.untyped_storage().data_ptr() == c.untyped_storage().data_ptr()


def stacked3(a, b, c):
    """torch.cat([a, b, c], 0) -- without the copy when the three already lie back to back."""
    if adjacent3(a, b, c):
        return _Adjacent3Fn.apply(a, b, c)
    return torch.cat([a, b, c], dim=0)


def linear2(x, w0, w1, b0=None, b1=None, relu=False, rowdiv=None, shared=False, addend=None, tail=None, x_relu=False, premasked=False,
            slot=None):
    """`linear` for the same layer of two networks at once: returns [2, ..., N]; x = the input both share ([..., K], shared=True) or
    their inputs stacked ([2, ..., K]); rowdiv stacked [2, ..., 1]; addend stacked [2, ..., N]; tail [2, ..., t] (or one both share,
    [..., t] / expanded)."""
    if _on_device_with_grad(x, w0, w1, b0, b1, rowdiv, addend, tail) and (addend is None or (not relu and rowdiv is None and tail is None)):
        if tail is not None and tail.dim() == x.dim() + (1 if shared else 0) and tail.stride(0) == 0:
            tail = tail[0]                          # an expanded pair: the one tensor both networks share
        return _Linear2Fn.apply(x, w0, w1, b0, b1, bool(relu), rowdiv, bool(shared), addend, tail, bool(x_relu), bool(premasked), slot)
    xs = (x, x) if shared else (x[0], x[1])
    ts = (None, None) if tail is None else ((tail[0], tail[1]) if tail.dim() == xs[0].dim() + 1 else (tail, tail))
    return torch.stack([linear(xs[0], w0, b0, relu, None if rowdiv is None else rowdiv[0], None if addend is None else addend[0], ts[0]),
                        linear(xs[1], w1, b1, relu, None if rowdiv is None else rowdiv[1], None if addend is None else addend[1], ts[1])])


def gram_fn(z):
    """z [..., 3, 32] -> (vec(Z'Z) [..., 1024], ||Z'Z||_F + 1 [..., 1])  (reference SEActor.py:94-98)."""
    if _on_device_with_grad(z):
        return _GramFn.apply(z)
    gram = torch.einsum("...sa,...sc->...ac", z, z).flatten(-2)
    return gram, gram.norm(dim=-1, keepdim=True) + 1.0


TRI_GRAM = True      # False (tests): the invariant layers on all 1 024 entries of Z'Z (rounds 2-4)


def tri_weights(weights, like):
    """The invariant layers' weights [rows, 1024] folded onto the lower triangle, [rows, 528] each (one launch for up to 16), or None
    where the own kernels do not run for a pass over `like` (the pass's input): then `gram_fn` and the unfolded weights are used
    (gram_tri_fn pairs with the folded ones)."""
    if not (TRI_GRAM and _on_device_with_grad(like, *weights) and len(weights) <= 16 and all(w.dim() == 2 and w.shape[1] == 1024 for w in weights)):
        return None
    out = _FoldFn.apply(*weights)
    for o, w in zip(out, weights):
        if w.is_leaf and w.requires_grad:
            o._sgrl_fold_leaf = w          # deferred_wgrads may postpone the folded weight's gradient and unfold it into w.grad (flush_wgrads)
    return out


def gram_tri_fn(z):
    """z [..., 3, 32] -> (tri(Z'Z) [..., 528], ||Z'Z||_F + 1 [..., 1]); only on the own kernels (callers hold folded weights)."""
    return _GramTriFn.apply(z)


def set_attention(qkv, vgp, gdir, bias, scale):
    """Limb attention of the SET layers (reference subequivariant_attentions.py:90-151 between the projections), 2 heads x 128
    channels: qkv [B, L, 768] = q | k | v (q is multiplied by `scale` here), vector values given in parts -- vgp [B, L, 3, 252]
    (126 projected channels per head) and gdir [B, L, 3, 2] (channels 126, 127 of BOTH heads) --, bias [2, L, L] or None ->
    (o [B, L, 256], og [B, L, 3, 256]) with w = softmax_j(scale q_i . k_j + bias) per head."""
    B, Ln = qkv.shape[:2]
    if _on_device_with_grad(qkv, vgp, gdir, bias) and qkv.shape[-1] == 768 and vgp.shape[-1] == 252 and Ln <= 14:
        return _AttnFn.apply(qkv, vgp, gdir, bias, float(scale))
    qh = (qkv[..., :256] * scale).view(B, Ln, 2, 128)
    kh, vh = qkv[..., 256:512].view(B, Ln, 2, 128), qkv[..., 512:].view(B, Ln, 2, 128)
    vg = torch.cat([vgp.view(B, Ln, 3, 2, 126), gdir.unsqueeze(3).expand(B, Ln, 3, 2, 2)], dim=-1)
    s = torch.einsum("bihd,bjhd->bhij", qh, kh)
    if bias is not None:
        s = s + bias.unsqueeze(0)
    w = F.softmax(s, dim=-1)
    o = torch.einsum("bhij,bjhd->bihd", w, vh).reshape(B, Ln, 256)
    og = torch.einsum("bhij,bjshd->bishd", w, vg).reshape(B, Ln, 3, 256)
    return o, og


# ---- counter-RNG dropout (include/sgrl_train.h "counter-RNG dropout"; csrc/dropout_rng.h) ------------------------------------------
# The masks of the SWAT networks' dropout sites are a function of (seed, step, site, element index), not a draw from torch's
# generator: the kernels regenerate them in the backward pass, and the PyTorch path below draws the SAME masks with integer tensor
# arithmetic -- slow and exact; it is what float64 comparisons and the no-grad target passes of an update run.
DROPOUT_STREAM_BASE = 0x100      # stream ids 0 and 1 are the replay draw's (csrc/replay_rng.h)
_M32 = 0xFFFFFFFF
# how often each dropout path was ENTERED since import (tests: an agent with dropout_rate 0 enters none): "kernel" / "attention_kernel"
# the HIP kernels, "counter" the torch restatement of the counter RNG, "torch" F.dropout (no dropout_rng context active)
dropout_calls = {"kernel": 0, "attention_kernel": 0, "counter": 0, "torch": 0}
_rng = None


class DropoutRng(object):
    """What the dropout calls of one update share: `seed` (a host int, 64 bits), `step` (a one-element int64 tensor holding the bits
    of the uint64 the kernels read; whoever owns it changes it between updates, never inside one) and `site`, the running number of
    the dropout call, which every call -- kernel or not -- takes in program order."""
    __slots__ = ("seed", "step", "site")

    def __init__(self, seed, step):
        if not (torch.is_tensor(step) and step.dtype == torch.int64 and step.numel() == 1 and step.is_contiguous()):
            raise ValueError("dropout_rng: step_tensor must be a one-element int64 tensor")
        self.seed, self.step, self.site = int(seed) & (2 ** 64 - 1), step, 0

    def next_site(self):
        s = self.site
        self.site = s + 1
        return s

    def reserve(self, n):
        """The running site number, advanced by n: for a caller that runs n dropout calls behind ONE library call (the HIP target
        chain of a SWAT update: 39) and takes their numbers in program order, where the calls themselves would have."""
        s = self.site
        self.site = s + int(n)
        return s


@contextlib.contextmanager
def dropout_rng(seed, step_tensor):
    """Inside this context every dropout of this module (dropout(), swat_attention(dropout_p=...)) takes its mask from the counter RNG
    with (seed, step_tensor's value, running site number from 0); outside any such context they fall back to F.dropout."""
    global _rng
    old, _rng = _rng, DropoutRng(seed, step_tensor)
    try:
        yield _rng
    finally:
        _rng = old


def _mul_hi_lo(a, c):
    """a: a 32-bit constant, c: int64 tensor of values < 2^32 -> (high, low) 32 bits of a * c, without leaving int64's range."""
    al, ah = a & 0xFFFF, a >> 16
    pl, ph = c * al, c * ah                     # < 2^48 each
    return (ph + (pl >> 16)) >> 16, (pl + ((ph & 0xFFFF) << 16)) & _M32


def counter_words(seed, step, stream, idx):
    """replay_word(seed, step, stream, idx) of csrc/replay_rng.h for an int64 tensor of element indices `idx`; step: a one-element
    int64 tensor on idx's device.  -> int64 tensor of the 32-bit words."""
    step = step.reshape(())
    c = [(idx >> 2) & _M32, (step & _M32).expand_as(idx), ((step >> 32) & _M32).expand_as(idx), torch.full_like(idx, int(stream) & _M32)]
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(10):
        h0, l0 = _mul_hi_lo(0xD2511F53, c[0])
        h1, l1 = _mul_hi_lo(0xCD9E8D57, c[2])
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return torch.stack(c, dim=-1).gather(-1, (idx & 3).unsqueeze(-1)).squeeze(-1)


def dropout_threshold_scale(p):
    """(thr, scale) of the definition for a probability p, which the ABI takes as a float32: thr = floor(p * 2^32), scale = the float32
    1 / (1 - p), as a Python float (0 at p = 1, where nothing is kept and the kernels never multiply)."""
    p32 = np.float32(p)
    thr = int(np.floor(np.float64(p32) * 4294967296.0))
    return thr, (0.0 if p32 >= 1 else float(np.float32(1.0) / (np.float32(1.0) - p32)))


def _counter_dropout(x, p, rng, site):
    """The definition on any device and dtype: the mask over x's row-major element index, x * scale where kept."""
    dropout_calls["counter"] += 1
    thr, scale = dropout_threshold_scale(p)
    idx = torch.arange(x.numel(), dtype=torch.int64, device=x.device)
    keep = (counter_words(rng.seed, rng.step.to(x.device), DROPOUT_STREAM_BASE + site, idx) >= thr).view(x.shape)
    return torch.where(keep, x * scale, torch.zeros((), dtype=x.dtype, device=x.device))


class _DropoutFn(torch.autograd.Function):
    """y = dropout(x) by the counter RNG, one launch forward and one backward (csrc/dropout.hip); nothing is saved but the call's
    (p, seed, step tensor, site)."""

    @staticmethod
    def forward(ctx, x, p, seed, step, site):
        x2 = _c(x)
        y = torch.empty_like(x2)
        ctx.call = (p, seed, step, site)
        _call("sgrl_dropout_forward", _p(x2), _p(y), x2.numel(), *_drop_args(ctx.call), _st(x.device))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy2 = _c(dy)
        dx = torch.empty_like(dy2)
        _call("sgrl_dropout_backward", _p(dy2), _p(dx), dy2.numel(), *_drop_args(ctx.call), _st(dy.device))
        return dx, None, None, None, None


def dropout(x, p, training=True):
    """F.dropout(x, p, training) with the mask of the active dropout_rng context: the element-wise kernels where autograd records on
    the GPU in float32, the torch restatement of the same definition elsewhere (CPU, float64, torch.no_grad()).  Without a context:
    F.dropout.  p == 0 or not training: x itself -- nothing is launched, allocated or recorded."""
    if not training or p <= 0.0:
        return x
    rng = _rng
    if rng is None:
        dropout_calls["torch"] += 1
        return F.dropout(x, float(p), True)
    site = rng.next_site()
    if x.numel() > 0 and _on_device_with_grad(x) and rng.step.device == x.device:
        dropout_calls["kernel"] += 1
        return _DropoutFn.apply(x, float(p), rng.seed, rng.step, site)
    return _counter_dropout(x, p, rng, site)


class _SwatAttnDropFn(torch.autograd.Function):
    """_SwatAttnFn with the softmax weights dropped by the counter RNG (k_swat_attn_fwd_drop / k_swat_attn_bwd_drop): the saved w is
    the undropped one, the backward regenerates the mask from (seed, step, site)."""

    @staticmethod
    def forward(ctx, qkv, bias, scale, p, seed, step, site):
        return _swat_attn_forward(ctx, "sgrl_swat_attention_forward_dropout", qkv, bias, scale, p, seed, step, site)

    @staticmethod
    def backward(ctx, d_o):
        return _swat_attn_backward(ctx, "sgrl_swat_attention_backward_dropout", d_o)


SWAT_MAX_LIMBS = 15      # SGRL_SWAT_MAX_LIMBS (include/sgrl_swat.h): what k_swat_attn_* hold in registers


def swat_attention(qkv, bias, scale, num_heads=2, dropout_p=0.0, training=False):
    """Limb attention of the SWAT networks (swat_policy._SelfAttention between in_proj and out_proj): qkv [B, L, 3 E] = q | k | v
    (q is multiplied by `scale` here), bias [H, L, L] or None -> o [B, L, E] with w = softmax_j(scale q_i . k_j + bias) per head.
    One launch forward and one backward when autograd records on the GPU, E = 128, H = 2 and L <= 15; the module's own operations,
    one for one, otherwise.  dropout_p > 0 and training: the softmax weights are dropped (reference attentions.py:163) -- inside the
    kernel pair's dropout variant under a dropout_rng context, by dropout() on the module's own operations otherwise; with
    dropout_p == 0 or not training nothing differs from the call without the two arguments."""
    B, Ln = qkv.shape[:2]
    drop = bool(training) and dropout_p > 0.0
    on_kernels = qkv.dim() == 3 and qkv.shape[-1] == 384 and num_heads == 2 and 1 <= Ln <= SWAT_MAX_LIMBS and B > 0 and _on_device_with_grad(qkv, bias)
    if on_kernels and not drop:
        return _SwatAttnFn.apply(qkv, bias, float(scale))
    if on_kernels and _rng is not None and _rng.step.device == qkv.device:
        dropout_calls["attention_kernel"] += 1
        return _SwatAttnDropFn.apply(qkv, bias, float(scale), float(dropout_p), _rng.seed, _rng.step, _rng.next_site())
    E = qkv.shape[-1] // 3
    H, hd = num_heads, E // num_heads
    q, k, v = qkv.chunk(3, dim=-1)
    q = (q * scale).view(B, Ln, H, hd)
    k, v = k.view(B, Ln, H, hd), v.view(B, Ln, H, hd)
    s = torch.einsum("bihd,bjhd->bhij", q, k)
    if bias is not None:
        s = s + bias.unsqueeze(0)
    w = F.softmax(s, dim=-1)
    if drop:
        w = dropout(w, dropout_p, True)
    return torch.einsum("bhij,bjhd->bihd", w, v).reshape(B, Ln, E)


def zmat(z, mat):
    """Per node: z [..., 3, 32] . mat [..., 32, 32] -> [..., 3, 32]  (reference SEActor.py:108-110: torch.bmm(g_src3, mat3))."""
    if _on_device_with_grad(z, mat) and z.shape[-2:] == (3, 32) and mat.shape[-2:] == (32, 32):
        return _ZmatFn.apply(z, mat)
    return torch.einsum("...sa,...ac->...sc", z, mat)


def add_layer_norm(x, res, norm):
    """norm(x + res) for an nn.LayerNorm over the last dimension (res may be None): one launch forward, one backward when autograd is
    recording on the GPU and the width is 128; the module itself otherwise."""
    if x.shape[-1] == 128 and norm.elementwise_affine and norm.bias is not None and _on_device_with_grad(x, res, norm.weight, norm.bias):
        return _AddLNFn.apply(x, res, norm.weight, norm.bias, None, None, float(norm.eps))
    return norm(x if res is None else x + res)


def add_layer_norm2(x, res, n0, n1):
    """The same for the stacked activations of two networks: x [2, ..., 128] -> stack(n0(x[0] + res[0]), n1(x[1] + res[1]))."""
    if x.shape[-1] == 128 and x.shape[0] == 2 and n0.elementwise_affine and n1.elementwise_affine and n0.bias is not None and \
            n1.bias is not None and n0.eps == n1.eps and _on_device_with_grad(x, res, n0.weight, n0.bias, n1.weight, n1.bias):
        return _AddLNFn.apply(x, res, n0.weight, n0.bias, n1.weight, n1.bias, float(n0.eps))
    s = x if res is None else x + res
    a, b = s.unbind(0)          # (not s[0], s[1]: each index costs a zero-filled gradient, a slice copy and an add going back)
    return torch.stack([n0(a), n1(b)])


_idx3_cache = {}


def embed3(embeddings, positional_indices):
    """torch.cat([emb(idx) for emb, idx in zip(embeddings, positional_indices)], dim=1) for three nn.Embedding tables of equal row
    count (the traversal embeddings of the SET models): one launch forward and one backward when autograd records on the GPU."""
    ws = [e.weight for e in embeddings]
    if len(ws) == 3 and _on_device_with_grad(*ws) and all(w.shape[0] == ws[0].shape[0] for w in ws) and sum(w.shape[1] for w in ws) <= 128 \
            and all(e.padding_idx is None and e.max_norm is None for e in embeddings) and all(i.dtype == torch.int64 and i.dim() == 1 for i in positional_indices):
        key = tuple((i.data_ptr(), i.shape[0], i._version) for i in positional_indices)
        ent = _idx3_cache.get(key)
        if ent is None:
            if len(_idx3_cache) > 256:
                _idx3_cache.clear()
            # the index tensors are kept alive with the entry, so their addresses cannot be reused by other tensors
            ent = _idx3_cache[key] = (torch.stack(list(positional_indices)).contiguous(), list(positional_indices))
        return _Embed3Fn.apply(ent[0], ws[0], ws[1], ws[2])
    return torch.cat([emb(idx) for emb, idx in zip(embeddings, positional_indices)], dim=1)


# ---- SMP networks (smp_policy `train_kernels`; csrc/smp_train.hip) -----------------------------------------------------------------
SMP_MAX_LIMBS, SMP_MAX_CHILDREN, SMP_MSG = 16, 8, 32      # SGRL_SMP_MAX_LIMBS / SGRL_SMP_MAX_CHILDREN (include/sgrl_smp.h), message width


class SmpTable(object):
    """The gather table of one tree level (include/sgrl_train.h sgrl_smp_gather_forward): node [n, S] = the row block of the source
    segment s of limb j comes from (-1: zeros), off [n, S] = its first column.  Host int32 arrays, built once per morphology by
    smp_policy from its _Tree; the kernels receive them in their arguments.  `one_reader`: no two entries read the same 32 columns
    of the same node -- what lets the backward write the source's gradient with plain stores (the kernels run only then)."""

    def __init__(self, node, off):
        self.node = np.ascontiguousarray(np.asarray(node, dtype=np.int32))
        self.off = np.ascontiguousarray(np.asarray(off, dtype=np.int32))
        assert self.node.ndim == 2 and self.node.shape == self.off.shape
        self.n, self.S = self.node.shape
        read = [(int(a), int(o)) for a, o in zip(self.node.ravel(), self.off.ravel()) if a >= 0]
        self.one_reader = len(set(read)) == len(read)
        self.max_node = max([a for a, _ in read], default=-1)
        self.max_off = max([o for _, o in read], default=0)
        self.aligned = all(o >= 0 and o % SMP_MSG == 0 for _, o in read)


class _SmpGatherFn(torch.autograd.Function):
    """own [n, B, W0] or None, src [n_src, B, Wsrc] or None -> act([own' | segments]) [n, B, W0 + 32 S]: one launch forward, one
    backward (csrc/smp_train.hip k_smp_gather_fwd / k_smp_gather_bwd)."""

    @staticmethod
    def forward(ctx, own, src, tab, normalize, act_tanh, B):
        dev = (own if own is not None else src).device
        n, S = tab.n, tab.S
        W0 = 0 if own is None else own.shape[-1]
        own_c, src_c = _c(own), _c(src)
        n_src, Wsrc = (0, 0) if src is None else (src.shape[0], src.shape[-1])
        normalize = bool(normalize) and W0 > 0
        out = _f32(dev, n, B, W0 + SMP_MSG * S)
        inv = _f32(dev, n, B) if normalize else None
        _call("sgrl_smp_gather_forward", _p(own_c), W0, 1 if normalize else 0, _p(src_c), n_src, Wsrc, ctypes.c_void_p(tab.node.ctypes.data),
              ctypes.c_void_p(tab.off.ctypes.data), S, 1 if act_tanh else 0, _p(out), _p(inv), n, B, _st(dev))
        ctx.save_for_backward(own_c if normalize else None, inv, out if act_tanh else None)
        ctx.tab, ctx.normalize, ctx.act, ctx.B, ctx.W0 = tab, normalize, bool(act_tanh), B, W0
        ctx.own_shape = None if own is None else own.shape
        ctx.src_shape = None if src is None else src.shape
        return out

    @staticmethod
    def backward(ctx, d_out):
        own, inv, out = ctx.saved_tensors
        tab, B, W0 = ctx.tab, ctx.B, ctx.W0
        d = _c(d_out)
        need_own = ctx.own_shape is not None and ctx.needs_input_grad[0]
        need_src = ctx.src_shape is not None and ctx.needs_input_grad[1]
        d_own = _f32(d.device, tab.n, B, W0) if need_own else None
        d_src = _f32(d.device, *ctx.src_shape) if need_src else None
        n_src, Wsrc = (0, 0) if ctx.src_shape is None else (ctx.src_shape[0], ctx.src_shape[-1])
        if need_own or need_src:
            _call("sgrl_smp_gather_backward", _p(d), _p(out), _p(own), _p(inv), W0, 1 if ctx.normalize else 0, n_src, Wsrc,
                  ctypes.c_void_p(tab.node.ctypes.data), ctypes.c_void_p(tab.off.ctypes.data), tab.S, 1 if ctx.act else 0,
                  _p(d_own), _p(d_src), tab.n, B, _st(d.device))
        return (None if d_own is None else d_own.view(ctx.own_shape)), d_src, None, None, None, None


def smp_gather(own, src, tab, normalize=False, act_tanh=False, batch=None):
    """The input of one tree level's shared module, rows [n, B, .] (n = tab.n limbs): act([own' | seg_0 | ... | seg_{S-1}]) with
    own' = F.normalize(own) or own (own None: no own part), seg_s = src[tab.node[j, s], :, tab.off[j, s] : + 32] or zeros (node -1, or
    src None), act = tanh or the identity.  One launch forward and one backward when autograd records on the GPU and the shapes are the
    kernels' (own 32 or 64 wide, at most 16 limbs and 8 segments, src a multiple of 32 up to 256 wide, every source segment read at
    most once); smp_policy's own operations -- zeros, slices, cat, stack, F.normalize, cat, tanh, in that order -- otherwise."""
    ref = own if own is not None else src
    n, S = tab.n, tab.S
    B = int(batch) if ref is None else ref.shape[1]
    if ref is not None and B > 0 and 1 <= n <= SMP_MAX_LIMBS and 1 <= S <= SMP_MAX_CHILDREN and tab.one_reader and tab.aligned \
            and (own is None or (own.dim() == 3 and own.shape[0] == n and own.shape[-1] in (32, 64))) \
            and (src is None or (src.dim() == 3 and src.shape[1] == B and 1 <= src.shape[0] <= SMP_MAX_LIMBS and src.shape[-1] % SMP_MSG == 0
                                 and SMP_MSG <= src.shape[-1] <= SMP_MSG * SMP_MAX_CHILDREN and tab.max_node < src.shape[0]
                                 and tab.max_off + SMP_MSG <= src.shape[-1])) \
            and (src is None or own is None or (src.dtype == own.dtype and src.device == own.device)) and _on_device_with_grad(ref, own, src):
        return _SmpGatherFn.apply(own, src, tab, bool(normalize), bool(act_tanh), B)
    rows = []
    if ref is None:
        raise ValueError("smp_gather: neither an own part nor a source")
    zero = torch.zeros((B, SMP_MSG), device=ref.device, dtype=ref.dtype)
    for j in range(n):
        segs = []
        for s in range(S):
            a, o = int(tab.node[j, s]), int(tab.off[j, s])
            segs.append(src[a][:, o:o + SMP_MSG] if (a >= 0 and src is not None) else zero)
        rows.append(torch.cat(segs, dim=-1) if S > 1 else segs[0])
    m = torch.stack(rows)
    if own is not None:
        m = torch.cat([F.normalize(own, dim=-1) if normalize else own, m], dim=-1)
    return torch.tanh(m) if act_tanh else m


class _SmpUpTailFn(torch.autograd.Function):
    """a [..., 64] -> F.normalize(fc3(tanh(a))) [..., 32]: one launch forward, one backward (csrc/smp_train.hip k_smp_up_tail_*); fc3's
    weight / bias gradients go through sgrl_linear_wgrad_group with (dy = dz, x = tanh(a)), postponed under deferred_wgrads exactly as
    a leaf _LinearFn layer's."""

    @staticmethod
    def forward(ctx, a, weight, bias):
        a2 = _c(a.reshape(-1, 64))
        w = _c(weight)
        R = a2.shape[0]
        dev = a.device
        t = _f32(dev, R, 64)
        u = _f32(dev, R, 32)
        inv = _f32(dev, R)
        _call("sgrl_smp_up_tail_forward", _p(a2), _p(w), _p(bias), _p(t), _p(u), _p(inv), R, _st(dev))
        ctx.save_for_backward(t, u, inv, w)
        ctx.targets = _leaf_targets(weight, bias) if weight.is_leaf else None       # fc3 is never a folded weight
        ctx.a_shape = a.shape
        return u.view(*a.shape[:-1], 32)

    @staticmethod
    def backward(ctx, du):
        t, u, inv, w = ctx.saved_tensors
        R = t.shape[0]
        d = _c(du.reshape(R, 32))
        dev = d.device
        dz = _f32(dev, R, 32)
        da = _f32(dev, R, 64)
        st = _st(dev)
        _call("sgrl_smp_up_tail_backward", _p(d), _p(u), _p(inv), _p(t), _p(w), _p(dz), _p(da), R, st)
        need_w, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gw = gb = None
        if need_w or need_b:
            ((gw, gb),), now = _settle([_Wgrad(dz, None, None, t, 32, False, ctx.targets, need_w, need_b, st)])
            flush_wgrads(now)
        return (da.view(ctx.a_shape) if ctx.needs_input_grad[0] else None), gw, gb


def smp_up_tail(a, weight, bias):
    """F.normalize(F.linear(torch.tanh(a), weight, bias), dim=-1) for fc3 [32, 64] of the SMP bottom-up modules (a = fc2's output): one
    launch forward and one backward when autograd records on the GPU; those three operations otherwise."""
    if a.shape[-1] == 64 and tuple(weight.shape) == (32, 64) and bias is not None and tuple(bias.shape) == (32,) and a.numel() > 0 \
            and _on_device_with_grad(a, weight, bias):
        return _SmpUpTailFn.apply(a, weight, bias)
    return F.normalize(F.linear(torch.tanh(a), weight, bias), dim=-1)


class _NormalizeRowsFn(torch.autograd.Function):
    """F.normalize(x, dim=-1) for rows up to 256 wide: one launch forward, one backward (csrc/smp_train.hip k_row_norm_*)."""

    @staticmethod
    def forward(ctx, x):
        W = x.shape[-1]
        x2 = _c(x.reshape(-1, W))
        R = x2.shape[0]
        y = _f32(x.device, R, W)
        inv = _f32(x.device, R)
        _call("sgrl_row_normalize_forward", _p(x2), _p(y), _p(inv), R, W, _st(x.device))
        ctx.save_for_backward(y, inv)
        ctx.x_shape = x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        R, W = y.shape
        d = _c(dy.reshape(R, W))
        dx = torch.empty_like(y)
        _call("sgrl_row_normalize_backward", _p(d), _p(y), _p(inv), _p(dx), R, W, _st(d.device))
        return dx.view(ctx.x_shape)


def _upstream(g):
    """The upstream gradient of a scalar loss as the device scalar the backward kernels read."""
    return g if g.dtype == torch.float32 else g.float()


class _TwinMseFn(torch.autograd.Function):
    """q1, q2, target (same shape, contiguous) -> mse(q1, target) + mse(q2, target), a 0-dim tensor: one launch forward, one
    backward (csrc/td3_loss.hip k_twin_mse_*); target receives no gradient."""

    @staticmethod
    def forward(ctx, q1, q2, target):
        loss = _f32(q1.device)
        _call("sgrl_td3_twin_mse_forward", _p(q1), _p(q2), _p(target), q1.numel(), _p(loss), _st(q1.device))
        ctx.save_for_backward(q1, q2, target)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        q1, q2, target = ctx.saved_tensors
        g = _upstream(g)
        dq1, dq2 = torch.empty_like(q1), torch.empty_like(q2)
        _call("sgrl_td3_twin_mse_backward", _p(q1), _p(q2), _p(target), q1.numel(), _p(g), _p(dq1), _p(dq2), _st(q1.device))
        return (dq1 if ctx.needs_input_grad[0] else None), (dq2 if ctx.needs_input_grad[1] else None), None


class _NegMeanFn(torch.autograd.Function):
    """q (contiguous) -> -q.mean(), a 0-dim tensor: one launch forward, one backward (csrc/td3_loss.hip k_neg_mean_*)."""

    @staticmethod
    def forward(ctx, q):
        loss = _f32(q.device)
        _call("sgrl_td3_neg_mean_forward", _p(q), q.numel(), _p(loss), _st(q.device))
        ctx.q_shape = q.shape
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = _upstream(g)
        dq = _f32(g.device, *ctx.q_shape)
        _call("sgrl_td3_neg_mean_backward", dq.numel(), _p(g), _p(dq), _st(g.device))
        return dq


def _loss_kernel_inputs(*ts):
    """The loss kernels apply: float32 tensors of one shape on one GPU, contiguous, non-empty, with autograd recording."""
    a = ts[0]
    return a.numel() > 0 and all(t.is_cuda and t.dtype == torch.float32 and t.device == a.device and t.shape == a.shape and
                                 t.is_contiguous() for t in ts) and _on_device_with_grad(*ts)


def twin_mse(q1, q2, target):
    """F.mse_loss(q1, target) + F.mse_loss(q2, target) -- the critic loss of a TD3 update (reference agent.py:145-147): one launch
    forward and one backward (float64 sums in a fixed order, include/sgrl_train.h sgrl_td3_twin_mse_*) when autograd records on the
    GPU over contiguous float32 tensors of one shape; that expression itself otherwise.  `target` receives no gradient from the
    kernels: pass a tensor that needs none (the update's target is computed under no_grad)."""
    if not target.requires_grad and _loss_kernel_inputs(q1, q2, target):
        return _TwinMseFn.apply(q1, q2, target)
    return F.mse_loss(q1, target) + F.mse_loss(q2, target)


def neg_mean(q):
    """-q.mean() -- the actor loss of a TD3 update (reference agent.py:167): one launch forward and one backward under the
    conditions of twin_mse; that expression itself otherwise."""
    if _loss_kernel_inputs(q):
        return _NegMeanFn.apply(q)
    return -q.mean()


def normalize_rows(x):
    """F.normalize(x, dim=-1): one launch forward and one backward when autograd records on the GPU and the rows are at most 256
    (32 x SGRL_SMP_MAX_CHILDREN) wide; F.normalize itself otherwise."""
    if x.dim() >= 2 and 1 <= x.shape[-1] <= SMP_MSG * SMP_MAX_CHILDREN and x.numel() > 0 and _on_device_with_grad(x):
        return _NormalizeRowsFn.apply(x)
    return F.normalize(x, dim=-1)
