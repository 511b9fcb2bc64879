"""NumPy float64 restatements of the three SMP training kernel pairs (csrc/smp_train.hip; include/sgrl_train.h), forward and
backward, driven by the same tables the binding hands the kernels (train_ops.SmpTable: node / off [n, S])."""
import numpy as np

EPS = 1e-12
MSG = 32


def _normalize(x):
    den = np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), EPS)
    return x / den, 1.0 / den[..., 0]


def _normalize_bwd(dy, y, inv):
    """dx of y = x / max(||x||, eps): a clamped row (||x|| < eps, inv = 1 / eps) passes dy / eps."""
    dot = (dy * y).sum(-1, keepdims=True)
    full = (dy - y * dot) * inv[..., None]
    return np.where((inv >= 1.0 / EPS)[..., None], dy * inv[..., None], full)


def gather_forward(own, src, node, off, normalize, act_tanh, B=None):
    """-> (out [n, B, W0 + 32 S], inv [n, B] or None)."""
    n, S = node.shape
    B = (own if own is not None else src).shape[1] if B is None else B
    W0 = 0 if own is None else own.shape[-1]
    out = np.zeros((n, B, W0 + MSG * S))
    inv = None
    if own is not None:
        o = np.asarray(own, dtype=np.float64)
        if normalize:
            o, inv = _normalize(o)
        out[..., :W0] = o
    if src is not None:
        for j in range(n):
            for s in range(S):
                if node[j, s] >= 0:
                    out[j, :, W0 + MSG * s:W0 + MSG * (s + 1)] = src[node[j, s], :, off[j, s]:off[j, s] + MSG]
    return (np.tanh(out) if act_tanh else out), inv


def gather_backward(d_out, out, own, inv, src_shape, node, off, normalize, act_tanh):
    """-> (d_own or None, d_src or None: ALL of src's gradient, zeros where nobody read)."""
    n, S = node.shape
    g = np.asarray(d_out, dtype=np.float64)
    if act_tanh:
        g = g * (1.0 - out * out)
    W0 = 0 if own is None else own.shape[-1]
    d_own = None
    if own is not None:
        d_own = g[..., :W0]
        if normalize:
            d_own = _normalize_bwd(d_own, np.asarray(own, dtype=np.float64) * inv[..., None], inv)
    d_src = None
    if src_shape is not None:
        d_src = np.zeros(src_shape)
        for j in range(n):
            for s in range(S):
                if node[j, s] >= 0:
                    d_src[node[j, s], :, off[j, s]:off[j, s] + MSG] = g[j, :, W0 + MSG * s:W0 + MSG * (s + 1)]     # one reader each
    return d_own, d_src


def up_tail_forward(a, w3, b3):
    """-> (t [R, 64], u [R, 32], inv [R])."""
    t = np.tanh(np.asarray(a, dtype=np.float64))
    u, inv = _normalize(t @ np.asarray(w3, dtype=np.float64).T + b3)
    return t, u, inv


def up_tail_backward(du, u, inv, t, w3):
    """-> (dz [R, 32], da [R, 64], dw3 [32, 64], db3 [32])."""
    dz = _normalize_bwd(np.asarray(du, dtype=np.float64), u, inv)
    da = (dz @ np.asarray(w3, dtype=np.float64)) * (1.0 - t * t)
    return dz, da, dz.T @ t, dz.sum(0)


def normalize_forward(x):
    return _normalize(np.asarray(x, dtype=np.float64))


def normalize_backward(dy, y, inv):
    return _normalize_bwd(np.asarray(dy, dtype=np.float64), y, inv)
