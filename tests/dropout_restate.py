"""NumPy restatement of the counter-RNG dropout (include/sgrl_train.h "counter-RNG dropout", csrc/dropout_rng.h): the mask of a
dropout call as a function of (seed, step, site, element index), the element-wise kernel pair (csrc/dropout.hip) and the SWAT
attention pair with dropped softmax weights (csrc/train_gemm.hip k_swat_attn_fwd_drop / k_swat_attn_bwd_drop): the arithmetic of
swat_attn_restate.py with the mask inserted.

    word = stream_words(seed, step, 0x100 + site, i)      Philox4x32-10, the replay draw's restatement (test_replay_sample.py)
    thr  = floor(float32(p) * 2^32)
    keep = word >= thr
    y    = keep ? x * (float32(1) / (float32(1) - float32(p))) : 0
"""
import numpy as np

import swat_attn_restate as A
from test_replay_sample import stream_words

STREAM_BASE = 0x100


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def scale32(p):
    """The float32 1 / (1 - p); 0 at p = 1, where nothing is kept."""
    p32 = np.float32(p)
    return np.float32(0.0) if p32 >= 1 else np.float32(1.0) / (np.float32(1.0) - p32)


def keep_mask(seed, step, site, n, p, start=0):
    """Keep decisions of elements start .. start + n - 1 -> bool [n]."""
    return stream_words(seed, step, STREAM_BASE + site, start, n).astype(np.uint64) >= np.uint64(threshold(p))


def dropout(x, p, seed, step, site):
    """The element-wise pair on an array of any shape (forward on x, backward on dy): float32 in, float32 arithmetic (bit for bit the
    kernel's); float64 in, the float32 scale widened."""
    x = np.asarray(x)
    keep = keep_mask(seed, step, site, x.size, p).reshape(x.shape)
    return np.where(keep, x * x.dtype.type(scale32(p)), x.dtype.type(0))


def attn_forward(qkv, bias, scale, p, seed, step, site):
    """-> (w [B, 2, L, L] UNDROPPED, o [B, L, 128], keep [B, 2, L, L]) in float64."""
    w, _ = A.forward(qkv, bias, scale)
    keep = keep_mask(seed, step, site, w.size, p).reshape(w.shape)
    wd = np.where(keep, w * np.float64(scale32(p)), 0.0)
    v = A._heads(np.asarray(qkv, dtype=np.float64)[..., 2 * A.E:])
    return w, A._flat(wd @ v), keep


def attn_backward(qkv, scale, w, d_o, p, seed, step, site):
    """w: the undropped weights -> (dqkv [B, L, 384], ds [B, 2, L, L]); the gradient of `bias` is ds.sum(0)."""
    qkv, w = np.asarray(qkv, dtype=np.float64), np.asarray(w, dtype=np.float64)
    q, k, v = A._heads(qkv[..., :A.E]), A._heads(qkv[..., A.E:2 * A.E]), A._heads(qkv[..., 2 * A.E:])
    a = A._heads(np.asarray(d_o, dtype=np.float64))
    m = np.where(keep_mask(seed, step, site, w.size, p).reshape(w.shape), np.float64(scale32(p)), 0.0)
    dw = (a @ v.transpose(0, 1, 3, 2)) * m
    ds = w * (dw - (w * dw).sum(axis=-1, keepdims=True))
    dq = scale * (ds @ k)
    dk = ds.transpose(0, 1, 3, 2) @ (scale * q)
    dv = (w * m).transpose(0, 1, 3, 2) @ a
    return np.concatenate([A._flat(dq), A._flat(dk), A._flat(dv)], axis=-1), ds
