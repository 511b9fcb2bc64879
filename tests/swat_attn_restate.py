"""NumPy float64 restatement of the SWAT attention kernels (csrc/train_gemm.hip k_swat_attn_fwd / k_swat_attn_bwd, C ABI in
include/sgrl_train.h): what `sgrl_swat_attention_forward` / `_backward` compute, written out index by index.

qkv [B, L, 384] = q | k | v (head h owns columns 64 h .. 64 h + 63 of each), bias [2, L, L] or None, d_o [B, L, 128]."""
import numpy as np

H, HD, E = 2, 64, 128


def _heads(x):
    """[B, L, 128] -> [B, 2, L, 64]."""
    B, L = x.shape[:2]
    return x.reshape(B, L, H, HD).transpose(0, 2, 1, 3)


def _flat(x):
    """[B, 2, L, 64] -> [B, L, 128]."""
    B, _, L, _ = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B, L, E)


def forward(qkv, bias, scale):
    """-> (w [B, 2, L, L], o [B, L, 128])."""
    qkv = np.asarray(qkv, dtype=np.float64)
    q, k, v = _heads(qkv[..., :E] * scale), _heads(qkv[..., E:2 * E]), _heads(qkv[..., 2 * E:])
    s = q @ k.transpose(0, 1, 3, 2)
    if bias is not None:
        s = s + np.asarray(bias, dtype=np.float64)[None]
    s = s - s.max(axis=-1, keepdims=True)
    w = np.exp(s)
    w = w / w.sum(axis=-1, keepdims=True)
    return w, _flat(w @ v)


def backward(qkv, scale, w, d_o):
    """-> (dqkv [B, L, 384], ds [B, 2, L, L]); the gradient of `bias` is ds.sum(0)."""
    qkv, w = np.asarray(qkv, dtype=np.float64), np.asarray(w, dtype=np.float64)
    q, k, v = _heads(qkv[..., :E]), _heads(qkv[..., E:2 * E]), _heads(qkv[..., 2 * E:])
    a = _heads(np.asarray(d_o, dtype=np.float64))
    dw = a @ v.transpose(0, 1, 3, 2)
    ds = w * (dw - (w * dw).sum(axis=-1, keepdims=True))
    dq = scale * (ds @ k)
    dk = ds.transpose(0, 1, 3, 2) @ (scale * q)
    dv = w.transpose(0, 1, 3, 2) @ a
    return np.concatenate([_flat(dq), _flat(dk), _flat(dv)], axis=-1), ds
