"""float64 NumPy restatement of the loss head of a TD3 update (include/sgrl_train.h sgrl_td3_*; reference src/agent.py:145-147, 167):
what the kernels of csrc/td3_loss.hip are held to.  No device code.

    d_k[i]  = q_k[i] - target[i]                          (in float64)
    loss    = (sum d_1^2 + sum d_2^2) / n
    dq_k[i] = g * 2 d_k[i] / n
    neg_mean: loss = -sum q / n,  dq[i] = -g / n
"""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64).reshape(-1)


def twin_mse_forward(q1, q2, target):
    q1, q2, t = _f64(q1), _f64(q2), _f64(target)
    d1, d2 = q1 - t, q2 - t
    return (np.sum(d1 * d1) + np.sum(d2 * d2)) / q1.size


def twin_mse_backward(q1, q2, target, g):
    q1, q2, t = _f64(q1), _f64(q2), _f64(target)
    n = q1.size
    return float(g) * (2.0 * (q1 - t)) / n, float(g) * (2.0 * (q2 - t)) / n


def neg_mean_forward(q):
    q = _f64(q)
    return -np.sum(q) / q.size


def neg_mean_backward(n, g):
    return np.full(int(n), -float(g) / int(n), dtype=np.float64)
