"""NumPy restatement of the batch prologue of the MLP agent's TD3 update (include/sgrl_mlp.h "batch prologue", csrc/mlp_batch.hip):
the scaled reward and its mean and unbiased variance, in float32 and in the kernel's FIXED order -- thread t of 256 adds elements
t, t + 256, ... serially, a wave adds its 64 lanes by a butterfly (xor 32 .. 1), the four waves are added in order -- so that the
kernel can be held to these bits; and the same in float64, the yardstick of both."""
import numpy as np

THREADS, WAVE = 256, 64
F = np.float32


def _group_sum(per_thread):
    """The workgroup's sum of 256 float32 per-thread values: butterfly per wave, then ((w0 + w1) + w2) + w3."""
    v = np.asarray(per_thread, dtype=F).reshape(THREADS // WAVE, WAVE).copy()
    lane = np.arange(WAVE)
    off = WAVE // 2
    while off > 0:
        v = (v + v[:, lane ^ off]).astype(F)
        off //= 2
    w = v[:, 0]
    return F(F(F(w[0] + w[1]) + w[2]) + w[3])


def _serial(x):
    """Per thread the serial float32 sum of x[t], x[t + 256], ... from 0."""
    n = x.shape[0]
    rows = -(-n // THREADS)
    pad = np.zeros(rows * THREADS, dtype=F)
    pad[:n] = x
    s = np.zeros(THREADS, dtype=F)
    for r in pad.reshape(rows, THREADS):           # a padded 0 adds nothing: x + 0 == x, and 0 + 0 == 0
        s = (s + r).astype(F)
    return s


def batch_stats_restated(reward, scale):
    """-> (reward_out float32 [n], mean float32, var float32) with the kernel's bits; n = 1 gives a NaN variance."""
    r = np.asarray(reward, dtype=F).reshape(-1)
    n = r.shape[0]
    out = (r * F(scale)).astype(F)
    mean = F(_group_sum(_serial(out)) / F(n))
    d = (out - mean).astype(F)
    q = _group_sum(_serial((d * d).astype(F)))
    with np.errstate(invalid="ignore", divide="ignore"):
        var = F(q / F(n - 1))
    return out, mean, var


def batch_stats_f64(reward, scale):
    """The float64 yardstick over the float32 product: (mean, unbiased variance; NaN at n = 1)."""
    x = (np.asarray(reward, dtype=F).reshape(-1) * F(scale)).astype(F).astype(np.float64)
    n = x.shape[0]
    mean = x.sum() / n
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.float64(((x - mean) ** 2).sum()) / np.float64(n - 1)
    return mean, var


def bars(reward, scale):
    """Worst-case summation bounds of the fixed order over n elements (no measurement enters): mean (n + 2) 2^-24 mean|x|, variance
    (n + 8) 2^-23 var64 + 2 (mean bar)^2."""
    x = (np.asarray(reward, dtype=F).reshape(-1) * F(scale)).astype(F).astype(np.float64)
    n = x.shape[0]
    mean_bar = (n + 2) * 2.0 ** -24 * np.abs(x).mean()
    _, var64 = batch_stats_f64(reward, scale)
    return mean_bar, (n + 8) * 2.0 ** -23 * var64 + 2 * mean_bar ** 2
