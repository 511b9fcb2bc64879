"""sgrl_explore_actions (include/sgrl_explore.h) restated in NumPy, on the Philox restatement of tests/test_replay_sample.py: the
same block layout as the replay's target-policy noise, stream tags 2 (exploration) and 3 (warm-up).  float64 for u, z and the
uniform's u1; float32 for the add, the clamp and the affine map, one rounding per operation, in the header's order.  Not a test."""
import numpy as np

from tests.test_replay_sample import stream_words

GAUSS, UNIFORM = 0, 1
TAG = {GAUSS: 2, UNIFORM: 3}


def element_words(n_env, act_max, env_id_base, seed, step, tag):
    """[n_env, act_max, 2] uint32: element e = (env_id_base + i) * act_max + c takes words 2 e and 2 e + 1 of stream `tag`."""
    e0 = int(env_id_base) * int(act_max)
    return stream_words(seed, step, tag, 2 * e0, 2 * n_env * act_max).reshape(n_env, act_max, 2)


def explore_actions(policy, act_len, act_max, env_id_base, seed, step, mode, std, lo, hi):
    """[n_env, act_max] float32.  policy: [n_env, >= act_max] (ignored, may be None, in UNIFORM mode); act_len: [n_env] live slots."""
    act_len = np.asarray(act_len, dtype=np.int64)
    n = act_len.size
    f32 = np.float32
    u = (element_words(n, act_max, env_id_base, seed, step, TAG[mode]).astype(np.float64) + 0.5) / 4294967296.0
    if mode == GAUSS:
        z = np.sqrt(-2.0 * np.log(u[:, :, 0])) * np.cos(2.0 * np.pi * u[:, :, 1])
        p = np.asarray(policy)[:, :act_max].astype(f32)
        out = np.minimum(np.maximum(p + z.astype(f32) * f32(std), f32(lo)), f32(hi))
    else:
        out = f32(lo) + (f32(hi) - f32(lo)) * u[:, :, 0].astype(f32)
    assert out.dtype == f32
    out[np.arange(act_max)[None, :] >= act_len[:, None]] = 0.0
    return out
