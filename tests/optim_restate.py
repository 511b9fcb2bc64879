"""The float64 yardstick of every optimizer kernel of the TD3 update -- the table optimizer (csrc/train_gemm.hip k_opt_*, td3.clip_and_step,
td3.soft_update_network: tests/test_table_optim_gpu.py) and the MLP agent's (csrc/mlp_optim.hip, mlp_hip.HipMlpOptim:
tests/test_mlp_optim_gpu.py through tests/mlp_optim_restate.py) -- and the inputs they are tested on.  NumPy only; held to
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64 by tests/test_table_optim.py.

One step over a list of tensors, each with a step count of its own:
    total = sum of g^2 over every tensor that has a gradient;  coef = max_norm / (sqrt(total) + 1e-6), 1 where that is > 1
    (torch.clamp(coef, max=1.0): a NaN total gives a NaN coef and with it NaN in every gradient; an infinite total gives coef = 0)
    g := g coef;  t := t + 1;  m := b1 m + (1 - b1) g;  v := b2 v + (1 - b2) g g
    p := p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps);  target := target (1 - tau) + tau p
A tensor whose gradient is None takes no part: not in the total, nothing of it moves, its count stays behind."""
import numpy as np

CHUNK = 1024                      # kOptChunk of csrc/train_gemm.hip (sgrl_optim_chunk), kChunk of csrc/mlp_optim.hip
EPS = 1e-8


def clip_coef(g, max_norm):
    """The factor clip_grad_norm_ multiplies every gradient by (None entries skipped); None for max_norm <= 0."""
    if not max_norm > 0:
        return None
    with np.errstate(all="ignore"):
        total = sum(float((x * x).sum()) for x in g if x is not None)
        coef = np.float64(max_norm) / (np.sqrt(np.float64(total)) + 1e-6)
    return np.float64(1.0) if coef > 1.0 else coef              # a NaN compares false and stays


def step_restated(p, g, m, v, t, lr, beta1, beta2, eps, max_norm, tau, target=None):
    """One step over lists of arrays, in float64.  t: the step counts BEFORE the step, one int per tensor (or one int for all);
    g[i] may be None.  Returns (p, g, m, v, t, target, step): g clipped when max_norm > 0 (else as given), t a list, target moved
    when tau > 0 (else as given, None when none was passed), step[i] = p_new[i] - p_old[i]."""
    n = len(p)
    p, m, v = ([np.asarray(x, dtype=np.float64) for x in xs] for xs in (p, m, v))
    g = [None if x is None else np.asarray(x, dtype=np.float64) for x in g]
    t = [int(t)] * n if np.isscalar(t) else [int(x) for x in t]
    coef = clip_coef(g, max_norm)
    p_new, m_new, v_new, t_new = [], [], [], []
    with np.errstate(all="ignore"):
        if coef is not None:
            g = [None if x is None else x * coef for x in g]
        for i in range(n):
            if g[i] is None:
                p_new.append(p[i]); m_new.append(m[i]); v_new.append(v[i]); t_new.append(t[i])
                continue
            ti = t[i] + 1
            mi = beta1 * m[i] + (1 - beta1) * g[i]
            vi = beta2 * v[i] + (1 - beta2) * g[i] * g[i]
            step_size = lr / (1 - beta1 ** ti)
            bc2_sqrt = np.sqrt(1 - beta2 ** ti)
            p_new.append(p[i] - step_size * mi / (np.sqrt(vi) / bc2_sqrt + eps))
            m_new.append(mi); v_new.append(vi); t_new.append(ti)
        step = [a - b for a, b in zip(p_new, p)]
        if target is not None:
            target = [np.asarray(x, dtype=np.float64) for x in target]
            if tau > 0:
                target = [x * (1 - tau) + tau * w for x, w in zip(target, p_new)]
    return p_new, g, m_new, v_new, t_new, target, step


def lerp_restated(dst, src, tau):
    """The soft target update (reference common/functional.py:7-10) in float64."""
    return [np.asarray(d, dtype=np.float64) * (1 - tau) + tau * np.asarray(s, dtype=np.float64) for d, s in zip(dst, src)]


def eps_share(v, t, beta2=0.999, eps=EPS):
    """The share of elements whose sqrt(v_hat) = sqrt(v / (1 - b2^t)) lies below eps: there Adam's step is lr m_hat / eps, not
    lr sign(g).  v: a list of arrays, t: a count per tensor (AFTER the step that wrote v)."""
    below = sum(int((np.sqrt(np.asarray(x, dtype=np.float64) / (1 - beta2 ** ti)) < eps).sum()) for x, ti in zip(v, t))
    return below / float(sum(np.asarray(x).size for x in v))


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
BIG = (300, 1024)                 # 300 chunks: more partials than k_opt_total has threads, its strided sum and its tree both run
SPECIAL = {0: (1,), 3: (1023,), 40: (1024,), 120: (3, 3, 3), 200: BIG, 255: (30, 128), 256: (1025,), 257: (1,), 290: (2049,)}
N_TENSORS = 300                   # row indices pass 256, the stride of k_opt_total's counter loop


def table_shapes():
    """About 300 tensors: the edges of the 1024-element chunk cut (1, 1023, 1024, 1025, 2049), (3, 3, 3), (30, 128), one tensor of
    300 chunks, the rest 1 to 7 elements; rows 256, 257 and 290 hold a two-chunk, a one-element and a three-chunk tensor."""
    return [SPECIAL.get(i, (1 + (5 * i + i // 7) % 7,)) for i in range(N_TENSORS)]


def sizes_of(shapes):
    return [int(np.prod(s)) for s in shapes]


def tensor_scales(kind, shapes, seed=0):
    """One gradient scale per tensor.  'unit': 1; 'tiny': 1e-11; 'mixed': 10^U(-13, -2), the ends 1e-13 and 1e-2 present, the
    300-chunk tensor at 1e-3 (so that the total norm lies between the two max_norm of the mixed regimes)."""
    n = len(shapes)
    if kind == "unit":
        return np.ones(n)
    if kind == "tiny":
        return np.full(n, 1e-11)
    assert kind == "mixed", kind
    s = 10.0 ** np.random.default_rng(1000 + seed).uniform(-13.0, -2.0, n)
    s[1], s[2] = 1e-13, 1e-2
    for i, shape in enumerate(shapes):
        if shape == BIG:
            s[i] = 1e-3
    return s


def draw_gradients(shapes, scales, seed):
    """Per tensor sign * scale * 2^U(-1, 1) as float32 arrays: every magnitude of a tensor within [scale / 2, 2 scale], so a
    per-tensor max-norm bar binds every element and nothing sits at a zero crossing.  scale >= 1e-13 keeps (1 - b2) g^2 a normal
    float32."""
    assert min(scales) >= 1e-13
    rng = np.random.default_rng(seed)
    out = []
    for shape, s in zip(shapes, scales):
        sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
        out.append((sign * s * 2.0 ** rng.uniform(-1.0, 1.0, shape)).astype(np.float32))
    return out


def with_total_norm(grads, norm):
    """The same gradients scaled by one factor so that their 2-norm over all tensors is `norm` (up to float32 rounding of the
    elements: 6e-8 relative)."""
    total = np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in grads))
    return [(x.astype(np.float64) * (norm / total)).astype(np.float32) for x in grads]


def total_norm(grads):
    return float(np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in grads if x is not None)))


MAX_NORM = 0.1                    # the reference's grad_clipping_value
STEPS = 5
# regime -> (scale kind, max_norm, the total norm the gradients are scaled to or None, whether the clip binds)
REGIMES = {
    "unit-clip": ("unit", MAX_NORM, None, True),
    "tiny-eps": ("tiny", MAX_NORM, None, False),
    "mixed-clip": ("mixed", MAX_NORM, None, True),
    "mixed-noclip": ("mixed", 10.0, None, False),
    "mixed-maxnorm0": ("mixed", 0.0, None, False),
    "just-under": ("unit", MAX_NORM, MAX_NORM * (1 - 1e-4), False),
    "just-over": ("unit", MAX_NORM, MAX_NORM * (1 + 1e-4), True),
}


def regime_gradients(name, shapes, steps=STEPS):
    """-> (max_norm, [gradients of step k]) of a regime of REGIMES; a fixed function of (name, shapes)."""
    kind, max_norm, norm, _ = REGIMES[name]
    scales = tensor_scales(kind, shapes)
    seed0 = 17 * sorted(REGIMES).index(name)
    gs = [draw_gradients(shapes, scales, seed0 + k) for k in range(steps)]
    if norm is not None:
        gs = [with_total_norm(g, norm) for g in gs]
    return max_norm, gs


def start_parameters(shapes, zero, seed=5):
    """Parameters as float32 arrays: zeros (they resolve any step: every bias the reference zero-initialises) or randn."""
    rng = np.random.default_rng(seed)
    return [np.zeros(s, dtype=np.float32) if zero else rng.standard_normal(s).astype(np.float32) for s in shapes]


MIXED_COUNTS = (0, 1, 1000, 100000)


def mixed_count_state(shapes, scales, seed=9):
    """Adam state with the counts 0, 1, 1000, 100000 dealt round the table (rows 256 and up hold all four), m and v at the
    tensors' own gradient scales: count 0 has m = v = 0, the others m = 0.3 scale * (+-2^U(-1, 1)), v = (scale 2^U(-1, 1))^2 / 4."""
    rng = np.random.default_rng(seed)
    counts = [MIXED_COUNTS[(i + i // 4) % 4] for i in range(len(shapes))]
    m, v = [], []
    for shape, s, c in zip(shapes, scales, counts):
        sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
        mm = (0.3 * sign * s * 2.0 ** rng.uniform(-1.0, 1.0, shape)).astype(np.float32)
        vv = (0.25 * (s * 2.0 ** rng.uniform(-1.0, 1.0, shape)) ** 2).astype(np.float32)
        m.append(mm * (c > 0))
        v.append(vv * (c > 0))
    return counts, m, v
