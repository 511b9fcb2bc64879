"""TEST INFRASTRUCTURE (oracle/): closed-form parameter values for the SET actor.

Golden SET-forward vectors are produced by the *reference* SEPolicy (src/SEActor.py:290-356)
whose parameters were overwritten with these formulas, so that only (inputs, outputs) have to
be committed under tests/golden/ -- not an 18.9 MB weight blob.  The same formulas are applied
to the build's SEPolicy / HIP weight pack in the tests.  Only tests/, __graft_entry__.smoke()
and bench.py's cpu_baseline leg may import anything under oracle/.
"""
import zlib

import numpy as np


# per-parameter gains chosen so that every branch of the network contributes O(0.1..1) to the output
# (with a plain 1/sqrt(fan_in) scale the equivariant stream dwarfs the rest and actions are ~1e-4,
# which would make an absolute-tolerance parity test blind to most of the graph)
_GAINS = (
    ("g_encoder.weight", 0.04),
    ("decoder_g.weight", 6.0),
    ("linear5.weight", 4.0),
    ("g_out.weight", 0.5),
    ("vg_proj.weight", 0.5),
    ("ng_out.weight", 6.0),
    ("linear_g1.weight", 0.5),
    ("linear1_g.weight", 0.5),
)


def _gain(name):
    for suffix, g in _GAINS:
        if name.endswith(suffix):
            return g
    return 1.0


def formula_values(name, shape):
    """Deterministic float64 array for parameter `name` (state_dict key without prefix games)."""
    numel = int(np.prod(shape)) if len(shape) else 1
    i = np.arange(numel, dtype=np.float64)
    h = float(zlib.crc32(name.encode("utf-8")) % 9973)
    v = 0.5 * np.sin(i * 0.7853 + h * 0.37) + 0.5 * np.sin(i * 0.0137 + h)
    if len(shape) == 2:
        if "embeddings" in name:
            out = 0.3 * v
        else:
            fan_in = shape[1]
            out = v * (1.2 / np.sqrt(fan_in)) * _gain(name)
    else:
        if "norm" in name and name.endswith("weight"):
            out = 1.0 + 0.1 * v
        else:
            out = 0.05 * v
    return out.reshape(shape)


def apply_formula_(module, dtype=None):
    """Overwrite every parameter of a torch module in place (module = SEPolicy-like)."""
    import torch
    with torch.no_grad():
        for name, p in module.state_dict().items():
            vals = formula_values(name, tuple(p.shape))
            p.copy_(torch.from_numpy(vals).to(p.dtype if dtype is None else dtype))
    return module


# ---- full-rank weights, regenerated from (name, seed) ------------------------------------------------------------------------
# formula_values is a sum of two sinusoids over the flattened index: every matrix has rank <= 4 and nearly repeats every 8 columns,
# so two exchanged weight columns (a wrong pack permutation, K-slice order or fragment layout) often move no output above the
# parity tolerance.  These values keep formula_values' scales (1/sqrt(fan_in) x _gain, every branch O(0.1..1)) with independent
# standard-normal entries.  qk_gain multiplies q_proj / k_proj: at gain 1 the attention is nearly uniform and the two projections
# are invisible in every output; the effect grows with the square of the gain (tests/test_set_full_rank.py counts it).
QK_GAIN = 40.0


def full_rank_values(name, shape, seed, qk_gain=QK_GAIN):
    """Deterministic float64 array for parameter `name` of weight set `seed`: N(0,1) entries, formula_values' scales."""
    rng = np.random.RandomState((zlib.crc32(name.encode("utf-8")) + 7919 * int(seed)) % (2 ** 32))
    v = rng.standard_normal(size=tuple(shape))
    if len(shape) == 2:
        if "embeddings" in name:
            return 0.3 * v
        gain = qk_gain if name.endswith(("q_proj.weight", "k_proj.weight")) else _gain(name)
        return v * (gain / np.sqrt(shape[1]))
    if "norm" in name and name.endswith("weight"):
        return 1.0 + 0.1 * v
    return 0.05 * v


def apply_full_rank_(module, seed, qk_gain=QK_GAIN):
    """Overwrite every parameter of a torch module in place (an SEPolicy / SECritic, any device or dtype) with full_rank_values."""
    import torch
    with torch.no_grad():
        for name, p in module.state_dict().items():
            p.copy_(torch.from_numpy(full_rank_values(name, tuple(p.shape), seed, qk_gain)).to(p.dtype))
    return module


def synth_obs(num_limbs, batch, seed):
    """Synthetic but plausible per-limb observations (layout of <env>.py:116-140), float64 [B, 41*L]."""
    rng = np.random.RandomState(seed)
    L = num_limbs
    obs = np.zeros((batch, L, 41))
    obs[:, :, 0:3] = rng.uniform(-0.6, 0.6, size=(batch, L, 3))
    obs[:, 0, 0:3] = 0.0
    obs[:, :, 5] = -9.81
    ang = rng.uniform(-np.pi, np.pi, size=(batch, 1))
    obs[:, :, 6] = np.cos(ang)
    obs[:, :, 7] = np.sin(ang)
    obs[:, :, 9:12] = np.clip(rng.normal(0, 2.0, size=(batch, L, 3)), -10, 10)
    obs[:, :, 12:15] = rng.normal(0, 3.0, size=(batch, L, 3))
    for k in range(3):
        ax = rng.normal(size=(batch, L, 3))
        ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
        obs[:, :, 15 + 3 * k:18 + 3 * k] = ax
    obs[:, 0, 15:24] = 0.0
    obs[:, :, 24:27] = rng.uniform(-1.0, 1.0, size=(batch, L, 3))
    obs[:, 0, 24:27] = 0.0
    for k in range(3):
        obs[:, :, 27 + 3 * k] = rng.uniform(-0.1, 1.1, size=(batch, L))
        lo = rng.uniform(0.05, 0.5, size=(batch, L))
        obs[:, :, 28 + 3 * k] = lo
        obs[:, :, 29 + 3 * k] = lo + rng.uniform(0.01, 0.45, size=(batch, L))
    obs[:, 0, 27:36] = 0.5
    types = rng.randint(0, 5, size=(batch, L))
    for t in range(4):
        obs[:, :, 36 + t] = (types == t + 1)
    obs[:, 0, 36:40] = [1, 0, 0, 0]
    obs[:, :, 40] = rng.uniform(0.0, 1.6, size=(batch, L))
    return obs.reshape(batch, L * 41)


def scripted_batch(L, B, seed):
    """A replay batch made from seeds only (tools/capture_golden_update.py feeds it to the reference's Agent.update; the tests
    regenerate it instead of storing a 256-row batch): observations synth_obs(seed) / synth_obs(seed + 1), uniform actions,
    N(1, 0.5) rewards, 30 % done flags.  float32, the dtype the replay buffer hands out."""
    rng = np.random.RandomState(seed)
    return dict(obs=synth_obs(L, B, seed).astype(np.float32), next_obs=synth_obs(L, B, seed + 1).astype(np.float32),
                action=rng.uniform(-1, 1, size=(B, 3 * L)).astype(np.float32),
                reward=rng.normal(1.0, 0.5, size=(B, 1)).astype(np.float32),
                done=(rng.uniform(size=(B, 1)) < 0.3).astype(np.float32))


# ---- default-LIKE initial weights, regenerated from seeds (tests/golden/td3_update_default_init.npz) -------------------------
# The TD3 fixtures above use formula weights (every branch O(0.1..1)).  The regime that decides whether config 5 takes off is the
# reference's DEFAULT initialisation (actor gradients through a critic that does not depend on the action yet).  A default-init
# state_dict is 57 MB, so the fixture stores the per-tensor RULE instead -- checked by tools/capture_golden_update_init.py against
# the reference's own freshly constructed networks (constant tensors equal, bounds never exceeded, spread within sampling error)
# -- and both sides regenerate identical values from (rule, name, seed).  The three encoder layers of the reference are deepcopy
# clones (SEActor.py:14-15): a name's `.layers.N.` is read as `.layers.0.` so that the clones stay identical.
def default_like_rule(name, shape):
    """(kind, value): 'c' constant value, 'n' normal(0, value), 'u' uniform(-value, value) -- torch's default initialisers for the
    module types the SET networks are made of, plus the two explicit U(-0.1, 0.1) of reference SEActor.py:232-235."""
    leaf = name.split(".")[-1]
    mod = name.split(".")[-2] if "." in name else ""
    if "embeddings" in name:
        return "n", 1.0                                           # nn.Embedding
    if mod.startswith("norm") and leaf in ("weight", "bias"):
        return "c", 1.0 if leaf == "weight" else 0.0              # nn.LayerNorm
    if leaf == "in_proj_weight":
        return "u", float(np.sqrt(6.0 / (shape[0] + shape[1])))   # nn.MultiheadAttention: xavier_uniform_
    if leaf == "in_proj_bias" or name.endswith("out_proj.bias"):
        return "c", 0.0
    if name.endswith(("g_encoder.weight", ".encoder.weight")) or name in ("encoder.weight",):
        return "u", 0.1                                           # init_weights(): uniform_(-0.1, 0.1)
    return "u", None                                              # nn.Linear: U(+-1/sqrt(fan_in)); a bias takes its weight's fan_in


def default_like_values(name, shape, seed, fan_in=None):
    kind, val = default_like_rule(name, shape)
    if kind == "c":
        return np.full(shape, val, dtype=np.float32)
    canon = name.replace(".layers.1.", ".layers.0.").replace(".layers.2.", ".layers.0.")
    rng = np.random.RandomState((zlib.crc32(canon.encode("utf-8")) + 7919 * int(seed)) % (2 ** 32))
    if kind == "n":
        return rng.normal(0.0, val, size=shape).astype(np.float32)
    if val is None:
        val = 1.0 / np.sqrt(shape[1] if len(shape) == 2 else fan_in)
    return rng.uniform(-val, val, size=shape).astype(np.float32)


def apply_default_like_(module, seed):
    """Overwrite every parameter of `module` (an SEPolicy / SECritic of either side) with default-like values of `seed`."""
    import torch
    sd = module.state_dict()
    with torch.no_grad():
        for name, p in sd.items():
            fan_in = None
            if p.dim() == 1 and name.endswith(".bias"):
                w = sd.get(name[:-len("bias")] + "weight")
                fan_in = int(w.shape[1]) if w is not None and w.dim() == 2 else None
            p.copy_(torch.from_numpy(default_like_values(name, tuple(p.shape), seed, fan_in)).to(p.dtype))
    return module
