"""Shared by the MLP tests and tools/capture_golden_mlp.py: seed-generated weights (the fixtures store seeds, not 1.7 MB of random
numbers), a float64 restatement of the MLP forward and a NumPy restatement of the library's padding plan."""
import zlib

import numpy as np


def seeded_values(name, shape, fan_in, seed):
    """U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) float32 -- nn.Linear's default rule -- from (name, seed) alone."""
    rng = np.random.RandomState((zlib.crc32(name.encode("utf-8")) + 7919 * int(seed)) % (2 ** 32))
    bound = 1.0 / np.sqrt(float(fan_in))
    return rng.uniform(-bound, bound, size=shape).astype(np.float32)


def apply_seeded_(module, seed, scale=1.0):
    """Overwrite every PARAMETER of `module` (an MlpPolicy / MlpCritic of either side; buffers are left alone) with seeded_values;
    a bias takes its weight's fan-in.  Full-rank random matrices."""
    import torch
    params = dict(module.named_parameters())
    with torch.no_grad():
        for name, p in params.items():
            w = params[name[:-len("bias")] + "weight"] if name.endswith(".bias") else p
            p.copy_(torch.from_numpy(scale * seeded_values(name, tuple(p.shape), int(w.shape[1]), seed)).to(p.dtype))
    return module


def forward64(linears, x, max_action=None):
    """float64 forward of a Linear / ReLU stack given [(weight, bias), ...] as arrays; max_action: the actor's tanh head."""
    h = np.asarray(x, dtype=np.float64)
    for i, (w, b) in enumerate(linears):
        h = h @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if i + 1 < len(linears):
            h = np.maximum(h, 0.0)
    return h if max_action is None else float(max_action) * np.tanh(h)


def module_linears(net):
    """[(weight, bias)] float64 arrays of an MLP stack (`networks` Sequential)."""
    import torch
    return [(m.weight.detach().double().cpu().numpy(), m.bias.detach().double().cpu().numpy())
            for m in net.networks if isinstance(m, torch.nn.Linear)]


def plan_restated(dims, n_env=None, tile_rows=32, lds_limit=160 * 1024):
    """include/sgrl_mlp.h sgrl_mlp_plan, restated: input rounded up to 16, outputs to 32, a layer's padded output is the next one's
    padded input; weights first, then biases; 1, 2 or 4 chunks of 256 columns; weight panels 16 deep unless LDS only has room for 8."""
    up = lambda x, m: (x + m - 1) // m * m
    nl = len(dims) - 1
    kpad, npad = [], []
    for l in range(nl):
        kpad.append(up(dims[0], 16) if l == 0 else npad[l - 1])
        npad.append(up(dims[l + 1], 32))
    sizes = [n * k for n, k in zip(npad, kpad)]
    w_off = [int(sum(sizes[:l])) for l in range(nl)]
    b_off = [int(sum(sizes) + sum(npad[:l])) for l in range(nl)]
    chunks = -(-max(npad) // 256)
    chunks = 1 if chunks <= 1 else (2 if chunks == 2 else 4)
    sx = max(kpad) + 4
    lds = lambda bk: 4 * (tile_rows * sx + 2 * 256 * (bk + 4))
    bk = 16 if lds(16) <= lds_limit else 8
    out = {"kpad": kpad, "npad": npad, "w_off": w_off, "b_off": b_off, "total": int(sum(sizes) + sum(npad)), "chunks": chunks, "bk": bk,
           "lds_bytes": lds(bk), "sx": sx, "tile_rows": tile_rows}
    if n_env is not None:
        out["tiles"] = -(-int(n_env) // tile_rows)
    return out
