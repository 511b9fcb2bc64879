"""NumPy restatements for the optimizer half of the MLP agent's TD3 update (include/sgrl_mlp.h "optimizer half"): how a handle's
tensors are cut into chunks (sgrl_mlp_optim_plan), and one step -- gradient clipping, Adam and the soft target update -- in
float64, the yardstick of tests/test_mlp_optim_gpu.py (held to torch.optim.Adam + clip_grad_norm_ + the reference's Polyak loop by
tests/test_mlp_optim_plan.py)."""
import numpy as np

CHUNK = 1024


def optim_plan_restated(dims, n_stacks):
    """Per stack W_l [dims[l + 1], dims[l]] and b_l [dims[l + 1]]; a tensor of n elements is ceil(n / CHUNK) chunks."""
    sizes = [n for _ in range(n_stacks) for k, o in zip(dims[:-1], dims[1:]) for n in (o * k, o)]
    return {"tensors": len(sizes), "elements": sum(sizes), "chunks": sum(-(-n // CHUNK) for n in sizes), "chunk": CHUNK}


def step_restated(p, g, m, v, t, lr, beta1, beta2, eps, max_norm, tau, target=None):
    """One step over lists of float64 arrays; t: the step count BEFORE the step.  Returns (p, g, m, v, t + 1, target): g clipped
    when max_norm > 0 (else as given), target moved when tau > 0 (else as given)."""
    p, g, m, v = ([np.asarray(x, dtype=np.float64) for x in xs] for xs in (p, g, m, v))
    if max_norm > 0:
        total = sum(float((x * x).sum()) for x in g)
        coef = min(1.0, max_norm / (np.sqrt(total) + 1e-6))
        g = [x * coef for x in g]
    t = t + 1
    m = [beta1 * a + (1 - beta1) * x for a, x in zip(m, g)]
    v = [beta2 * a + (1 - beta2) * x * x for a, x in zip(v, g)]
    step_size = lr / (1 - beta1 ** t)
    bc2_sqrt = np.sqrt(1 - beta2 ** t)
    p = [w - step_size * a / (np.sqrt(b) / bc2_sqrt + eps) for w, a, b in zip(p, m, v)]
    if target is not None:
        target = [np.asarray(x, dtype=np.float64) for x in target]
        if tau > 0:
            target = [x * (1 - tau) + tau * w for x, w in zip(target, p)]
    return p, g, m, v, t, target
