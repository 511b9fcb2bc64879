"""NumPy restatements for the optimizer half of the MLP agent's TD3 update (include/sgrl_mlp.h "optimizer half"): how a handle's
tensors are cut into chunks (sgrl_mlp_optim_plan), and one step -- gradient clipping, Adam and the soft target update -- in
float64, the yardstick of tests/test_mlp_optim_gpu.py (held to torch.optim.Adam + clip_grad_norm_ + the reference's Polyak loop by
tests/test_mlp_optim_plan.py)."""
import numpy as np

import optim_restate

CHUNK = optim_restate.CHUNK


def optim_plan_restated(dims, n_stacks):
    """Per stack W_l [dims[l + 1], dims[l]] and b_l [dims[l + 1]]; a tensor of n elements is ceil(n / CHUNK) chunks."""
    sizes = [n for _ in range(n_stacks) for k, o in zip(dims[:-1], dims[1:]) for n in (o * k, o)]
    return {"tensors": len(sizes), "elements": sum(sizes), "chunks": sum(-(-n // CHUNK) for n in sizes), "chunk": CHUNK}


def step_restated(p, g, m, v, t, lr, beta1, beta2, eps, max_norm, tau, target=None):
    """One step over lists of float64 arrays; t: the step count BEFORE the step, shared by all tensors.  Returns (p, g, m, v, t + 1,
    target): g clipped when max_norm > 0 (else as given), target moved when tau > 0 (else as given).  The arithmetic is
    optim_restate.step_restated's (a NaN total of squares gives NaN gradients, as torch.clamp gives them in clip_grad_norm_)."""
    p, g, m, v, _, target, _ = optim_restate.step_restated(p, g, m, v, int(t), lr, beta1, beta2, eps, max_norm, tau, target)
    return p, g, m, v, t + 1, target
