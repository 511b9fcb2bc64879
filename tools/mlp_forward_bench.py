#!/usr/bin/env python3
"""Timing of the fused HIP MLP actor forward (sgrl_amd/mlp_hip.py) against the PyTorch module on the same rows, and of a
collection step (engine step + actor forward) with the MLP actor next to the SET actor.

usage: mlp_forward_bench.py [envs=8192] [reps=50] [out.json]
One process, one morphology (3d_walker_7_full), hidden widths [256, 256], seeded weights, observations ~ N(0, 1) for the forward
timings (the same buffer every repetition: caches hot, weights held = packed once) and the engine's own observations for the
collection step.  Device events around each repetition, 10 untimed repetitions first, median of `reps` (>= 50).  Prints one JSON
line and, with a third argument, writes it there."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from mlp_restate import apply_seeded_
from sgrl_amd import graph as G, mjcf
from sgrl_amd.mlp_hip import HipMlpActor
from sgrl_amd.mlp_policy import MlpPolicy
from sgrl_amd.rollout import Rollout
from sgrl_amd.set_policy import make_policy
from sgrl_amd.td3 import default_train_args

NAME = "3d_walker_7_full"


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "p90_ms": round(float(np.percentile(ms, 90)), 4)}


def collection(policy, n, reps):
    ro = Rollout([NAME], n, policy=policy, seed=3, device="cuda:0", hold_weights=True)
    ro.reset()

    def step():
        ro.step(ro.policy_forward())
    both = timed(step, reps)
    fwd = timed(lambda: ro.policy_forward(), reps)
    return {"step_plus_forward": both, "forward_alone": fwd, "launches_per_forward": ro.actor.launches() if hasattr(ro.actor, "launches") else None}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    reps = max(50, int(sys.argv[2]) if len(sys.argv) > 2 else 50)
    dev = torch.device("cuda:0")
    L = mjcf.load_asset(NAME).num_limbs
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L)
    pol = apply_seeded_(MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, args).eval(), 5).to(dev)
    g = G.getGraphDict(mjcf.load_asset(NAME).parents, ["pre", "inlcrs", "postlcrs"], [], device=dev)
    obs = torch.randn((n, 41 * L), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    actor = HipMlpActor(pol)
    actor.configure([g], [n])
    out = torch.zeros((n, 3 * L), device=dev)
    actor.hold_weights(True)
    hip_held = timed(lambda: actor.forward_batch(obs, out=out), reps)
    actor.hold_weights(False)
    hip_packing = timed(lambda: actor.forward_batch(obs, out=out), reps)
    with torch.no_grad():
        torch_eager = timed(lambda: pol(obs), reps)
        ref = pol(obs)
    actor.forward_batch(obs, out=out)
    torch.cuda.synchronize()
    dims = actor.dims
    flop = 2 * n * sum(a * b for a, b in zip(dims[:-1], dims[1:]))
    res = {"workload": "%d x %s, hidden %s" % (n, NAME, dims[1:-1]), "envs": n, "reps": reps, "untimed_first": 10,
           "timing": "device events around each repetition, one process, same buffers every repetition (hot caches)",
           "hip_forward_weights_held": hip_held, "hip_forward_packing_every_call": hip_packing, "torch_module_forward": torch_eager,
           "speedup_vs_torch_median": round(torch_eager["median_ms"] / hip_held["median_ms"], 2),
           "flop_per_forward": flop, "hip_tflops": round(flop / hip_held["median_ms"] / 1e9, 2),
           "launches_per_forward": actor.launches(), "plan": actor.plan(), "max_abs_diff_vs_torch": float((out - ref).abs().max()),
           "collection_step_mlp": collection(pol, n, reps), "collection_step_set": collection(make_policy(device="cuda:0").eval(), n, reps),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line, flush=True)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
