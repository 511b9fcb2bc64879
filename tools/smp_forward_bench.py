#!/usr/bin/env python3
"""Timing of the batched HIP SMP actor forward (sgrl_amd/smp_hip.py) against the PyTorch path it replaces.

usage: smp_forward_bench.py [config3|config5] [reps=60]
  config3  3D_Walker++: the 8 walker variants x 1024 environments
  config5  one GPU's share of 3D_CWHH++: the 23 training morphologies, 8188 environments
Prints one JSON line: HIP forward ms (device events around each forward, 10 untimed forwards first, median of `reps`), the
same for the PyTorch path (per morphology: change_morphology + ActorGraphPolicy.forward under no_grad, the whole batch per
sample), FLOP per forward, launches and tree levels per forward and the largest |HIP - PyTorch| over the batch.
Default-initialised weights (td and bu, max_children 5: the cheetahs need it), observations ~ N(0, 1).
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from sgrl_amd import graph as G, mjcf
from sgrl_amd.smp_hip import HipSmpActor
from sgrl_amd.smp_policy import ActorGraphPolicy

MAX_CHILDREN = 5

HELD = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
        "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}


def workload(which):
    if which == "config3":
        names = sorted(n for n in mjcf.list_assets() if n.split("_")[1] == "walker")
        return names, [1024] * len(names)
    names = sorted(n for n in mjcf.list_assets() if n not in HELD)
    return names, [8188 // len(names)] * len(names)


def flop(graphs, counts, mc=MAX_CHILDREN):
    """Multiply-adds x 2 of one forward as the HIP path computes it: fc1, fc2, fc3 and action_base for every node, msg_base for
    the limbs that have children (a leaf's outgoing message is never read)."""
    F, O, K1, MC = 41, 3, 64 + 32 * mc, 32 * mc
    node = 2 * (F * 64 + K1 * 64 + 64 * 32) + 2 * (64 * 400 + 400 * 300 + 300 * O)
    msg = 2 * (64 * 400 + 400 * 300 + 300 * MC)
    total = 0
    for g, c in zip(graphs, counts):
        parents = [int(p) for p in g["parents"]]
        inner = sum(1 for i in range(len(parents)) if i in parents)
        total += c * (len(parents) * node + inner * msg)
    return total


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
    return float(np.median(ms)), float(np.min(ms))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "config3"
    reps = max(50, int(sys.argv[2]) if len(sys.argv) > 2 else 60)
    names, counts = workload(which)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pol = ActorGraphPolicy(41, 3, 32, 1, 1.0, MAX_CHILDREN, True, True, True, None, device=dev).eval()
    graphs = [G.getGraphDict(mjcf.load_asset(n).parents, ["pre", "inlcrs", "postlcrs"], [], device=dev) for n in names]
    Ls = [len(g["parents"]) for g in graphs]
    Lmax = max(Ls)
    n_env = int(sum(counts))
    gen = torch.Generator(device=dev).manual_seed(1)
    obs = torch.zeros((n_env, 41 * Lmax), dtype=torch.float32, device=dev)
    blocks, row = [], 0
    for L, c in zip(Ls, counts):
        obs[row:row + c, :41 * L] = torch.randn((c, 41 * L), device=dev, generator=gen)
        blocks.append((row, c, L))
        row += c
    actor = HipSmpActor(pol)
    actor.configure(graphs, counts)
    out = torch.zeros((n_env, 3 * Lmax), dtype=torch.float32, device=dev)
    hip_ms, hip_min = timed(lambda: actor.forward_batch(obs, out=out), reps)
    ref = torch.zeros_like(out)

    def torch_path():
        with torch.no_grad():
            for g, (r, c, L) in zip(graphs, blocks):
                pol.change_morphology(g)
                ref[r:r + c, :3 * L] = pol(obs[r:r + c, :41 * L])
    torch_ms, torch_min = timed(torch_path, reps)
    actor.forward_batch(obs, out=out)
    torch_path()
    torch.cuda.synchronize()
    fl = flop(graphs, counts)
    res = {"workload": which, "morphologies": len(names), "envs": n_env, "nodes": int(sum(L * c for L, c in zip(Ls, counts))),
           "hip_forward_ms_median": round(hip_ms, 4), "hip_forward_ms_min": round(hip_min, 4),
           "torch_forward_ms_median": round(torch_ms, 4), "torch_forward_ms_min": round(torch_min, 4),
           "speedup": round(torch_ms / hip_ms, 2), "flop_per_forward": fl, "hip_tflops": round(fl / hip_ms / 1e9, 2),
           "launches_per_forward": actor.launches(), "levels_per_forward": actor.num_levels, "max_children": MAX_CHILDREN,
           "max_abs_diff_vs_torch": float((out - ref).abs().max()), "reps": reps,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
