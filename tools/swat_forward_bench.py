#!/usr/bin/env python3
"""Timing of the batched HIP SWAT actor forward (sgrl_amd/swat_hip.py) against the PyTorch path it replaces.

usage: swat_forward_bench.py [config3|config5] [reps=60]
  config3  3D_Walker++: the 8 walker variants x 1024 environments
  config5  one GPU's share of 3D_CWHH++: the 23 training morphologies, 8188 environments
Prints one JSON line: HIP forward ms (device events around each forward, 10 untimed forwards first, median of `reps`), the
same for the PyTorch path (per morphology: change_morphology + StructurePolicy.forward under no_grad, the whole batch per
sample), FLOP per forward, launches per forward and the largest |HIP - PyTorch| over the batch.  Default-initialised weights,
observations ~ N(0, 1).
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from sgrl_amd import graph as G, mjcf
from sgrl_amd.set_policy import default_args
from sgrl_amd.swat_hip import HipSwatActor
from sgrl_amd.swat_policy import StructurePolicy

HELD = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
        "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}


def workload(which):
    if which == "config3":
        names = sorted(n for n in mjcf.list_assets() if n.split("_")[1] == "walker")
        return names, [1024] * len(names)
    names = sorted(n for n in mjcf.list_assets() if n not in HELD)
    return names, [8188 // len(names)] * len(names)


def flop(Ls, counts):
    """Multiply-adds x 2 of one forward: encoder, 3 x (in_proj, q k^T, w v, out_proj, linear1, linear2), decoder."""
    E, FF, F, O = 128, 256, 41, 3
    per_node = 2 * F * E + 3 * 2 * (E * 3 * E + E * E + E * FF + FF * E) + 2 * E * O
    total = 0
    for L, c in zip(Ls, counts):
        total += c * L * (per_node + 3 * 2 * (2 * L * E))
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
    pol = StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False, default_args(), device=dev).eval()
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
    actor = HipSwatActor(pol)
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
    fl = flop(Ls, counts)
    res = {"workload": which, "morphologies": len(names), "envs": n_env, "nodes": int(sum(L * c for L, c in zip(Ls, counts))),
           "hip_forward_ms_median": round(hip_ms, 4), "hip_forward_ms_min": round(hip_min, 4),
           "torch_forward_ms_median": round(torch_ms, 4), "torch_forward_ms_min": round(torch_min, 4),
           "speedup": round(torch_ms / hip_ms, 2), "flop_per_forward": fl, "hip_tflops": round(fl / hip_ms / 1e9, 2),
           "launches_per_forward": actor.launches(), "max_abs_diff_vs_torch": float((out - ref).abs().max()), "reps": reps,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
