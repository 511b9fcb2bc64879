#!/usr/bin/env python3
"""Timing of the HIP SMP twin critic forward and of an eager TD3 update of an SMP agent with / without the HIP target chain and
with its differentiable passes on the training kernels.

usage: smp_update_bench.py forward [config3|config5] [reps=60]
       smp_update_bench.py update [morphology=3d_walker_7_full] [hip|pytorch|auto|kernels|graphed] [updates=40]
  forward  twin critic forward (smp_hip.HipSmpCritic, both heads, max_children 5) over the 8 walker variants x 1024 environments
           (config3) or one GPU's share of 3D_CWHH++ (config5: 23 morphologies, 8188 environments), against the PyTorch path
           (per morphology: change_morphology + CriticGraphPolicy.forward under no_grad).  Device events around each forward,
           10 untimed forwards first, median of `reps`.
  update   one eager Agent.update (td3.py) of an SMP agent (td and bu, max_children 5) at batch 256 on one morphology: 8 untimed
           updates, then `updates` timed ones (host clock around update + device synchronisation; every second update includes
           the delayed actor step, as in training).  `hip`: the target chain on HIP (Agent(use_hip=True)); `pytorch`:
           Agent(use_hip=False); `auto`: the build's default; `kernels`: the HIP target chain AND the differentiable passes on the
           training kernels (Agent(smp_train_kernels=True)); `graphed`: that agent with the loss kernels as well (loss_kernels=True),
           its updates replayed from hipGraphs (td3.GraphedUpdates(hip_kernels=True): two eager warm-up updates, the captures fall
           among the untimed ones; the timed call includes filling the slot's static batch and noise).  The pytorch / auto arms use
           no API newer than Agent.update, so this mode also runs on a checkout that has no HIP target chain
           (SGRL_BENCH_TREE=<checkout> times its package).
Prints one JSON line per run.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SGRL_BENCH_TREE", REPO))       # A/B: time the package of another checkout with this script
import numpy as np
import torch

from sgrl_amd import graph as G, mjcf

HELD = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
        "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}
TRAV = ["pre", "inlcrs", "postlcrs"]
MC = 5


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


def forward(which, reps):
    from sgrl_amd.smp_hip import HipSmpCritic
    from sgrl_amd.smp_policy import CriticGraphPolicy
    if which == "config3":
        names = sorted(n for n in mjcf.list_assets() if n.split("_")[1] == "walker")
        counts = [1024] * len(names)
    else:
        names = sorted(n for n in mjcf.list_assets() if n not in HELD)
        counts = [8188 // len(names)] * len(names)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    crit = CriticGraphPolicy(41, 3, 32, 1, MC, True, True, True, None, device=dev).eval()
    graphs = [G.getGraphDict(mjcf.load_asset(n).parents, TRAV, [], device=dev) for n in names]
    Ls = [len(g["parents"]) for g in graphs]
    Lmax, n_env = max(Ls), int(sum(counts))
    gen = torch.Generator(device=dev).manual_seed(1)
    obs = torch.zeros((n_env, 41 * Lmax), dtype=torch.float32, device=dev)
    act = torch.zeros((n_env, 3 * Lmax), dtype=torch.float32, device=dev)
    blocks, row = [], 0
    for L, c in zip(Ls, counts):
        obs[row:row + c, :41 * L] = torch.randn((c, 41 * L), device=dev, generator=gen)
        act[row:row + c, :3 * L] = torch.rand((c, 3 * L), device=dev, generator=gen) * 2 - 1
        blocks.append((row, c, L))
        row += c
    hip = HipSmpCritic(crit)
    hip.configure(graphs, counts)
    got = [None]

    def hip_path():
        got[0] = hip.forward_q(obs, act)
    twin_ms, twin_min = timed(hip_path, reps)
    single_ms, _ = timed(lambda: hip.forward_q(obs, act, twin=False), reps)
    ref = torch.zeros((2, n_env, 1), dtype=torch.float32, device=dev)

    def torch_path():
        with torch.no_grad():
            for g, (r, c, L) in zip(graphs, blocks):
                crit.change_morphology(g)
                q1, q2 = crit(obs[r:r + c, :41 * L], act[r:r + c, :3 * L])
                ref[0, r:r + c], ref[1, r:r + c] = q1, q2
    torch_ms, torch_min = timed(torch_path, reps)
    hip_path()
    torch_path()
    torch.cuda.synchronize()
    diff = max(float((got[0][k] - ref[k]).abs().max()) for k in range(2))
    print(json.dumps({"mode": "forward", "workload": which, "morphologies": len(names), "envs": n_env,
                      "nodes": int(sum(L * c for L, c in zip(Ls, counts))), "tree_levels": hip.num_levels,
                      "hip_twin_ms_median": round(twin_ms, 4), "hip_twin_ms_min": round(twin_min, 4),
                      "hip_q1_only_ms_median": round(single_ms, 4),
                      "torch_twin_ms_median": round(torch_ms, 4), "torch_twin_ms_min": round(torch_min, 4),
                      "speedup": round(torch_ms / twin_ms, 2), "launches_per_twin_forward": hip.launches(),
                      "max_abs_diff_vs_torch": diff, "reps": reps, "device": torch.cuda.get_device_name(0)}), flush=True)


def update(name, arm, updates):
    from sgrl_amd.td3 import Agent, default_train_args
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    args = default_train_args(actor_type="smp", critic_type="smp", td=True, bu=True, max_children=MC)
    if arm == "kernels":
        agent = Agent(args, device=dev, smp_train_kernels=True)
    elif arm == "graphed":
        agent = Agent(args, device=dev, smp_train_kernels=True, loss_kernels=True)
    else:
        agent = Agent(args, device=dev) if arm == "auto" else Agent(args, device=dev, use_hip=(arm == "hip"))
    g = G.getGraphDict(mjcf.load_asset(name).parents, TRAV, [], device=dev)
    L, B = len(g["parents"]), 256
    agent.change_morphology(g)
    agent.models2train()
    gen = torch.Generator(device=dev).manual_seed(1)
    batches = []
    for _ in range(4):
        r = lambda *s: torch.rand(s, device=dev, generator=gen)
        batches.append({"obs": torch.randn((B, 41 * L), device=dev, generator=gen), "next_obs": torch.randn((B, 41 * L), device=dev, generator=gen),
                        "action": r(B, 3 * L) * 2 - 1, "reward": r(B, 1) * 2 - 1, "done": (r(B, 1) < 0.05).float()})
    step = lambda it: agent.update(batches[it % 4], it, lazy_stats=True)
    first = 0
    if arm == "graphed":
        from sgrl_amd.td3 import GraphedUpdates
        gu = GraphedUpdates(agent, B, hip_kernels=True)
        gu.warm(0, g, L, lambda: batches[0], iters=2)
        step, first = (lambda it: gu.update(0, g, L, batches[it % 4], it)), 2
    loss = None
    for it in range(first, 8):
        loss = step(it)
    torch.cuda.synchronize()
    ms = []
    for it in range(8, 8 + updates):
        t0 = time.perf_counter()
        loss = step(it)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.asarray(ms)
    print(json.dumps({"mode": "update", "morphology": name, "limbs": L, "batch": B, "arm": arm,
                      "tree": os.environ.get("SGRL_BENCH_TREE", "this"),
                      "hip_target_chain": getattr(agent, "_targets", None) is not None,
                      "train_kernels": bool(getattr(agent, "use_smp_train_kernels", False)),
                      "update_ms_mean": round(float(ms.mean()), 4), "update_ms_median": round(float(np.median(ms)), 4),
                      "update_ms_min": round(float(ms.min()), 4), "update_ms_max": round(float(ms.max()), 4),
                      "critic_only_ms_median": round(float(np.median(ms[1::2])), 4),
                      "with_actor_ms_median": round(float(np.median(ms[0::2])), 4), "updates": int(updates),
                      "critic_loss": float(loss["loss/critic_loss"]), "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "forward"
    if mode == "forward":
        forward(sys.argv[2] if len(sys.argv) > 2 else "config3", max(50, int(sys.argv[3]) if len(sys.argv) > 3 else 60))
    elif mode == "update":
        update(sys.argv[2] if len(sys.argv) > 2 else "3d_walker_7_full", sys.argv[3] if len(sys.argv) > 3 else "auto",
               int(sys.argv[4]) if len(sys.argv) > 4 else 40)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
