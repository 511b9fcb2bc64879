#!/usr/bin/env python3
"""Timing of the HIP SWAT twin critic forward and of an eager TD3 update of a SWAT agent with / without the HIP target chain.

usage: swat_update_bench.py forward [config3|config5] [reps=60]
       swat_update_bench.py update [morphology=3d_walker_7_full] [hip|pytorch|auto|kernels|graphed] [updates=40] [streams=1] [dropout=0]
  forward  twin critic forward (swat_hip.HipSwatCritic, both networks) over the 8 walker variants x 1024 environments (config3)
           or one GPU's share of 3D_CWHH++ (config5: 23 morphologies, 8188 environments), against the PyTorch path (per
           morphology: change_morphology + CriticStructurePolicy.forward under no_grad).  With two streams and with the second
           chain queued behind the first on one stream (sgrl_swat_debug_twin_streams).  Device events around each forward,
           10 untimed forwards first, median of `reps`.
  update   one eager Agent.update (td3.py) of a SWAT agent at batch 256 on one morphology: 8 untimed updates, then `updates`
           timed ones (host clock around update + device synchronisation; every second update includes the delayed actor
           step, as in training).  `hip`: the target chain on HIP (Agent(use_hip=True)); `pytorch`: Agent(use_hip=False);
           `auto`: the build's default; `kernels`: the HIP target chain AND the differentiable passes on the training kernels
           (Agent(swat_train_kernels=True)); `graphed`: that agent with the loss kernels as well (loss_kernels=True), its updates
           replayed from hipGraphs (td3.GraphedUpdates(hip_kernels=True): two eager warm-up updates, the captures fall among the
           untimed ones; the timed call includes filling the slot's static batch and noise).  The pytorch / auto arms use no API
           newer than Agent.update, so this mode also runs on a checkout that has no HIP target chain.  streams=0: the chain's
           second critic on the caller's stream.  dropout: args.dropout_rate of the agent (eager arms only; with a rate the target
           chain runs the modules).  After the timed updates two more (one without, one with the actor step) run under
           torch.profiler: `launches_per_two_updates` counts their kernel launches (copies and fills excluded; null when the
           profiler is not available).
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
from sgrl_amd.set_policy import default_args

HELD = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
        "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}
TRAV = ["pre", "inlcrs", "postlcrs"]


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
    from sgrl_amd.swat_hip import HipSwatCritic
    from sgrl_amd.swat_policy import CriticStructurePolicy
    if which == "config3":
        names = sorted(n for n in mjcf.list_assets() if n.split("_")[1] == "walker")
        counts = [1024] * len(names)
    else:
        names = sorted(n for n in mjcf.list_assets() if n not in HELD)
        counts = [8188 // len(names)] * len(names)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    crit = CriticStructurePolicy(41, 3, 32, 1, 3, True, False, False, default_args(), device=dev).eval()
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
    hip = HipSwatCritic(crit)
    hip.configure(graphs, counts)
    got = [None]

    def hip_path():
        got[0] = hip.forward_batch(obs, act)
    two_ms, two_min = timed(hip_path, reps)
    hip.L.sgrl_swat_debug_twin_streams(0)
    one_ms, one_min = timed(hip_path, reps)
    hip.L.sgrl_swat_debug_twin_streams(1)
    single_ms, _ = timed(lambda: hip.forward_batch(obs, act, which=(1,)), reps)
    ref = torch.zeros((2, n_env, Lmax), dtype=torch.float32, device=dev)

    def torch_path():
        with torch.no_grad():
            for g, (r, c, L) in zip(graphs, blocks):
                crit.change_morphology(g)
                q1, q2 = crit(obs[r:r + c, :41 * L], act[r:r + c, :3 * L])
                ref[0, r:r + c, :L], ref[1, r:r + c, :L] = q1, q2
    torch_ms, torch_min = timed(torch_path, reps)
    hip_path()
    torch_path()
    torch.cuda.synchronize()
    diff = max(float((got[0][k] - ref[k]).abs().max()) for k in range(2))
    print(json.dumps({"mode": "forward", "workload": which, "morphologies": len(names), "envs": n_env,
                      "nodes_per_network": int(sum(L * c for L, c in zip(Ls, counts))),
                      "hip_twin_two_streams_ms_median": round(two_ms, 4), "hip_twin_two_streams_ms_min": round(two_min, 4),
                      "hip_twin_one_stream_ms_median": round(one_ms, 4), "hip_twin_one_stream_ms_min": round(one_min, 4),
                      "hip_single_q1_ms_median": round(single_ms, 4),
                      "torch_twin_ms_median": round(torch_ms, 4), "torch_twin_ms_min": round(torch_min, 4),
                      "speedup": round(torch_ms / two_ms, 2), "launches_per_twin_forward": hip.launches(),
                      "max_abs_diff_vs_torch": diff, "reps": reps, "device": torch.cuda.get_device_name(0)}), flush=True)


def count_launches(step, it0):
    """Kernel launches of the updates it0 (odd: no actor step) and it0 + 1, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step(it0)
            step(it0 + 1)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return sum(1 for n in names if not n.lower().startswith(("memcpy", "memset")))
    except Exception:
        return None


def update(name, arm, updates, streams, dropout=0.0):
    from sgrl_amd.td3 import Agent, default_train_args
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    args = default_train_args(actor_type="swat", critic_type="swat", dropout_rate=float(dropout))
    if arm == "kernels":
        agent = Agent(args, device=dev, swat_train_kernels=True)
    elif arm == "graphed":
        agent = Agent(args, device=dev, swat_train_kernels=True, loss_kernels=True)
    else:
        agent = Agent(args, device=dev) if arm == "auto" else Agent(args, device=dev, use_hip=(arm == "hip"))
    g = G.getGraphDict(mjcf.load_asset(name).parents, TRAV, [], device=dev)
    L, B = len(g["parents"]), 256
    agent.change_morphology(g)
    agent.models2train()
    if not streams:
        from sgrl_amd import _lib
        from sgrl_amd.swat_hip import _bind
        _bind(_lib.lib())
        _lib.lib().sgrl_swat_debug_twin_streams(0)
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
    critic_loss = float(loss["loss/critic_loss"])
    launches = count_launches(step, 9 + updates - (updates % 2))        # an odd iteration first
    print(json.dumps({"mode": "update", "morphology": name, "limbs": L, "batch": B, "arm": arm, "dropout_rate": float(dropout),
                      "launches_per_two_updates": launches,
                      "hip_target_chain": getattr(agent, "_targets", None) is not None, "twin_streams": bool(streams),
                      "train_kernels": bool(getattr(agent, "use_swat_train_kernels", False)),
                      "update_ms_mean": round(float(ms.mean()), 4), "update_ms_median": round(float(np.median(ms)), 4),
                      "update_ms_min": round(float(ms.min()), 4), "critic_only_ms_median": round(float(np.median(ms[1::2])), 4),
                      "with_actor_ms_median": round(float(np.median(ms[0::2])), 4), "updates": int(updates),
                      "critic_loss": critic_loss, "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "forward"
    if mode == "forward":
        forward(sys.argv[2] if len(sys.argv) > 2 else "config3", max(50, int(sys.argv[3]) if len(sys.argv) > 3 else 60))
    elif mode == "update":
        update(sys.argv[2] if len(sys.argv) > 2 else "3d_walker_7_full", sys.argv[3] if len(sys.argv) > 3 else "auto",
               int(sys.argv[4]) if len(sys.argv) > 4 else 40, int(sys.argv[5]) if len(sys.argv) > 5 else 1,
               float(sys.argv[6]) if len(sys.argv) > 6 else 0.0)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
