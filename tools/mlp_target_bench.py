#!/usr/bin/env python3
"""Timing of the TD3 target chain of an MLP agent (td3.Agent.update_targets) with the fused HIP chain (use_hip=True:
mlp_hip.HipMlpTargets, two pack launches + one chain launch) against the PyTorch chain (use_hip=False: about 25 eager launches), and
of a whole Agent.update both ways.

usage: mlp_target_bench.py [reps=50] [out.json]
One process, one morphology (3d_walker_7_full), hidden widths [256, 256], seeded weights, batches ~ N(0, 1) at B = 256 (the
reference's batch) and B = 4096; the same buffers every repetition.  Two figures per arm: device events around each of `reps`
(>= 50) calls after 10 untimed ones (median), and wall clock per call over 200 back-to-back calls with one synchronise at the end
(the PyTorch chain is host-launch-bound, which device events around a single call show only in part).  The two arms alternate in
blocks.  Prints one JSON line and, with a second argument, writes it there."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from mlp_restate import apply_seeded_
from sgrl_amd import graph as G, mjcf
from sgrl_amd.td3 import Agent, default_train_args

NAME = "3d_walker_7_full"
BACK_TO_BACK = 200


def events(fn, reps):
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


def wall(fn, calls=BACK_TO_BACK, blocks=3):
    """ms per call over `calls` back-to-back calls and one synchronise; the best and the median of `blocks` such windows."""
    out = []
    for _ in range(blocks):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    return {"median_ms_per_call": round(float(np.median(out)), 4), "min_ms_per_call": round(float(min(out)), 4)}


def make_agent(use_hip, L, g, dev):
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L)
    agent = Agent(args, device=dev, use_hip=use_hip)
    for mod, seed in ((agent.actor, 3), (agent.critic, 4), (agent.actor_target, 5), (agent.critic_target, 6)):
        apply_seeded_(mod, seed)
    agent.change_morphology(g)
    agent.models2train()
    return agent


def batch(B, L, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(s, device=dev, generator=gen)
    b = {"obs": rn(B, 41 * L), "next_obs": rn(B, 41 * L), "action": rn(B, 3 * L).clamp(-1, 1), "reward": rn(B, 1),
         "done": (torch.rand((B, 1), device=dev, generator=gen) < 0.3).float()}
    return b, rn(B, 3 * L) * 0.2


def main():
    reps = max(50, int(sys.argv[1]) if len(sys.argv) > 1 else 50)
    dev = torch.device("cuda:0")
    L = mjcf.load_asset(NAME).num_limbs
    g = G.getGraphDict(mjcf.load_asset(NAME).parents, ["pre", "inlcrs", "postlcrs"], [], device=dev)
    hip, pt = make_agent(True, L, g, dev), make_agent(False, L, g, dev)
    res = {"workload": "%s, hidden [256, 256], td3.Agent.update_targets" % NAME, "reps": reps, "untimed_first": 10,
           "back_to_back_calls": BACK_TO_BACK,
           "timing": "one process, arms alternating; device events around each call (median of reps) and wall clock per call over "
                     "back-to-back calls with one synchronise at the end (median and best of 3 windows)",
           "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in (256, 4096):
        b, noise = batch(B, L, dev, seed=B)
        f_hip = lambda: hip.update_targets(b, noise)
        f_pt = lambda: pt.update_targets(b, noise)
        t_hip, t_pt = f_hip()[1], f_pt()[1]
        ent = {"max_abs_diff_hip_vs_torch": float((t_hip - t_pt).abs().max()), "max_abs_target": float(t_pt.abs().max()),
               "events_hip": events(f_hip, reps), "events_torch": events(f_pt, reps), "wall_hip": wall(f_hip), "wall_torch": wall(f_pt)}
        ent["events_hip_2"], ent["events_torch_2"] = events(f_hip, reps), events(f_pt, reps)       # the same again: the spread
        ent["speedup_events_median"] = round(ent["events_torch"]["median_ms"] / ent["events_hip"]["median_ms"], 2)
        ent["speedup_wall_median"] = round(ent["wall_torch"]["median_ms_per_call"] / ent["wall_hip"]["median_ms_per_call"], 2)
        res["batches"][str(B)] = ent
    res["launches"] = {"hip_chain": hip._targets.launches(), "hip_packs": 2 * hip._targets.actor.pack_launches()}
    res["chain_plan"] = hip._targets.plan()
    # a whole update (target chain + critic forward / backward / Adam, every second one with the actor step and the soft update)
    b, noise = batch(256, L, dev, seed=7)
    it = [0, 0]

    def upd(agent, k):
        agent.update(b, it[k], noise=noise, lazy_stats=True)
        it[k] += 1
    res["update_B256"] = {"events_hip": events(lambda: upd(hip, 0), reps), "events_torch": events(lambda: upd(pt, 1), reps),
                          "wall_hip": wall(lambda: upd(hip, 0)), "wall_torch": wall(lambda: upd(pt, 1))}
    line = json.dumps(res)
    print(line, flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
