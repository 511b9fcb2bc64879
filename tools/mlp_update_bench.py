#!/usr/bin/env python3
"""Timing of a whole TD3 update of an MLP agent (td3.Agent.update) with the gradient half on the HIP kernels
(Agent(mlp_hip_grads=True): mlp_hip.HipMlpGrads) against the parent's path (use_hip=True with the gradient half on PyTorch autograd).

usage: mlp_update_bench.py [reps=50] [out.json]
The method of tools/mlp_target_bench.py: one process, one morphology (3d_walker_7_full), hidden widths [256, 256], seeded weights,
batches ~ N(0, 1) at B = 256 (the reference's batch) and B = 4096, the same buffers every repetition, the two arms alternating.  Per
arm: device events around each of `reps` (>= 50) updates after 10 untimed ones (median), and wall clock per update over 200
back-to-back updates with one synchronise at the end, in three windows (median, best, and the spread max - min of the three).
Every second update carries the actor step and the soft target update (policy_freq 2).

Decision recorded in the output: the new path becomes td3.MLP_HIP_GRADS_DEFAULT only if its wall clock per update at B = 256 is below
the parent arm's by more than the larger of the two arms' spreads.

Eager launches per update are COUNTED (torch.profiler device events of one update with and one without the actor step, after the
timing).  Not measured here: kernel times in isolation (they need a profiler run of their own), and hipGraph replay (tools/mlp_graph_bench.py)."""
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


def wall_window(fn, calls=BACK_TO_BACK):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def wall_summary(windows):
    return {"windows_ms_per_update": [round(w, 4) for w in windows], "median_ms_per_update": round(float(np.median(windows)), 4),
            "min_ms_per_update": round(float(min(windows)), 4), "spread_ms": round(float(max(windows) - min(windows)), 4)}


def make_agent(grads, L, g, dev):
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L)
    agent = Agent(args, device=dev, use_hip=True, mlp_hip_grads=grads)
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


def count_launches(fn):
    """Device-side events (kernels, copies, fills) of one fn(it=0) -- with the actor step -- and one fn(it=1) -- without."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    out = {}
    for tag, it in (("with_actor_step", 0), ("without_actor_step", 1)):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(it)
            torch.cuda.synchronize()
        out[tag] = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    out["mean_per_update"] = (out["with_actor_step"] + out["without_actor_step"]) / 2.0
    return out


def main():
    reps = max(50, int(sys.argv[1]) if len(sys.argv) > 1 else 50)
    dev = torch.device("cuda:0")
    L = mjcf.load_asset(NAME).num_limbs
    g = G.getGraphDict(mjcf.load_asset(NAME).parents, ["pre", "inlcrs", "postlcrs"], [], device=dev)
    new, parent = make_agent(True, L, g, dev), make_agent(False, L, g, dev)
    res = {"workload": "%s, hidden [256, 256], td3.Agent.update (lazy_stats), every second update with the actor step" % NAME, "reps": reps,
           "untimed_first": 10, "back_to_back_updates": BACK_TO_BACK, "windows": 3,
           "arms": {"hip_grads": "Agent(use_hip=True, mlp_hip_grads=True)", "parent": "Agent(use_hip=True, mlp_hip_grads=False): target chain on HIP, "
                    "gradient half on PyTorch autograd"},
           "timing": "one process, arms alternating window by window; device events around each update (median of reps) and wall clock per "
                     "update over back-to-back updates with one synchronise at the end (3 windows: median, best, spread = max - min)",
           "device": torch.cuda.get_device_name(0), "batches": {}}
    its = {id(new): 0, id(parent): 0}
    for B in (256, 4096):
        b, noise = batch(B, L, dev, seed=B)

        def upd(agent):
            agent.update(b, its[id(agent)], noise=noise, lazy_stats=True)
            its[id(agent)] += 1
        f_new, f_par = (lambda: upd(new)), (lambda: upd(parent))
        ent = {"events_hip_grads": events(f_new, reps), "events_parent": events(f_par, reps)}
        w_new, w_par = [], []
        for _ in range(3):
            w_new.append(wall_window(f_new))
            w_par.append(wall_window(f_par))
        ent["wall_hip_grads"], ent["wall_parent"] = wall_summary(w_new), wall_summary(w_par)
        ent["speedup_wall_median"] = round(ent["wall_parent"]["median_ms_per_update"] / ent["wall_hip_grads"]["median_ms_per_update"], 3)
        ent["speedup_events_median"] = round(ent["events_parent"]["median_ms"] / ent["events_hip_grads"]["median_ms"], 3)
        res["batches"][str(B)] = ent
    e = res["batches"]["256"]
    margin = max(e["wall_hip_grads"]["spread_ms"], e["wall_parent"]["spread_ms"])
    gain = e["wall_parent"]["median_ms_per_update"] - e["wall_hip_grads"]["median_ms_per_update"]
    res["decision"] = {"rule": "default on only if wall clock per update at B = 256 (median of 3 windows) is below the parent arm's by more than the "
                               "larger of the two arms' spreads", "gain_ms": round(gain, 4), "margin_ms": round(margin, 4),
                       "hip_grads_becomes_default": bool(gain > margin)}
    assert new._mlp_grads is not None and parent._mlp_grads is None
    res["train_plan"] = new._mlp_grads.plan(256)
    res["library_launches"] = {"critic_step": new._mlp_grads.critic_launches(), "actor_step": new._mlp_grads.actor_launches()}
    b, noise = batch(256, L, dev, seed=256)
    try:
        res["eager_launches_per_update_B256"] = {
            "hip_grads": count_launches(lambda it: new.update(b, it, noise=noise, lazy_stats=True)),
            "parent": count_launches(lambda it: parent.update(b, it, noise=noise, lazy_stats=True)),
            "method": "torch.profiler device events (kernels, copies, fills) of one update, counted"}
    except Exception as ex:             # the profiler is not part of the timing: say so instead of failing the run
        res["eager_launches_per_update_B256"] = {"not_measured": repr(ex)}
    res["not_measured"] = "kernel times in isolation (a profiler run of their own); hipGraph replay of the update (GraphedUpdates refuses mlp agents)"
    line = json.dumps(res)
    print(line, flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
