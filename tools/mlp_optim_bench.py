#!/usr/bin/env python3
"""Timing of a whole TD3 update of an MLP agent (td3.Agent.update) with the optimizer half on the HIP kernels
(Agent(mlp_hip_grads=True, mlp_hip_optim=True): mlp_hip.HipMlpOptim, clip + Adam + soft update of a network in two launches) against
the parent's optimizer side: plain Adam groups (the default: clip_grad_norm_ + opt.step() + the table lerp) and capturable groups
(td3.clip_and_step's three table launches per network + the table lerp).  All three arms run the gradient half on HIP.

usage: mlp_optim_bench.py [reps=50] [out.json]
The method of tools/mlp_update_bench.py: one process, one morphology (3d_walker_7_full), hidden widths [256, 256], seeded weights,
batches ~ N(0, 1) at B = 256 (the reference's batch) and B = 4096, the same buffers every repetition, the arms alternating window by
window.  Per arm: device events around each of `reps` (>= 50) updates after 10 untimed ones (median), and wall clock per update over
200 back-to-back updates (lazy_stats) with one synchronise at the end, in three windows (median, best, spread = max - min).  Every
second update carries the actor step and the soft target update (policy_freq 2).

Recorded in the output: whether the new arm's wall clock per update at B = 256 is below the plain-group parent arm's by more than the
larger of the two arms' spreads -- the condition under which td3.MLP_HIP_OPTIM_DEFAULT should be flipped (the rule that decided
MLP_HIP_GRADS_DEFAULT).  The code stays opt-in either way.

Device events per update are COUNTED (torch.profiler, one update with and one without the actor step, after the timing).  Not
measured here: kernel times in isolation, and hipGraph replay (tools/mlp_graph_bench.py)."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch

from mlp_restate import apply_seeded_
from mlp_update_bench import BACK_TO_BACK, NAME, batch, count_launches, events, wall_summary, wall_window
from sgrl_amd import graph as G, mjcf
from sgrl_amd.td3 import Agent, default_train_args

ARMS = {"hip_optim": "Agent(mlp_hip_grads=True, mlp_hip_optim=True), plain Adam groups",
        "parent_plain": "Agent(mlp_hip_grads=True): plain Adam groups (the default): clip_grad_norm_ + opt.step() + sgrl_optim_lerp",
        "parent_capturable": "Agent(mlp_hip_grads=True) with capturable Adam groups: sgrl_optim_clip_adam + sgrl_optim_lerp"}


def make_agent(arm, L, g, dev):
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L)
    agent = Agent(args, device=dev, use_hip=True, mlp_hip_grads=True, mlp_hip_optim=(arm == "hip_optim"))
    if arm == "parent_capturable":
        agent.actor_optimizer = torch.optim.Adam(agent.actor.parameters(), lr=args.lr, capturable=True)
        agent.critic_optimizer = torch.optim.Adam(agent.critic.parameters(), lr=args.lr, capturable=True)
    for mod, seed in ((agent.actor, 3), (agent.critic, 4), (agent.actor_target, 5), (agent.critic_target, 6)):
        apply_seeded_(mod, seed)
    agent.change_morphology(g)
    agent.models2train()
    return agent


def main():
    reps = max(50, int(sys.argv[1]) if len(sys.argv) > 1 else 50)
    dev = torch.device("cuda:0")
    L = mjcf.load_asset(NAME).num_limbs
    g = G.getGraphDict(mjcf.load_asset(NAME).parents, ["pre", "inlcrs", "postlcrs"], [], device=dev)
    agents = {arm: make_agent(arm, L, g, dev) for arm in ARMS}
    res = {"workload": "%s, hidden [256, 256], td3.Agent.update (lazy_stats), every second update with the actor step" % NAME, "reps": reps,
           "untimed_first": 10, "back_to_back_updates": BACK_TO_BACK, "windows": 3, "arms": ARMS,
           "timing": "one process, arms alternating window by window; device events around each update (median of reps) and wall clock per "
                     "update over back-to-back updates with one synchronise at the end (3 windows: median, best, spread = max - min)",
           "device": torch.cuda.get_device_name(0), "batches": {}}
    its = {arm: 0 for arm in ARMS}
    for B in (256, 4096):
        b, noise = batch(B, L, dev, seed=B)

        def upd(arm):
            agents[arm].update(b, its[arm], noise=noise, lazy_stats=True)
            its[arm] += 1
        fns = {arm: (lambda arm=arm: upd(arm)) for arm in ARMS}
        ent = {"events_" + arm: events(fns[arm], reps) for arm in ARMS}
        windows = {arm: [] for arm in ARMS}
        for _ in range(3):
            for arm in ARMS:
                windows[arm].append(wall_window(fns[arm]))
        for arm in ARMS:
            ent["wall_" + arm] = wall_summary(windows[arm])
        for arm in ("parent_plain", "parent_capturable"):
            ent["speedup_wall_median_over_" + arm] = round(ent["wall_" + arm]["median_ms_per_update"] / ent["wall_hip_optim"]["median_ms_per_update"], 3)
            ent["speedup_events_median_over_" + arm] = round(ent["events_" + arm]["median_ms"] / ent["events_hip_optim"]["median_ms"], 3)
        res["batches"][str(B)] = ent
    e = res["batches"]["256"]
    margin = max(e["wall_hip_optim"]["spread_ms"], e["wall_parent_plain"]["spread_ms"])
    gain = e["wall_parent_plain"]["median_ms_per_update"] - e["wall_hip_optim"]["median_ms_per_update"]
    res["decision"] = {"rule": "the default should be flipped only if wall clock per update at B = 256 (median of 3 windows) is below the plain-group "
                               "parent arm's by more than the larger of the two arms' spreads", "gain_ms": round(gain, 4), "margin_ms": round(margin, 4),
                       "gain_exceeds_spread": bool(gain > margin), "default_in_this_build": False}
    new = agents["hip_optim"]
    assert new._mlp_optim is not None and new.mlp_hip_optim_refusal is None
    assert agents["parent_plain"]._mlp_optim is None and agents["parent_capturable"]._mlp_optim is None
    res["optim_plan"] = new._mlp_optim.plan()
    res["library_launches"] = {"critic_step_grads": new._mlp_grads.critic_launches(), "actor_step_grads": new._mlp_grads.actor_launches(),
                               "optim_step": new._mlp_optim.launches()}
    b, noise = batch(256, L, dev, seed=256)
    try:
        res["device_events_per_update_B256"] = {arm: count_launches(lambda it, arm=arm: agents[arm].update(b, it, noise=noise, lazy_stats=True))
                                                for arm in ARMS}
        res["device_events_per_update_B256"]["method"] = "torch.profiler device events (kernels, copies, fills) of one update, counted"
    except Exception as ex:             # the profiler is not part of the timing: say so instead of failing the run
        res["device_events_per_update_B256"] = {"not_measured": repr(ex)}
    res["not_measured"] = "kernel times in isolation (a profiler run of their own); hipGraph replay of the update (GraphedUpdates refuses mlp agents)"
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
