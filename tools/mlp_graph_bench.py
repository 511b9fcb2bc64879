#!/usr/bin/env python3
"""Timing of a whole TD3 update of an MLP agent replayed from hipGraphs (td3.GraphedMlpUpdates.update_from: one sample_into launch,
then a replay of 9 or 15 kernel nodes) against the same update issued eagerly (Agent(mlp_hip_grads=True, mlp_hip_optim=True).update:
the same library launches one by one, the reward scaling and the two statistics as PyTorch operators).

usage: mlp_graph_bench.py [reps=50] [out.json]
The method of tools/mlp_update_bench.py / mlp_optim_bench.py: one process, one morphology (3d_walker_7_full), hidden widths [256, 256],
seeded weights, the arms alternating window by window.  Both arms draw every batch and its target-policy noise by ONE
DeviceReplayBuffer.sample_into from a filled ring of 4096 rows (~ N(0, 1), rewards ~ N(1, 0.5)) with the same (seed, draw) sequence,
at B = 256 (the reference's batch) and B = 1024 (the sampler's maximum).  Per arm: device events around each of `reps` (>= 50) updates
after 10 untimed ones (median), and wall clock per update over 200 back-to-back updates with one synchronise at the end, in three
windows (median, best, spread = max - min).  Every second update carries the actor step and the soft target update (policy_freq 2).
The graphed arm's first two updates (one of each kind) run eagerly and its next two capture: all four fall into the untimed ones.

Recorded in the output: whether the graphed arm's wall clock per update at B = 256 is below the eager arm's by more than the larger of
the two arms' spreads.  The feature stays opt-in either way (DeviceTrainer(graph_updates=True)).

Not measured here: kernel times in isolation, the graph's launch cost apart from its kernels, a trainer round end to end."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch

from mlp_restate import apply_seeded_
from mlp_update_bench import BACK_TO_BACK, NAME, events, wall_summary, wall_window
from sgrl_amd import graph as G, mjcf
from sgrl_amd.replay import DeviceReplayBuffer
from sgrl_amd.td3 import Agent, GraphedMlpUpdates, default_train_args

ARMS = {"eager": "Agent(mlp_hip_grads=True, mlp_hip_optim=True).update(lazy_stats=True) on a batch drawn by sample_into",
        "graphed": "GraphedMlpUpdates.update_from: sample_into, then one hipGraph replay"}
RING, SEED = 4096, 11


def make_agent(L, g, dev):
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L)
    agent = Agent(args, device=dev, use_hip=True, mlp_hip_grads=True, mlp_hip_optim=True)
    for mod, seed in ((agent.actor, 3), (agent.critic, 4), (agent.actor_target, 5), (agent.critic_target, 6)):
        apply_seeded_(mod, seed)
    agent.change_morphology(g)
    agent.models2train()
    return agent


def filled_ring(L, dev):
    gen = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(s, generator=gen)
    buf = DeviceReplayBuffer(41 * L, 3 * L, RING, device=dev)
    buf.add_transitions(rn(RING, 41 * L), rn(RING, 3 * L).clamp(-1, 1), rn(RING, 41 * L), rn(RING) * 0.5 + 1.0,
                        (torch.rand(RING, generator=gen) < 0.3).float())
    assert buf.max_sample_size == RING
    return buf


def main():
    reps = max(50, int(sys.argv[1]) if len(sys.argv) > 1 else 50)
    dev = torch.device("cuda:0")
    L = mjcf.load_asset(NAME).num_limbs
    g = G.getGraphDict(mjcf.load_asset(NAME).parents, ["pre", "inlcrs", "postlcrs"], [], device=dev)
    buf = filled_ring(L, dev)
    res = {"workload": "%s, hidden [256, 256], one TD3 update per call fed by sample_into from a ring of %d rows, every second update with the "
                       "actor step" % (NAME, RING), "reps": reps, "untimed_first": 10, "back_to_back_updates": BACK_TO_BACK, "windows": 3, "arms": ARMS,
           "timing": "one process, arms alternating window by window; device events around each update (median of reps) and wall clock per "
                     "update over back-to-back updates with one synchronise at the end (3 windows: median, best, spread = max - min)",
           "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in (256, 1024):
        eager = make_agent(L, g, dev)
        gu = GraphedMlpUpdates(make_agent(L, g, dev), B)
        z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
        batch, noise = {"obs": z(B, 41 * L), "action": z(B, 3 * L), "next_obs": z(B, 41 * L), "reward": z(B, 1), "done": z(B, 1)}, z(B, 3 * L)
        its = {"eager": 0, "graphed": 0}

        def upd_eager():
            it = its["eager"]
            buf.sample_into(batch, B, SEED, it, noise=noise, noise_std=eager.args.policy_noise)
            eager.update(batch, it, noise=noise, lazy_stats=True)
            its["eager"] = it + 1

        def upd_graphed():
            it = its["graphed"]
            gu.update_from(0, g, L, buf, it, SEED, it)
            its["graphed"] = it + 1
        fns = {"eager": upd_eager, "graphed": upd_graphed}
        ent = {"events_" + arm: events(fns[arm], reps) for arm in ARMS}
        windows = {arm: [] for arm in ARMS}
        for _ in range(3):
            for arm in ARMS:
                windows[arm].append(wall_window(fns[arm]))
        for arm in ARMS:
            ent["wall_" + arm] = wall_summary(windows[arm])
        ent["speedup_wall_median"] = round(ent["wall_eager"]["median_ms_per_update"] / ent["wall_graphed"]["median_ms_per_update"], 3)
        ent["speedup_events_median"] = round(ent["events_eager"]["median_ms"] / ent["events_graphed"]["median_ms"], 3)
        ent["graphed_updates"], ent["graphed_replays"] = its["graphed"], gu.replays
        assert gu.replays == its["graphed"] - 2 and not gu.stale(0) and not gu.stale(1)        # everything but the first two replayed
        ent["graph_nodes"] = {"with_actor_step": gu.launches(0), "without_actor_step": gu.launches(1)}
        res["batches"][str(B)] = ent
    e = res["batches"]["256"]
    margin = max(e["wall_graphed"]["spread_ms"], e["wall_eager"]["spread_ms"])
    gain = e["wall_eager"]["median_ms_per_update"] - e["wall_graphed"]["median_ms_per_update"]
    res["decision"] = {"rule": "the gain counts only if wall clock per update at B = 256 (median of 3 windows) is below the eager arm's by more than "
                               "the larger of the two arms' spreads", "gain_ms": round(gain, 4), "margin_ms": round(margin, 4),
                       "gain_exceeds_spread": bool(gain > margin), "default_in_this_build": "opt-in (DeviceTrainer(graph_updates=True))"}
    res["not_measured"] = "kernel times in isolation (a profiler run of their own); the graph's launch cost apart from its kernels; a trainer round end to end"
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
