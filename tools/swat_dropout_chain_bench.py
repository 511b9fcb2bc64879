#!/usr/bin/env python3
"""Timing of the TD3 update of a SWAT agent WITH dropout, and of its no-grad target part alone, in three arms:

  a  swat_hip_dropout off, eager   the target networks (training mode) run the MODULES under torch.no_grad(), every dropout site
                                   through train_ops._counter_dropout (the torch restatement of the counter RNG)
  b  swat_hip_dropout on, eager    the target chain is ONE call of sgrl_swat_td_target_dropout (75 launches)
  c  swat_hip_dropout on, graphed  b's update replayed from hipGraphs (td3.GraphedUpdates(hip_kernels=True)); its target part: the
                                   chain call alone recorded into a graph of its own

usage: swat_dropout_chain_bench.py [morphology=3d_walker_7_full] [batch=256] [dropout=0.1] [rounds=4] [per_round=10] [out.json]

One process, one agent per arm from one seed, the arms ALTERNATING in rounds of `per_round` timed calls (so drift of the box hits all
three alike); 8 untimed updates per arm first (the graphed arm's two eager warm-up updates and its captures fall among them).  An
update: host clock around the call + device synchronisation, every second one with the delayed actor step.  The target part:
`Agent.update_targets` under the agent's dropout context (arm c: the replay of the recorded chain), device events around it.  Medians
over rounds * per_round samples, with the 10th / 90th percentile and the medians of the single rounds as the spread.  Launch counts:
kernels seen by torch.profiler in one target part resp. two consecutive updates (copies and fills excluded; null without a profiler),
and the library's own count for the chain.  Both settings of the online passes (PyTorch autograd / `swat_train_kernels` with
`loss_kernels`).  Prints one JSON document; with a path, writes it there too.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from sgrl_amd import graph as G, mjcf, train_ops

TRAV = ["pre", "inlcrs", "postlcrs"]


def kernel_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return sum(1 for n in names if not n.lower().startswith(("memcpy", "memset")))
    except Exception:
        return None


def stats(ms, per_round):
    ms = np.asarray(ms)
    rounds = [float(np.median(ms[i:i + per_round])) for i in range(0, len(ms), per_round)]
    return {"median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4),
            "p90_ms": round(float(np.percentile(ms, 90)), 4), "round_medians_ms": [round(r, 4) for r in rounds], "samples": int(ms.size)}


class Arm(object):
    def __init__(self, tag, name, B, dropout, kernels):
        from sgrl_amd.td3 import Agent, GraphedUpdates, default_train_args
        dev = torch.device("cuda:0")
        self.tag, self.B = tag, B
        torch.manual_seed(0)
        args = default_train_args(actor_type="swat", critic_type="swat", dropout_rate=float(dropout), seed=7)
        kw = dict(swat_train_kernels=True, loss_kernels=True) if kernels else {}
        self.agent = Agent(args, device=dev, swat_hip_dropout=(tag != "a"), **kw)
        self.g = G.getGraphDict(mjcf.load_asset(name).parents, TRAV, [], device=dev)
        self.L = L = len(self.g["parents"])
        self.agent.change_morphology(self.g)
        self.agent.models2train()
        gen = torch.Generator(device=dev).manual_seed(1)
        r = lambda *s: torch.rand(s, device=dev, generator=gen)
        self.batches = [{"obs": torch.randn((B, 41 * L), device=dev, generator=gen), "next_obs": torch.randn((B, 41 * L), device=dev, generator=gen),
                         "action": r(B, 3 * L) * 2 - 1, "reward": r(B, 1) * 2 - 1, "done": (r(B, 1) < 0.05).float()} for _ in range(4)]
        self.noise = torch.randn((B, 3 * L), device=dev, generator=gen) * 0.2
        self.it = 0
        self.gu = None
        if tag == "c":
            self.gu = GraphedUpdates(self.agent, B, hip_kernels=True)
            self.gu.warm(0, self.g, L, lambda: self.batches[0], iters=2)
            self.it = 2
        while self.it < 8:
            self.update()
        torch.cuda.synchronize()
        self.chain_graph = None
        if tag == "c":                   # the chain alone, recorded after the eager updates above have made its handles' first calls
            self.tq = None
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._targets_eager()
            torch.cuda.current_stream().wait_stream(s)
            self.chain_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.chain_graph):
                self.tq = self._targets_eager()

    def update(self):
        it, b = self.it, self.batches[self.it % 4]
        self.it += 1
        if self.gu is not None:
            return self.gu.update(0, self.g, self.L, b, it)
        return self.agent.update(b, it, lazy_stats=True)

    def _targets_eager(self):
        a = self.agent
        with train_ops.dropout_rng(a.dropout_seed, a._dropout_step):
            return a.update_targets(self.batches[0], self.noise)[1]

    def targets(self):
        if self.chain_graph is not None:
            self.chain_graph.replay()
        else:
            self._targets_eager()

    def time_updates(self, n):
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            self.update()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    def time_targets(self, n):
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.targets()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms


def run(name, B, dropout, rounds, per_round, kernels):
    arms = [Arm(t, name, B, dropout, kernels) for t in "abc"]
    for arm in arms:
        for _ in range(5):
            arm.targets()
    torch.cuda.synchronize()
    upd, tgt = {a.tag: [] for a in arms}, {a.tag: [] for a in arms}
    for _ in range(rounds):
        for arm in arms:
            upd[arm.tag] += arm.time_updates(per_round)
        for arm in arms:
            tgt[arm.tag] += arm.time_targets(per_round)
    out = {}
    for arm in arms:
        if arm.it % 2 == 0:
            arm.update()                 # the two counted updates: one without, one with the actor step, in every arm
        t = arm.agent._hip_targets(arm.batches[0]["next_obs"])
        out[arm.tag] = {"swat_hip_dropout": bool(arm.agent.swat_hip_dropout), "graphed": arm.gu is not None,
                        "target_part": dict(stats(tgt[arm.tag], per_round), kernel_launches=kernel_launches(arm.targets),
                                            chain_launches_by_the_library=None if t is None else t.dropout_launches()),
                        "update": dict(stats(upd[arm.tag], per_round),
                                       kernel_launches_per_two_updates=kernel_launches(lambda: (arm.update(), arm.update()))),
                        "dropout_step": int(arm.agent._dropout_step)}
    return out


def main():
    argv = sys.argv[1:]
    name = argv[0] if len(argv) > 0 else "3d_walker_7_full"
    B = int(argv[1]) if len(argv) > 1 else 256
    dropout = float(argv[2]) if len(argv) > 2 else 0.1
    rounds = int(argv[3]) if len(argv) > 3 else 4
    per_round = int(argv[4]) if len(argv) > 4 else 10
    if not torch.cuda.is_available():
        raise SystemExit("swat_dropout_chain_bench.py times the MI355X: no device, no number")
    doc = {"what": "TD3 update of a SWAT agent with dropout: target part and whole update, arms a / b / c (tools/swat_dropout_chain_bench.py)",
           "morphology": name, "batch": B, "dropout_rate": dropout, "rounds": rounds, "per_round": per_round,
           "device": torch.cuda.get_device_name(0),
           "notes": ["kernel_launches / kernel_launches_per_two_updates are what torch.profiler saw; later profiler sessions of one process "
                     "have been seen to lose events (57 of a chain's 75 launches): chain_launches_by_the_library is the exact count of the "
                     "chain, asserted in tests/test_swat_hip_dropout_gpu.py",
                     "the graphed arm's update time includes filling the slot's static batch and noise"],
           "online_passes_pytorch": run(name, B, dropout, rounds, per_round, kernels=False),
           "online_passes_train_kernels": run(name, B, dropout, rounds, per_round, kernels=True)}
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if len(argv) > 5:
        with open(argv[5], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
