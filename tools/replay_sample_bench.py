#!/usr/bin/env python3
"""The read side of the replay, before and after sgrl_replay_sample (include/sgrl_replay.h), on one GPU.

usage: replay_sample_bench.py [out=profiles/replay_sample_bench.json] [iters=2000] [updates=40]
For walker_7 (L = 7) and cheetah_14 (L = 14), B = 256, a ring filled to 200 000 rows, per iteration:
  (a) sample(B, generator) + the five copies of GraphedUpdates._load into static tensors + normal_()   -- the path it replaces
  (b) one sample_into with noise
Per arm: host time (wall clock around `iters` iterations with no synchronisation inside, 200 untimed ones first), GPU time (device
events around the same loop) and the kernel launches of one iteration (rocprofv3 --kernel-trace of a child process that runs the
arm n times, for two values of n: the difference of the two kernel counts over the difference of n; the tracer goes in front of
python, no counters in the same run).  The arms alternate four times in one process; every run is written, not a mean alone.
Then a graphed walker_7 update at B = 256: sample + GraphedUpdates.update against GraphedUpdates.update_from, `updates` updates
per run (host clock around them, ending in a device synchronisation), the same four alternations.
"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

B, FILL, STD, SEED = 256, 200000, 0.2, 5
MORPHS = {"walker_7": 7, "cheetah_14": 14}


def make(L, dev):
    from sgrl_amd.replay import DeviceReplayBuffer
    buf = DeviceReplayBuffer(41 * L, 3 * L, FILL, device=dev)
    for t in (buf.obs_buffer, buf.action_buffer, buf.next_obs_buffer, buf.reward_buffer):
        t.normal_()
    buf.max_sample_size = FILL
    z = lambda *s: torch.zeros(s, device=dev)
    static = {"obs": z(B, 41 * L), "action": z(B, 3 * L), "next_obs": z(B, 41 * L), "reward": z(B, 1), "done": z(B, 1)}
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    noise = z(B, 3 * L)
    draw = [0]

    def arm_a():
        batch = buf.sample(B, generator=gen)
        for k, t in static.items():
            t.copy_(batch[k].reshape(t.shape))
        noise.normal_(0, STD)

    def arm_b():
        buf.sample_into(static, B, SEED, draw[0], noise=noise, noise_std=STD)
        draw[0] += 1
    return {"a": arm_a, "b": arm_b}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    t1 = time.perf_counter()
    e1.synchronize()
    return {"host_us": 1e6 * (t1 - t0) / iters, "gpu_us": 1e3 * e0.elapsed_time(e1) / iters}


def trace_child(name, arm, n):
    arms = make(MORPHS[name], torch.device("cuda:0"))
    for _ in range(n):
        arms[arm]()
    torch.cuda.synchronize()


def launches(name, arm):
    """Kernel launches of one iteration: kernel-trace rows of a child running 30 iterations minus those of one running 10, over 20."""
    rows = []
    for n in (10, 30):
        with tempfile.TemporaryDirectory() as d:
            subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable,
                            os.path.abspath(__file__), "--trace-child", name, arm, str(n)], check=True, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL, timeout=300)
            with open(glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]) as f:
                rows.append(sum(1 for _ in csv.DictReader(f)))
    assert (rows[1] - rows[0]) % 20 == 0, rows
    return (rows[1] - rows[0]) // 20


def graphed_update(updates):
    from sgrl_amd import graph as G, mjcf
    from sgrl_amd.rollout import TRAV
    from sgrl_amd.td3 import Agent, GraphedUpdates, default_train_args
    dev = torch.device("cuda:0")
    m = mjcf.load_asset("3d_walker_7_full")
    L = m.num_limbs
    gd = G.getGraphDict(m.parents, TRAV, [], device=dev)
    torch.manual_seed(0)
    agent = Agent(default_train_args(), device=dev)
    agent.models2train()
    gu = GraphedUpdates(agent, B)
    from sgrl_amd.replay import DeviceReplayBuffer
    buf = DeviceReplayBuffer(41 * L, 3 * L, FILL, device=dev)
    for t in (buf.obs_buffer, buf.action_buffer, buf.next_obs_buffer, buf.reward_buffer):
        t.normal_()
    buf.max_sample_size = FILL
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    gu.warm_from(0, gd, L, buf, SEED, 0, iters=2)
    draw = [2]

    def old(it):
        gu.update(0, gd, L, buf.sample(B, generator=gen), it)

    def new(it):
        gu.update_from(0, gd, L, buf, it, SEED, draw[0])
        draw[0] += 1
    for it in range(6):                      # captures both graphs, then replays
        old(it)
        new(it)
    runs = []
    for alt in range(4):
        for label, fn in (("update+sample", old), ("update_from", new)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(updates):
                fn(it)
            torch.cuda.synchronize()
            runs.append({"alternation": alt, "arm": label, "ms_per_update": 1e3 * (time.perf_counter() - t0) / updates})
    return runs


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace-child":
        return trace_child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "replay_sample_bench.json")
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    updates = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    dev = torch.device("cuda:0")
    from sgrl_amd import _lib
    from sgrl_amd.replay import _bind
    _bind(_lib.lib())
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "fill": FILL, "iters": iters, "warmup": 200,
           "library_launches": int(_lib.lib().sgrl_replay_sample_launches()), "morphologies": {}}
    for name, L in MORPHS.items():
        arms = make(L, dev)
        for fn in arms.values():
            for _ in range(200):
                fn()
        runs = []
        for alt in range(4):
            for arm in ("a", "b"):
                runs.append(dict(alternation=alt, arm=arm, **timed(arms[arm], iters)))
        ent = {"runs": runs, "launches_per_iteration": {arm: launches(name, arm) for arm in ("a", "b")}}
        pairs = [(runs[2 * i], runs[2 * i + 1]) for i in range(4)]
        ent["b_below_a_in_every_alternation"] = {k: all(b[k] < a[k] for a, b in pairs) for k in ("host_us", "gpu_us")}
        res["morphologies"][name] = ent
        print(json.dumps({name: ent}), flush=True)
        del arms
        torch.cuda.empty_cache()
    res["graphed_walker_7_update"] = {"updates_per_run": updates, "runs": graphed_update(updates)}
    print(json.dumps(res["graphed_walker_7_update"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
