#!/usr/bin/env python3
"""The action choice of a collection step, before and after sgrl_explore_actions (include/sgrl_explore.h), on one GPU.

usage: explore_bench.py [out=profiles/explore_actions_bench.json] [iters=2000] [alternations=5]
At the config-5 shape (8188 environments x 42 action slots, live slots 3 L with L cycling over limb counts from 3 to 14), per
iteration and per mode:
  exploration  (a) torch.randn, *, +, clamp_, * act_mask, actions.copy_   (Rollout.add_exploration_noise + collect_step's copy)
               (b) one sgrl_explore_actions in GAUSS mode
  warm-up      (a) uniform_, mul_                                          (Rollout.random_actions)
               (b) one sgrl_explore_actions in UNIFORM mode
Per arm: host time (wall clock around `iters` iterations with no synchronisation inside, 200 untimed ones first) and GPU time
(device events around the same loop).  The arms alternate in one process; every run is written and the median over the
alternations reported.  The tensors of arm (a) are what the rollout holds; nothing is built from environments, so the tool needs
only the library and a device.
"""
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

N_ENV, ACT_MAX, STD, SEED = 8188, 42, 0.126, 5
LIMBS = [3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14]      # live slots = 3 L


def make(dev):
    from sgrl_amd import _lib
    L = _lib.bind_explore(_lib.lib())
    live = np.array([3 * LIMBS[i % len(LIMBS)] for i in range(N_ENV)], dtype=np.int32)
    act_len = torch.from_numpy(live).to(dev)
    act_mask = torch.from_numpy((np.arange(ACT_MAX)[None, :] < live[:, None]).astype(np.float32)).to(dev)
    policy = torch.zeros((N_ENV, ACT_MAX), device=dev).uniform_(-1, 1) * act_mask
    actions = torch.zeros((N_ENV, ACT_MAX), device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    step = [0]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def gauss_a():
        noise = torch.randn(policy.shape, device=dev, generator=gen) * STD
        actions.copy_(((policy + noise).clamp_(-1.0, 1.0)) * act_mask)

    def uniform_a():
        actions.uniform_(-1.0, 1.0, generator=gen)
        actions.mul_(act_mask)

    def library(mode):
        def fn():
            rc = L.sgrl_explore_actions(vp(policy), ACT_MAX, vp(actions), ACT_MAX, vp(act_len), N_ENV, ACT_MAX, 0, SEED, step[0], mode, STD,
                                        -1.0, 1.0, stream)
            if rc != 0:
                raise _lib.SgrlError(L.sgrl_explore_last_error().decode())
            step[0] += 1
        return fn
    return {"exploration": {"a": gauss_a, "b": library(_lib.EXPLORE_GAUSS)}, "warm-up": {"a": uniform_a, "b": library(_lib.EXPLORE_UNIFORM)}}, L


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


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "explore_actions_bench.json")
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    alts = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    if not torch.cuda.is_available():
        raise SystemExit("explore_bench.py measures on the GPU: no device is visible")
    dev = torch.device("cuda:0")
    modes, L = make(dev)
    res = {"device": torch.cuda.get_device_name(0), "n_env": N_ENV, "act_max": ACT_MAX, "std": STD, "iters": iters, "warmup": 200,
           "alternations": alts, "library_launches": int(L.sgrl_explore_actions_launches()), "modes": {}}
    for mode, arms in modes.items():
        for fn in arms.values():
            for _ in range(200):
                fn()
        runs = []
        for alt in range(alts):
            for arm in ("a", "b"):
                runs.append(dict(alternation=alt, arm=arm, **timed(arms[arm], iters)))
        ent = {"runs": runs, "median": {arm: {k: float(np.median([r[k] for r in runs if r["arm"] == arm])) for k in ("host_us", "gpu_us")}
                                        for arm in ("a", "b")}}
        pairs = [(runs[2 * i], runs[2 * i + 1]) for i in range(alts)]
        ent["b_below_a_in_every_alternation"] = {k: all(b[k] < a[k] for a, b in pairs) for k in ("host_us", "gpu_us")}
        res["modes"][mode] = ent
        print(json.dumps({mode: {"median": ent["median"], "b_below_a_in_every_alternation": ent["b_below_a_in_every_alternation"]}}), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
