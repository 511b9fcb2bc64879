#!/usr/bin/env python3
"""BASELINE.json config 5 on one GPU (the 23 cwhh training morphologies x 356 environments, tools/train_bench.py's setting): the
collection step and the rows a round stores under DeviceTrainer's two continuous-collection switches.

For each mode -- default, store_all_episodes, true_next_obs, both -- two warm-up rounds of random actions (steps and rows stored per
round), then eight untimed and 40 timed policy collection steps (ms per step, as tools/train_bench.py times them).  No TD3 update
runs: the update schedule is not what the switches change.  Prints one JSON object and writes it to --out (default
profiles/continuous_collection.json).  Usage: collect_modes_bench.py [--out FILE] [envs_per_morph] [mode ...]"""
import json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
from sgrl_amd import mjcf
from sgrl_amd.td3 import default_train_args
from sgrl_amd.train_loop import DeviceTrainer
HELD_OUT = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
            "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}
MODES = {"default": {}, "store_all_episodes": {"store_all_episodes": True}, "true_next_obs": {"true_next_obs": True},
         "both": {"store_all_episodes": True, "true_next_obs": True}}
names = sorted(n for n in mjcf.list_assets() if n not in HELD_OUT)
argv = sys.argv[1:]
out_path = os.path.join(REPO, "profiles", "continuous_collection.json")
if argv[:1] == ["--out"]:
    out_path, argv = argv[1], argv[2:]
per = int(argv[0]) if argv else 8192 // len(names)
modes = argv[1:] or list(MODES)
out = {"morphologies": len(names), "envs_per_morph": per, "modes": {}}
for mode in modes:
    tr = DeviceTrainer(names, per, args=default_train_args(), seed=1, device="cuda:0", max_buffer_size=200000, **MODES[mode])
    n = tr.ro.env.num_envs
    rounds = []
    for _ in range(2):
        steps, before = 0, tr.sink.stored
        while True:
            steps += 1
            if tr.collect_step(random_actions=True):
                break
        mean_len = tr.sink.collector.episode_timesteps.float().mean().item()
        rounds.append({"steps": steps, "rows_stored": tr.sink.stored - before, "env_steps_simulated": steps * n,
                       "mean_first_episode_length": round(mean_len, 2)})
        tr.begin_round()
    for _ in range(8):
        if tr.collect_step():
            tr.begin_round()
    torch.cuda.synchronize()
    t0 = time.time(); K = 40
    for _ in range(K):
        if tr.collect_step():
            tr.begin_round()
    torch.cuda.synchronize()
    t = (time.time() - t0) / K
    out["envs"] = n
    out["modes"][mode] = {"ms_per_collection_step": round(t * 1e3, 3), "collection_env_steps_per_s": round(n / t, 1),
                          "warmup_rounds": rounds,
                          "stored_fraction": round(sum(r["rows_stored"] for r in rounds) / sum(r["env_steps_simulated"] for r in rounds), 4)}
    print(mode, json.dumps(out["modes"][mode]), flush=True)
    del tr
    torch.cuda.empty_cache()
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(out, open(out_path, "w"), indent=1)
