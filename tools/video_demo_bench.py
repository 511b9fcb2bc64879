#!/usr/bin/env python3
"""Frames of the policy video demo through the host-assembled path (BatchedModularVecEnv.get_images: records to the host, forward
kinematics in Python, scene upload, ray caster, frame to the host) against the device path (get_images_device: sgrl_scene +
sgrl_render, include/sgrl_render.h), on one GPU.

usage: video_demo_bench.py [out=profiles/video_demo_bench.json] [steps=200] [size=256]
The 23 training morphologies of config 5, ONE environment each, `size` x `size` frames, the same SET policy (seed 0, untrained):
  (1) time per frame of all 23 environments: `get_images()` against `get_images_device()` (synchronised after the last repetition)
      and against `get_images_device().cpu()` (the frame brought to the host as well, as get_images does);
  (2) wall time of one demo of at most `steps` steps: evaluate.VideoDemo.run() against the same loop -- reset, frame, then per step
      policy, engine step, DeviceEvaluator.record, frame, stop when every environment has finished once -- with get_images() for
      the frames and the stop flag read at once (the reference's loop, common/trainer.py:149-258).
Each pair is alternated three times in one process after one untimed run of each; medians are reported next to every run.
This process never opens the GPU: the measurement is a child process under its own `timeout -k 10`, and a failure ends the run.
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MAX_JOBS = int(os.environ.get("MAX_JOBS", 16))      # cap on host threads of the child (never the machine's CPU count)
HELD_OUT = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
            "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}
ALTERNATIONS = 3
FRAME_REPS = 10


def config5():
    from sgrl_amd import mjcf
    return sorted(n for n in mjcf.list_assets() if n not in HELD_OUT)


def host_demo(ro, ev, size, max_len):
    """The demo loop with host-assembled frames: -> (frames kept, steps taken)."""
    import numpy as np
    env = ro.env
    obs = ro.reset()
    ev.begin()
    frames = [env.get_images(None, size, size)]
    steps = 0
    for step in range(max_len):
        obs, rew, done = ro.step(ro.policy_forward(obs))[:3]
        ev.record(rew, done, step)
        frames.append(env.get_images(None, size, size))
        steps += 1
        if int(ev.open.item()) == 0:
            break
    return np.stack(frames).shape[0], steps


def child(out_path, max_len, size):
    import torch
    torch.set_num_threads(max(1, min(torch.get_num_threads(), MAX_JOBS)))
    from sgrl_amd.evaluate import DeviceEvaluator, VideoDemo
    from sgrl_amd.rollout import Rollout
    from sgrl_amd.set_policy import make_policy
    import numpy as np
    names = config5()
    torch.manual_seed(0)
    policy = make_policy(device="cuda:0").eval()
    ro = Rollout(names, 1, policy=policy, seed=1, device="cuda:0")
    env = ro.env
    n = env.num_envs
    ro.reset()
    res = {"morphologies": len(names), "envs": n, "size": size, "alternations": ALTERNATIONS}

    def frame_host():
        for _ in range(FRAME_REPS):
            env.get_images(None, size, size)

    def frame_device():
        for _ in range(FRAME_REPS):
            env.get_images_device(None, size, size)

    def frame_device_fetched():
        for _ in range(FRAME_REPS):
            env.get_images_device(None, size, size).cpu()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    arms = (("get_images", frame_host), ("get_images_device", frame_device), ("get_images_device_to_host", frame_device_fetched))
    for _, fn in arms:
        fn()
    runs = {k: [] for k, _ in arms}
    for _ in range(ALTERNATIONS):
        for k, fn in arms:
            runs[k].append(timed(fn)[0] / FRAME_REPS * 1e3)
    res["ms_per_frame_of_all_envs"] = {k: {"runs": v, "median": statistics.median(v)} for k, v in runs.items()}
    print(json.dumps(res["ms_per_frame_of_all_envs"]), flush=True)

    ev = DeviceEvaluator(ro, num_eval_trajectories=1, max_trajectory_length=max_len, group=np.zeros(n, dtype=np.int64))
    demo = VideoDemo(ro, width=size, height=size, max_trajectory_length=max_len)

    def demo_host():
        return host_demo(ro, ev, size, max_len)

    def demo_device():
        frames, _, _ = demo.run()
        return frames.shape[0], demo.last_steps
    arms = (("host_frames", demo_host), ("video_demo", demo_device))
    for _, fn in arms:
        fn()
    runs = {k: [] for k, _ in arms}
    for _ in range(ALTERNATIONS):
        for k, fn in arms:
            wall, (kept, steps) = timed(fn)
            runs[k].append({"wall_s": wall, "frames": kept, "steps": steps, "ms_per_frame": wall / kept * 1e3})
            print(k, json.dumps(runs[k][-1]), flush=True)
    res["demo"] = {k: {"runs": v, "median_wall_s": statistics.median(r["wall_s"] for r in v),
                       "median_ms_per_frame": statistics.median(r["ms_per_frame"] for r in v)} for k, v in runs.items()}
    res["demo"]["max_trajectory_length"] = max_len
    with open(out_path, "w") as f:
        json.dump(res, f)


def step(cmd, limit):
    """One child under its own time limit; a failure ends the whole run."""
    full = ["timeout", "-k", "10", str(int(limit))] + cmd
    print("+ " + " ".join(full), flush=True)
    rc = subprocess.run(full).returncode
    if rc != 0:
        raise SystemExit("video_demo_bench: `%s` ended with status %d: stopping here" % (" ".join(cmd[:6]), rc))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "video_demo_bench.json")
    max_len = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    size = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    with tempfile.TemporaryDirectory() as d:
        part = os.path.join(d, "part.json")
        step([sys.executable, os.path.abspath(__file__), "--child", part, str(max_len), str(size)], 420)
        res = json.load(open(part))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
