#!/usr/bin/env python3
"""One evaluation of the deterministic policy, trajectory after trajectory (evaluate.BatchedEvaluator) against all trajectories in
one batched pass (evaluate.DeviceEvaluator, include/sgrl_eval.h), on one GPU.

usage: eval_bench.py [out=profiles/eval_device_bench.json] [trajectories=10] [max_len=1000]
For the eight walker variants and for the 23 training morphologies of config 5, the same SET policy (seed 0, untrained) and the
same trajectory count on both sides:
  (a) BatchedEvaluator over a Rollout with ONE environment per morphology, its trajectories one after the other
  (b) DeviceEvaluator over a Rollout with `trajectories` environments per morphology, one trajectory group each
alternated three times in one process (one untimed evaluation of each first).  Per run: wall time of the evaluation (host clock,
the evaluation ends synchronised) and the engine steps it took.  The two sides draw different initial states (other environment
counts, other episode numbers), so their returns are not compared here: tests/test_eval_device_gpu.py does that on equal inputs.
Bookkeeping launches per step: a kernel trace (a run of its own per arm, nothing else collected in it) of a child that drives
either evaluator over a scripted environment that launches nothing itself, for two step counts; the difference of the kernel
counts over the difference of the steps, by kernel name, the runtime's own copy kernels (each side fetches one word per step: the
`all(done)` flag / the open-group count) counted apart.
This process never opens the GPU: every step that does is a child process under its own `timeout -k 10`, one after the other, and
the first one that fails ends the run.
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

MAX_JOBS = int(os.environ.get("MAX_JOBS", 16))      # cap on host threads of the children (never the machine's CPU count)
HELD_OUT = {"3d_walker_3_left_knee_right_knee", "3d_walker_6_right_foot", "3d_humanoid_7_left_leg", "3d_humanoid_8_right_knee",
            "3d_cheetah_11_leftbkneen_rightffoot", "3d_cheetah_12_tail_leftffoot"}
ALTERNATIONS = 3
TRACE_STEPS = (10, 30)


def mixes():
    from sgrl_amd import mjcf
    names = mjcf.list_assets()
    return {"walker++": sorted(n for n in names if n.startswith("3d_walker_")),
            "config5": sorted(n for n in names if n not in HELD_OUT)}


class _RolloutEnv(object):
    """reset() / step() of a Rollout as BatchedEvaluator's `env`, counting steps."""

    def __init__(self, ro):
        self.ro, self.steps = ro, 0

    def reset(self):
        return self.ro.reset()

    def step(self, actions):
        self.steps += 1
        return self.ro.step(actions)


def time_child(mix, out_path, n_traj, max_len):
    import torch
    torch.set_num_threads(max(1, min(torch.get_num_threads(), MAX_JOBS)))
    from sgrl_amd.evaluate import BatchedEvaluator, DeviceEvaluator
    from sgrl_amd.rollout import Rollout
    from sgrl_amd.set_policy import make_policy
    names = mixes()[mix]
    torch.manual_seed(0)
    policy = make_policy(device="cuda:0").eval()
    ro_a = Rollout(names, 1, policy=policy, seed=1, device="cuda:0")
    ro_b = Rollout(names, n_traj, policy=policy, seed=1, device="cuda:0")
    env_a = _RolloutEnv(ro_a)
    ev_a = BatchedEvaluator(env_a, ro_a.policy_forward, num_eval_trajectories=n_traj, max_trajectory_length=max_len)
    ev_b = DeviceEvaluator(ro_b, num_eval_trajectories=n_traj, max_trajectory_length=max_len)

    def run_a():
        env_a.steps = 0
        out = ev_a.evaluate()
        return out, env_a.steps

    def run_b():
        out = ev_b.evaluate()
        return out, ev_b.last_steps
    arms = (("batched", run_a), ("device", run_b))
    for _, fn in arms:                       # untimed: code objects load, the weights are packed
        fn()
    runs = []
    for alt in range(ALTERNATIONS):
        for arm, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, steps = fn()
            torch.cuda.synchronize()
            runs.append({"alternation": alt, "arm": arm, "wall_s": time.perf_counter() - t0, "steps": steps,
                         "eval_return": out["performance/eval_return"], "eval_length": out["performance/eval_length"]})
            print(json.dumps(runs[-1]), flush=True)
    pairs = [(runs[2 * i], runs[2 * i + 1]) for i in range(ALTERNATIONS)]
    res = {"morphologies": len(names), "envs": {"batched": ro_a.env.num_envs, "device": ro_b.env.num_envs}, "runs": runs,
           "device_below_batched_in_every_alternation": {k: all(b[k] < a[k] for a, b in pairs) for k in ("wall_s", "steps")}}
    with open(out_path, "w") as f:
        json.dump(res, f)


class _QuietEnv(object):
    """Eight environments that never finish and launch nothing: the kernels of a run are the evaluator's own bookkeeping."""

    def __init__(self, torch):
        self.device = torch.device("cuda:0")
        self.obs = torch.zeros((8, 1), device=self.device)
        self.rew = torch.ones(8, device=self.device)
        self.done = torch.zeros(8, dtype=torch.uint8, device=self.device)
        # the Rollout surface DeviceEvaluator reads
        self.env = self
        self.num_envs, self.env_names, self.env_morph, self.morph_slices = 8, ["quiet"], [0] * 8, [slice(0, 8)]

    def reset(self):
        return self.obs

    def policy_forward(self, obs):
        return obs

    def step(self, actions):
        return self.obs, self.rew, self.done, None


def trace_child(arm, n):
    import torch
    from sgrl_amd.evaluate import BatchedEvaluator, DeviceEvaluator
    env = _QuietEnv(torch)
    if arm == "batched":
        ev = BatchedEvaluator(env, env.policy_forward, num_eval_trajectories=1, max_trajectory_length=n, max_episode_steps=10 ** 6)
    else:
        ev = DeviceEvaluator(env, num_eval_trajectories=8, max_trajectory_length=n, max_episode_steps=10 ** 6)
    ev.evaluate()
    torch.cuda.synchronize()


def step(cmd, limit):
    """One child under its own time limit; a failure ends the whole run."""
    full = ["timeout", "-k", "10", str(int(limit))] + cmd
    print("+ " + " ".join(full), flush=True)
    rc = subprocess.run(full).returncode
    if rc != 0:
        raise SystemExit("eval_bench: `%s` ended with status %d: stopping here" % (" ".join(cmd[:6]), rc))


def launches_per_step(arm):
    """{"kernels": launches per step, "copies": the runtime's own copy kernels per step (a small device-to-host copy shows up
    in a kernel trace as one), "by_name": per kernel name}."""
    import collections
    rows = []
    for n in TRACE_STEPS:
        with tempfile.TemporaryDirectory() as d:
            step(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable,
                  os.path.abspath(__file__), "--trace-child", arm, str(n)], 300)
            with open(glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]) as f:
                rows.append(collections.Counter(r["Kernel_Name"] for r in csv.DictReader(f)))
    dn = TRACE_STEPS[1] - TRACE_STEPS[0]
    by_name = {}
    for name in rows[1]:
        diff = rows[1][name] - rows[0][name]
        assert diff % dn == 0, (name, rows[0][name], rows[1][name])
        if diff:
            by_name[name] = diff // dn
    is_copy = lambda name: "rocclr" in name.lower()
    return {"kernels": sum(v for k, v in by_name.items() if not is_copy(k)), "copies": sum(v for k, v in by_name.items() if is_copy(k)),
            "by_name": by_name}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--time-child":
        return time_child(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    if len(sys.argv) > 1 and sys.argv[1] == "--trace-child":
        return trace_child(sys.argv[2], int(sys.argv[3]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "eval_device_bench.json")
    n_traj = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    max_len = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    res = {"trajectories": n_traj, "max_trajectory_length": max_len, "alternations": ALTERNATIONS, "mixes": {}}
    for mix in mixes():
        with tempfile.TemporaryDirectory() as d:
            part = os.path.join(d, "part.json")
            step([sys.executable, os.path.abspath(__file__), "--time-child", mix, part, str(n_traj), str(max_len)], 420)
            res["mixes"][mix] = json.load(open(part))
    res["bookkeeping_launches_per_step"] = {arm: launches_per_step(arm) for arm in ("batched", "device")}
    print(json.dumps(res["bookkeeping_launches_per_step"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
