"""NumPy restatement of the grouped evaluation rule (include/sgrl_eval.h) and the scripts the evaluation tests share: the golden
evaluator cases laid side by side, and a random case whose groups straddle workgroups.  Scalar code, environment by environment,
in the order of the rule's lines: what the kernel and DeviceEvaluator are compared against."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["mixed", "time_limit", "never_all_done", "zero_reward_relatch"]
STATE = ("done_ever", "ep_steps", "ep_reward", "acc", "remaining", "close_step", "open")


class GroupedEval(object):
    def __init__(self, group, n_groups, max_episode_steps):
        self.group = np.asarray(group, dtype=np.int32)
        n = self.group.size
        self.n_groups, self.max_episode_steps = int(n_groups), int(max_episode_steps)
        self.done_ever = np.zeros(n, dtype=np.uint8)
        self.ep_steps = np.zeros(n, dtype=np.int64)
        self.ep_reward = np.zeros(n, dtype=np.float64)
        self.acc = np.zeros(n, dtype=np.float64)
        self.remaining = np.bincount(self.group, minlength=self.n_groups).astype(np.int32)
        self.close_step = np.zeros(self.n_groups, dtype=np.int32)
        self.open = np.array([self.n_groups], dtype=np.int32)

    def record(self, reward, done, step):
        """One launch.  The freeze test looks at the closing steps as they were BEFORE the launch or as a member of this launch
        wrote them (step + 1): both read "not frozen", so walking the environments in order is any schedule."""
        for i in range(self.group.size):
            g = self.group[i]
            if self.close_step[g] != 0 and self.close_step[g] <= step:
                continue
            self.acc[i] += np.float64(reward[i])
            cur = bool(done[i]) or self.ep_steps[i] + 1 == self.max_episode_steps
            if cur and self.ep_reward[i] == 0:
                self.ep_reward[i] = self.acc[i]
                self.acc[i] = 0.0
            if not self.done_ever[i]:
                self.ep_steps[i] += 1
            if cur and not self.done_ever[i]:
                self.done_ever[i] = 1
                self.remaining[g] -= 1
                if self.remaining[g] == 0:
                    self.close_step[g] = step + 1
                    self.open[0] -= 1

    def state(self):
        return {k: getattr(self, k).copy() for k in STATE}


def golden_case(case):
    """(rewards float64 [max_len, n_env], dones bool [max_len, n_env], group [n_env], env_morph [n_env], fixture dict): the case's
    n_traj trajectories side by side, environment (m, t) = index m * n_traj + t in group t, its step-s reward rew[t, s, m]."""
    z = np.load(os.path.join(GOLD, "evaluator.npz"))
    g = {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(case + "__")}
    n_traj, max_len, n_morph = g["rew"].shape
    assert n_traj == int(g["n_traj"]) and max_len == int(g["max_len"])
    rew = np.ascontiguousarray(g["rew"].transpose(1, 2, 0).reshape(max_len, n_morph * n_traj))
    done = np.ascontiguousarray(g["done"].transpose(1, 2, 0).reshape(max_len, n_morph * n_traj))
    group = np.tile(np.arange(n_traj), n_morph)
    env_morph = np.repeat(np.arange(n_morph), n_traj)
    return rew, done, group, env_morph, g


# 600 environments in 7 unequal groups, interleaved: sizes 1, 2, 250, 7, 300, 20, 20.  600 is the smallest shape in which the member
# that closes a group and other members of it sit in different 256-thread workgroups (groups 2 and 4 both span all three).
RANDOM_SIZES = [1, 2, 250, 7, 300, 20, 20]
RANDOM_MAX_EP = 9
RANDOM_STEPS = 14


def random_case(seed=11):
    """(rewards float32 [steps, 600] with about 10 % exact zeros, dones bool [steps, 600], group [600])."""
    rng = np.random.RandomState(seed)
    group = rng.permutation(np.repeat(np.arange(len(RANDOM_SIZES)), RANDOM_SIZES))
    n = group.size
    rew = rng.normal(0.0, 1.0, size=(RANDOM_STEPS, n)).astype(np.float32)
    rew[rng.uniform(size=rew.shape) < 0.10] = 0.0
    done = rng.uniform(size=rew.shape) < 0.12
    return rew, done, group.astype(np.int64)
