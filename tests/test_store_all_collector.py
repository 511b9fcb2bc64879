"""RoundCollector(store_all=True) -- the round record that keeps every episode of a round -- against the rule restated as plain
per-environment loops (the way the reference's `for i in range(num_envs)` reads, reference src/trainer.py:205-232): the first-episode
block is the reference's, unchanged; `cur_steps` dates the time limit of the later episodes; every step is stored except one taken after
the round was already complete.  CPU tensors; exact equality throughout (the float32 sums are restated in float32)."""
import numpy as np
import pytest
import torch

from sgrl_amd.replay import DeviceReplayBuffer
from sgrl_amd.rollout import RoundCollector, TransitionSink


class LoopRecord(object):
    """The rule, one environment at a time."""

    def __init__(self, n, max_steps, store_all):
        self.n, self.max_steps, self.store_all = n, max_steps, store_all
        self.begin_round()

    def begin_round(self):
        n = self.n
        self.done_list = [False] * n
        self.ep_steps = [0] * n
        self.ep_reward = [np.float32(0)] * n
        self.reward_buf = [np.float32(0)] * n
        self.cur_steps = [0] * n
        self.was_complete = False

    def record(self, reward, done):
        store, done_bool = [], []
        for i in range(self.n):
            # the first-episode block (trainer.py:205-232), on its own lists
            curr = bool(done[i])
            db = 1.0 if curr else 0.0
            if self.ep_steps[i] + 1 == self.max_steps:
                db = 0.0
                curr = True
            self.reward_buf[i] = np.float32(self.reward_buf[i] + np.float32(reward[i]))
            if curr and self.ep_reward[i] == 0:            # the latch of trainer.py:213: a return of exactly 0.0 latches again
                self.ep_reward[i] = self.reward_buf[i]
                self.reward_buf[i] = np.float32(0)
            first = not self.done_list[i]
            if first:
                self.ep_steps[i] += 1
                self.done_list[i] = curr
            if not self.store_all:
                store.append(first)
                done_bool.append(db)
                continue
            # every episode: the time limit of the episode in progress
            timeout = self.cur_steps[i] + 1 == self.max_steps
            done_bool.append(1.0 if (bool(done[i]) and not timeout) else 0.0)
            self.cur_steps[i] = 0 if (bool(done[i]) or timeout) else self.cur_steps[i] + 1
            store.append(not self.was_complete)
        finished = all(self.done_list)
        self.was_complete = finished
        return store, done_bool, finished


def parent_record(rc, reward, curr_done):
    """RoundCollector.record's tensor form as it stood before the switch existed, on the collector's own state."""
    curr_done = curr_done.to(torch.bool).clone()
    done_bool = curr_done.to(torch.float32)
    timeout = (rc.episode_timesteps + 1) == rc.max_episode_steps
    done_bool = torch.where(timeout, torch.zeros_like(done_bool), done_bool)
    curr_done |= timeout
    rc._reward_buf += reward.to(torch.float32)
    first = curr_done & (rc.episode_reward == 0)
    rc.episode_reward = torch.where(first, rc._reward_buf, rc.episode_reward)
    rc._reward_buf = torch.where(first, torch.zeros_like(rc._reward_buf), rc._reward_buf)
    store = ~rc.done_list
    rc.episode_timesteps += store.to(torch.long)
    rc.done_list |= store & curr_done
    return store, done_bool, bool(rc.done_list.all())


def streams(n, T, seed, p_fast=0.45, p_slow=0.04):
    """Environment 0 finishes rarely, the others often: while it is still in its first episode the others run through several."""
    rng = np.random.RandomState(seed)
    p = np.full(n, p_fast)
    p[0] = p_slow if n > 1 else 0.15
    return rng.normal(size=(T, n)).astype(np.float32), rng.rand(T, n) < p


def assert_state(rc, ref, where):
    assert rc.done_list.tolist() == ref.done_list, where
    assert rc.episode_timesteps.tolist() == ref.ep_steps, where
    assert np.array_equal(rc.episode_reward.numpy(), np.array(ref.ep_reward, dtype=np.float32)), where
    assert np.array_equal(rc._reward_buf.numpy(), np.array(ref.reward_buf, dtype=np.float32)), where
    if ref.store_all:
        assert rc.cur_steps.tolist() == ref.cur_steps, where


def drive(rc, ref, rewards, dones, late_steps):
    """Both through the same streams; a finished round takes `late_steps` more steps (a flag read late) before it begins anew.
    Returns (rounds finished, largest number of episodes one environment ran inside a round, rows stored)."""
    rounds, most, stored, late_left = 0, 0, 0, None
    episodes = np.zeros(rc.n, dtype=int)
    for t in range(rewards.shape[0]):
        store, done_bool, fin = rc.record(torch.from_numpy(rewards[t]), torch.from_numpy(dones[t]))
        r_store, r_db, r_fin = ref.record(rewards[t], dones[t])
        assert store.tolist() == r_store, t
        assert done_bool.tolist() == r_db, t
        assert fin == r_fin, t
        assert_state(rc, ref, t)
        stored += sum(r_store)
        if late_left is None:
            episodes += np.array([d == 1.0 or (ref.store_all and c == 0) for d, c in zip(r_db, ref.cur_steps)])
        if fin and late_left is None:
            late_left = late_steps
        if late_left is not None:
            if late_left == 0:
                rounds += 1
                most = max(most, int(episodes.max()))
                episodes[:] = 0
                rc.begin_round()
                ref.begin_round()
                late_left = None
            else:
                late_left -= 1
    return rounds, most, stored


@pytest.mark.parametrize("max_steps", [1, 2, 3, 1000])
@pytest.mark.parametrize("n", [1, 5])
def test_store_all_equals_the_loop_restatement(n, max_steps):
    for seed in range(4):
        rewards, dones = streams(n, 160, 10 * seed + n)
        late = seed % 2                                     # odd seeds: one step after the round was complete, as lag_flag takes
        rounds, most, stored = drive(RoundCollector(n, max_steps, store_all=True), LoopRecord(n, max_steps, True), rewards, dones, late)
        assert rounds >= 2
        if n > 1 and max_steps == 1000:
            assert most >= 3                                # the fast environments ran three or more episodes in some round
        if late == 0:
            assert stored == 160 * n                        # nothing is dropped when the flag is read at once


@pytest.mark.parametrize("max_steps", [1, 2, 3, 1000])
@pytest.mark.parametrize("n", [1, 5])
def test_default_mode_is_the_parent_rule(n, max_steps):
    """store_all=False: same outputs and state as the tensor form before the switch existed, and as the loops."""
    for seed in range(3):
        rewards, dones = streams(n, 120, 77 + seed)
        a, b, ref = RoundCollector(n, max_steps), RoundCollector(n, max_steps), LoopRecord(n, max_steps, False)
        assert not hasattr(a, "cur_steps")
        for t in range(120):
            r, d = torch.from_numpy(rewards[t]), torch.from_numpy(dones[t])
            s0, d0, f0 = a.record(r, d)
            s1, d1, f1 = parent_record(b, r, d)
            s2, d2, f2 = ref.record(rewards[t], dones[t])
            assert torch.equal(s0, s1) and torch.equal(d0, d1) and f0 == f1 == f2
            assert s0.tolist() == s2 and d0.tolist() == d2
            for name in ("done_list", "episode_timesteps", "episode_reward", "_reward_buf"):
                assert torch.equal(getattr(a, name), getattr(b, name)), (name, t)
            assert_state(a, ref, t)
            if f0:
                a.begin_round(), b.begin_round(), ref.begin_round()


def test_termination_on_the_time_limit_step_is_stored_as_a_cut():
    """max_episode_steps = 3, two rounds.  Round 1: environment 0 terminates exactly on the time-limit step (the rule reads
    `done_bool = 0` there, as the reference does: trainer.py:207-209).  Round 2: it terminates at once, and again on the second step of
    its second episode -- stored with done = 1, which the first-episode counter (stuck at 1) could not have dated -- while environment
    1 is cut by the limit; then one late step, which stores nothing."""
    T = 3
    dones = np.array([[0, 0], [0, 0], [1, 0], [1, 0], [0, 0], [1, 0], [0, 1]], dtype=bool)
    rewards = np.ones(dones.shape, dtype=np.float32)
    rc, ref = RoundCollector(2, T, store_all=True), LoopRecord(2, T, True)
    got = []
    for t in range(dones.shape[0]):
        store, done_bool, fin = rc.record(torch.from_numpy(rewards[t]), torch.from_numpy(dones[t]))
        assert (store.tolist(), done_bool.tolist(), fin) == ref.record(rewards[t], dones[t])
        assert_state(rc, ref, t)
        got.append((store.tolist(), done_bool.tolist(), fin))
        if t == 2:
            assert fin and rc.episode_timesteps.tolist() == [3, 3]
            rc.begin_round(), ref.begin_round()
    assert [g[0] for g in got] == [[True, True]] * 6 + [[False, False]]
    assert [g[1][0] for g in got[:6]] == [0, 0, 0, 1, 0, 1]
    assert [g[1][1] for g in got[:6]] == [0, 0, 0, 0, 0, 0]
    assert [g[2] for g in got] == [False, False, True, False, False, True, True]
    assert rc.episode_timesteps.tolist() == [1, 3]


def test_a_first_return_of_exactly_zero_latches_again():
    """trainer.py:213 tests `episode_reward == 0`: a first episode whose return is exactly 0.0 leaves the latch open and the next
    finished episode's return replaces it.  store_all keeps that quirk, bit for bit, beside the rows it adds."""
    rewards = np.array([[1.0, 0.5], [-1.0, 0.5], [2.0, 0.5], [0.25, 0.5], [4.0, 0.5]], dtype=np.float32)
    dones = np.array([[0, 0], [1, 0], [0, 0], [1, 0], [1, 1]], dtype=bool)
    for store_all in (False, True):
        rc, ref = RoundCollector(2, 1000, store_all=store_all), LoopRecord(2, 1000, store_all)
        for t in range(5):
            store, done_bool, fin = rc.record(torch.from_numpy(rewards[t]), torch.from_numpy(dones[t]))
            assert (store.tolist(), done_bool.tolist(), fin) == ref.record(rewards[t], dones[t])
            assert_state(rc, ref, t)
            if t == 1:
                assert rc.episode_reward[0].item() == 0.0 and rc.done_list[0].item()
            assert store.tolist() == ([True, True] if store_all else [t < 2, True])
        assert rc.episode_reward.tolist() == [2.25, 2.5] and rc.episode_timesteps.tolist() == [2, 5] and fin


LIMBS = [3, 5]
PER = [2, 3]
OBS, ACT = 41 * 5, 3 * 5


def test_sink_stores_every_row_in_environment_order_and_none_after_the_round():
    """One CPU rank, plain-tensor rings: a round of S steps leaves S x n rows -- each morphology's ring its environments' rows in
    step-then-environment order, cut to its 41 L / 3 L columns -- and the late step a lagged flag takes adds none."""
    env_morph = np.repeat(np.arange(len(LIMBS)), PER)
    n = env_morph.size
    rng = np.random.RandomState(5)
    T = 400
    obs = rng.rand(T + 1, n, OBS).astype(np.float32)
    act = rng.rand(T, n, ACT).astype(np.float32)
    rew, done = streams(n, T, 3)
    buffers = [DeviceReplayBuffer(41 * L, 3 * L, max_buffer_size=4096) for L in LIMBS]
    sink = TransitionSink(env_morph, LIMBS, OBS, ACT, max_episode_steps=12, buffers=buffers, store_all=True)
    ref = LoopRecord(n, 12, True)
    rows = [[] for _ in LIMBS]

    def push(t):
        _, db, _ = ref.record(rew[t], done[t])
        return sink.push(torch.from_numpy(obs[t]), torch.from_numpy(act[t]), torch.from_numpy(obs[t + 1]), torch.from_numpy(rew[t]),
                         torch.from_numpy(done[t])), db
    t = 0
    for _round in range(2):
        steps = 0
        while True:
            fin, db = push(t)
            for i in range(n):
                k = env_morph[i]
                rows[k].append((obs[t, i, :41 * LIMBS[k]], act[t, i, :3 * LIMBS[k]], obs[t + 1, i, :41 * LIMBS[k]], rew[t, i], db[i]))
            t += 1
            steps += 1
            if fin:
                break
        before = sink.stored
        assert before == sum(len(r) for r in rows)
        fin, _ = push(t)                                   # the step a lagged flag would still take
        t += 1
        assert fin and sink.stored == before
        sink.begin_round()
        ref.begin_round()
    assert sink.stored == sum(len(r) for r in rows) == (t - 2) * n
    for k, b in enumerate(buffers):
        assert b.curr == len(rows[k]) == (t - 2) * PER[k]
        for j, (o, a, nx, r, d) in enumerate(rows[k]):
            assert np.array_equal(b.obs_buffer[j].numpy(), o) and np.array_equal(b.action_buffer[j].numpy(), a)
            assert np.array_equal(b.next_obs_buffer[j].numpy(), nx)
            assert b.reward_buffer[j].item() == r and b.done_buffer[j].item() == d
    # the default sink on the same streams keeps fewer rows: first episodes only
    few = TransitionSink(env_morph, LIMBS, OBS, ACT, max_episode_steps=12,
                         buffers=[DeviceReplayBuffer(41 * L, 3 * L, max_buffer_size=4096) for L in LIMBS])
    t2 = 0
    while not few.push(torch.from_numpy(obs[t2]), torch.from_numpy(act[t2]), torch.from_numpy(obs[t2 + 1]), torch.from_numpy(rew[t2]),
                       torch.from_numpy(done[t2])):
        t2 += 1
    assert few.stored == few.total_episode_timesteps() < (t2 + 1) * n
