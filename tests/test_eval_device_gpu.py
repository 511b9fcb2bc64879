"""Grouped evaluation on the GPU (include/sgrl_eval.h, sgrl_amd/evaluate.py DeviceEvaluator, DeviceTrainer.evaluate): the kernel
against the NumPy restatement (tests/eval_restate.py) bit for bit after every step; the lagged early stop against the full-length
run; DeviceEvaluator on the engine against the restatement fed the step outputs the engine actually produced; the trainer's
entry point, which must leave the training state alone."""
import numpy as np
import pytest

from eval_restate import CASES, RANDOM_MAX_EP, RANDOM_SIZES, RANDOM_STEPS, STATE, GroupedEval, golden_case, random_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class _Env(object):
    def __init__(self, counts):
        self.num_envs = int(sum(counts))
        self.env_names = ["m%d" % k for k in range(len(counts))]
        self.env_morph = np.repeat(np.arange(len(counts)), counts)
        self.morph_slices, off = [], 0
        for c in counts:
            self.morph_slices.append(slice(off, off + c))
            off += c


class _ScriptedRollout(object):
    """The Rollout surface DeviceEvaluator drives, with rewards / dones replayed from a script held on the device."""

    def __init__(self, rew, done, counts):
        import torch
        self.device = torch.device(DEV)
        self.env = _Env(counts)
        self.rew, self.done = torch.from_numpy(rew).to(self.device), torch.from_numpy(done).to(self.device)
        self.obs = torch.zeros((self.env.num_envs, 1), dtype=torch.float32, device=self.device)
        self.k = 0

    def reset(self):
        self.k = 0
        return self.obs

    def policy_forward(self, obs):
        return obs

    def step(self, actions):
        r, d = self.rew[self.k], self.done[self.k]
        self.k += 1
        return self.obs, r, d, None


def _assert_state_equal(ev, ref, where):
    """Every state array of the evaluator against the restatement's, bit for bit (floats by their bytes)."""
    import torch
    torch.cuda.synchronize()
    want = ref.state()
    for name in STATE:
        got = getattr(ev, name).cpu().numpy()
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, (where, name)
        assert got.tobytes() == want[name].tobytes(), (where, name, got, want[name])


def _step_by_step(ro, ev, rew, done, group, n_groups, max_ep):
    ref = GroupedEval(group, n_groups, max_ep)
    ro.reset()
    ev.begin()
    _assert_state_equal(ev, ref, "begin")
    for step in range(rew.shape[0]):
        _, r, d, _ = ro.step(None)
        ev.record(r, d, step)
        ref.record(rew[step], done[step], step)
        _assert_state_equal(ev, ref, step)
    return ref


@pytest.mark.parametrize("case", CASES)
def test_kernel_equals_the_restatement_on_the_golden_cases(case):
    """float64 rewards through the float64 pointer, default groups (environment t of every morphology = trajectory t)."""
    from sgrl_amd.evaluate import DeviceEvaluator, reduce_groups
    rew, done, group, env_morph, g = golden_case(case)
    n_traj, n_morph = int(g["n_traj"]), rew.shape[1] // int(g["n_traj"])
    ro = _ScriptedRollout(rew, done, [n_traj] * n_morph)
    ev = DeviceEvaluator(ro, num_eval_trajectories=n_traj, max_trajectory_length=int(g["max_len"]), max_episode_steps=int(g["max_ep"]))
    assert np.array_equal(ev.group.cpu().numpy(), group)
    _step_by_step(ro, ev, rew, done, group, n_traj, int(g["max_ep"]))
    out = reduce_groups(ev.ep_reward, ev.ep_steps, ev.group, ev.close_step)
    for key, want in (("performance/eval_return", float(g["eval_return"])), ("performance/eval_length", float(g["eval_length"]))):
        if np.isnan(want):
            assert np.isnan(out[key]), (case, key)
        else:
            assert out[key] == pytest.approx(want, rel=1e-12, abs=1e-12), (case, key)


def test_kernel_equals_the_restatement_when_groups_straddle_workgroups():
    """600 environments, 7 interleaved groups of 1 .. 300 members, float32 rewards with exact zeros, a time limit of 9 that closes
    the large groups from several workgroups in one launch, and five more steps on frozen groups."""
    from sgrl_amd.evaluate import DeviceEvaluator
    rew, done, group = random_case()
    assert rew.dtype == np.float32 and 0.05 < (rew == 0).mean() < 0.15 and group.size == 600
    for g, size in enumerate(RANDOM_SIZES):      # the two large groups have members in all three workgroups
        assert (group == g).sum() == size
        if size >= 250:
            assert {int(i) // 256 for i in np.nonzero(group == g)[0]} == {0, 1, 2}
    ro = _ScriptedRollout(rew, done, [600])
    ev = DeviceEvaluator(ro, num_eval_trajectories=len(RANDOM_SIZES), max_trajectory_length=RANDOM_STEPS, max_episode_steps=RANDOM_MAX_EP,
                         group=group)
    ref = _step_by_step(ro, ev, rew, done, group, len(RANDOM_SIZES), RANDOM_MAX_EP)
    assert int(ref.open[0]) == 0 and ref.close_step.max() == RANDOM_MAX_EP and ref.close_step.min() < RANDOM_MAX_EP


def test_lagged_early_stop_returns_what_the_full_length_run_returns():
    from sgrl_amd.evaluate import DeviceEvaluator, reduce_groups
    rew, done, group = random_case()
    ro = _ScriptedRollout(rew, done, [600])
    ev = DeviceEvaluator(ro, num_eval_trajectories=len(RANDOM_SIZES), max_trajectory_length=RANDOM_STEPS, max_episode_steps=RANDOM_MAX_EP,
                         group=group)
    early = ev.evaluate()
    early_steps = ev.last_steps
    full = ev.evaluate(early_stop=False)
    assert ev.last_steps == RANDOM_STEPS
    # every group has closed after step 9 (the time limit); the count read one step late ends the loop after step 10
    assert early_steps == RANDOM_MAX_EP + 1 < RANDOM_STEPS
    assert early == full and not any(np.isnan(v) for v in full.values())
    ref = GroupedEval(group, len(RANDOM_SIZES), RANDOM_MAX_EP)
    for step in range(RANDOM_STEPS):
        ref.record(rew[step], done[step], step)
    want = reduce_groups(ref.ep_reward, ref.ep_steps, ref.group, ref.close_step, np.zeros(600, dtype=np.int64), ["m0"])
    assert full == want


def test_device_evaluator_on_the_engine_equals_the_restatement_of_its_own_steps():
    import torch
    from sgrl_amd.evaluate import DeviceEvaluator, reduce_groups
    from sgrl_amd.rollout import Rollout
    from sgrl_amd.set_policy import make_policy
    names = ["3d_hopper_5_full", "3d_walker_7_full"]
    torch.manual_seed(4)
    ro = Rollout(names, 3, policy=make_policy(device=DEV).eval(), seed=2, device=DEV, max_episode_steps=20)
    tape, step = [], ro.step

    def taped(actions):
        out = step(actions)
        tape.append((out[1].clone(), out[2].clone()))
        return out
    ro.step = taped
    ev = DeviceEvaluator(ro, num_eval_trajectories=3, max_trajectory_length=40, max_episode_steps=20)
    out = ev.evaluate()
    assert len(tape) == ev.last_steps <= 21            # every environment hits the 20-step limit at the latest; read one step late
    group = np.tile(np.arange(3), 2)
    assert np.array_equal(ev.group.cpu().numpy(), group)
    ref = GroupedEval(group, 3, 20)
    for t, (r, d) in enumerate(tape):
        ref.record(r.cpu().numpy(), d.cpu().numpy(), t)
    for name in STATE:
        assert getattr(ev, name).cpu().numpy().tobytes() == getattr(ref, name).tobytes(), name
    want = reduce_groups(ref.ep_reward, ref.ep_steps, ref.group, ref.close_step, np.repeat(np.arange(2), 3), names)
    assert sorted(out) == sorted(want) and len(out) == 6
    for nm in names:
        assert "performance/eval_return/" + nm in out and "performance/eval_length/" + nm in out
    for key, v in want.items():
        print(key, out[key], v)
        assert np.isfinite(v)
        if "eval_length" in key:
            assert out[key] == v, key
        else:
            assert out[key] == pytest.approx(v, rel=1e-12), key
    assert 1 <= out["performance/eval_length"] <= 20
    ro.env.close()


def test_trainer_evaluate_leaves_the_training_state_alone_and_runs_zero_shot():
    import torch
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_hopper_5_full", "3d_walker_7_full"]
    tr = DeviceTrainer(names, 2, args=default_train_args(max_episode_steps=20, batch_size=16), seed=3, device=DEV, max_buffer_size=256)
    tr.warmup(6)
    col = tr.sink.collector

    def snapshot():
        torch.cuda.synchronize()
        return ([t.clone() for t in (tr.ro.env.obs, col.done_list, col.episode_timesteps, col.episode_reward, col._reward_buf)],
                (tr.sink.stored, tr.tot_env_steps, [(b.curr, b.max_sample_size) for b in tr.buffers]))
    before = snapshot()

    def check(out, keys):
        assert sorted(out) == sorted(["performance/eval_return", "performance/eval_length"] +
                                     ["performance/eval_%s/%s" % (w, nm) for w in ("return", "length") for nm in keys])
        for k, v in out.items():
            assert isinstance(v, float) and (np.isfinite(v) or np.isnan(v)), k
    out = tr.evaluate(num_eval_trajectories=2, max_trajectory_length=30)
    check(out, names)
    assert np.isfinite(out["performance/eval_length"]) and out["performance/eval_length"] <= 20      # the 20-step limit closes every group
    assert list(tr.eval_rollouts) == [tuple(names)]
    ro_eval = tr.eval_rollouts[tuple(names)][1]
    assert ro_eval is not tr.ro and ro_eval.env is not tr.ro.env and ro_eval.policy is tr.agent.actor and not ro_eval.holds_weights
    check(tr.evaluate(num_eval_trajectories=2, max_trajectory_length=30), names)
    assert tr.eval_rollouts[tuple(names)][1] is ro_eval      # cached
    held_out = ["3d_hopper_3_shin"]
    assert held_out[0] not in names
    check(tr.evaluate(num_eval_trajectories=2, max_trajectory_length=30, env_names=held_out), held_out)
    assert sorted(tr.eval_rollouts) == sorted([tuple(names), tuple(held_out)])
    after = snapshot()
    assert after[1] == before[1]
    for a, b in zip(before[0], after[0]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    tr.collect_step(random_actions=True)                 # the training loop goes on
    torch.cuda.synchronize()
