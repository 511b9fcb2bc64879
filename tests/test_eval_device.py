"""Grouped evaluation without a GPU (sgrl_amd/evaluate.py reduce_groups / DeviceEvaluator, include/sgrl_eval.h): the rule restated
in NumPy (tests/eval_restate.py) meets the reference's evaluator fixtures with the trajectories laid side by side; reduce_groups'
per-morphology means; DeviceEvaluator's host-side checks; the C ABI's argument errors, which return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from eval_restate import CASES, GroupedEval, golden_case
from sgrl_amd import _lib, evaluate
from sgrl_amd.evaluate import DeviceEvaluator, reduce_groups


@pytest.mark.parametrize("case", CASES)
def test_grouped_restatement_meets_the_reference_fixtures(case):
    """rel = abs = 1e-12 is the bar tests/test_evaluator_snapshot.py holds BatchedEvaluator to against the same fixtures; only the
    order of the final mean's summation differs (environment order here, trajectory order there)."""
    rew, done, group, env_morph, g = golden_case(case)
    ev = GroupedEval(group, int(g["n_traj"]), int(g["max_ep"]))
    for step in range(int(g["max_len"])):
        ev.record(rew[step], done[step], step)
    out = reduce_groups(ev.ep_reward, ev.ep_steps, ev.group, ev.close_step)
    assert sorted(out) == ["performance/eval_length", "performance/eval_return"]
    for key, ref in (("performance/eval_return", float(g["eval_return"])), ("performance/eval_length", float(g["eval_length"]))):
        print(case, key, out[key], ref)
        if np.isnan(ref):
            assert np.isnan(out[key]), (case, key)
        else:
            assert out[key] == pytest.approx(ref, rel=1e-12, abs=1e-12), (case, key)
    assert int(ev.open[0]) == int((ev.close_step == 0).sum())


def test_reduce_groups_per_morphology_means_skip_the_open_group():
    # 3 morphologies x 4 groups, environment (m, t) = index 4 m + t in group t; group 2 never completed
    ret = np.array([1.0, 2.0, 100.0, 4.0, -1.5, 0.25, 100.0, 8.0, 0.0, 3.0, 100.0, -7.0])
    steps = np.array([5, 6, 99, 8, 10, 11, 99, 13, 1, 2, 99, 4])
    group = np.tile(np.arange(4), 3)
    close = np.array([9, 12, 0, 3], dtype=np.int32)
    morph = np.repeat(np.arange(3), 4)
    names = ["a", "b", "c"]
    for wrap in (np.asarray, torch.as_tensor):
        out = reduce_groups(wrap(ret), wrap(steps), wrap(group), wrap(close), env_morph=wrap(morph), names=names)
        assert out["performance/eval_return"] == pytest.approx((1 + 2 + 4 - 1.5 + 0.25 + 8 + 0 + 3 - 7) / 9.0, rel=1e-15)
        assert out["performance/eval_length"] == pytest.approx((5 + 6 + 8 + 10 + 11 + 13 + 1 + 2 + 4) / 9.0, rel=1e-15)
        assert out["performance/eval_return/a"] == pytest.approx(7.0 / 3, rel=1e-15)
        assert out["performance/eval_return/b"] == pytest.approx(6.75 / 3, rel=1e-15)
        assert out["performance/eval_return/c"] == pytest.approx(-4.0 / 3, rel=1e-15)
        assert out["performance/eval_length/a"] == pytest.approx(19.0 / 3, rel=1e-15)
        assert out["performance/eval_length/b"] == pytest.approx(34.0 / 3, rel=1e-15)
        assert out["performance/eval_length/c"] == pytest.approx(7.0 / 3, rel=1e-15)
        assert len(out) == 8
    # nothing completed: NaN everywhere, as the reference's mean of an empty list
    out = reduce_groups(ret, steps, group, np.zeros(4, dtype=np.int32), env_morph=morph, names=names)
    assert len(out) == 8 and all(np.isnan(v) for v in out.values())
    out = reduce_groups(ret, steps, group, np.zeros(4, dtype=np.int32))
    assert len(out) == 2 and all(np.isnan(v) for v in out.values())


class _Env(object):
    def __init__(self, counts):
        self.num_envs = sum(counts)
        self.env_names = ["m%d" % k for k in range(len(counts))]
        self.env_morph = np.repeat(np.arange(len(counts)), counts)
        self.morph_slices, off = [], 0
        for c in counts:
            self.morph_slices.append(slice(off, off + c))
            off += c


class _CpuRollout(object):
    """The surface DeviceEvaluator reads, on the CPU."""
    device = torch.device("cpu")

    def __init__(self, counts):
        self.env = _Env(counts)

    def policy_forward(self, obs):
        return obs


def test_device_evaluator_validates_groups_and_refuses_a_cpu_rollout():
    ro = _CpuRollout([3, 3])
    for bad, what in (([0, 1, 2, 0, 1, 3], "id out of range"), ([0, 1, -1, 0, 1, 2], "negative id"), ([0, 1, 1, 0, 1, 0], "group 2 empty"),
                      ([0, 1, 2, 0, 1], "wrong length"), ([0, 1, 2, 0, 1, 2, 0], "wrong length"),
                      (np.array([0, 1, 2, 0, 1, 2], dtype=np.float32), "not integers")):
        with pytest.raises(ValueError):
            DeviceEvaluator(ro, num_eval_trajectories=3, group=bad)
        pytest.raises(ValueError, DeviceEvaluator, ro, num_eval_trajectories=3, group=torch.as_tensor(np.asarray(bad)))
    # the default groups need num_eval_trajectories environments of every morphology
    with pytest.raises(ValueError):
        DeviceEvaluator(_CpuRollout([3, 3]), num_eval_trajectories=2)
    with pytest.raises(ValueError):
        DeviceEvaluator(_CpuRollout([2, 2]), num_eval_trajectories=3)
    # valid groups on a CPU rollout: there is no fallback
    with pytest.raises(_lib.SgrlError):
        DeviceEvaluator(ro, num_eval_trajectories=3)
    with pytest.raises(_lib.SgrlError):
        DeviceEvaluator(ro, num_eval_trajectories=3, group=[2, 1, 0, 0, 1, 2])


def test_c_abi_argument_errors_return_before_any_launch():
    """Host memory stands in for the device arrays: every call below must be refused before anything is launched or read."""
    L = _lib.lib()
    evaluate._bind(L)
    assert L.sgrl_eval_record_launches() == 1
    n, ng = 6, 2
    bufs = [np.zeros(n, dtype=np.int64) for _ in range(10)]
    ptr = [b.ctypes.data for b in bufs]
    fields = [f for f, _ in evaluate._EvalState._fields_]
    assert fields == ["group", "done_ever", "ep_steps", "ep_reward", "acc", "remaining", "close_step", "open"]
    good = evaluate._EvalState(*ptr[:8])
    rew, done = ctypes.c_void_p(ptr[8]), ctypes.c_void_p(ptr[9])
    ARG = -1

    def record(state=good, r32=rew, r64=None, d=done, n_env=n, n_groups=ng, step=0, max_ep=10):
        return L.sgrl_eval_record(ctypes.byref(state) if state is not None else None, r32, r64, d, n_env, n_groups, step, max_ep, None)

    def begin(state=good, n_env=n, n_groups=ng):
        return L.sgrl_eval_begin(ctypes.byref(state) if state is not None else None, n_env, n_groups, None)

    assert record(state=None) == ARG and begin(state=None) == ARG
    assert b"null state" in L.sgrl_eval_last_error()
    for f in fields:
        st = evaluate._EvalState(*ptr[:8])
        setattr(st, f, None)
        assert record(state=st) == ARG, f
        assert begin(state=st) == ARG, f
        assert b"member" in L.sgrl_eval_last_error()
    for bad in (0, -3):
        assert record(n_env=bad) == ARG and record(n_groups=bad) == ARG and record(max_ep=bad) == ARG
        assert begin(n_env=bad) == ARG and begin(n_groups=bad) == ARG
    assert record(step=-1) == ARG
    assert record(r32=rew, r64=rew) == ARG               # both reward forms
    assert b"exactly one" in L.sgrl_eval_last_error()
    assert record(r32=None, r64=None) == ARG             # neither
    assert record(d=None) == ARG
    assert not bufs[0].any() and not bufs[7].any()       # nothing was written
