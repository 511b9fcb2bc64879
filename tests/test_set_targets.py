"""Host side of the one-call TD3 target chain of a SET agent (sgrl_amd/set_hip.py HipSetTargets, include/sgrl_set.h
sgrl_set_td_target): the inputs tests/test_set_targets_gpu.py runs are qualified on the float64 restatement alone
(tests/set_targets_restate.py), the restatement's mutants say what a comparison at the GPU file's bound can tell apart, and the
agent's switch changes nothing on the CPU.

Figures of this file's run (weight set 3, noise N(0, 1), noise_clip 0.9, max_action 1, done = 1 on two rows):
  case      noise clipped   action clamped   critic1 smaller
  walker        31 %             16 %             94 %
  cheetah       32 %             23 %             87 %
  mixed         32 %             17 %             98 %
Which critic is the smaller one depends on the weight set (set 1: critic2 everywhere), so the GPU file runs both handle orders."""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

import set_full_rank_ref as R
import set_targets_restate as S
from sgrl_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def base():
    """The float64 modules of the GPU file's weight set and the restatement of every case, computed once and never changed."""
    pol, crit = S.cpu_pair(S.SEED)
    return pol, crit, {k: S.restate_case(pol, crit, *S.CASES[k]) for k in S.CASES}


def _cat(out, key):
    return np.concatenate([d[key].ravel() for *_, d in out])


@pytest.mark.parametrize("case", list(S.CASES))
def test_inputs_exercise_every_branch_of_the_chain(base, case):
    out = base[2][case]
    noise, noisy, q1, q2 = (_cat(out, k) for k in ("noise", "noisy", "q1", "q2"))
    clipped, clamped, first = (np.abs(noise) > S.NOISE_CLIP).mean(), (np.abs(noisy) > S.MAX_ACTION).mean(), (q1 < q2).mean()
    print("SETTARGETS %s | noise clipped %.3f | action clamped %.3f | critic1 smaller %.3f | critic2 smaller %.3f"
          % (case, clipped, clamped, first, (q2 < q1).mean()))
    assert clipped >= 0.10 and clamped >= 0.10
    # "the first handle's critic is the smaller one" in the order (critic1, critic2) and "the second handle's" in the order
    # (critic2, critic1) are the same entries: one of the two orders puts a >= 10 % share on each side of the kernel's minimum
    assert max(first, (q2 < q1).mean()) >= 0.10
    _, reward, done = S.inputs(*S.CASES[case])
    assert done.sum() == 2 and done.size >= 5


def test_every_mutant_moves_the_restatement_beyond_the_gpu_bound(base):
    pol, crit, ref = base
    moved = {m: 0.0 for m in S.MUTANTS}
    for case in S.CASES:
        t = _cat(ref[case], "target")
        bar = R.TOL_Q * np.abs(t).max()
        for m in S.MUTANTS:
            shift = np.abs(_cat(S.restate_case(pol, crit, *S.CASES[case], mutant=m), "target") - t).max()
            print("SETTARGETS mutant %s on %s | moves %.3e | bound %.3e" % (m, case, shift, bar))
            moved[m] = max(moved[m], shift / bar)
    assert all(v > 1.0 for v in moved.values()), moved


def test_restatement_of_done_rows_is_the_reward(base):
    for case in S.CASES:
        _, reward, done = S.inputs(*S.CASES[case])
        for n, r0, c, L, d in base[2][case]:
            rows = done[r0:r0 + c] == 1
            assert (d["target"][rows] == reward[r0:r0 + c][rows].astype(np.float64)[:, None]).all()


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sgrl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_the_chain_and_the_header_declares_it():
    so = ctypes.CDLL(_lib.build())
    names = _declared("sgrl_set.h")
    assert "sgrl_set_td_target" in names
    for n in names:
        assert hasattr(so, n), n


def test_null_handles_are_an_argument_error():
    from sgrl_amd.set_hip import _bind
    L = _lib.lib()
    _bind(L)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sgrl_set_td_target(None, None, None, p, 41, p, 3, p, p, 1.0, 0.5, 0.99, p, 1, None) == -1
    assert b"sgrl_set_td_target" in L.sgrl_set_last_error()


def test_no_cpu_fallback_without_a_device():
    if torch.cuda.is_available():
        return                  # with a device the class is what tests/test_set_targets_gpu.py runs
    from sgrl_amd.set_hip import HipSetTargets
    from sgrl_amd.set_policy import make_critic, make_policy
    with pytest.raises(_lib.SgrlError, match="no CPU fallback"):
        HipSetTargets(make_policy(device="cpu"), make_critic(device="cpu"))


class _StubHandle(object):
    """Stands for the device-side target object: refuses to be copied or pickled, as a ctypes pointer does."""

    def __reduce_ex__(self, protocol):
        raise TypeError("a device handle must not travel with the agent")


def _batch(B, L, seed):
    from oracle.formula import scripted_batch
    return {k: torch.from_numpy(v) for k, v in scripted_batch(L, B, seed).items()}


def test_cpu_agent_with_the_switch_is_the_agent_without_it():
    from sgrl_amd import td3
    from sgrl_amd.td3 import Agent, default_train_args
    assert td3.SET_HIP_TARGETS_DEFAULT is False
    gd = R.graph_dict("3d_walker_7_full")
    B, L = 4, R.num_limbs("3d_walker_7_full")
    batch = _batch(B, L, 5)
    noise = torch.from_numpy(np.random.RandomState(6).standard_normal((B, 3 * L)).astype(np.float32)) * 0.4
    got, agents = [], []
    for flag in (True, False, None):
        torch.manual_seed(1)
        agent = Agent(default_train_args(), set_hip_targets=flag)
        assert agent.use_set_hip == bool(flag)
        agent.change_morphology(gd)
        got.append(agent.update_targets(batch, noise))
        assert agent._targets is None and agent.actor_target._hip is None and agent.critic_target._hip is None
        agents.append(agent)
    for r, t in got[1:]:
        assert torch.equal(r, got[0][0]) and torch.equal(t, got[0][1])
    on, off = agents[0], agents[1]
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    assert not any("hip" in k or "targets" in k for k in on.state_dict())
    # the switch also comes from args; use_hip=False keeps it off
    assert Agent(default_train_args(set_hip_targets=True)).use_set_hip
    assert not Agent(default_train_args(set_hip_targets=True), set_hip_targets=False).use_set_hip
    assert not Agent(default_train_args(), use_hip=False, set_hip_targets=True).use_set_hip
    # the target object never travels with the agent
    on._targets = _StubHandle()
    on.actor.clear_buffer()
    on.actor_target.clear_buffer()
    for twin in (copy.deepcopy(on), pickle.loads(pickle.dumps(on))):
        assert twin._targets is None and twin.use_set_hip
    assert isinstance(on._targets, _StubHandle)


def test_other_agent_types_ignore_the_switch():
    from sgrl_amd.td3 import Agent, default_train_args
    agent = Agent(default_train_args(actor_type="swat", critic_type="swat"), set_hip_targets=True)
    assert not agent.use_set_hip and agent._targets is None
    mixed = Agent(default_train_args(actor_type="swat", critic_type="set"), set_hip_targets=True)
    assert not mixed.use_set_hip
