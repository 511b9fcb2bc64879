"""The step kernel on the packer's derived constants (include/sgrl_model.h geom_axis, pair_rowc, jnt_rowc; csrc/step_body.h),
on the device against the CPU oracle, which reads none of them.  Three environments per walker variant -- each light variant
steps one pair on a shared wavefront (csrc/wave_half.h) and one environment alone -- plus one humanoid_9 and one cheetah_14.

Tolerances and flag checks are those of tests/test_parity_matrix_gpu.py: 1e-9 relative per teacher-forced step (1e-7 cheetah),
1e-6 relative free-running; done flags, counters and padding exact; no dropped rows; and the solver diagnostics of every step
(cnt[3]) report no block-pivot failure."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import WALKERS

pytestmark = pytest.mark.gpu

_POOL = ThreadPoolExecutor(max_workers=16)     # the oracle is a C library called through ctypes: the GIL is released


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _make(names, per, seed=5):
    from sgrl_amd.vec_env import BatchedModularVecEnv
    env = BatchedModularVecEnv(names, per, seed=seed, device="cuda:0")
    env.enable_f64_outputs()
    return env


def _oracle_envs(env, seed):
    from oracle import physics_ref
    out = []
    for i in range(env.num_envs):
        ib, fb = env._blobs[env.env_morph[i]]      # the very blobs the engine was created with
        out.append(physics_ref.OracleEnv(physics_ref.OracleModel(ib, fb), seed=seed, env_id=i))
    return out


def _teacher_forced(env, oes, steps, rng, tol_of):
    """Every step starts from the oracle's state (sgrl_set_records): errors cannot accumulate."""
    torch = _torch()
    for t in range(steps):
        rec, cnt = env.get_records()
        for i, oe in enumerate(oes):
            m = env.models[env.env_morph[i]]
            rec[i, :m.nq] = oe.qpos
            rec[i, m.nq:m.nq + m.nv] = oe.qvel
            rec[i, m.nq + m.nv:m.nq + m.nv + 2] = oe.torso_xy_stale
            rec[i, m.nq + m.nv + 2:m.nq + m.nv + 4] = oe.target
            cnt[i, 0], cnt[i, 1] = oe.counters[0], oe.counters[1]
        env.set_records(rec, cnt)
        a = rng.uniform(-1, 1, size=(env.num_envs, env.action_max_len)).astype(np.float32)
        env.step_device(torch.from_numpy(a).cuda(), auto_reset=False)
        torch.cuda.synchronize()
        obs, rew = env.obs64.cpu().numpy(), env.rew64.cpu().numpy()
        done, dist = env.done.cpu().numpy(), env.dist.cpu().numpy()
        rec2, cnt2 = env.get_records()
        ods = list(_POOL.map(lambda ia: ia[1].step(a[ia[0]].astype(np.float64), auto_reset=False), enumerate(oes)))
        for i, oe in enumerate(oes):
            o, r, d, info = ods[i]
            tol = tol_of(i)
            q, v, xy, tg = env.state_of(rec2, i)
            assert np.abs(q - oe.qpos).max() < tol * (1 + np.abs(oe.qpos).max()), (i, t)
            assert np.abs(v - oe.qvel).max() < tol * (1 + np.abs(oe.qvel).max()), (i, t)
            assert np.abs(obs[i, :o.size] - o).max() < tol * (1 + np.abs(o).max()), (i, t)
            assert (obs[i, o.size:] == 0).all()
            assert abs(rew[i] - r) < tol * 100 * (1 + abs(r)), (i, t)
            assert bool(done[i]) == d, (i, t)
            assert abs(dist[i] - info["dist"]) < 1e-3 * (1 + info["dist"])
            assert cnt2[i, 2] == 0, "constraint rows dropped"
            assert (int(cnt2[i, 3]) >> 8) & 255 == 0, "block pivoting gave up"
            if d:
                oe.counters[1] += 1
                oe.reset()


def test_walker_variants_three_each_teacher_forced_then_free():
    torch = _torch()
    env = _make(WALKERS, 3)
    assert env.num_envs == 24
    assert env.fixed_dim_groups > 0 and env.paired_envs >= 2      # the walker family kernel, pairs among the light variants
    env.reset_device()
    oes = _oracle_envs(env, 5)
    for oe in oes:
        oe.reset()
    rng = np.random.RandomState(0)
    _teacher_forced(env, oes, 30, rng, lambda i: 1e-9)
    # ... then 100 free steps from where the last forced step left both sides (auto-reset on, same counter RNG)
    rec, cnt = env.get_records()
    for i, oe in enumerate(oes):
        m = env.models[env.env_morph[i]]
        rec[i, :m.nq] = oe.qpos
        rec[i, m.nq:m.nq + m.nv] = oe.qvel
        rec[i, m.nq + m.nv:m.nq + m.nv + 2] = oe.torso_xy_stale
        rec[i, m.nq + m.nv + 2:m.nq + m.nv + 4] = oe.target
        cnt[i, 0], cnt[i, 1] = oe.counters[0], oe.counters[1]
    env.set_records(rec, cnt)
    worst = 0.0
    for t in range(100):
        a = rng.uniform(-1, 1, size=(env.num_envs, env.action_max_len)).astype(np.float32)
        env.step_device(torch.from_numpy(a).cuda())
        ods = list(_POOL.map(lambda ia: ia[1].step(a[ia[0]].astype(np.float64)), enumerate(oes)))
        if t % 10 == 9:
            torch.cuda.synchronize()
            done = env.done.cpu().numpy()
            rec, cnt = env.get_records()
            for i, oe in enumerate(oes):
                q, v, xy, tg = env.state_of(rec, i)
                assert cnt[i, 1] == oe.counters[1] and cnt[i, 0] == oe.counters[0], (i, t)
                assert bool(done[i]) == ods[i][2], (i, t)
                assert cnt[i, 2] == 0, "constraint rows dropped"
                assert (int(cnt[i, 3]) >> 8) & 255 == 0, "block pivoting gave up"
                eq = np.abs(q - oe.qpos).max() / (1 + np.abs(oe.qpos).max())
                ev = np.abs(v - oe.qvel).max() / (1 + np.abs(oe.qvel).max())
                worst = max(worst, eq, ev)
    print("walkers x 3, 100 free steps: worst relative deviation %.2e" % worst)
    assert worst < 1e-6
    env.close()


def test_humanoid_9_and_cheetah_14_teacher_forced():
    names = ["3d_humanoid_9_full", "3d_cheetah_14_full"]
    env = _make(names, 1)
    env.reset_device()
    oes = _oracle_envs(env, 5)
    for oe in oes:
        oe.reset()
    _teacher_forced(env, oes, 30, np.random.RandomState(0), lambda i: 1e-7 if "cheetah" in names[env.env_morph[i]] else 1e-9)
    env.close()
