"""sgrl_explore_actions on the GPU (include/sgrl_explore.h, sgrl_amd/csrc/explore_actions.hip) against the NumPy restatement of
tests/explore_restate.py, then Rollout(device_noise=True) and DeviceTrainer(device_noise=True).

Shapes, the smallest at which the kernel can still go wrong: 70 rows in three groups with 9, 21 and 42 live slots of act_max = 42
(twelve workgroups of six rows, row boundaries inside a wavefront, element pairs across row ends), ld_in = 42 and ld_out = 48,
env_id_base = 1000003, two steps and two seeds, one of each above 2^32.  Tolerance: 1e-6 absolute at std <= 1, the project's
tolerance for this formula (tests/test_replay_sample_gpu.py: the noise to float32 rounding); no element is excluded."""
import ctypes

import numpy as np
import pytest
import torch

from sgrl_amd import _lib
from tests.explore_restate import GAUSS, UNIFORM, explore_actions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, ACT, LD_IN, LD_OUT, BASE = 70, 42, 42, 48, 1000003
LIVE = np.repeat([9, 21, 42], [24, 23, 23]).astype(np.int32)
MASK = np.arange(ACT)[None, :] < LIVE[:, None]
SEEDS = (1, 0xDEADBEEFCAFEF00D)
STEPS = (3, 2 ** 32 + 5)
NAN, INF = float("nan"), float("inf")
TOL = 1e-6
POLICY = np.random.RandomState(0).uniform(-1, 1, (N, ACT)).astype(np.float32)
_refs = {}


def _ref(seed, step, mode, std, lo=-1.0, hi=1.0):
    """The restatement at the shapes above (computed once, shared, never written)."""
    key = (seed, step, mode, std, lo, hi)
    if key not in _refs:
        _refs[key] = explore_actions(POLICY, LIVE, ACT, BASE, seed, step, mode, std, lo, hi)
        _refs[key].setflags(write=False)
    return _refs[key]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _call(policy, out, act_len, seed, step, mode, std, n_env=None, act_max=ACT, base=BASE, ld_in=None, ld_out=None, lo=-1.0, hi=1.0):
    L = _lib.bind_explore(_lib.lib())
    stride = lambda t: int(t.stride(0)) if t is not None else 0
    return L.sgrl_explore_actions(_vp(policy), stride(policy) if ld_in is None else ld_in, _vp(out), stride(out) if ld_out is None else ld_out,
                                  _vp(act_len), (N if act_len is None else int(act_len.numel())) if n_env is None else n_env,
                                  act_max, base, seed, step, mode, std, lo, hi,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _inputs():
    return torch.from_numpy(POLICY).to(DEV), torch.full((N, LD_OUT), NAN, device=DEV), torch.from_numpy(LIVE).to(DEV)


def _check_frame(got):
    """Padding slots exactly 0, columns act_max .. ld_out-1 still NaN."""
    assert (got[:, :ACT][~MASK] == 0).all()
    assert np.isnan(got[:, ACT:]).all()


@pytest.mark.parametrize("std", [1.0, 0.126])
def test_gauss_equals_the_restatement(std):
    policy, out, act_len = _inputs()
    assert policy.stride(0) == LD_IN
    for seed in SEEDS:
        for step in STEPS:
            out.fill_(NAN)
            assert _call(policy, out, act_len, seed, step, GAUSS, std) == 0
            got = out.cpu().numpy()
            ref = _ref(seed, step, GAUSS, std)
            err = float(np.abs(got[:, :ACT] - ref).max())
            print("seed %x step %d std %g: max |kernel - restatement| = %.3e" % (seed, step, std, err))
            assert err <= TOL, (seed, step, err)
            _check_frame(got)
            assert (np.abs(got[:, :ACT]) <= 1).all()
            # what the clamp pins is the bound itself, not a neighbour of it
            free = _ref(seed, step, GAUSS, std, -INF, INF)
            up, down = MASK & (free > 1 + TOL), MASK & (free < -1 - TOL)
            assert (got[:, :ACT][up] == 1).all() and (got[:, :ACT][down] == -1).all()
            if std == 1.0:
                assert up.any() and down.any()
    assert torch.equal(policy, torch.from_numpy(POLICY).to(DEV))          # the input is only read


def test_uniform_equals_the_restatement_and_reads_no_policy():
    _, out, act_len = _inputs()
    for seed in SEEDS:
        for step in STEPS:
            out.fill_(NAN)
            assert _call(None, out, act_len, seed, step, UNIFORM, 0.0) == 0
            got = out.cpu().numpy()
            ref = _ref(seed, step, UNIFORM, 0.0)
            err = float(np.abs(got[:, :ACT] - ref).max())
            print("seed %x step %d: max |kernel - restatement| = %.3e" % (seed, step, err))
            assert err <= TOL, (seed, step, err)
            _check_frame(got)
            assert (got[:, :ACT][MASK] != 0).all()
    # another range: the affine map, not a clamp
    out.fill_(NAN)
    assert _call(None, out, act_len, 1, 3, UNIFORM, 0.0, lo=0.25, hi=3.0) == 0
    got = out.cpu().numpy()
    assert float(np.abs(got[:, :ACT] - _ref(1, 3, UNIFORM, 0.0, 0.25, 3.0)).max()) <= TOL
    assert (got[:, :ACT][MASK] >= 0.25).all() and (got[:, :ACT][MASK] <= 3.0).all()
    # a row wider than a workgroup (one workgroup's threads stride over it), with an odd width and an odd base
    wide, n = 601, 3
    live = torch.tensor([601, 300, 1], dtype=torch.int32, device=DEV)
    big = torch.full((n, wide + 2), NAN, device=DEV)
    assert _call(None, big, live, 1, 3, UNIFORM, 0.0, act_max=wide, base=7) == 0
    got = big.cpu().numpy()
    ref = explore_actions(None, live.cpu().numpy(), wide, 7, 1, 3, UNIFORM, 0.0, -1.0, 1.0)
    assert float(np.abs(got[:, :wide] - ref).max()) <= TOL and np.isnan(got[:, wide:]).all()


def test_argument_errors_launch_nothing():
    policy, out, act_len = _inputs()
    L = _lib.bind_explore(_lib.lib())
    cases = [dict(out=None), dict(act_len=None), dict(policy=None), dict(ld_in=41), dict(ld_out=41), dict(n_env=-1), dict(act_max=0),
             dict(mode=2), dict(std=-0.5), dict(lo=1.0, hi=-1.0), dict(base=-1), dict(base=2 ** 33 // ACT)]
    for kw in cases:
        a = dict(policy=policy, out=out, act_len=act_len, seed=1, step=0, mode=GAUSS, std=0.2)
        a.update(kw)
        assert _call(**a) == -1, kw                    # SGRL_ERR_ARG
        assert b"sgrl_explore_actions" in L.sgrl_explore_last_error()
    assert _call(policy, out, act_len, 1, 0, GAUSS, 0.2, n_env=0) == 0      # nothing to do: success, no launch
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert _call(policy, out, act_len, 1, 0, GAUSS, 0.2) == 0               # the same call with nothing wrong
    assert float(np.abs(out.cpu().numpy()[:, :ACT] - explore_actions(POLICY, LIVE, ACT, BASE, 1, 0, GAUSS, 0.2, -1.0, 1.0)).max()) <= TOL
    assert L.sgrl_explore_actions_launches() == 1


@pytest.mark.parametrize("mode", [GAUSS, UNIFORM])
def test_in_place_and_row_slices_are_bit_equal(mode):
    policy, out, act_len = _inputs()
    seed, step, std = SEEDS[1], STEPS[1], 0.5
    assert _call(policy, out, act_len, seed, step, mode, std) == 0
    # out == policy_act: every element is read and written by the same thread
    same = torch.full((N, LD_OUT), NAN, device=DEV)
    same[:, :ACT] = policy
    assert _call(same, same, act_len, seed, step, mode, std) == 0
    assert torch.equal(same[:, :ACT], out[:, :ACT]) and bool(torch.isnan(same[:, ACT:]).all())
    # rows [a, b) of the call above from a call of their own that starts at environment BASE + a
    a, b = 5, 23
    part = torch.full((b - a, LD_OUT), NAN, device=DEV)
    assert _call(policy[a:b], part, act_len[a:b], seed, step, mode, std, base=BASE + a) == 0
    assert torch.equal(part[:, :ACT], out[a:b, :ACT])
    # ... and from a call with env_id_base = 0 that computes every row below them as well (7 rows here: the slice, not 1000003 rows)
    lead = torch.full((b, LD_OUT), NAN, device=DEV)
    low = torch.full((b - a, LD_OUT), NAN, device=DEV)
    assert _call(policy[:b], lead, act_len[:b], seed, step, mode, std, base=0) == 0
    assert _call(policy[a:b], low, act_len[a:b], seed, step, mode, std, base=a) == 0
    assert torch.equal(low[:, :ACT], lead[a:b, :ACT])
    assert not torch.equal(low[:, :ACT], part[:, :ACT])


# ---- Rollout ----------------------------------------------------------------------------------------------------------------------------
NAMES = ["3d_hopper_3_shin", "3d_walker_7_full", "3d_cheetah_14_full"]
LIMBS = [3, 7, 14]


def _live(limbs, per):
    return np.repeat([3 * L for L in limbs], per).astype(np.int32)


def test_rollout_with_device_noise():
    from oracle.formula import apply_formula_
    from sgrl_amd.rollout import Rollout
    from sgrl_amd.set_policy import make_policy
    seed, rank, per = 5, 1, 4
    pol = make_policy(device=DEV).eval()
    apply_formula_(pol)
    ro = Rollout(NAMES, per, policy=pol, seed=seed, device=DEV, rank=rank, device_noise=True)
    n, amax = ro.env.num_envs, ro.env.action_max_len
    assert (n, amax) == (12, 42) and list(ro.env.num_limbs) == LIMBS
    live = _live(LIMBS, per)
    assert ro.act_len.dtype == torch.int32 and np.array_equal(ro.act_len.cpu().numpy(), live)
    assert ro.noise_seed == seed and ro.noise_step == 0
    gen0 = ro.gen.get_state().clone()
    ro.reset()
    pa = ro.policy_forward().clone()
    a = ro.explore_into(ro.policy_actions, 0.126)
    assert a is ro.actions and ro.noise_step == 1
    assert torch.equal(ro.policy_actions, pa)                               # read, not written
    ref = explore_actions(pa.cpu().numpy(), live, amax, rank * n, seed, 0, GAUSS, 0.126, -1.0, 1.0)
    assert float(np.abs(a.cpu().numpy() - ref).max()) <= TOL
    moved = np.abs(a.cpu().numpy() - pa.cpu().numpy())[np.arange(amax)[None, :] < live[:, None]] > 0
    assert moved.mean() > 0.9                                               # noise was added (an output already at a bound may stay there)
    u = ro.random_actions()
    assert u is ro.actions and ro.noise_step == 2
    ref = explore_actions(None, live, amax, rank * n, seed, 1, UNIFORM, 0.0, -1.0, 1.0)
    assert float(np.abs(u.cpu().numpy() - ref).max()) <= TOL
    # in place on the rollout's own action tensor, at the step the counter says
    ro.noise_step = 2 ** 32 + 5
    ro.actions.copy_(pa)
    ro.explore_into(ro.actions, 1.0)
    ref = explore_actions(pa.cpu().numpy(), live, amax, rank * n, seed, 2 ** 32 + 5, GAUSS, 1.0, -1.0, 1.0)
    assert float(np.abs(ro.actions.cpu().numpy() - ref).max()) <= TOL and ro.noise_step == 2 ** 32 + 6
    assert torch.equal(ro.gen.get_state(), gen0)                            # the torch generator is not consulted
    with pytest.raises(_lib.SgrlError, match="policy_actions"):
        ro.explore_into(pa.double(), 0.126)
    with pytest.raises(_lib.SgrlError, match="policy_actions"):
        ro.explore_into(pa[:, :10], 0.126)
    assert ro.noise_step == 2 ** 32 + 6


def test_rollout_without_the_flag_draws_from_its_generator_as_before():
    from sgrl_amd.rollout import Rollout
    seed, rank, per = 5, 1, 4
    ro = Rollout(NAMES, per, seed=seed, device=DEV, rank=rank)
    n, amax = ro.env.num_envs, ro.env.action_max_len
    assert ro.device_noise is False and ro.act_len is None
    mask = torch.from_numpy((np.arange(amax)[None, :] < _live(LIMBS, per)[:, None]).astype(np.float32)).to(DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed * 1000003 + rank)
    want_u = torch.zeros((n, amax), device=DEV).uniform_(-1.0, 1.0, generator=gen) * mask
    got_u = ro.random_actions().clone()
    assert torch.equal(got_u, want_u)
    x = torch.from_numpy(np.random.RandomState(2).uniform(-1, 1, (n, amax)).astype(np.float32)).to(DEV)
    want_g = (x + torch.randn(x.shape, device=DEV, generator=gen) * 0.126).clamp_(-1.0, 1.0) * mask
    assert torch.equal(ro.add_exploration_noise(x, 0.126), want_g)
    assert torch.equal(ro.gen.get_state(), gen.get_state()) and ro.noise_step == 0
    with pytest.raises(_lib.SgrlError, match="device_noise"):
        ro.explore_into(x, 0.126)


# ---- DeviceTrainer ----------------------------------------------------------------------------------------------------------------------
def test_trainer_with_device_noise():
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names, limbs, per, seed = NAMES[:2], LIMBS[:2], 4, 3
    args = default_train_args(max_episode_steps=30)
    tr = DeviceTrainer(names, [per, per], args=args, seed=seed, device=DEV, max_buffer_size=256, batch_size=16, device_noise=True)
    assert tr.device_noise is True and tr.ro.device_noise is True and tr.ro.noise_step == 0
    amax, live = tr.ro.env.action_max_len, _live(limbs, per)
    gen0 = tr.ro.gen.get_state().clone()

    def step_and_check(step):
        tr.collect_step()
        pa, a = tr.ro.policy_actions.cpu().numpy(), tr.ro.actions.cpu().numpy()      # the actor's output, what the engine was handed
        ref = explore_actions(pa, live, amax, 0, seed, step, GAUSS, args.expl_noise, -1.0, 1.0)
        err = float(np.abs(a - ref).max())
        print("step %d: max |actions - restatement| = %.3e" % (step, err))
        assert err <= TOL, (step, err)
        assert tr.ro.noise_step == step + 1
    for t in range(3):
        step_and_check(t)
    tr.tot_env_steps = 500                                                 # a resumed run: the step number restarts at the restored count
    assert tr.ro.noise_step == 500 and tr.draw == 500
    step_and_check(500)
    # warm-up actions take the next step number on their own stream
    tr.collect_step(random_actions=True)
    ref = explore_actions(None, live, amax, 0, seed, 501, UNIFORM, 0.0, -1.0, 1.0)
    assert float(np.abs(tr.ro.actions.cpu().numpy() - ref).max()) <= TOL and tr.ro.noise_step == 502
    assert torch.equal(tr.ro.gen.get_state(), gen0)                         # the torch generator is not consulted
    # the evaluation rollouts never add noise and are built without the flag
    tr.evaluate(num_eval_trajectories=1, max_trajectory_length=2)
    assert all(entry[1].device_noise is False for entry in tr.eval_rollouts.values())


def test_trainer_without_the_flag_keeps_the_tensor_op_path():
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    tr = DeviceTrainer(NAMES[:2], [4, 4], args=default_train_args(max_episode_steps=30), seed=3, device=DEV, max_buffer_size=256,
                       batch_size=16)
    assert tr.device_noise is False and tr.ro.device_noise is False
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3 * 1000003)
    tr.collect_step()
    pa = tr.ro.policy_actions
    want = (pa + torch.randn(pa.shape, device=DEV, generator=gen) * tr.args.expl_noise).clamp_(-1.0, 1.0) * tr.ro.act_mask
    assert torch.equal(tr.ro.actions, want) and tr.ro.noise_step == 0
