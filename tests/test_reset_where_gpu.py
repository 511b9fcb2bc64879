"""The engine's partial reset (include/sgrl.h sgrl_reset_where, BatchedModularVecEnv.reset_where): selected environments get exactly
the in-step auto-reset, unselected ones are neither read nor written, and a step with auto_reset=False followed by
reset_where(done) leaves the engine where the fused step leaves it -- with the true post-step observation in between.

3d_hopper_3_shin steps two environments to a wavefront: an even and an odd count.  Records, counters and float64 observations
throughout (enable_f64_outputs)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(["3d_hopper_3_shin"], 2), (["3d_hopper_3_shin"], 3), (["3d_walker_7_full"], 3), (["3d_cheetah_14_full"], 3),
         (["3d_humanoid_9_full"], 3),
         (["3d_cheetah_14_full", "3d_hopper_3_shin", "3d_humanoid_9_full", "3d_walker_7_full"], 3)]      # several launch groups
IDS = ["hopper2", "hopper3", "walker3", "cheetah3", "humanoid3", "mixed"]
SENTINEL = -777.25


def _make(names, per, seed=11, **kw):
    import torch
    from sgrl_amd.vec_env import BatchedModularVecEnv
    assert torch.cuda.is_available()
    env = BatchedModularVecEnv(names, per, seed=seed, device="cuda:0", **kw)
    env.enable_f64_outputs()
    return env


def _actions(env, g):
    import torch
    return (torch.rand((env.num_envs, env.action_max_len), device="cuda", generator=g) * 2 - 1).contiguous()


def _mid_episode_state(env, steps=5):
    """A state a few random steps into the episodes (different step counts and episode numbers would do as well): records, counters."""
    import torch
    env.reset_device()
    g = torch.Generator(device="cuda").manual_seed(2)
    for _ in range(steps):
        env.step_device(_actions(env, g))
    torch.cuda.synchronize()
    return env.get_records()


def _snapshot(env):
    import torch
    torch.cuda.synchronize()
    rec, cnt = env.get_records()
    return rec, cnt, env.obs.cpu().numpy().copy(), env.obs64.cpu().numpy().copy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("names,per", CASES, ids=IDS)
def test_all_ones_is_sgrl_reset_and_masks_touch_only_their_environments(names, per):
    """(a) reset_where(all ones) against reset_device() of a twin from the same records and counters: bit for bit (one kernel body,
    one instantiation).  (b) masks none / one / alternating: the selected environments equal the twin's reset bit for bit; of the
    others nothing moved -- records, counters, and the sentinel written into their observation rows beforehand."""
    import torch
    twin, env = _make(names, per), _make(names, per)
    rec0, cnt0 = _mid_episode_state(twin)
    twin.set_records(rec0, cnt0)
    twin.reset_device()
    r_ref, c_ref, o_ref, o64_ref = _snapshot(twin)
    assert (c_ref[:, 0] == 0).all() and (c_ref[:, 1] == cnt0[:, 1] + 1).all() and (cnt0[:, 0] > 0).any()
    n = env.num_envs
    masks = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "one": np.arange(n) == n - 1, "alternating": np.arange(n) % 2 == 0}
    for key, mask in masks.items():
        env.set_records(rec0, cnt0)
        env.obs.fill_(SENTINEL)
        env.obs64.fill_(SENTINEL)
        m = torch.from_numpy(mask).cuda()
        out = env.reset_where(m if key != "alternating" else m.to(torch.uint8))      # bool and uint8 masks both
        assert out is env.obs
        rec, cnt, o, o64 = _snapshot(env)
        sel, rest = np.flatnonzero(mask), np.flatnonzero(~mask)
        assert _same_bits(rec[sel], r_ref[sel]) and _same_bits(cnt[sel], c_ref[sel]), key
        assert _same_bits(o[sel], o_ref[sel]) and _same_bits(o64[sel], o64_ref[sel]), key
        assert _same_bits(rec[rest], rec0[rest]) and _same_bits(cnt[rest], cnt0[rest]), key
        assert (o[rest] == np.float32(SENTINEL)).all() and (o64[rest] == SENTINEL).all(), key
    twin.close()
    env.close()


def _topple(env, which):
    """Lay the environments `which` on their side, at rest, 5 cm above the floor: their next step ends the episode by itself."""
    import torch
    torch.cuda.synchronize()
    rec, cnt = env.get_records()
    for i in which:
        m = env.models[env.env_morph[i]]
        rec[i, 2] = 0.05
        rec[i, 3:7] = [0.70710678, 0.70710678, 0, 0]
        rec[i, m.nq:m.nq + m.nv] = 0
    env.set_records(rec, cnt)


@pytest.mark.parametrize("specs", ["1", "0"])
@pytest.mark.parametrize("names,per", CASES, ids=IDS)
def test_split_step_equals_the_fused_step(monkeypatch, names, per, specs):
    """(c) A: step(auto_reset=True).  B: step(auto_reset=False) + reset_where(done).  Same seed, same actions, time limit 7, 30
    steps: every environment is reset at least four times, at least three of them by the limit.  Uniform actions alone end no episode of these morphologies within seven
    steps (none in 144 runs over seeds when this test was written), so before steps 9 and 18 the first environment of every
    morphology is laid on its side in all three engines and terminates by itself there -- in a hopper pair, one half of the
    wavefront resets while its mate goes on: resets of both kinds occur in every case.  Flags and counters identical at every step; records and float64 observations after the last step within the bar the suite holds two instantiations of the same source
    to (test_engine_gpu.py test_fixed_dimension_kernels_agree_with_the_generic_kernel, also 30 free-running steps): in A the reset
    runs inside a fixed-dimension or half-wave kernel, in B in the generic one.  And what B shows between its two calls is the true
    post-step observation: that of C, which takes B's state before every step and never resets."""
    import torch
    monkeypatch.setenv("SGRL_SPECS", specs)
    A, B, C = (_make(names, per, max_episode_steps=7) for _ in range(3))
    assert (A.fixed_dim_groups > 0) == (specs == "1")
    for e in (A, B, C):
        e.reset_device()
    g = torch.Generator(device="cuda").manual_seed(5)
    cuts = np.zeros(A.num_envs, dtype=int)
    terminations = np.zeros(A.num_envs, dtype=int)
    firsts = [sl.start for sl in A.morph_slices]
    for t in range(30):
        a = _actions(A, g)
        if t in (9, 18):
            _topple(A, firsts)
            _topple(B, firsts)
        torch.cuda.synchronize()
        C.set_records(*B.get_records())
        A.step_device(a)
        B.step_device(a, auto_reset=False)
        C.step_device(a, auto_reset=False)
        torch.cuda.synchronize()
        done, trunc = B.done.cpu().numpy().astype(bool), B.trunc.cpu().numpy().astype(bool)
        assert _same_bits(A.done.cpu().numpy(), B.done.cpu().numpy()) and _same_bits(A.trunc.cpu().numpy(), B.trunc.cpu().numpy()), t
        assert _same_bits(B.done.cpu().numpy(), C.done.cpu().numpy()), t
        cuts += done & trunc
        terminations += done & ~trunc
        fin = np.flatnonzero(done)
        assert _same_bits(B.obs64.cpu().numpy()[fin], C.obs64.cpu().numpy()[fin]), t       # the pre-reset observation, bit for bit
        assert _same_bits(B.obs.cpu().numpy()[fin], C.obs.cpu().numpy()[fin]), t
        B.reset_where(B.done)
        torch.cuda.synchronize()
        ca, cb = A.get_counters(), B.get_counters()
        assert _same_bits(ca[:, :3], cb[:, :3]), t
    ra, rb = A.get_records()[0], B.get_records()[0]
    oa, ob = A.obs64.cpu().numpy(), B.obs64.cpu().numpy()
    print("cuts per env", cuts.tolist(), "terminations per env", terminations.tolist(),
          "max |rec diff| %.3e max |obs64 diff| %.3e" % (abs(ra - rb).max(), abs(oa - ob).max()))
    assert (cuts + terminations >= 4).all()                 # a time limit of 7 in 30 steps
    assert (cuts >= 3).all() and (terminations[firsts] >= 2).all()      # resets of both kinds really occurred, in every morphology
    assert abs(ra - rb).max() < 1e-9 * (1 + abs(ra).max()) and abs(oa - ob).max() < 1e-9 * (1 + abs(oa).max())
    for e in (A, B, C):
        e.close()


def test_argument_errors_launch_nothing():
    """(d) a null engine, mask or obs is SGRL_ERR_ARG from the library, and nothing ran; a mask of the wrong shape, dtype or device is
    a ValueError on the host."""
    import torch
    from sgrl_amd import _lib
    env = _make(["3d_hopper_3_shin"], 3)
    rec0, cnt0 = _mid_episode_state(env)
    env.obs.fill_(SENTINEL)
    env.obs64.fill_(SENTINEL)
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    mask = torch.ones(3, dtype=torch.uint8, device="cuda")
    null = ctypes.c_void_p(0)
    assert L.sgrl_reset_where(null, p(mask), p(env.obs), p(env.obs64), null) == -1
    assert L.sgrl_reset_where(env._h, null, p(env.obs), p(env.obs64), null) == -1
    assert L.sgrl_reset_where(env._h, p(mask), null, p(env.obs64), null) == -1
    assert b"sgrl_reset_where" in L.sgrl_last_error()
    for bad in (torch.ones(4, dtype=torch.bool, device="cuda"), torch.ones((3, 1), dtype=torch.bool, device="cuda"),
                torch.ones(3, dtype=torch.float32, device="cuda"), torch.ones(3, dtype=torch.int64, device="cuda"),
                torch.ones(3, dtype=torch.bool), [1, 1, 1]):
        with pytest.raises(ValueError):
            env.reset_where(bad)
    rec, cnt, o, o64 = _snapshot(env)
    assert _same_bits(rec, rec0) and _same_bits(cnt, cnt0) and (o == np.float32(SENTINEL)).all() and (o64 == SENTINEL).all()
    env.reset_where(mask)                                    # ... and with its arguments in place it runs
    rec, cnt, o, o64 = _snapshot(env)
    assert (cnt[:, 0] == 0).all() and (o64 != SENTINEL).any()
    env.close()
