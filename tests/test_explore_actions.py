"""The exploration noise and the warm-up actions of include/sgrl_explore.h on the restatement of tests/explore_restate.py: it is the
replay noise's definition on other stream tags, a row depends on its global environment number alone, the draws are standard normal
/ uniform, the clamp and the padding hold; then the host side of the library: the header's names are exported, one launch, every
argument error comes back without a device, there is no CPU fallback.  tests/test_explore_actions_gpu.py holds the kernel to the
restatement."""
import ctypes

import numpy as np
import pytest
import torch

from sgrl_amd import _lib
from tests import test_replay_sample as rs
from tests.explore_restate import GAUSS, UNIFORM, explore_actions
from tests.test_replay_sample import _declared, draw_noise, stream_words

INF = float("inf")
GAUSS_SEED, UNIFORM_SEED = 11, 12      # committed: the restatement itself satisfies the distribution bounds below with these seeds


def _full(n, act_max):
    return np.full(n, act_max, dtype=np.int64)


# ---- one definition, two tags ---------------------------------------------------------------------------------------------------------
def test_gauss_is_the_replay_noise_formula_on_stream_two(monkeypatch):
    k, act = 37, 45
    for seed, step, std in ((11, 4, 1.0), (0xDEADBEEFCAFEF00D, 2 ** 32 + 5, 0.2)):
        got = explore_actions(np.zeros((k, act), np.float32), _full(k, act), act, 0, seed, step, GAUSS, std, -INF, INF)
        on_one = draw_noise(k, act, seed, step, std)
        # draw_noise itself, reading stream 2 wherever it asks for stream 1
        monkeypatch.setattr(rs, "stream_words", lambda s, d, stream, start, count: stream_words(s, d, 2 if stream == 1 else stream, start, count))
        on_two = draw_noise(k, act, seed, step, std)
        monkeypatch.undo()
        assert got.dtype == np.float32 and np.array_equal(got, on_two)
        assert not np.array_equal(on_one, on_two)


def test_the_four_stream_tags_share_no_words():
    w = [stream_words(7, 3, tag, 0, 4096) for tag in range(4)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert (w[a] == w[b]).mean() < 0.01, (a, b)
    # warm-up and exploration at one step number are different draws: the uniform is the affine map of stream 3's u1, not stream 2's
    act = 42
    u = explore_actions(None, _full(8, act), act, 0, 7, 3, UNIFORM, 0.0, 0.0, 1.0)
    for tag, same in ((3, True), (2, False)):
        u1 = ((w[tag][:2 * 8 * act:2].astype(np.float64) + 0.5) / 4294967296.0).astype(np.float32).reshape(8, act)
        assert np.array_equal(u, u1) == same, tag


# ---- row independence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [GAUSS, UNIFORM])
def test_a_row_depends_on_its_global_number_alone(mode):
    n, act, a, b = 70, 42, 5, 23
    rng = np.random.RandomState(0)
    pol = rng.uniform(-1, 1, (n, act)).astype(np.float32)
    live = np.array([9, 21, 42])[np.arange(n) % 3]
    whole = explore_actions(pol, live, act, 0, 5, 9, mode, 0.5, -1.0, 1.0)
    part = explore_actions(pol[a:b], live[a:b], act, a, 5, 9, mode, 0.5, -1.0, 1.0)
    assert np.array_equal(whole[a:b], part)
    # an odd base times an odd width: the rows start on the second half of a block
    odd = explore_actions(pol[:, :41], np.minimum(live, 41), 41, 3, 5, 9, mode, 0.5, -1.0, 1.0)
    assert np.array_equal(odd[4:9], explore_actions(pol[4:9, :41], np.minimum(live, 41)[4:9], 41, 7, 5, 9, mode, 0.5, -1.0, 1.0))
    # another step, another seed: every live element moves (unclamped, so that no two are pinned to the same bound)
    lo, hi = (-INF, INF) if mode == GAUSS else (-1.0, 1.0)
    base = explore_actions(pol, live, act, 0, 5, 9, mode, 0.5, lo, hi)
    mask = np.arange(act)[None, :] < live[:, None]
    for seed, step in ((5, 10), (6, 9), (5, 9 + 2 ** 32), (5 + 2 ** 32, 9)):
        other = explore_actions(pol, live, act, 0, seed, step, mode, 0.5, lo, hi)
        assert (other[mask] != base[mask]).all(), (seed, step)
        assert (other[~mask] == 0).all()


# ---- distribution -----------------------------------------------------------------------------------------------------------------------
def test_gauss_draws_are_standard_normal():
    n, act = 256, 45
    z = explore_actions(np.zeros((n, act), np.float32), _full(n, act), act, 1000003, GAUSS_SEED, 4, GAUSS, 1.0, -INF, INF)
    print("mean %.5f std %.5f over %d" % (z.mean(), z.std(), z.size))
    assert abs(float(z.mean())) < 5 / np.sqrt(z.size) and abs(float(z.std()) - 1.0) < 5 / np.sqrt(2 * z.size)
    scaled = explore_actions(np.zeros((n, act), np.float32), _full(n, act), act, 1000003, GAUSS_SEED, 4, GAUSS, 0.126, -INF, INF)
    assert np.array_equal(scaled, z * np.float32(0.126))


@pytest.mark.parametrize("lo, hi", [(-1.0, 1.0), (0.25, 3.0)])
def test_uniform_draws_lie_in_the_range_with_the_mean_at_its_midpoint(lo, hi):
    n, act = 256, 45
    u = explore_actions(None, _full(n, act), act, 1000003, UNIFORM_SEED, 4, UNIFORM, 0.0, lo, hi)
    se = (hi - lo) / np.sqrt(12.0 * u.size)                # standard error of the mean of U(lo, hi)
    print("min %.6f max %.6f mean %.5f (5 se = %.5f)" % (u.min(), u.max(), u.mean(), 5 * se))
    assert u.dtype == np.float32 and (u >= lo).all() and (u < hi).all()
    assert abs(float(u.mean(dtype=np.float64)) - 0.5 * (lo + hi)) < 5 * se


# ---- clamp and padding ------------------------------------------------------------------------------------------------------------------
def test_clamp_and_padding():
    n, act = 70, 42
    rng = np.random.RandomState(1)
    pol = rng.uniform(-1, 1, (n, act)).astype(np.float32)
    live = np.repeat([9, 21, 42], [24, 23, 23])
    mask = np.arange(act)[None, :] < live[:, None]
    out = explore_actions(pol, live, act, 1000003, 3, 2, GAUSS, 1.0, -1.0, 1.0)
    assert (np.abs(out) <= 1).all() and (out[~mask] == 0).all()
    free = explore_actions(pol, live, act, 1000003, 3, 2, GAUSS, 1.0, -INF, INF)
    assert (out[mask & (free > 1)] == 1).all() and (out[mask & (free < -1)] == -1).all()
    assert (mask & (free > 1)).any() and (mask & (free < -1)).any()
    inside = mask & (np.abs(free) <= 1)
    assert np.array_equal(out[inside], free[inside]) and inside.any()
    uni = explore_actions(None, live, act, 1000003, 3, 2, UNIFORM, 0.0, -1.0, 1.0)
    assert (np.abs(uni) <= 1).all() and (uni[~mask] == 0).all() and (uni[mask] != 0).all()


# ---- header and library -----------------------------------------------------------------------------------------------------------------
def test_library_exports_every_name_the_header_declares():
    so = ctypes.CDLL(_lib.build())
    names = _declared("sgrl_explore.h")
    assert names == ["sgrl_explore_actions", "sgrl_explore_actions_launches", "sgrl_explore_last_error"]
    for n in names:
        assert hasattr(so, n), n
    assert "explore_actions.hip" in _lib.SOURCES
    # bound by _lib.bind_explore: sgrl.h and _lib.EXPORTS do not list them
    assert not set(names) & set(_lib.EXPORTS) and not set(names) & set(_declared("sgrl.h"))


def _host_call():
    L = _lib.bind_explore(_lib.lib())
    buf = (ctypes.c_float * (4 * 8))()
    lens = (ctypes.c_int32 * 4)(3, 6, 6, 3)
    p, pl = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p)

    def call(policy=p, ld_in=8, out=p, ld_out=8, act_len=pl, n_env=4, act_max=6, base=0, mode=GAUSS, std=0.2, lo=-1.0, hi=1.0):
        return L.sgrl_explore_actions(policy, ld_in, out, ld_out, act_len, n_env, act_max, base, 1, 0, mode, std, lo, hi, None)
    return L, call, buf


ARG_ERRORS = [dict(out=None), dict(act_len=None), dict(policy=None), dict(ld_in=5), dict(ld_out=5), dict(mode=UNIFORM, ld_out=5), dict(n_env=-1),
              dict(act_max=0), dict(act_max=-6), dict(mode=2), dict(mode=-1), dict(std=-0.5), dict(lo=1.0, hi=-1.0), dict(base=-1),
              dict(base=2 ** 33 // 6 + 1 - 4), dict(base=2 ** 33), dict(base=2 ** 62), dict(n_env=0, base=2 ** 33 // 6 + 1)]


def test_launch_count_and_argument_errors_need_no_device():
    L, call, buf = _host_call()
    assert L.sgrl_explore_actions_launches() == 1
    for kw in ARG_ERRORS:
        assert call(**kw) == -1, kw                    # SGRL_ERR_ARG
        assert b"sgrl_explore_actions" in L.sgrl_explore_last_error(), kw
    # nothing to do is not an error, and the last block number that fits is accepted as far as the arguments go
    assert call(n_env=0) == 0
    assert call(n_env=0, policy=None, ld_in=0, mode=UNIFORM) == 0
    assert call(n_env=0, base=2 ** 33 // 6) == 0       # 1431655765 rows of 6 slots end below 2^33 elements
    assert all(v == 0 for v in buf)


def test_no_cpu_fallback_without_a_device():
    from sgrl_amd.rollout import Rollout
    with pytest.raises(_lib.SgrlError, match="no CPU fallback"):
        Rollout(["3d_hopper_3_shin"], 2, seed=1, device="cpu", device_noise=True)
    if torch.cuda.is_available():
        return                          # the library call below is the no-device case
    L, call, buf = _host_call()
    assert call() == -3                 # SGRL_ERR_HIP
    assert b"no CPU fallback" in L.sgrl_explore_last_error()
    assert all(v == 0 for v in buf)
