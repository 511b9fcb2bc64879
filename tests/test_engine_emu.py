"""CPU-side checks of the ENGINE SOURCE (sgrl_amd/csrc/step_body.h) compiled with a serial lane emulator
(tests/emu/emu_step.cpp) against the oracle.  This is a unit test of the kernel logic in the GPU-less build
container; the GPU parity tests proper are in test_engine_gpu.py and go through the C ABI."""
import numpy as np
import pytest

import emu_ref
from helpers import packed, oracle_model
from oracle import physics_ref

NAMES = ["3d_hopper_3_shin", "3d_hopper_5_full", "3d_walker_2_right_leg_left_knee", "3d_walker_7_full",
         "3d_walker_v2_5_foot", "3d_humanoid_9_full", "3d_cheetah_14_full"]


LAYOUTS = ["dieted", "default"]      # emu_ref.set_layout: both slab layouts the device kernels compute


def _on_both_layouts(names):
    """(name, layout) cases: the dieted case keeps the id the test had when the emulator knew that layout only."""
    return pytest.mark.parametrize("name,layout", [pytest.param(n, "dieted", id=n) for n in names] +
                                   [pytest.param(n, "default", id=n + "-default") for n in names], indirect=["layout"])


@pytest.fixture
def layout(request):
    emu_ref.set_layout(request.param)
    try:
        yield request.param
    finally:
        emu_ref.set_layout("dieted")


@_on_both_layouts(NAMES)
def test_forward_dynamics_match_oracle(name, layout):
    m, ib, fb = packed(name)
    _, om = oracle_model(name)
    env = physics_ref.OracleEnv(om, seed=1)
    env.reset()
    rng = np.random.RandomState(0)
    for t in range(60):
        a = rng.uniform(-1, 1, size=3 * om.L)
        if t % 5 == 0:
            q1, _, d1 = om.forward(env.qpos, env.qvel, a[3:])
            q2, d2 = emu_ref.forward(ib, fb, env.qpos, env.qvel, a[3:])
            assert d1["nrow"] == d2["nrow"] and d1["ncon"] == d2["ncon"]
            assert np.abs(q1 - q2).max() <= 1e-9 * (1 + np.abs(q1).max())
        env.step(a)


@_on_both_layouts(NAMES)
def test_free_running_episodes_match_oracle_and_lane_order_is_irrelevant(name, layout):
    m, ib, fb = packed(name)
    _, om = oracle_model(name)
    trajs = []
    for rev in (False, True):
        emu_ref.set_reverse(rev)
        try:
            e1 = physics_ref.OracleEnv(om, seed=7, env_id=3)
            e2 = emu_ref.EmuEnv(ib, fb, seed=7, env_id=3)
            o1, o2 = e1.reset(), e2.reset()
            assert np.abs(o1 - o2).max() < 1e-13
            rng = np.random.RandomState(1)
            traj = []
            ndone = 0
            for t in range(80):
                a = rng.uniform(-1, 1, size=3 * om.L).astype(np.float32)
                o1, r1, d1, i1 = e1.step(a.astype(np.float64))
                o2, r2, d2, i2 = e2.step(a)
                assert d1 == d2
                ndone += d1
                tol = 1e-7 if "cheetah" in name else 1e-9
                assert np.abs(o1 - o2).max() < tol and abs(r1 - r2) < tol * 10
                assert abs(i1["dist"] - i2["dist"]) < 1e-2  # float32 output
                assert np.array_equal(i2["obs32"], o2.astype(np.float32))
                traj.append(o2.copy())
            trajs.append(np.array(traj))
        finally:
            emu_ref.set_reverse(False)
    # ascending vs descending lane execution must agree bit for bit (no intra-phase cross-lane dependency)
    assert np.array_equal(trajs[0], trajs[1])


def test_observation_padding_and_time_limit():
    m, ib, fb = packed("3d_walker_2_right_leg_left_knee")
    e = emu_ref.EmuEnv(ib, fb, seed=1, max_episode_steps=2, obs_max_len=287)
    o = e.reset()
    assert o.shape == (287,) and (o[82:] == 0).all() and np.abs(o[:82]).max() > 0
    z = np.zeros(21, dtype=np.float32)
    _, _, d1, i1 = e.step(z)
    _, _, d2, i2 = e.step(z)
    assert (d1, d2) == (False, True) and i2["TimeLimit.truncated"]
    assert e.cnt[0] == 0 and e.cnt[1] == 1   # auto-reset started episode 1


def test_rng_matches_oracle_bit_for_bit():
    m, ib, fb = packed("3d_cheetah_14_full")
    _, om = oracle_model("3d_cheetah_14_full")
    for env_id in (0, 5, 8191):
        e1 = physics_ref.OracleEnv(om, seed=123456789012345, env_id=env_id)
        e2 = emu_ref.EmuEnv(ib, fb, seed=123456789012345, env_id=env_id)
        e1.reset()
        e2.reset()
        assert np.array_equal(e1.target, e2.target)
        # normal draws go through libm log/cos in both builds here
        np.testing.assert_allclose(e1.qvel, e2.qvel, rtol=0, atol=1e-15)
        np.testing.assert_allclose(e1.qpos, e2.qpos, rtol=0, atol=1e-15)


@_on_both_layouts(["3d_walker_7_full", "3d_hopper_4_lower_shin"])
def test_explicit_inverse_path_and_factor_path_agree(name, layout):
    """nv <= 24: the engine source has two formulations of the mass-matrix solves (explicit L^-1 products, which the
    HIP wave policy selects, and in-place L substitutions).  Both must follow the oracle, and each other to rounding."""
    m, ib, fb = packed(name)
    _, om = oracle_model(name)
    outs = []
    for linv in (True, False):
        emu_ref.set_linv(linv)
        try:
            e1 = physics_ref.OracleEnv(om, seed=11, env_id=2)
            e2 = emu_ref.EmuEnv(ib, fb, seed=11, env_id=2)
            e1.reset(); e2.reset()
            rng = np.random.RandomState(4)
            tr = []
            for t in range(60):
                a = rng.uniform(-1, 1, size=3 * om.L).astype(np.float32)
                o1, r1, d1, _ = e1.step(a.astype(np.float64))
                o2, r2, d2, _ = e2.step(a)
                assert d1 == d2 and np.abs(o1 - o2).max() < 1e-9
                tr.append(o2.copy())
            outs.append(np.array(tr))
        finally:
            emu_ref.set_linv(True)
    assert np.abs(outs[0] - outs[1]).max() < 1e-9


# ---- contact-rich states: the slab path, the register Gauss-Seidel's dispatch and pgs_big in the one-environment emulator -----------
LYING = ["3d_humanoid_9_full", "3d_humanoid_7_left_arm", "3d_walker_7_full", "3d_hopper_5_full", "3d_cheetah_14_full"]
QUATS = [[1, 0, 0, 0], [0.70710678, 0.70710678, 0, 0], [0.70710678, 0, 0.70710678, 0]]
DEVICE_ROWS = 256      # the cap the vec-env packs with (sgrl_amd/_lib.py default_max_rows; pack_model lowers it to the geometric worst case)


def _lying_run(name, solver, pose, reverse):
    """6 teacher-forced steps from a pose lying on the floor.  Returns (observations, cnt[3] per step, step-start row counts of the
    oracle, worst relative observation error where Gauss-Seidel ran, worst where it did not)."""
    m, ib, fb = packed(name, max_rows=DEVICE_ROWS, solver=solver)
    _, om = oracle_model(name, max_rows=DEVICE_ROWS, solver=solver)
    emu_ref.set_reverse(reverse)
    try:
        e1 = physics_ref.OracleEnv(om, seed=2, env_id=pose)
        e2 = emu_ref.EmuEnv(ib, fb, seed=2, env_id=pose)
        e1.reset(); e2.reset()
        q = np.array(fb[16:16 + om.nq])
        q[2] = 0.05
        q[3:7] = QUATS[pose]
        e1.qpos[:] = q
        e1.qvel[:] = 0
        rng = np.random.RandomState(4 + pose)
        obs, diag, rows, worst_gs, worst_exact = [], [], [], 0.0, 0.0
        for t in range(6):
            e2.rec[:om.nq] = e1.qpos
            e2.rec[om.nq:om.nq + om.nv] = e1.qvel
            e2.rec[om.nq + om.nv:om.nq + om.nv + 2] = e1.torso_xy_stale
            e2.rec[om.nq + om.nv + 2:om.nq + om.nv + 4] = e1.target
            e2.cnt[0], e2.cnt[1] = e1.counters[0], e1.counters[1]
            a = rng.uniform(-1, 1, size=3 * om.L).astype(np.float32)
            rows.append(om.forward(e1.qpos, e1.qvel, a[3:3 + om.nu].astype(np.float64))[2]["nrow"])
            o1, r1, d1, i1 = e1.step(a.astype(np.float64), auto_reset=False)
            o2, r2, d2, i2 = e2.step(a, auto_reset=False)
            assert d1 == d2 and i1["overflow"] == 0 and e2.cnt[2] == 0, (name, solver, pose, t)
            c3 = int(e2.cnt[3])
            err = np.abs(o1 - o2).max() / (1 + np.abs(o1).max())
            if solver == 1 and rows[-1] > 64:
                assert c3 & 0xFF, "more than 64 rows and no Gauss-Seidel evaluation"
            if c3 & 0xFF:
                worst_gs = max(worst_gs, err)
            else:
                worst_exact = max(worst_exact, err)
            obs.append(o2.copy())
            diag.append(c3)
        return np.array(obs), diag, rows, worst_gs, worst_exact
    finally:
        emu_ref.set_reverse(False)


@pytest.mark.parametrize("name", LYING)
def test_contact_rich_states_on_both_layouts_and_both_solvers(name):
    """Lying poses fill the constraint rows: evaluations beyond the LDS row arrays (lrows) take the HBM slab path, those beyond 64
    rows the streamed Gauss-Seidel.  Both slab layouts, SOLVER 1 (block pivoting) and 0 (Gauss-Seidel only), both lane orders.
    The emulator's pgs shares the oracle's sweep order, so agreement is to rounding (measured <= 1.2e-14); ASSERTED at 1e-9 where
    block pivoting solved every evaluation of the step and at the 1e-6 of a tolerance-stopped iteration where Gauss-Seidel ran."""
    evals = 4 if "cheetah" in name else 16       # dynamics evaluations per step: frame_skip 4 x (RK4: 4 stages; Euler: 1)
    slab = {}
    worst = [0.0, 0.0]
    classes = set()
    for layout in LAYOUTS:
        emu_ref.set_layout(layout)
        try:
            for solver in (1, 0):
                for pose in range(3):
                    fwd = _lying_run(name, solver, pose, False)
                    rev = _lying_run(name, solver, pose, True)
                    assert np.array_equal(fwd[0], rev[0]) and fwd[1] == rev[1], (layout, solver, pose)
                    obs, diag, rows, w_gs, w_exact = fwd
                    worst = [max(worst[0], w_gs), max(worst[1], w_exact)]
                    assert w_gs < 1e-6 and w_exact < 1e-9, (layout, solver, pose, w_gs, w_exact)
                    assert all((c >> 8) & 0xFF == 0 for c in diag), "block pivoting gave up"
                    if solver == 1:
                        slab[layout, pose] = sum(c >> 16 for c in diag)
                    else:
                        assert all(c >> 16 == 0 for c in diag)
                        for c, n in zip(diag, rows):
                            assert (c & 0xFF) <= evals
                            if n > 0:       # every evaluation with rows is a Gauss-Seidel evaluation
                                assert (c & 0xFF) == evals, (layout, pose, c, n)
                        classes |= set("lds" if n <= 19 else "slab" if 33 <= n <= 64 else "big" if n > 64 else "" for n in rows)
        finally:
            emu_ref.set_layout("dieted")
    print("%s: worst relative observation error %.1e where Gauss-Seidel ran, %.1e where not; slab evaluations %s; row classes %s"
          % (name, worst[0], worst[1], slab, sorted(classes - {""})))
    if name in ("3d_walker_7_full", "3d_humanoid_7_left_arm", "3d_humanoid_9_full"):
        for layout in LAYOUTS:
            assert sum(slab[layout, p] for p in range(3)) > 0, "no evaluation took the slab path under the %s layout" % layout
    if name == "3d_hopper_5_full":
        assert slab["dieted", 0] > 0 and slab["default", 0] > 0
    if name == "3d_walker_7_full":
        # the default layout cuts the walker's LDS rows further (24 against the dieted 32): more evaluations leave LDS -- the switch
        # changes which path runs
        assert sum(slab["default", p] for p in range(3)) > sum(slab["dieted", p] for p in range(3))


@pytest.mark.parametrize("name", ["3d_walker_7_full", "3d_cheetah_14_full", "3d_humanoid_9_full", "3d_humanoid_8_left_knee",
                                  "3d_hopper_3_shin"])
def test_the_two_layout_variants_differ_as_intended(name):
    """step_body.h make_layout: without an LDS copy of the int tables (n_int = 0) contact frames keep 6 doubles and the row cut goes
    for the most resident workgroups down to 19 rows; with the copy frames are 9 doubles and the cut stops at 20 rows."""
    m, ib, fb = packed(name, max_rows=DEVICE_ROWS)
    diet, dflt = emu_ref.layout_info(ib, "dieted"), emu_ref.layout_info(ib, "default")
    assert (diet["fstride"], dflt["fstride"]) == (6, 9)
    assert diet["lrows"] >= min(19, int(ib[16])) and dflt["lrows"] >= min(20, int(ib[16]))
    assert diet["bytes"] != dflt["bytes"]
    assert diet["workgroups_per_cu"] >= dflt["workgroups_per_cu"]
    for variant, info in (("dieted", diet), ("default", dflt)):      # the selected variant is the one the emulator allocates
        emu_ref.set_layout(variant)
        try:
            assert emu_ref.lib().sgrl_emu_layout_bytes(ib.ctypes.data_as(emu_ref._i32p)) == info["bytes"]
        finally:
            emu_ref.set_layout("dieted")
