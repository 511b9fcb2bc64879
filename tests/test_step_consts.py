"""The per-morphology constants the packer derives for the step kernel (include/sgrl_model.h geom_axis, pair_rowc, jnt_rowc) and
the engine source that reads them (sgrl_amd/csrc/step_body.h: geom_pose, build_rows_and_halfsolve, count_rows / fill_rows, the
warm start), on the CPU: the tables against a float64 NumPy re-derivation from the model for every shipped morphology, and the
lane emulators (tests/emu) against the oracle, which reads none of the new tables.

Tolerances.  Tables: the re-derivation below evaluates the same real-valued expressions in another association (vectorised, the
rotation through the Rodrigues form instead of the matrix entries), so the two differ by a few roundings of at most seven
operations: 2e-15 relative (9 ulp), plus 4.5e-16 absolute (2 ulp of 1) for the axis components, which are sums of products of
magnitude <= 1 that may cancel to zero.  Emulator against oracle: what tests/test_engine_emu.py asserts for free-running episodes,
1e-9 on the observation (1e-7 cheetah) and ten times that on the reward."""
import numpy as np
import pytest

import emu_ref
from helpers import WALKERS, oracle_model, packed
from oracle import physics_ref
from sgrl_amd import mjcf, model_pack

ROWC = 12
(RC_DMIN, RC_DMAX, RC_WIDTH, RC_MID, RC_POWER, RC_K, RC_B, RC_MARGIN, RC_MU, RC_TRAN, RC_RF1, RC_RF2) = range(ROWC)


def _tables(ib, fb):
    """Every float table of the blob by name, walked in the order of include/sgrl_model.h sgrl_model_view_dims()."""
    nb, nj, nq, nv, nu, ng, npair = (int(x) for x in ib[1:8])
    sizes = [("qpos0", nq), ("body_pos", 3 * nb), ("body_quat", 4 * nb), ("body_ipos", 3 * nb), ("body_inertia", 6 * nb),
             ("body_mass", nb), ("body_invweight0", 2 * nb), ("jnt_pos", 3 * nj), ("jnt_axis", 3 * nj), ("jnt_range", 2 * nj),
             ("jnt_stiffness", nj), ("jnt_solref", 2 * nj), ("jnt_solimp", 5 * nj), ("jnt_margin", nj), ("dof_armature", nv),
             ("dof_damping", nv), ("dof_invweight0", nv), ("geom_pos", 3 * ng), ("geom_quat", 4 * ng), ("geom_size", 3 * ng),
             ("pair_mu", npair), ("pair_margin", npair), ("pair_solref", 2 * npair), ("pair_solimp", 5 * npair),
             ("act_gear", nu), ("act_ctrlrange", 2 * nu),
             ("geom_axis", 3 * ng), ("pair_rowc", ROWC * npair), ("jnt_rowc", ROWC * nj)]
    out, p = {}, model_pack.NFHDR
    for k, n in sizes:
        out[k] = np.array(fb[p:p + n])
        p += n
    assert p == len(fb)
    return out


def _rowc64(solref, solimp, margin, mu, tran, h):
    """[n, ROWC] records from [n, 2] solref, [n, 5] solimp and [n] margin / mu / tran, vectorised in float64."""
    si = np.array(solimp, dtype=np.float64)
    si[:, [0, 1, 3]] = np.clip(si[:, [0, 1, 3]], 0.0001, 0.9999)
    si[:, 2] = np.maximum(si[:, 2], 0.0)
    si[:, 4] = np.maximum(si[:, 4], 1.0)
    tc = np.maximum(solref[:, 0], 2 * h)
    k = (si[:, 1] * tc * solref[:, 1]) ** -2.0
    b = 2.0 / (tc * si[:, 1])
    return np.column_stack([si, k, b, margin, mu, tran, tran * (1 + mu ** 2), 2 * mu ** 2])


@pytest.mark.parametrize("name", mjcf.list_assets())
def test_derived_tables_match_a_float64_rederivation(name):
    m, ib, fb = packed(name)
    t = _tables(ib, fb)
    ng, npair, nj = m.ngeom, m.npair, m.njnt
    # the blob's own fields are what they were, where they were
    for k in mjcf.Model.F64_FIELDS:
        assert np.array_equal(t[k], np.asarray(getattr(m, k), dtype=np.float64).ravel()), k
    # geom_axis: e_z turned by the geom's quaternion, v' = v + 2 w (u x v) + 2 u x (u x v)
    q = t["geom_quat"].reshape(ng, 4)
    ez = np.tile([0.0, 0.0, 1.0], (ng, 1))
    uxv = np.cross(q[:, 1:], ez)
    ref_axis = ez + 2 * q[:, :1] * uxv + 2 * np.cross(q[:, 1:], uxv)
    np.testing.assert_allclose(t["geom_axis"].reshape(ng, 3), ref_axis, rtol=2e-15, atol=4.5e-16)
    assert np.abs(np.linalg.norm(ref_axis, axis=1) - 1).max() < 1e-12
    h = float(fb[model_pack.F_TIMESTEP])
    iwb = t["body_invweight0"].reshape(-1, 2)[:, 0]
    gb = np.asarray(m.geom_body, dtype=int)
    tran = iwb[gb[np.asarray(m.pair_g1, dtype=int)]] + iwb[gb[np.asarray(m.pair_g2, dtype=int)]]
    ref_pair = _rowc64(t["pair_solref"].reshape(npair, 2), t["pair_solimp"].reshape(npair, 5), t["pair_margin"], t["pair_mu"], tran, h)
    np.testing.assert_allclose(t["pair_rowc"].reshape(npair, ROWC), ref_pair, rtol=2e-15, atol=0)
    jt = t["dof_invweight0"][np.asarray(m.jnt_dofadr, dtype=int)]
    ref_jnt = _rowc64(t["jnt_solref"].reshape(nj, 2), t["jnt_solimp"].reshape(nj, 5), t["jnt_margin"], np.zeros(nj), jt, h)
    np.testing.assert_allclose(t["jnt_rowc"].reshape(nj, ROWC), ref_jnt, rtol=2e-15, atol=0)
    # the floor belongs to the world body (collide() takes its pose from the model alone)
    planes = [g for g in range(ng) if int(m.geom_type[g]) == mjcf.GEOM_PLANE]
    assert planes and all(int(m.geom_body[g]) == 0 for g in planes)


# ---- the emulators against the oracle ----------------------------------------------------------------------------------------------
STEPS = 40
DEVICE_ROWS = 256      # the row cap the vec-env packs with (sgrl_amd/_lib.py default_max_rows): a lying body drops no row
# (name, layout): both slab layouts on the eight walkers, then one hopper (capsule-capsule pairs, condim 1 and 3), one cheetah (Euler),
# one humanoid beyond 64 row items (serial prefix in fill_rows) and the humanoid with exactly 64 (the last lane of the ballot prefix)
CASES = [(n, lay) for n in WALKERS for lay in ("dieted", "default")] + \
        [("3d_hopper_5_full", "default"), ("3d_cheetah_14_full", "default"), ("3d_humanoid_9_full", "dieted"),
         ("3d_humanoid_7_lower_arms", "dieted")]


def _lying(name, m, qpos0):
    """On the floor.  Walkers, humanoids, cheetah: every hinge turned to 0.8 rad, beyond most ranges, so limit rows and pyramidal
    floor contacts occur in one evaluation.  The hopper folds its leg instead (shin by 0.15 rad, lower shin back up by pi - 0.14:
    a hair off parallel to the thigh, 0.075 beside it): limit rows, floor contacts and closed capsule-capsule pairs -- condim-1
    rows from the closest points of two segments -- together."""
    q = np.array(qpos0)
    q[2] = 0.05
    if "hopper" in name:
        jy = lambda part: [i for i, n in enumerate(m.joint_names) if n.startswith(part) and n.endswith("_y")][0]
        q[3:7] = [0.70710678, 0, 0.70710678, 0]
        q[m.jnt_qposadr[jy("shin")]] = 0.15
        q[m.jnt_qposadr[jy("lower_shin")]] = np.pi - 0.14
    else:
        q[7:] = 0.8
    return q


def _place(e, om, q):
    """Put an oracle or emulator environment at (q, 0) keeping its target and counters."""
    if isinstance(e, emu_ref.EmuEnv):
        e.rec[:om.nq] = q
        e.rec[om.nq:om.nq + om.nv] = 0
    else:
        e.qpos[:] = q
        e.qvel[:] = 0


def _row_kinds(m, om, q):
    """(limit rows, floor contacts, capsule-capsule contacts) of the oracle's forward pass at (q, 0, 0).  The shipped models give
    floor pairs condim 3 (four pyramid rows a contact) and capsule-capsule pairs condim 1 (one row), so the oracle's row and contact
    counts and the limit rows counted here from the joint ranges settle the split."""
    plane = np.array([int(m.geom_type[int(g)]) == mjcf.GEOM_PLANE for g in m.pair_g1])
    assert (np.asarray(m.pair_condim)[plane] == 3).all() and (np.asarray(m.pair_condim)[~plane] == 1).all()
    d = om.forward(q, np.zeros(om.nv), np.zeros(m.nu))[2]
    assert d["nrow"] == d["nrow_wanted"]
    rng, mg = np.reshape(m.jnt_range, (-1, 2)), np.ravel(m.jnt_margin)
    nlim = sum(int(q[m.jnt_qposadr[j]] - rng[j, 0] < mg[j]) + int(rng[j, 1] - q[m.jnt_qposadr[j]] < mg[j])
               for j in range(m.njnt) if m.jnt_limited[j])
    ncap, rem = divmod(4 * d["ncon"] - (d["nrow"] - nlim), 3)
    assert rem == 0 and 0 <= ncap <= d["ncon"]
    return nlim, d["ncon"] - ncap, ncap


def _assert_all_row_kinds(name, m, om, q):
    nlim, nfloor, ncap = _row_kinds(m, om, q)
    assert nlim >= 1 and nfloor >= 2, "the pose does not give limit rows and floor contacts together"
    if "hopper" in name:
        assert ncap >= 1, "the folded leg closes no capsule-capsule pair"


@pytest.mark.parametrize("start", ["reset", "lying"])
@pytest.mark.parametrize("name,layout", CASES, ids=["%s-%s" % c for c in CASES])
def test_emulator_follows_the_oracle_free_running(name, layout, start):
    m, ib, fb = packed(name, max_rows=DEVICE_ROWS)
    _, om = oracle_model(name, max_rows=DEVICE_ROWS)
    tol = 1e-7 if "cheetah" in name else 1e-9
    emu_ref.set_layout(layout)
    try:
        e1 = physics_ref.OracleEnv(om, seed=13, env_id=2)
        e2 = emu_ref.EmuEnv(ib, fb, seed=13, env_id=2)
        o1, o2 = e1.reset(), e2.reset()
        assert np.abs(o1 - o2).max() < 1e-13
        keep = start == "reset"        # a lying body is "done" at once: without auto-reset it stays down for the whole run
        if start == "lying":
            q = _lying(name, m, fb[16:16 + om.nq])
            _assert_all_row_kinds(name, m, om, q)
            _place(e1, om, q)
            _place(e2, om, q)
        rng = np.random.RandomState(3)
        worst = 0.0
        for t in range(STEPS):
            a = rng.uniform(-1, 1, size=3 * om.L).astype(np.float32)
            o1, r1, d1, i1 = e1.step(a.astype(np.float64), auto_reset=keep)
            o2, r2, d2, i2 = e2.step(a, auto_reset=keep)
            worst = max(worst, np.abs(o1 - o2).max())
            assert d1 == d2, t
            assert np.abs(o1 - o2).max() < tol and abs(r1 - r2) < tol * 10, (t, np.abs(o1 - o2).max())
            assert i1["overflow"] == 0 and e2.cnt[2] == 0
            assert (int(e2.cnt[3]) >> 8) & 0xFF == 0, "block pivoting gave up"
        print("%s %s %s: worst |obs diff| %.2e" % (name, layout, start, worst))
    finally:
        emu_ref.set_layout("dieted")


@pytest.mark.parametrize("start", ["reset", "lying"])
def test_pair_emulator_follows_the_oracle_free_running(start):
    """Two walker_3 environments on one emulated wavefront (wave_half.h: the ballot prefix runs per half)."""
    name = "3d_walker_3_left_leg_right_foot"
    m, ib, fb = packed(name, max_rows=DEVICE_ROWS)
    _, om = oracle_model(name, max_rows=DEVICE_ROWS)
    ids = (4, 5)
    pe = emu_ref.PairEmu(ib, fb, seed=13, env_ids=ids)
    oracles = [physics_ref.OracleEnv(om, seed=13, env_id=e) for e in ids]
    o_pair = pe.reset()
    for h in range(2):
        assert np.abs(o_pair[h] - oracles[h].reset()).max() < 1e-13
    keep = start == "reset"
    if start == "lying":       # one half on the floor, its mate in its reset state: the halves build different row tables
        q = _lying(name, m, fb[16:16 + om.nq])
        _assert_all_row_kinds(name, m, om, q)
        _place(oracles[0], om, q)
        _place(pe.envs[0], om, q)
    rng = np.random.RandomState(5)
    for t in range(STEPS):
        acts = [rng.uniform(-1, 1, size=3 * om.L).astype(np.float32) for _ in range(2)]
        res = pe.step(acts, auto_reset=keep)
        for h in range(2):
            o1, r1, d1, _ = oracles[h].step(acts[h].astype(np.float64), auto_reset=keep)
            o2, r2, d2, _ = res[h]
            assert d1 == d2, (t, h)
            assert np.abs(o1 - o2).max() < 1e-9 and abs(r1 - r2) < 1e-8, (t, h, np.abs(o1 - o2).max())
