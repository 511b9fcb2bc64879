"""Independent checks of the MJCF compile step (sgrl_amd/mjcf.py) -- the one piece BOTH the HIP engine and the CPU oracle
consume, so that engine-vs-oracle parity cannot see an error in it.  Nothing here pins MuJoCo itself
(unavailable: DESIGN.md section 2); each check compares the compiler's output with a second, differently derived value."""
import json
import math
import os

import numpy as np
import pytest

from helpers import packed
from oracle import physics_ref
from sgrl_amd import mjcf

# the reference's MJCF files (src/environments), stored as test fixtures
REF_ENVS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mjcf")


# ---- inertia from geoms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,h", [(0.05, 0.2), (0.07, 0.3), (0.046, 0.0725), (0.06, 0.001)])
def test_capsule_inertia_against_numerical_quadrature(r, h):
    """Solid capsule of uniform density: I_zz = rho * Int pi/2 R(z)^4 dz, I_xx = rho * Int (pi/4 R(z)^4 + pi R(z)^2 z^2) dz with
    R(z) the radius of the slice at height z (cylinder for |z| <= h, spherical caps beyond)."""
    from scipy.integrate import quad

    def R(z):
        a = abs(z)
        return r if a <= h else math.sqrt(max(r * r - (a - h) ** 2, 0.0))
    vol = quad(lambda z: math.pi * R(z) ** 2, -h - r, h + r, points=[-h, h], epsabs=1e-14)[0]
    assert abs(vol - mjcf.capsule_volume(r, h, "exact")) < 1e-12
    izz = quad(lambda z: 0.5 * math.pi * R(z) ** 4, -h - r, h + r, points=[-h, h], epsabs=1e-15)[0]
    ixx = quad(lambda z: 0.25 * math.pi * R(z) ** 4 + math.pi * R(z) ** 2 * z * z, -h - r, h + r, points=[-h, h], epsabs=1e-15)[0]
    mass = 1000.0 * vol
    got = mjcf._capsule_inertia(mass, r, h)
    np.testing.assert_allclose(got, (1000.0 * ixx, 1000.0 * ixx, 1000.0 * izz), rtol=1e-9)


def test_body_inertia_is_the_parallel_axis_sum_of_its_geoms():
    """humanoid torso: several capsules + spheres per body.  Recompute mass, centre of mass and inertia tensor by brute-force
    quadrature over a point cloud of each geom and compare with the compiled body_ipos / body_mass / body_inertia."""
    m = mjcf.load_asset("3d_humanoid_9_full")
    rng = np.random.RandomState(0)
    for b in (1, 2):
        gs = [g for g in range(m.ngeom) if m.geom_body[g] == b]
        assert len(gs) >= 1
        pts, wts = [], []
        for g in gs:
            r, h = m.geom_size[g, 0], m.geom_size[g, 1]
            n = 400000
            if m.geom_type[g] == mjcf.GEOM_SPHERE:
                box = np.array([r, r, r]); vol_box = 8 * r ** 3
                p = rng.uniform(-1, 1, size=(n, 3)) * box
                inside = (p ** 2).sum(1) <= r * r
                true_vol = 4.0 / 3.0 * math.pi * r ** 3
            else:
                box = np.array([r, r, h + r]); vol_box = 8 * r * r * (h + r)
                p = rng.uniform(-1, 1, size=(n, 3)) * box
                dz = np.maximum(np.abs(p[:, 2]) - h, 0.0)
                inside = p[:, 0] ** 2 + p[:, 1] ** 2 + dz ** 2 <= r * r
                true_vol = mjcf.capsule_volume(r, h)      # the compiler's (selectable) volume rule sets the MASS
            p = p[inside]
            rg = mjcf.quat_to_mat(m.geom_quat[g])
            pts.append(p @ rg.T + m.geom_pos[g])
            wts.append(np.full(len(p), 1000.0 * true_vol / len(p)))
        pts, wts = np.concatenate(pts), np.concatenate(wts)
        mass = wts.sum()
        com = (pts * wts[:, None]).sum(0) / mass
        d = pts - com
        inert = (wts[:, None, None] * ((d ** 2).sum(1)[:, None, None] * np.eye(3) - d[:, :, None] * d[:, None, :])).sum(0)
        assert abs(mass - m.body_mass[b]) < 1e-9 * mass
        np.testing.assert_allclose(com, m.body_ipos[b], atol=2e-3 * np.abs(pts).max())
        ib = m.body_inertia[b]
        full = np.array([[ib[0], ib[3], ib[4]], [ib[3], ib[1], ib[5]], [ib[4], ib[5], ib[2]]])
        np.testing.assert_allclose(inert, full, atol=1.5e-2 * np.abs(full).max())     # Monte-Carlo accuracy


# ---- invweight0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3d_walker_7_full", "3d_hopper_3_shin", "3d_humanoid_9_full", "3d_cheetah_14_full"])
def test_invweight0_against_a_direct_jacobian_solve(name):
    """dof_invweight0 / body_invweight0 at qpos0 (mj_setConst [3P-knowledge]: diagonal of M^-1, and the mean diagonal of
    J M^-1 J' for the translational / rotational body Jacobians).  Second derivation: M from the ORACLE's CRBA (C code,
    composite inertias), Jacobians by central finite differences of mjcf.kinematics_np."""
    m, ib, fb = packed(name)
    om = physics_ref.OracleModel(ib, fb)
    _, M, _ = om.forward(m.qpos0, np.zeros(m.nv), np.zeros(m.nu))
    Minv = np.linalg.inv(M)
    # diagonal rule per joint
    for j in range(m.njnt):
        d = m.jnt_dofadr[j]
        if m.jnt_type[j] == mjcf.JNT_FREE:
            np.testing.assert_allclose(m.dof_invweight0[d:d + 3], np.mean(np.diag(Minv)[d:d + 3]), rtol=1e-9)
            np.testing.assert_allclose(m.dof_invweight0[d + 3:d + 6], np.mean(np.diag(Minv)[d + 3:d + 6]), rtol=1e-9)
        else:
            assert abs(m.dof_invweight0[d] - Minv[d, d]) < 1e-9 * Minv[d, d]

    def integrate(qpos, dq):     # qpos (+) dq : free joint = translation + body-frame rotation vector, hinges add
        q = np.array(qpos)
        q[:3] += dq[:3]
        w = dq[3:6]
        ang = np.linalg.norm(w)
        if ang > 0:
            q[3:7] = mjcf.quat_mul(q[3:7], mjcf.axisangle_to_quat(w / ang, ang))
        q[7:] += dq[6:]
        return q

    def com_and_frame(q):
        xpos, xquat, _, _ = mjcf.kinematics_np(m, q)
        coms = np.array([xpos[b] + mjcf.quat_to_mat(xquat[b]) @ m.body_ipos[b] for b in range(m.nbody)])
        return coms, xquat
    eps = 1e-6
    for b in range(1, m.nbody):
        jp = np.zeros((3, m.nv))
        jr = np.zeros((3, m.nv))
        for d in range(m.nv):
            e = np.zeros(m.nv); e[d] = eps
            cp, qp = com_and_frame(integrate(m.qpos0, e))
            cm, qm = com_and_frame(integrate(m.qpos0, -e))
            jp[:, d] = (cp[b] - cm[b]) / (2 * eps)
            dq = mjcf.quat_mul(qp[b], mjcf.quat_conj(qm[b]))     # world-frame rotation between the two poses
            jr[:, d] = 2 * dq[1:] / (2 * eps) * np.sign(dq[0])
        tran = np.trace(jp @ Minv @ jp.T) / 3.0
        rot = np.trace(jr @ Minv @ jr.T) / 3.0
        assert abs(m.body_invweight0[b, 0] - tran) < 1e-6 * tran, (name, b)
        assert abs(m.body_invweight0[b, 1] - rot) < 1e-6 * rot, (name, b)


# ---- coordinate="global" -> local frames ---------------------------------------------------------------------------
def test_global_coordinates_become_the_hand_derived_local_frames_walker7():
    """reference src/environments/3d_walkers/3d_walker_7_full.xml (coordinate="global", all frames axis-aligned): torso at
    z 1.6, hips at 1.0, knees at 0.52, ankles at 0.136; thigh capsule 1.0 -> 0.52, shin 0.52 -> 0.136, foot capsule
    (0,0,0.136) -> (0.2,0,0.136).  Local values derived by hand: child position minus parent position, capsule centre
    minus body position, half-length = half the from-to distance, joint anchors at the body origin."""
    m = mjcf.load_asset("3d_walker_7_full")
    assert m.body_names == ["world", "torso", "right_thigh", "right_shin", "right_foot", "left_thigh", "left_shin", "left_foot"]
    exp_pos = {"torso": (0, 0, 1.6), "right_thigh": (0, 0, -0.6), "right_shin": (0, 0, -0.48), "right_foot": (0, 0, -0.384),
               "left_thigh": (0, 0, -0.6), "left_shin": (0, 0, -0.48), "left_foot": (0, 0, -0.384)}
    for b, n in enumerate(m.body_names[1:], start=1):
        np.testing.assert_allclose(m.body_pos[b], exp_pos[n], atol=1e-12, err_msg=n)
        np.testing.assert_allclose(m.body_quat[b], [1, 0, 0, 0], atol=1e-12)
    np.testing.assert_allclose(m.qpos0[:7], [0, 0, 1.6, 1, 0, 0, 0])
    # capsules: (centre in the body frame, half length, radius)
    exp_geom = {1: ((0, 0, -0.3), 0.3, 0.07), 2: ((0, 0, -0.24), 0.24, 0.056), 3: ((0, 0, -0.192), 0.192, 0.0448),
                4: ((0.1, 0, 0), 0.1, 0.06)}
    for g, (c, h, r) in exp_geom.items():
        np.testing.assert_allclose(m.geom_pos[g], c, atol=1e-12)
        assert abs(m.geom_size[g, 1] - h) < 1e-12 and abs(m.geom_size[g, 0] - r) < 1e-12
        axis = mjcf.quat_to_mat(m.geom_quat[g])[:, 2]
        want = (1, 0, 0) if g == 4 else (0, 0, 1)
        assert abs(abs(np.dot(axis, want)) - 1) < 1e-12          # capsule axis (sign free)
    # hinge anchors coincide with the body origins, axes x / -y / z; ranges in radians
    for j in range(1, m.njnt):
        np.testing.assert_allclose(m.jnt_pos[j], 0, atol=1e-12)
    np.testing.assert_allclose(m.jnt_axis[1:4], [[1, 0, 0], [0, -1, 0], [0, 0, 1]], atol=1e-12)
    np.testing.assert_allclose(m.jnt_range[1], np.radians([-25, 5]))
    np.testing.assert_allclose(m.jnt_range[5], np.radians([-160, -2]))
    # masses from the geometry: density 1000 x capsule volume (the compiler's selectable rule)
    np.testing.assert_allclose(m.body_mass[1], 1000 * mjcf.capsule_volume(0.07, 0.3), rtol=1e-12)
    np.testing.assert_allclose(m.body_ipos[1], (0, 0, -0.3), atol=1e-12)
    # shin x/z and foot x motors are dead (gear 0), everything else gear 100 (xml lines 16-22)
    assert sorted(set(m.act_gear.tolist())) == [0.0, 100.0] and int((m.act_gear == 0).sum()) == 6


# ---- nothing in the shipped files is dropped silently --------------------------------------------------------------------
def test_unknown_attributes_are_refused(tmp_path):
    xml = """<mujoco model="t"><compiler angle="degree" coordinate="local" inertiafromgeom="true"/>
      <worldbody><geom name="floor" type="plane" size="1 1 1" conaffinity="1"/>
        <body name="torso" pos="0 0 1"><joint type="free" name="root"/><geom type="sphere" size="0.1"/>
          <body name="thigh" pos="0 0 -0.2"><joint type="hinge" axis="1 0 0" name="j" %s/><geom type="capsule" fromto="0 0 0 0 0 -0.3" size="0.04"/></body>
        </body></worldbody><actuator><motor joint="j" gear="10"/></actuator></mujoco>"""
    ok = tmp_path / "ok.xml"
    ok.write_text(xml % "")
    assert mjcf.audit_mjcf(str(ok)) == []
    mjcf.compile_mjcf(str(ok))
    for extra, what in (('springref="10"', "joint@springref"), ('frictionloss="0.1"', "joint@frictionloss"), ('ref="5"', "joint@ref")):
        bad = tmp_path / "bad.xml"
        bad.write_text(xml % extra)
        assert what in mjcf.audit_mjcf(str(bad))
        with pytest.raises(ValueError, match="not understood"):
            mjcf.compile_mjcf(str(bad))
        mjcf.compile_mjcf(str(bad), strict=False)
    inert = tmp_path / "inertial.xml"
    inert.write_text(xml.replace('<geom type="sphere" size="0.1"/>', '<geom type="sphere" size="0.1"/><inertial pos="0 0 0" mass="1" diaginertia="1 1 1"/>') % "")
    assert "inertial" in mjcf.audit_mjcf(str(inert))


def test_every_attribute_of_every_shipped_xml_is_consumed():
    # REF_ENVS/shipped.json: every XML under the reference's src/environments (sub-folder/file) -> the stored file with its
    # contents (the 90 shipped files are 29 distinct ones)
    with open(os.path.join(REF_ENVS, "shipped.json")) as f:
        shipped = json.load(f)
    n = 0
    for path, name in sorted(shipped.items()):
        assert mjcf.audit_mjcf(os.path.join(REF_ENVS, name + ".xml")) == [], path
        n += 1
    assert n >= 29 and len(set(shipped.values())) == 29


# ---- parallel capsule - capsule: two contacts ------------------------------------------------------------------------
def _folded_hopper(theta):
    """hopper_5 with the shin rotated by theta and the lower shin by pi - theta about the same (-y) axis: the lower shin
    points back up, exactly parallel to the thigh, 0.5 sin(theta) beside it."""
    m, ib, fb = packed("3d_hopper_5_full")
    q = m.qpos0.copy()
    jy_shin = m.joint_names.index("shin_joint_y") if "shin_joint_y" in m.joint_names else None
    names = m.joint_names
    shin_y = [i for i, n in enumerate(names) if n.startswith("shin") and n.endswith("_y")][0]
    lshin_y = [i for i, n in enumerate(names) if n.startswith("lower_shin") and n.endswith("_y")][0]
    q[m.jnt_qposadr[shin_y]] = theta
    q[m.jnt_qposadr[lshin_y]] = math.pi - theta
    return m, ib, fb, q


def test_parallel_capsules_make_two_contacts_and_engine_source_agrees():
    """The folded leg touches several capsules (the foot lies against the thigh and shin); what is tested is the thigh /
    lower-shin pair: exactly parallel -> two contacts, a hair off parallel -> one, in the oracle AND in the engine source."""
    import emu_ref
    m, ib, fb, q = _folded_hopper(0.15)
    om = physics_ref.OracleModel(ib, fb)
    ctrl = np.zeros(m.nu)
    qacc, _, d = om.forward(q, np.zeros(m.nv), ctrl)
    qe, de = emu_ref.forward(ib, fb, q, np.zeros(m.nv), ctrl)
    assert de["ncon"] == d["ncon"] and de["nrow"] == d["nrow"]
    assert np.abs(qacc - qe).max() <= 1e-9 * (1 + np.abs(qacc).max())
    q2 = q.copy()
    q2[m.jnt_qposadr[[i for i, n in enumerate(m.joint_names) if n.startswith("lower_shin") and n.endswith("_y")][0]]] += 1e-5
    qacc2, _, d2 = om.forward(q2, np.zeros(m.nv), ctrl)
    qe2, de2 = emu_ref.forward(ib, fb, q2, np.zeros(m.nv), ctrl)
    assert de2["ncon"] == d2["ncon"]
    assert d["ncon"] == d2["ncon"] + 1 == 4                 # the parallel pair contributes its second contact
    assert np.abs(qacc2 - qe2).max() <= 1e-9 * (1 + np.abs(qacc2).max())
    # thigh and lower shin separated beyond the margin (0.5 sin 0.25 = 0.124 > 0.091): that pair makes no contact in
    # either branch; the foot still touches
    m3, ib3, fb3, q3 = _folded_hopper(0.25)
    _, _, d3 = physics_ref.OracleModel(ib3, fb3).forward(q3, np.zeros(m.nv), ctrl)
    q4 = q3.copy()
    q4[m.jnt_qposadr[[i for i, n in enumerate(m.joint_names) if n.startswith("lower_shin") and n.endswith("_y")][0]]] += 1e-5
    _, _, d4 = physics_ref.OracleModel(ib3, fb3).forward(q4, np.zeros(m.nv), ctrl)
    assert d3["ncon"] == d4["ncon"] == 2
