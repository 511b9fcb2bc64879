"""GPU tests of the step kernel's Gauss-Seidel path (wave_hip.h HipWaveT::pgs / pgs_big through step_body.h pgs_and_finish) and of
the slab layouts, against the CPU oracle.

SOLVER = 0 makes the register Gauss-Seidel the whole solver of every evaluation with constraint rows; a SOLVER = 0 blob has no
fixed-dimension instance, so these engines run on the generic kernel (default slab layout).  States are teacher-forced from the
oracle (sgrl_set_records) unless a test says otherwise.  The iteration is stopped by its tolerance, so agreement with the oracle
(same sweep order, another summation order inside a sweep) is asserted at 1e-6 relative, the figure the project allows such an
iteration elsewhere (test_contact_rich_states_keep_every_constraint_row, test_gauss_seidel_fallback_of_the_half_wave).

Measured on an MI355X (worst relative deviation of qpos / qvel / observation / reward from the oracle; each test prints its own):
  B1 reset states, 40 steps   hopper_5    qpos 1.3e-16  qvel 1.4e-15  obs 9.4e-16  reward 1.2e-10   (up to 12 rows at a step start)
                              walker_7    qpos 5.0e-16  qvel 7.9e-15  obs 5.4e-15  reward 2.1e-10   (20 rows)
                              humanoid_9  qpos 2.3e-16  qvel 4.6e-15  obs 3.8e-15  reward 1.5e-10   (14 rows)
                              cheetah_14  qpos 7.3e-15  qvel 2.5e-13  obs 1.8e-13  reward 4.5e-11   (34 rows)
  B2 lying poses, 6 steps                 qpos 3.6e-16  qvel 3.3e-15  obs 6.0e-15  reward 1.3e-10
     steps that start with 1..19 rows (LDS rows, register pgs): 12; with 33..64 (slab rows, register pgs): 37; with > 64 (pgs_big): 10
  B3 converged Gauss-Seidel (1000 sweeps) against block pivoting, qpos / qvel, device pair (CPU oracle pair):
     hopper_5 1.4e-16 (2.3e-16), walker_7 1.2e-15 (1.5e-15), humanoid_9 7.4e-16 (9.6e-16), cheetah_14 1.1e-14 (1.4e-14),
     humanoid_7 lying with 38..61 rows 7.4e-16 (1.9e-15); asserted at 1e-10
  B4 300 free-running steps, walker_7 + hopper_3: 3.4e-13, 15 episodes, the twin engine bit-identical
  B5 shipped mode on the lying poses      qpos 2.9e-16  qvel 4.7e-15  obs 6.0e-15  reward 1.5e-10; 632 slab block-pivot evaluations, no give-up
The device follows the oracle to rounding here although the iteration stops by its tolerance: both sweep the rows in the same order,
and a sweep's dot products differ in summation order only.  (The reward is the worst column in the shipped mode too: (distance before - distance after) / dt
cancels; test_teacher_forced_step_parity allows it 100 x the state's tolerance, here it gets the same 1e-6 as everything else.)
"""
import numpy as np
import pytest

import emu_ref

pytestmark = pytest.mark.gpu

QUATS = [[1, 0, 0, 0], [0.70710678, 0.70710678, 0, 0], [0.70710678, 0, 0.70710678, 0]]
FAMILIES = ["3d_hopper_5_full", "3d_walker_7_full", "3d_humanoid_9_full", "3d_cheetah_14_full"]      # nv 18 / 24 / 30 / 45 (Euler)
LYING = ["3d_humanoid_9_full", "3d_humanoid_7_left_arm", "3d_walker_7_full", "3d_hopper_5_full"]
PAIR_SWEEPS = 1000          # B3: sweeps of the converged Gauss-Seidel engine (see test_converged_gauss_seidel_meets_block_pivoting)
ORACLE_PAIR_WORST = 1.5e-14


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _make(names, per, seed=5, **kw):
    from sgrl_amd.vec_env import BatchedModularVecEnv
    env = BatchedModularVecEnv(names, per, seed=seed, device="cuda:0", **kw)
    env.enable_f64_outputs()
    return env


def _make_pgs(names, per, seed=5, **kw):
    env = _make(names, per, seed=seed, solver=0, **kw)
    assert env.fixed_dim_groups == 0 and all(int(b[0][18]) == 0 for b in env._blobs)      # SOLVER = 0: the generic kernel
    return env


def _oracle_envs(env, seed):
    from oracle import physics_ref
    out = []
    for i in range(env.num_envs):
        ib, fb = env._blobs[env.env_morph[i]]      # the very blobs the engine was created with (solver and row caps included)
        out.append(physics_ref.OracleEnv(physics_ref.OracleModel(ib, fb), seed=seed, env_id=i))
    return out


def _lie_down(env, oes, pose=None):
    """The poses of test_contact_rich_states_keep_every_constraint_row: 5 cm above the floor, quaternion i mod 3 of QUATS (or `pose`)."""
    for i, oe in enumerate(oes):
        m = env.models[env.env_morph[i]]
        q = np.array(env._blobs[env.env_morph[i]][1][16:16 + m.nq])
        q[2] = 0.05
        q[3:7] = QUATS[i % len(QUATS) if pose is None else pose]
        oe.qpos[:] = q
        oe.qvel[:] = 0


def _force(env, oes):
    rec, cnt = env.get_records()
    for i, oe in enumerate(oes):
        m = env.models[env.env_morph[i]]
        rec[i, :m.nq] = oe.qpos
        rec[i, m.nq:m.nq + m.nv] = oe.qvel
        rec[i, m.nq + m.nv:m.nq + m.nv + 2] = oe.torso_xy_stale
        rec[i, m.nq + m.nv + 2:m.nq + m.nv + 4] = oe.target
        cnt[i, 0], cnt[i, 1] = oe.counters[0], oe.counters[1]
    env.set_records(rec, cnt)


def _start_rows(oes, a):
    """Constraint rows of the evaluation every step starts with, from the oracle (the row count depends on the state only)."""
    return [oe.m.forward(oe.qpos, oe.qvel, a[i, 3:3 + oe.m.nu].astype(np.float64))[2]["nrow"] for i, oe in enumerate(oes)]


def _rel(x, ref):
    return float(np.abs(np.asarray(x) - np.asarray(ref)).max() / (1 + np.abs(ref).max()))


class _Step(object):
    """One teacher-forced step of engine and oracles: relative deviations per environment and the engine's diagnostics."""

    def __init__(self, env, oes, a, rebuild=False):
        torch = _torch()
        _force(env, oes)
        self.rows = _start_rows(oes, a)
        env.step_device(torch.from_numpy(a).cuda(), auto_reset=False)
        torch.cuda.synchronize()
        obs, rew, done = env.obs64.cpu().numpy(), env.rew64.cpu().numpy(), env.done.cpu().numpy()
        rec, self.cnt = env.get_records()
        self.q, self.v = [], []
        self.err = np.zeros((env.num_envs, 4))
        for i, oe in enumerate(oes):
            o, r, d, info = oe.step(a[i].astype(np.float64), auto_reset=False)
            q, v, _, _ = env.state_of(rec, i)
            self.q.append(q.copy())
            self.v.append(v.copy())
            self.err[i] = _rel(q, oe.qpos), _rel(v, oe.qvel), _rel(obs[i, :o.size], o), _rel(rew[i], r)
            assert bool(done[i]) == d, i                                       # exact
            assert info["overflow"] == 0 and self.cnt[i, 2] == 0, i            # exact: no constraint row dropped
            if d and rebuild:
                oe.counters[1] += 1
                oe.reset()


def _assert_gauss_seidel_everywhere(step):
    diag = step.cnt[:, 3]
    for i, n in enumerate(step.rows):
        if n > 0:
            assert diag[i] & 0xFF > 0, "rows and no Gauss-Seidel evaluation (env %d)" % i
    assert ((diag >> 8) & 0xFF == 0).all()


@pytest.mark.parametrize("name", FAMILIES)
def test_gauss_seidel_only_step_parity_from_reset_states(name):
    """B1: SOLVER = 0 from reset states, 40 teacher-forced steps per family (the cheetah integrates with Euler): HipWaveT::pgs over
    LDS rows is the solver of every evaluation."""
    env = _make_pgs([name], 2)
    env.reset_device()
    oes = _oracle_envs(env, 5)
    for oe in oes:
        oe.reset()
    rng = np.random.RandomState(0)
    worst = np.zeros(4)
    rows_seen = 0
    for t in range(40):
        a = rng.uniform(-1, 1, size=(env.num_envs, env.action_max_len)).astype(np.float32)
        s = _Step(env, oes, a, rebuild=True)
        worst = np.maximum(worst, s.err.max(axis=0))
        rows_seen = max(rows_seen, max(s.rows))
        _assert_gauss_seidel_everywhere(s)
    print("B1 %s: worst relative deviation qpos %.1e qvel %.1e obs %.1e reward %.1e (most rows at a step start: %d)"
          % ((name,) + tuple(worst) + (rows_seen,)))
    assert rows_seen > 0
    assert (worst < 1e-6).all(), worst


def test_gauss_seidel_only_on_contact_rich_states_reaches_every_row_class():
    """B2: SOLVER = 0 from lying poses.  The three classes of an evaluation's row count (from the oracle: the device's counter has
    no slab bit under SOLVER = 0): up to 19 rows sit in LDS under every layout (register pgs), 33..64 rows are beyond any lrows and
    live in the HBM slab with the warm start partly read from it (register pgs over global rows: pgs_and_finish<true>), more than
    64 rows stream through pgs_big."""
    env = _make_pgs(LYING, 3, seed=2)
    env.reset_device()
    oes = _oracle_envs(env, 2)
    for oe in oes:
        oe.reset()
    _lie_down(env, oes)
    rng = np.random.RandomState(4)
    worst = np.zeros(4)
    classes = {"lds": 0, "slab": 0, "big": 0}
    for t in range(6):
        a = rng.uniform(-1, 1, size=(env.num_envs, env.action_max_len)).astype(np.float32)
        s = _Step(env, oes, a)
        worst = np.maximum(worst, s.err.max(axis=0))
        _assert_gauss_seidel_everywhere(s)
        assert (s.cnt[:, 3] >> 16 == 0).all()
        for n in s.rows:
            classes["lds"] += 0 < n <= 19
            classes["slab"] += 33 <= n <= 64
            classes["big"] += n > 64
    print("B2: worst relative deviation qpos %.1e qvel %.1e obs %.1e reward %.1e; steps starting in each row class: %s"
          % (tuple(worst) + (classes,)))
    assert classes["lds"] > 0 and classes["slab"] > 0 and classes["big"] > 0, classes
    assert (worst < 1e-6).all(), worst


@pytest.mark.parametrize("name,lying,steps", [(n, False, 10) for n in FAMILIES] + [("3d_humanoid_7_left_arm", True, 4)])
def test_converged_gauss_seidel_meets_block_pivoting(name, lying, steps):
    """B3: a converged Gauss-Seidel run (engine P: SOLVER = 0, tolerance 0, PAIR_SWEEPS sweeps, generic kernel) and the block-pivot
    solve (engine B: the shipped mode on the family kernels) are independent routes to the one optimum of the LCP.  Both engines
    are fed the same states (the block-pivot oracle's) and actions; humanoid_7 lying upright keeps 33..64 rows, where the slab
    block-pivot path meets the register pgs over slab rows.

    The bound is measured on the CPU oracle, not on the device: oracle-P against oracle-B on these very states agree to
    ORACLE_PAIR_WORST = 1.5e-14 relative on qpos and qvel with 1000 sweeps, the smallest of {1000, 3000, 10000} that reaches 1e-9
    (hopper 1.8e-16, walker 9.5e-16, humanoid_9 7.3e-16, cheetah 7.7e-15, humanoid_7 lying 1.1e-15; 3000 and 10000 sweeps give the
    same figures).  The device pair is asserted at 100 x that figure (the device sums a sweep's dot products in another order), and
    not below 1e-10.  Not part of the set, because plain Gauss-Seidel has not converged on them: walker_7 lying upright (5.8e-2
    away at the default 300 sweeps, 7e-6 after 3000), cheetah_10 and cheetah_14 on the side (3e-5 / 1e-7 after 3000)."""
    envP = _make_pgs([name], 2, pgs_tol=0.0, pgs_iters=PAIR_SWEEPS)
    envB = _make([name], 2)
    assert envB.fixed_dim_groups > 0 and int(envB._blobs[0][0][18]) == 1
    for env in (envP, envB):
        env.reset_device()
    oesB, oesP = _oracle_envs(envB, 5), _oracle_envs(envP, 5)
    for oe in oesB + oesP:
        oe.reset()
    if lying:
        _lie_down(envB, oesB, pose=0)       # both environments in pose 0, with their own targets and actions
    rng = np.random.RandomState(6)
    pair = oracle_pair = 0.0
    worstB, worstP = np.zeros(4), np.zeros(4)
    for t in range(steps):
        for oB, oP in zip(oesB, oesP):
            oP.buf[:] = oB.buf              # the Gauss-Seidel oracle starts every step from the block-pivot oracle's state
        a = rng.uniform(-1, 1, size=(envB.num_envs, envB.action_max_len)).astype(np.float32)
        sB, sP = _Step(envB, oesB, a), _Step(envP, oesP, a)
        assert max(sB.rows) <= 64, "beyond 64 rows both engines run pgs_big"
        if lying:
            assert min(sB.rows) >= 33
        assert ((sB.cnt[:, 3] >> 8) & 0xFF == 0).all() and (sB.cnt[:, 3] & 0xFF == 0).all()      # B never ran Gauss-Seidel
        _assert_gauss_seidel_everywhere(sP)
        worstB, worstP = np.maximum(worstB, sB.err.max(axis=0)), np.maximum(worstP, sP.err.max(axis=0))
        for i in range(envB.num_envs):
            pair = max(pair, _rel(sP.q[i], sB.q[i]), _rel(sP.v[i], sB.v[i]))
            oracle_pair = max(oracle_pair, _rel(oesP[i].qpos, oesB[i].qpos), _rel(oesP[i].qvel, oesB[i].qvel))
    bound = max(100 * ORACLE_PAIR_WORST, 1e-10)
    print("B3 %s: device pair %.1e (bound %.1e), oracle pair %.1e; engine B against its oracle %s, engine P against its oracle %s"
          % (name, pair, bound, oracle_pair, ["%.1e" % x for x in worstB], ["%.1e" % x for x in worstP]))
    assert oracle_pair <= 1e-9, oracle_pair          # the criterion PAIR_SWEEPS was chosen by still holds
    tolB = 1e-7 if "cheetah" in name else 1e-9
    assert (worstB[:3] < tolB).all() and worstB[3] < 100 * tolB, worstB      # as test_teacher_forced_step_parity
    assert (worstP < 1e-6).all(), worstP
    assert pair <= bound, (pair, bound)


def test_gauss_seidel_only_free_running_and_run_to_run_identical():
    """B4: SOLVER = 0 free-running with auto-reset and the oracle's counter RNG, 300 steps; a second engine with the same seed and
    actions is bit-identical."""
    torch = _torch()
    names = ["3d_walker_7_full", "3d_hopper_3_shin"]
    env, twin = _make_pgs(names, 2), _make_pgs(names, 2)
    env.reset_device()
    twin.reset_device()
    oes = _oracle_envs(env, 5)
    for oe in oes:
        oe.reset()
    rng = np.random.RandomState(1)
    worst = 0.0
    episodes = 0
    for t in range(300):
        a = rng.uniform(-1, 1, size=(env.num_envs, env.action_max_len)).astype(np.float32)
        ad = torch.from_numpy(a).cuda()
        o1, r1, d1, _ = env.step_device(ad)
        o2, r2, d2, _ = twin.step_device(ad)
        check = t % 50 == 49
        if check:
            torch.cuda.synchronize()
            assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
            assert torch.equal(env.obs64, twin.obs64)
            done = env.done.cpu().numpy()
            rec, cnt = env.get_records()
        ods = [oe.step(a[i].astype(np.float64)) for i, oe in enumerate(oes)]
        episodes += sum(od[2] for od in ods)
        if check:
            for i, oe in enumerate(oes):
                q, v, _, _ = env.state_of(rec, i)
                assert cnt[i, 1] == oe.counters[1], "episode count diverged at step %d env %d" % (t, i)
                assert cnt[i, 0] == oe.counters[0] and cnt[i, 2] == 0
                assert bool(done[i]) == ods[i][2]
                worst = max(worst, _rel(q, oe.qpos), _rel(v, oe.qvel))
    print("B4: free-running worst relative deviation %.1e, episodes %d" % (worst, episodes))
    assert episodes > 2
    assert worst < 1e-6, worst


def test_block_pivoting_never_gives_up_on_the_contact_rich_states():
    """B5: the shipped mode (SOLVER = 1, family kernels) on the lying poses: lcp_block_pivot's "not converged (never observed)"
    holds on the states we have -- the give-up count stays 0 while the slab block-pivot path does run."""
    env = _make(LYING, 3, seed=2)
    assert env.fixed_dim_groups > 0
    env.reset_device()
    oes = _oracle_envs(env, 2)
    for oe in oes:
        oe.reset()
    _lie_down(env, oes)
    rng = np.random.RandomState(4)
    worst = np.zeros(4)
    slab = 0
    for t in range(6):
        a = rng.uniform(-1, 1, size=(env.num_envs, env.action_max_len)).astype(np.float32)
        s = _Step(env, oes, a)
        worst = np.maximum(worst, s.err.max(axis=0))
        assert ((s.cnt[:, 3] >> 8) & 0xFF == 0).all(), "block pivoting gave up"
        slab += int((s.cnt[:, 3] >> 16).sum())
    print("B5: worst relative deviation qpos %.1e qvel %.1e obs %.1e reward %.1e; slab block-pivot evaluations %d"
          % (tuple(worst) + (slab,)))
    assert slab > 0
    assert (worst < 1e-6).all(), worst      # (beyond 64 rows the tolerance-stopped pgs_big runs in this mode too)


@pytest.mark.parametrize("name", ["3d_walker_7_full", "3d_humanoid_9_full"])
@pytest.mark.parametrize("specs", ["0", "1"])
def test_emulator_layouts_are_the_step_kernels(name, specs, monkeypatch):
    """B6: the slab the step kernel is launched with is the layout variant the CPU emulator runs under that name (emu_ref.set_layout):
    "default" on the generic kernel, and on a family kernel "dieted" exactly where the family reads its int tables from global memory."""
    from sgrl_amd import _lib
    monkeypatch.setenv("SGRL_SPECS", specs)
    env = _make([name], 2)
    assert (env.fixed_dim_groups > 0) == (specs == "1")
    variant = "dieted" if specs == "1" and name.split("_")[1] in _lib.ITAB_GLOBAL else "default"
    assert env.lds_bytes == emu_ref.layout_bytes(env._blobs[0][0], variant), variant
    env.close()
