"""Qualifies the inputs of tests/test_set_full_rank_gpu.py on the CPU, in float64, before any device is involved.

The device parity tests of the SET forwards used to run on oracle.formula.formula_values alone: rank <= 4 matrices, nearly periodic
in 8 columns.  The census below exchanges two input columns of every 2-D parameter (what a wrong pack permutation, K-slice order,
perm32, Gram fold or fragment layout does) and counts the exchanges that stay below the device tests' bounds: with the formula
weights more than a third of them would pass, with oracle.formula.full_rank_values (seed SEED, q / k gain QK_GAIN) none may.
The weight seed and the observation seed were picked by scanning eight of them with this census; the conditions are assertions,
so a change to the generator or the modules that loses them fails here and not silently on the device."""
import numpy as np
import pytest
import torch

import set_full_rank_ref as R
from oracle import set_ref
from oracle.formula import QK_GAIN, apply_formula_, apply_full_rank_, synth_obs

NAME, L, B = "3d_walker_7_full", 7, 2
SEED, OBS_SEED, ACT_SEED = 8, 108, 208
MIN_RATIO = 3.0             # every live exchange moves some compared quantity by at least this many device-test bounds
HEADROOM = 8.0              # the float32 CPU module stays this far inside every bound


def _full_rank(m):
    return apply_full_rank_(m, SEED)


@pytest.fixture(scope="module")
def inputs():
    return synth_obs(L, B, OBS_SEED), R.critic_actions(L, B, ACT_SEED)


def _actor_census(apply, obs):
    pol = R.cpu_modules("actor", apply, torch.float64)
    a, st = R.actor_forward(pol, NAME, obs)
    bounds = dict(R.stage_bounds(st), out=R.TOL_ACTION)

    def run():
        a, st = R.actor_forward(pol, NAME, obs)
        return dict(st, out=a)
    return R.census(pol.actor, run, bounds)


def _critic_census(apply, obs, act, k):
    crit = R.cpu_modules("critic", apply, torch.float64)
    qs, sts = R.critic_forward(crit, NAME, obs, act)
    bounds = dict(R.stage_bounds(sts[k]), out=R.TOL_Q * np.abs(qs[k]).max())

    def run():
        qs, sts = R.critic_forward(crit, NAME, obs, act)
        return dict(sts[k], out=qs[k])
    return R.census((crit.critic1, crit.critic2)[k], run, bounds)


@pytest.mark.parametrize("net", ["actor", "critic1", "critic2"])
def test_every_live_column_exchange_is_visible_at_full_rank(inputs, net):
    obs, act = inputs
    for label, apply in (("formula", apply_formula_), ("full-rank seed %d, q/k gain %g" % (SEED, QK_GAIN), _full_rank)):
        rows = _actor_census(apply, obs) if net == "actor" else _critic_census(apply, obs, act, int(net[-1]) - 1)
        s = R.census_summary(rows)
        print("census %s, %s: %d exchanges, %d live, %d below the bound in the %s, %d below every bound; weakest %.3g x bound (%s)"
              % (net, label, s["swaps"], s["live"], s["hidden_in_output"], "action" if net == "actor" else "Q", s["hidden_everywhere"],
                 s["weakest"], s["weakest_name"]))
    # the last census is the full-rank one: a condition; the formula row above is printed for the record only
    assert s["live"] >= 120, s
    weak = [(r[0], r[3]) for r in rows if r[1] and r[3] < MIN_RATIO]
    assert not weak, weak


def test_float32_arithmetic_stays_far_inside_every_bound(inputs):
    obs, act = inputs
    a64, st64 = R.actor_forward(R.cpu_modules("actor", _full_rank, torch.float64), NAME, obs)
    a32, st32 = R.actor_forward(R.cpu_modules("actor", _full_rank, torch.float32), NAME, obs.astype(np.float32), f64=False)
    used = {"action": np.abs(a32 - a64).max() / R.TOL_ACTION}
    bounds = R.stage_bounds(st64)
    for k in st64:
        used["actor " + k] = np.abs(st32[k] - st64[k]).max() / bounds[k]
    q64, s64 = R.critic_forward(R.cpu_modules("critic", _full_rank, torch.float64), NAME, obs, act)
    q32, s32 = R.critic_forward(R.cpu_modules("critic", _full_rank, torch.float32), NAME, obs.astype(np.float32),
                                act.astype(np.float32), f64=False)
    for i in (0, 1):
        used["q%d" % (i + 1)] = np.abs(q32[i] - q64[i]).max() / (R.TOL_Q * np.abs(q64[i]).max())
        bounds = R.stage_bounds(s64[i])
        for k in s64[i]:
            used["critic%d %s" % (i + 1, k)] = np.abs(s32[i][k] - s64[i][k]).max() / bounds[k]
    worst = max(used, key=used.get)
    print("float32 CPU module against float64, as a fraction of the device bound: action %.4f, q1 %.4f, q2 %.4f, worst %s %.4f"
          % (used["action"], used["q1"], used["q2"], worst, used[worst]))
    assert used[worst] <= 1.0 / HEADROOM, (worst, used[worst])


def test_the_outputs_carry_signal(inputs):
    obs, act = inputs
    a, _ = R.actor_forward(R.cpu_modules("actor", _full_rank, torch.float64), NAME, obs)
    med, sat = float(np.median(np.abs(a))), float((np.abs(a) > 0.99).mean())
    (q1, q2), _ = R.critic_forward(R.cpu_modules("critic", _full_rank, torch.float64), NAME, obs, act)
    print("median |action| %.3f, above 0.99: %.1f %%; max |q1| %.3e std %.3e, max |q2| %.3e std %.3e"
          % (med, 100 * sat, np.abs(q1).max(), q1.std(), np.abs(q2).max(), q2.std()))
    assert 0.05 <= med <= 0.8 and sat < 0.02
    for q in (q1, q2):          # not a constant: the Q bound is relative to max |q|, a flat Q would hide every error in its offset
        assert np.abs(q).max() >= 1e-3 and q.std() >= 1e-4 and q.std() >= 0.1 * np.abs(q).max()


@pytest.mark.parametrize("name", ["3d_hopper_3_shin", "3d_walker_7_full", "3d_humanoid_9_full", "3d_cheetah_14_full"])
def test_the_numpy_restatement_and_the_float64_module_agree(name):
    """Two independent float64 evaluations of the full-rank actor: oracle/set_ref.py (NumPy, pinned to the reference's fixtures by
    tests/test_oracle_set.py) and the module the device tests take as their reference."""
    gd = R.graph_dict(name, f64=True)          # the graph the module itself is given: same traversals, same float32-born relation
    obs = synth_obs(R.num_limbs(name), 3, OBS_SEED + 1)
    pol = R.cpu_modules("actor", _full_rank, torch.float64)
    a, _ = R.actor_forward(pol, name, obs)
    sd = {k[len("actor."):]: v.numpy() for k, v in pol.state_dict().items()}
    ref = set_ref.set_actor_forward(sd, obs, [np.asarray(t) for t in gd["traversals"]], gd["relation"].numpy())
    assert np.abs(a - ref).max() < 1e-12
