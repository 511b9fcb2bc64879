"""The layer-0 fold of the SET forward (include/sgrl_set.h) on the device, against the float64 CPU modules at full-rank weights.

tests/test_set_layer0_fold.py holds the fold's algebra in float64 and shows that a wrong fold moves the layer-0 attention outputs far
beyond the bounds used here.  This file runs the folded forward just above the tile threshold (2 048 nodes), where it is the
default: action / Q and the hooked layer-0 attention outputs against float64 with the bounds of tests/set_full_rank_ref.py, the same
forward with the fold switched off (sgrl_set_debug_l0fold) as the ceiling -- the fold's error is at most twice the unfolded path's --
then repeatability, the small-batch path (which does not fold) and a re-fold under a weight hold.  Every figure is printed before
anything is asserted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 8                    # qualified by tests/test_set_full_rank.py
WALKER, CHEETAH = "3d_walker_7_full", "3d_cheetah_14_full"
L0_STAGES = ("layer0/attn/out0", "layer0/attn/out1")


class Ctx(object):
    def __init__(self):
        import torch
        import set_full_rank_ref as R
        from oracle.formula import apply_full_rank_
        from sgrl_amd.set_policy import make_critic, make_policy
        assert torch.cuda.is_available()
        self.torch, self.R = torch, R
        fr = lambda m: apply_full_rank_(m, SEED)
        self.pol = fr(make_policy(device="cuda:0", use_hip=True).eval())
        self.crit = fr(make_critic(device="cuda:0").eval())
        self.cpu = {k: R.cpu_modules(k, fr, torch.float64) for k in ("actor", "critic")}
        self._refs = {}

    def inputs(self, name, B):
        from oracle.formula import synth_obs
        L = self.R.num_limbs(name)
        seed = 3000 + 17 * L + B
        return synth_obs(L, B, seed).astype(np.float32), self.R.critic_actions(L, B, seed + 1).astype(np.float32)

    def actor_ref(self, name, B):
        """(obs f32, action f64, stages f64) -- computed once, never changed"""
        key = ("actor", name, B)
        if key not in self._refs:
            obs, _ = self.inputs(name, B)
            a64, s64 = self.R.actor_forward(self.cpu["actor"], name, obs.astype(np.float64))
            self._refs[key] = (obs, a64, s64)
        return self._refs[key]

    def critic_ref(self, name, B):
        key = ("critic", name, B)
        if key not in self._refs:
            obs, act = self.inputs(name, B)
            q64, s64 = self.R.critic_forward(self.cpu["critic"], name, obs.astype(np.float64), act.astype(np.float64))
            self._refs[key] = (obs, act, q64, s64)
        return self._refs[key]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


class Ledger(object):
    """One line per compared quantity: error of the folded forward, of the unfolded one, the bound; keeps what is out of line."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def check(self, what, fold, plain, ref, bound):
        ref = np.asarray(ref)
        ef = float(np.abs(np.asarray(fold, dtype=np.float64).reshape(ref.shape) - ref).max())
        ep = float(np.abs(np.asarray(plain, dtype=np.float64).reshape(ref.shape) - ref).max())
        print("L0FOLD %s | %s | folded %.3e | unfolded %.3e | ratio %.2f | bound %.3e | %.3f of bound"
              % (self.tag, what, ef, ep, ef / ep if ep > 0 else float("inf"), bound, ef / bound))
        if not ef < bound:
            self.bad.append((what, "bound", ef, bound))
        if not ef <= 2.0 * ep:
            self.bad.append((what, "ceiling", ef, 2.0 * ep))

    def close(self):
        assert not self.bad, (self.tag, self.bad)


def _both(h, run):
    """{fold on / off: (g1, delta of stage 0, output of the full forward, last_split)} of one handle"""
    got = {}
    try:
        for on in (True, False):
            h.debug_l0fold(on)
            h.debug_stop_after(0)
            run()
            g1, delta = h.peek(8, 384), h.peek(9, 128)
            h.debug_stop_after(-1)
            out = run().cpu().numpy()
            got[on] = (g1, delta, out, h.last_split())
    finally:
        h.debug_stop_after(-1)
        h.debug_l0fold(True)
    return got


def _stages(led, R, got, s64, rows):
    for k, i in zip(L0_STAGES, (0, 1)):
        led.check(k, got[True][i][rows], got[False][i][rows], s64[k], R.TOL_STAGE * (1.0 + np.abs(s64[k]).max()))


def _batch(ctx, names, counts):
    R = ctx.R
    Ls = [R.num_limbs(n) for n in names]
    obs = np.zeros((sum(counts), 41 * max(Ls)), dtype=np.float32)
    parts, r, node = [], 0, 0
    for n, c, L in zip(names, counts, Ls):
        obs[r:r + c, :41 * L] = ctx.actor_ref(n, c)[0]
        parts.append((n, r, c, L, node))
        r += c
        node += c * L
    return obs, parts


@pytest.mark.parametrize("names,counts,nodes", [([WALKER], [293], 2051), ([CHEETAH, WALKER], [80, 150], 2170)],
                         ids=["walker7x293", "cheetah14x80+walker7x150"])
def test_actor_just_above_the_tile_threshold(ctx, names, counts, nodes):
    """2 051 nodes: the first size the folded path serves by default.  2 170 nodes of two morphologies: a ragged batch, the L > 8
    attention branch, the two-half split.  Stage 0 (a probe: single pass) and the action (two halves) per morphology."""
    from sgrl_amd.set_hip import HipSetActor
    t, R = ctx.torch, ctx.R
    obs, parts = _batch(ctx, names, counts)
    act = HipSetActor(ctx.pol)
    act.configure([R.graph_dict(n, "cuda:0") for n in names], counts)
    assert act.num_nodes == nodes
    x = t.from_numpy(obs).cuda()
    act.scale_redos()
    got = _both(act, lambda: act.forward_batch(x))
    again = act.forward_batch(x)
    redos = act.scale_redos()
    print("L0FOLD actor %d nodes: last_split folded %d / unfolded %d, scale_redos %d" % (nodes, got[True][3], got[False][3], redos))
    led = Ledger("actor %d" % nodes)
    for n, r0, c, L, node0 in parts:
        _, a64, s64 = ctx.actor_ref(n, c)
        led.tag = "actor %d %s" % (nodes, n)
        _stages(led, R, got, s64, slice(node0, node0 + c * L))
        led.check("action", got[True][2][r0:r0 + c, :3 * L], got[False][2][r0:r0 + c, :3 * L], a64, R.TOL_ACTION)
        assert (got[True][2][r0:r0 + c, 3 * L:] == 0).all(), n
    assert 0 < got[True][3] < nodes and got[True][3] == got[False][3]
    assert redos == 0
    assert np.array_equal(again.cpu().numpy(), got[True][2])           # (the last forward of _both ran unfolded; `again` is folded)
    assert not np.array_equal(got[True][0], got[False][0])             # the switch switches: another summation order
    led.close()


def test_critic_just_above_the_tile_threshold(ctx):
    """Both critic networks at B = 300 on walker_7 (2 100 nodes): the action slots enter the scalar embedding only, the fold is the same."""
    from sgrl_amd.set_hip import HipSetCritic
    t, R, B = ctx.torch, ctx.R, 300
    obs, action, q64, s64 = ctx.critic_ref(WALKER, B)
    qs = HipSetCritic(ctx.crit)
    x, u = t.from_numpy(obs).cuda(), t.from_numpy(action).cuda()
    led = Ledger("critic")
    for k, h in enumerate((qs.q1, qs.q2)):
        h.configure([R.graph_dict(WALKER, "cuda:0")], [B])
        assert h.num_nodes == 2100
        h.scale_redos()
        got = _both(h, lambda: h.forward_q(x, u))
        again = h.forward_q(x, u)
        redos = h.scale_redos()
        print("L0FOLD critic%d: last_split %d, scale_redos %d" % (k + 1, got[True][3], redos))
        led.tag = "critic%d" % (k + 1)
        _stages(led, R, got, s64[k], slice(None))
        led.check("q", got[True][2], got[False][2], q64[k], R.TOL_Q * np.abs(q64[k]).max())
        assert redos == 0 and got[True][3] > 0
        assert np.array_equal(again.cpu().numpy(), got[True][2])
    led.close()


def test_the_small_batch_path_does_not_fold(ctx):
    from sgrl_amd.set_hip import HipSetActor
    t, R, B = ctx.torch, ctx.R, 3
    obs = ctx.inputs(WALKER, B)[0]
    act = HipSetActor(ctx.pol)
    act.configure([R.graph_dict(WALKER, "cuda:0")], [B])
    x = t.from_numpy(obs).cuda()
    got = _both(act, lambda: act.forward_batch(x))
    for i in range(3):
        assert np.array_equal(got[True][i], got[False][i]), i
    assert got[True][3] == 0


def test_a_weight_update_under_a_hold_is_folded_again(ctx):
    """tests/test_set_full_rank_gpu.py's re-pack case under a weight hold on the folded path (21 nodes sent through the tile kernels):
    the forward behind the next hold_weights() packs AND folds the new weights."""
    from oracle.formula import apply_full_rank_
    from sgrl_amd.set_hip import HipSetActor
    from sgrl_amd.set_policy import make_policy
    t, R, B = ctx.torch, ctx.R, 3
    obs = ctx.inputs(WALKER, B)[0]
    pol = apply_full_rank_(make_policy(device="cuda:0", use_hip=True).eval(), SEED)
    act = HipSetActor(pol)
    act.debug_small_nodes(0)
    act.configure([R.graph_dict(WALKER, "cuda:0")], [B])
    x = t.from_numpy(obs).cuda()
    act.hold_weights(True)
    before = act.forward_batch(x).cpu().numpy()
    held = act.forward_batch(x).cpu().numpy()
    with t.no_grad():
        apply_full_rank_(pol, SEED + 1)
    act.hold_weights(True)
    after = act.forward_batch(x).cpu().numpy()
    act.debug_l0fold(False)
    plain = act.forward_batch(x).cpu().numpy()
    a64, _ = R.actor_forward(R.cpu_modules("actor", lambda m: apply_full_rank_(m, SEED + 1), t.float64), WALKER, obs.astype(np.float64))
    led = Ledger("re-fold under a hold")
    led.check("action after the in-place update", after, plain, a64, R.TOL_ACTION)
    assert np.array_equal(before, held)
    assert np.abs(after - before).max() > 1e-2
    led.close()
