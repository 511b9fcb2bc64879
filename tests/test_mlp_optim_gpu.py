"""The optimizer half of the MLP agent's TD3 update on HIP (csrc/mlp_optim.hip over include/sgrl_mlp.h, mlp_hip.HipMlpOptim,
td3.Agent(mlp_hip_grads=True, mlp_hip_optim=True)) on the MI355X.

1  one step against the float64 restatement (tests/mlp_optim_restate.py, itself held to torch.optim.Adam + clip_grad_norm_ + the
   reference's Polyak loop by test_mlp_optim_plan.py): step counts 1 and 2 from fresh state and a preloaded state (step 1000,
   random m, v >= 0), clip active (|g| = 10 max_norm) and inactive (0.5 max_norm), tau in {0, 0.005, 1}.  A twin copy of the same
   state on the parent path -- td3.clip_and_step with capturable groups, its plain-group fall-through, soft_update_network -- gives
   the ceiling.  Per tensor, in the 2-norm and the max-norm, for g, m and v:
       |HIP - f64| <= 10 |parent32 - f64| + 1e-5 |x64|            parent32: the closer of the two parent paths
   (the floor: the longest chain of additions into the gradient norm is 128 at most, 128 * 2^-24 = 7.6e-6 relative on `total`,
   half of that on coef, at most that on g^2; the factor 10 is test_mlp_grads_gpu._check_grads'); for p and the target the
   project's step bar, 2e-3 |step64| + sqrt(numel) max|x| 1.2e-7.
   The same bars where Adam's eps decides the step: gradients from tests/optim_restate.py's generator, every tensor at 1e-11 and
   scales 1e-13 ... 1e-2 mixed across the tensors, three steps from the seeded parameters and from parameters at zero (which resolve
   a step of 1e-7: the step bar's floor vanishes).  And one NaN / one inf element in one gradient: the NaN pattern of both parent
   paths and of the restatement in g, m, v, p and the target of every tensor, the finite values under the same bars.
2  bit-exact: tau = 1 leaves target == p; max_norm = 0 and an inactive clip give the same p, m, v and leave .grad alone; zero
   gradients from fresh state leave p alone and everything finite; the same state twice gives the same bits; tau = 0 leaves the
   targets alone; a critic step leaves the actor's side alone and the reverse
3  path switching: 3 steps here then 2 on clip_and_step, and the reverse, against 5 on clip_and_step, plain and capturable groups
4  argument errors before any launch, the tensors read back unchanged
5  agent level: twenty updates against Agent(mlp_hip_grads=True); tests/golden/td3_update_mlp.npz through the new path; a
   DeviceTrainer with args.mlp_hip_optim; tensors replaced between two steps are bound again; a second step allocates nothing

Measured on the MI355X (the printed lines of a run), worst error / bar per net over all cases of test 1, critic / actor:
L3 [256, 256] 0.016 / 0.018, [40, 72] 0.037 / 0.023, [1, 7] 0.12 / 0.11, [64, 48, 80, 33] 0.047 / 0.026; L7 [256, 256] 0.011 / 0.013,
[40, 72] 0.030 / 0.023, [1, 7] 0.11 / 0.10, [64, 48, 80, 33] 0.062 / 0.026; L14 [512, 500] 0.020 / 0.017.  For g, m and v the float32
rounding of the result is the whole error (2e-3 ... 6e-3 of the bar, which the 1e-5 |x64| floor dominates; exact zeros where the clip is
inactive); p and the target sit at 6e-3 of the step bar and below; the [1, 7] nets' single-element tensors carry the largest ratios.
Twenty agent updates: |new - parent| 0 ... 1.4e-7 per tensor under tolerances of 7.5e-7 ... 1.3e-3.  The reference replay: critic loss
2.52044296 / 1.08880043 against 2.52044344 / 1.08880043, step norms within 8.8e-3 of their tolerance.  Two deliberately wrong builds fail:
bias correction at t - 1 fails 19 of the 22 tests, the lerp reading the pre-step parameter 15.
Where eps decides, worst error / bar from the seeded parameters | from zero: [1, 7] critic 0.36 | 0.018 (1e-11) and 0.50 | 0.012 (mixed),
actor 0.56 | 0.006 and 0.66 | 0.008; [40, 72] critic 0.42 | 0.009 and 0.29 | 0.019, actor 0.26 | 0.007 and 0.22 | 0.016 (from the seeded
parameters the figure is the rounding of p itself against the bar's floor; from zero it is the step's error against 2e-3 of the step).
Non-finite: NaN with the clip, every value of the side (1 550 / 1 050 / 83 450 / 42 845) NaN on all three paths and in float64; NaN without
the clip and inf with it, 5 values (the element in g, m, v, p, target); inf without the clip, 2 (p and the target: inf / inf).  The build
with fminf for the clip factor (the code before) fails both NaN cases.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import optim_restate
from mlp_optim_restate import step_restated
from mlp_restate import apply_seeded_

pytestmark = pytest.mark.gpu

TRAV = ["pre", "inlcrs", "postlcrs"]
MORPHS = {3: "3d_hopper_3_shin", 7: "3d_walker_7_full", 14: "3d_cheetah_14_full"}
HIDDEN = [(256, 256), (40, 72), (1, 7), (64, 48, 80, 33)]
NETS = [(L, h) for L in (3, 7) for h in HIDDEN] + [(14, (512, 500))]
NET_IDS = ["L%d-%s" % (L, "x".join(str(x) for x in h)) for L, h in NETS]
LR, BETAS, EPS, MAX_NORM = 1e-4, (0.9, 0.999), 1e-8, 0.1        # the reference's optimizers and grad_clipping_value
SIDES = ("critic", "actor")


def _graph(L, device="cuda:0"):
    from sgrl_amd import graph as G, mjcf
    return G.getGraphDict(mjcf.load_asset(MORPHS[L]).parents, TRAV, [], device=torch.device(device))


def _args(L, hidden=(256, 256), **over):
    from sgrl_amd.td3 import default_train_args
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L, **over)
    args.agent.policy_network = {"hidden_dims": list(hidden)}
    args.agent.q_network = {"hidden_dims": list(hidden)}
    return args


def _pair(L, hidden, seed):
    from sgrl_amd.mlp_policy import MlpCritic, MlpPolicy
    torch.manual_seed(seed)
    pol = MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, _args(L, hidden))
    crit = MlpCritic(41, 3, 32, 100, 3, True, False, False, _args(L, hidden))
    apply_seeded_(pol, seed)
    apply_seeded_(crit, seed + 1)
    return pol.to("cuda:0").train(), crit.to("cuda:0").train()


class Twin(object):
    """The four networks of one agent, persistent `.grad` tensors and one HipMlpGrads over them.  `reset` puts a state back and builds
    fresh optimizers (and a fresh HipMlpOptim) over it, so the same tensors serve the new path and both parent paths in turn."""

    def __init__(self, L, hidden, seed=5):
        from sgrl_amd.mlp_hip import HipMlpGrads
        pol, crit = _pair(L, hidden, seed)
        pol_t, crit_t = _pair(L, hidden, seed + 20)
        self.net = {"actor": pol, "critic": crit}
        self.target = {"actor": pol_t, "critic": crit_t}
        for s in SIDES:
            for p in self.net[s].parameters():
                p.grad = torch.zeros_like(p)
        self.grads = HipMlpGrads(pol, crit)
        self.start = {s: {"p": [p.detach().clone() for p in self.net[s].parameters()],
                          "t": [p.detach().clone() for p in self.target[s].parameters()]} for s in SIDES}
        self.opt, self.optim = {}, None

    def params(self, s):
        return list(self.net[s].parameters())

    def tparams(self, s):
        return list(self.target[s].parameters())

    def state(self, s, preload_seed=None):
        """A state of side s: the seeded parameters and targets, and either no Adam state or step 1000 with random m, v >= 0."""
        st = {"p": self.start[s]["p"], "t": self.start[s]["t"], "m": None, "v": None, "step": 0}
        if preload_seed is not None:
            g = torch.Generator(device="cuda:0").manual_seed(preload_seed)
            st["m"] = [torch.randn(p.shape, generator=g, device="cuda:0") * 1e-3 for p in st["p"]]
            st["v"] = [torch.randn(p.shape, generator=g, device="cuda:0") ** 2 * 1e-6 for p in st["p"]]
            st["step"] = 1000
        return st

    def gradients(self, s, seed, norm):
        """Seeded randn over all tensors of side s, scaled to the 2-norm `norm` (0: all zeros)."""
        g = torch.Generator(device="cuda:0").manual_seed(seed)
        gs = [torch.randn(p.shape, generator=g, device="cuda:0") for p in self.params(s)]
        total = float(torch.sqrt(sum((x.double() ** 2).sum() for x in gs)))
        return [x * (norm / total) for x in gs]

    def reset(self, states, capturable, hip):
        """states: {side: state}; sides not named keep what they hold (and their optimizer)."""
        from sgrl_amd.mlp_hip import HipMlpOptim
        with torch.no_grad():
            for s, st in states.items():
                for p, x in zip(self.params(s), st["p"]):
                    p.copy_(x)
                for p, x in zip(self.tparams(s), st["t"]):
                    p.copy_(x)
                opt = torch.optim.Adam(self.params(s), lr=LR, betas=BETAS, eps=EPS, capturable=capturable)
                if st["m"] is not None:
                    for p, m, v in zip(self.params(s), st["m"], st["v"]):
                        step = torch.tensor(float(st["step"]), dtype=torch.float32, device="cuda:0" if capturable else "cpu")
                        opt.state[p] = {"step": step, "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                self.opt[s] = opt
        for s in SIDES:
            if s not in self.opt:
                self.opt[s] = torch.optim.Adam(self.params(s), lr=LR, betas=BETAS, eps=EPS)
        self.optim = HipMlpOptim(self.grads, self.opt["actor"], self.opt["critic"], self.target["actor"], self.target["critic"]) if hip else None

    def set_grads(self, s, gs):
        with torch.no_grad():
            for p, x in zip(self.params(s), gs):
                p.grad.copy_(x)

    def step(self, s, max_norm, tau):
        """One optimizer step of side s on the path `reset` chose."""
        from sgrl_amd import td3
        if self.optim is not None:
            getattr(self.optim, s + "_step")(max_norm, tau)
        else:
            td3.clip_and_step(self.opt[s], max_norm)
            if tau > 0:
                td3.soft_update_network(self.net[s], self.target[s], tau)

    def read(self, s):
        """Clones of everything a step of side s may write."""
        ps = self.params(s)
        st = [self.opt[s].state[p] for p in ps]
        return {"p": [p.detach().clone() for p in ps], "g": [p.grad.clone() for p in ps],
                "m": [x["exp_avg"].clone() if x else torch.zeros_like(p) for x, p in zip(st, ps)],
                "v": [x["exp_avg_sq"].clone() if x else torch.zeros_like(p) for x, p in zip(st, ps)],
                "t": [p.detach().clone() for p in self.tparams(s)], "steps": [float(x["step"]) if x else 0.0 for x in st]}


@functools.lru_cache(maxsize=None)
def _twin(L, hidden):
    return Twin(L, hidden)


def _np64(xs):
    return [x.detach().double().cpu().numpy() for x in xs]


def _norms(xs, refs):
    """Per tensor (2-norm, max-norm) of x - ref in float64 -> two lists (one device sync)."""
    d = [x.double() - r for x, r in zip(xs, refs)]
    out = torch.stack([torch.stack([x.norm(), x.abs().max()]) for x in d]).cpu().numpy()
    return out[:, 0], out[:, 1]


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def _one_case(tw, s, what, state, grad_steps, tau, hip_capturable):
    """The new path and both parent paths from `state` over the gradients of grad_steps, checked after every step; returns the worst
    error / bar."""
    runs = {}
    for kind, cap, hip in (("hip", hip_capturable, True), ("capturable", True, False), ("plain", False, False)):
        tw.reset({s: state}, capturable=cap, hip=hip)
        outs = []
        for gs in grad_steps:
            tw.set_grads(s, gs)
            tw.step(s, MAX_NORM, tau)
            outs.append(tw.read(s))
        runs[kind] = outs
    names = [n for n, _ in tw.net[s].named_parameters()]
    p, t = _np64(state["p"]), _np64(state["t"])
    m = _np64(state["m"]) if state["m"] is not None else [np.zeros_like(x) for x in p]
    v = _np64(state["v"]) if state["v"] is not None else [np.zeros_like(x) for x in p]
    count, worst = state["step"], 0.0
    for k, gs in enumerate(grad_steps):
        p0, t0 = p, t
        p, g, m, v, count, t = step_restated(p, _np64(gs), m, v, count, LR, BETAS[0], BETAS[1], EPS, MAX_NORM, tau, t)
        ref = {key: [torch.from_numpy(x).cuda() for x in val] for key, val in (("p", p), ("g", g), ("m", m), ("v", v), ("t", t))}
        got = runs["hip"][k]
        assert got["steps"] == [float(count)] * len(names), (what, got["steps"])
        for key in ("g", "m", "v"):
            mag = _norms(ref[key], [torch.zeros_like(x) for x in ref[key]])
            e_hip, e_cap, e_plain = _norms(got[key], ref[key]), _norms(runs["capturable"][k][key], ref[key]), _norms(runs["plain"][k][key], ref[key])
            for i, nm in enumerate(("2", "max")):
                bar = 10.0 * np.minimum(e_cap[i], e_plain[i]) + 1e-5 * mag[i]
                ratio = np.where(bar > 0, e_hip[i] / np.where(bar > 0, bar, 1.0), 0.0)
                print("%s step %d %s %s-norm: error / bar %s" % (what, k + 1, key, nm, np.array2string(ratio, precision=3)))
                bad = np.nonzero(e_hip[i] > bar)[0]
                assert bad.size == 0, (what, k + 1, key, nm, [(names[j], e_hip[i][j], e_cap[i][j], e_plain[i][j], mag[i][j]) for j in bad])
                worst = max(worst, float(ratio.max()))
        for key, after, before in (("p", p, p0), ("t", t, t0)):
            err = _norms(got[key], ref[key])[0]
            step64 = np.array([float(np.sqrt(((a - b) ** 2).sum())) for a, b in zip(after, before)])
            bar = 2e-3 * step64 + np.array([np.sqrt(b.size) * np.abs(b).max() * 1.2e-7 for b in before])
            ratio = err / bar
            print("%s step %d %s: |step64| %s  error / bar %s" % (what, k + 1, key, np.array2string(step64, precision=3), np.array2string(ratio, precision=3)))
            assert (err <= bar).all(), (what, k + 1, key, [(names[j], err[j], bar[j]) for j in np.nonzero(err > bar)[0]])
            assert all(bool(torch.isfinite(x).all()) for x in got[key])
            worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("L,hidden", NETS, ids=NET_IDS)
def test_step_against_float64(L, hidden):
    tw = _twin(L, hidden)
    for s in SIDES:
        worst = 0.0
        for preload in (False, True):
            for scale, clip in ((10.0, "active"), (0.5, "inactive")):
                for tau in (0.0, 0.005, 1.0):
                    state = tw.state(s, preload_seed=77 if preload else None)
                    gsteps = [tw.gradients(s, 100 + k, scale * MAX_NORM) for k in range(1 if preload else 2)]
                    what = "L%d %s %s %s clip %s tau %g" % (L, hidden, s, "step 1000" if preload else "fresh", clip, tau)
                    worst = max(worst, _one_case(tw, s, what, state, gsteps, tau, hip_capturable=(L == 7)))
        print("L%d %s %s: worst error / bar %.3g" % (L, hidden, s, worst))


def _generated(tw, s, kind, seed):
    """Gradients of side s from optim_restate's generator (per tensor sign * scale * 2^U(-1, 1)): 'tiny' -- every tensor at 1e-11,
    where Adam's eps decides the step -- or 'mixed' -- scales 1e-13 ... 1e-2 across the tensors."""
    shapes = [tuple(p.shape) for p in tw.params(s)]
    return [torch.from_numpy(x).cuda() for x in optim_restate.draw_gradients(shapes, optim_restate.tensor_scales(kind, shapes, seed=3), seed)]


def _zero_start(tw, s):
    """The fresh state of side s with every parameter at zero: such parameters resolve any step (the step bar's floor vanishes)."""
    st = tw.state(s)
    return dict(st, p=[torch.zeros_like(x) for x in st["p"]])


@pytest.mark.parametrize("L,hidden", [(3, (1, 7)), (3, (40, 72))], ids=["L3-1x7", "L3-40x72"])
def test_step_against_float64_where_eps_decides(L, hidden):
    """The bars of test_step_against_float64 on the generator's gradient sets, from the seeded parameters and from zero: at 1e-11
    sqrt(v_hat) lies three decades below eps and the step is lr m_hat / eps, 1e-7 per element, which only the zero-start
    parameters (bar: 2e-3 of the step) and the m, v state resolve."""
    tw = _twin(L, hidden)
    for s in SIDES:
        worst = {}
        for kind in ("tiny", "mixed"):
            gsteps = [_generated(tw, s, kind, 500 + k) for k in range(3)]
            if kind == "tiny":
                v = _np64([(1 - BETAS[1]) * g.double() ** 2 for g in gsteps[0]])
                assert optim_restate.eps_share(v, [1] * len(v)) == 1.0
            for start, state in (("seeded", tw.state(s)), ("zero", _zero_start(tw, s))):
                for tau in (0.0, 0.005):
                    what = "L%d %s %s %s gradients from %s tau %g" % (L, hidden, s, kind, start, tau)
                    w = _one_case(tw, s, what, state, gsteps, tau, hip_capturable=(tau > 0))
                    worst[(kind, start)] = max(worst.get((kind, start), 0.0), w)
        print("L%d %s %s: worst error / bar %s" % (L, hidden, s, {"%s/%s" % k: "%.3g" % v for k, v in worst.items()}))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("L,hidden", [(3, (1, 7)), (3, (40, 72))], ids=["L3-1x7", "L3-40x72"])
def test_non_finite_gradients_spread_as_on_the_parent_path(L, hidden, bad):
    """One NaN (one inf) element in one gradient, ordinary floats in ordinary launches: with the clip a NaN total gives a NaN
    coefficient (torch.clamp propagates it in clip_grad_norm_) and NaN in g, m, v, p and the target of every tensor; an infinite
    total gives coef = 0 and a NaN in the element alone.  The NaN pattern of both parent paths and of the restatement; the finite
    values within the bars of test 1."""
    tw = _twin(L, hidden)
    tau = 0.005
    for s in SIDES:
        for max_norm in (MAX_NORM, 0.0):
            state = tw.state(s)
            gs = [x.clone() for x in tw.gradients(s, 61, 10 * MAX_NORM)]
            gs[1].view(-1)[-1] = bad
            runs = {}
            for kind, cap, hip in (("hip", False, True), ("capturable", True, False), ("plain", False, False)):
                tw.reset({s: state}, capturable=cap, hip=hip)
                tw.set_grads(s, gs)
                tw.step(s, max_norm, tau)
                runs[kind] = {k: _np64(v) if k != "steps" else v for k, v in tw.read(s).items()}
            zeros = [np.zeros(x.shape) for x in state["p"]]
            p, g, m, v, count, t = step_restated(_np64(state["p"]), _np64(gs), zeros, zeros, 0, LR, BETAS[0], BETAS[1], EPS, max_norm, tau, _np64(state["t"]))
            ref = {"p": p, "g": g, "m": m, "v": v, "t": t}
            assert runs["hip"]["steps"] == runs["plain"]["steps"] == [1.0] * len(p)
            n_nan = 0
            for key in ("p", "g", "m", "v", "t"):
                for i, (a, r) in enumerate(zip(runs["hip"][key], ref[key])):
                    nan = np.isnan(a)
                    n_nan += int(nan.sum())
                    for other in (runs["capturable"][key][i], runs["plain"][key][i], r):
                        assert np.array_equal(nan, np.isnan(other)), (s, max_norm, key, i)
                        assert np.array_equal(np.isinf(a), np.isinf(other)) and np.array_equal(a[np.isinf(a)], other[np.isinf(a)]), (s, max_norm, key, i)
                    fin = np.isfinite(r)
                    if not fin.any():
                        continue
                    if key in ("g", "m", "v"):                     # max-norm: the parents' ceiling and the floor
                        e = lambda x: float(np.abs(x[fin] - r[fin]).max())
                        bar = 10.0 * min(e(runs["capturable"][key][i]), e(runs["plain"][key][i])) + 1e-5 * float(np.abs(r[fin]).max())
                    else:                                          # 2-norm: the step bar
                        e = lambda x: float(np.sqrt(((x[fin] - r[fin]) ** 2).sum()))
                        before = _np64(state[key])[i]
                        bar = 2e-3 * float(np.sqrt(((r - before)[fin] ** 2).sum())) + np.sqrt(r.size) * float(np.abs(before).max()) * 1.2e-7
                    assert e(a) <= bar, (s, max_norm, key, i, e(a), bar)
            total = sum(x.size for key in ("p", "g", "m", "v", "t") for x in ref[key])
            print("L%d %s %s %s max_norm %g: %d of %d values NaN" % (L, hidden, s, bad, max_norm, n_nan, total))
            assert n_nan == (total if (np.isnan(bad) and max_norm > 0) else (5 if (np.isnan(bad) or max_norm > 0) else 2))
    tw.reset({s: tw.state(s) for s in SIDES}, capturable=False, hip=False)     # the shared twin is left finite
    for s in SIDES:
        tw.set_grads(s, [torch.zeros_like(p) for p in tw.params(s)])


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hidden,capturable", [(3, (1, 7), False), (7, (256, 256), True), (3, (64, 48, 80, 33), False)],
                         ids=["L3-1x7-plain", "L7-256x256-capturable", "L3-64x48x80x33-plain"])
def test_bit_exact_properties(L, hidden, capturable):
    tw = _twin(L, hidden)
    fresh = {s: tw.state(s) for s in SIDES}
    loaded = {s: tw.state(s, preload_seed=31) for s in SIDES}

    def run(states, s, gs, max_norm, tau):
        tw.reset(states, capturable=capturable, hip=True)
        tw.set_grads(s, gs)
        tw.step(s, max_norm, tau)
        return tw.read(s)

    for s in SIDES:
        other = "actor" if s == "critic" else "critic"
        big, small = tw.gradients(s, 5, 10 * MAX_NORM), tw.gradients(s, 6, 0.5 * MAX_NORM)
        # tau = 1: the lerp reads the parameter the same pass has just written
        out = run(loaded, s, big, MAX_NORM, 1.0)
        assert _equal(out["t"], out["p"]) and not _equal(out["p"], loaded[s]["p"])
        # the same state twice: the same bits (clip active: the sum of squares included)
        again = run(loaded, s, big, MAX_NORM, 1.0)
        assert all(_equal(out[k], again[k]) for k in ("p", "g", "m", "v", "t"))
        assert not _equal(out["g"], big)                                         # the clip bit: .grad was scaled
        # max_norm = 0 and an inactive clip: the same p, m, v; .grad untouched by either
        a, b = run(loaded, s, small, 0.0, 0.005), run(loaded, s, small, MAX_NORM, 0.005)
        assert all(_equal(a[k], b[k]) for k in ("p", "m", "v", "t"))
        assert _equal(a["g"], small) and _equal(b["g"], small)
        # tau = 0: the target is left alone
        z = run(loaded, s, small, MAX_NORM, 0.0)
        assert _equal(z["t"], loaded[s]["t"]) and _equal(z["p"], b["p"])
        # all-zero gradients from fresh state: p unchanged, everything finite
        zero = [torch.zeros_like(x) for x in big]
        for mn in (MAX_NORM, 0.0):
            o = run(fresh, s, zero, mn, 0.005)
            assert _equal(o["p"], fresh[s]["p"]) and o["steps"] == [1.0] * len(zero)
            assert all(bool(torch.isfinite(x).all()) for k in ("p", "g", "m", "v", "t") for x in o[k])
        # a step of one side leaves the other side's parameters, gradients, state and target alone
        tw.reset(loaded, capturable=capturable, hip=True)
        tw.set_grads(other, tw.gradients(other, 9, 10 * MAX_NORM))
        tw.step(other, MAX_NORM, 0.005)                                          # so that the other side has state of its own
        before = tw.read(other)
        tw.set_grads(s, big)
        tw.step(s, MAX_NORM, 0.005)
        after = tw.read(other)
        assert all(_equal(before[k], after[k]) for k in ("p", "g", "m", "v", "t")) and before["steps"] == after["steps"]


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True], ids=["plain", "capturable"])
def test_switching_between_the_paths(capturable):
    """3 steps here then 2 on clip_and_step, and 2 there then 3 here, against 5 on clip_and_step: parameters and targets within the
    step bar accumulated over the five steps, every state[p]["step"] == 5."""
    from sgrl_amd import td3
    tw = _twin(7, (40, 72))
    tau = 0.005
    for s in SIDES:
        state = tw.state(s, preload_seed=None)
        gsteps = [tw.gradients(s, 300 + k, (10.0 if k % 2 == 0 else 0.5) * MAX_NORM) for k in range(5)]

        def parent_step():
            td3.clip_and_step(tw.opt[s], MAX_NORM)
            td3.soft_update_network(tw.net[s], tw.target[s], tau)

        results, tol = {}, {"p": 0.0, "t": 0.0}
        for name, here in (("parent", ()), ("here-first", (0, 1, 2)), ("here-last", (2, 3, 4))):
            tw.reset({s: state}, capturable=capturable, hip=True)
            for k, gs in enumerate(gsteps):
                tw.set_grads(s, gs)
                before = tw.read(s) if name == "parent" else None
                if k in here:
                    tw.step(s, MAX_NORM, tau)
                else:
                    parent_step()
                if name == "parent":
                    after = tw.read(s)
                    for key in ("p", "t"):
                        step = np.array([float((a.double() - b.double()).norm()) for a, b in zip(after[key], before[key])])
                        floor = np.array([np.sqrt(b.numel()) * float(b.abs().max()) * 1.2e-7 for b in before[key]])
                        tol[key] = tol[key] + 2e-3 * step + floor
            results[name] = tw.read(s)
            assert results[name]["steps"] == [5.0] * len(gsteps[0]), (name, results[name]["steps"])
        for name in ("here-first", "here-last"):
            for key in ("p", "t"):
                d = _norms(results[name][key], [x.double() for x in results["parent"][key]])[0]
                print("switching %s %s %s %s: |here - parent| %s  tolerance %s" % ("capturable" if capturable else "plain", s, name, key,
                                                                                 np.array2string(d, precision=3), np.array2string(tol[key], precision=3)))
                assert (d <= tol[key]).all(), (s, name, key)
        # and the optimizer's own step() continues the count from here
        tw.opt[s].step()
        assert [float(tw.opt[s].state[p]["step"]) for p in tw.params(s)] == [6.0] * len(gsteps[0])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_returned_before_any_launch():
    from sgrl_amd.mlp_hip import HipMlpActor
    tw = _twin(3, (40, 72))
    tw.reset({s: tw.state(s, preload_seed=3) for s in SIDES}, capturable=True, hip=True)
    for s in SIDES:
        tw.set_grads(s, tw.gradients(s, 1, 1.0))
        tw.step(s, MAX_NORM, 0.005)                      # bound, with targets
    torch.cuda.synchronize()
    L = tw.grads.L
    h = {"actor": tw.grads.actor.h, "critic": tw.grads.critic.h}
    null = ctypes.c_void_p(None)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = lambda: L.sgrl_mlp_last_error()
    step = lambda hh, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, mn=0.1, tau=0.005: L.sgrl_mlp_optim_step(hh, lr, b1, b2, eps, mn, tau, st)
    ERR = -1
    everything = []
    for s in SIDES:
        ps = tw.params(s)
        everything += [p.data for p in ps] + [p.grad for p in ps] + [p.data for p in tw.tparams(s)]
        everything += [tw.opt[s].state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq", "step")]
    for t in everything:
        t.fill_(7.0)
    assert step(null) == ERR and b"null handle" in err()
    for s in SIDES:
        assert L.sgrl_mlp_optim_bound(h[s]) == 1
        assert step(h[s], tau=-0.1) == ERR and b"tau outside" in err()
        assert step(h[s], tau=1.5) == ERR and b"tau outside" in err()
        assert step(h[s], mn=-1.0) == ERR and b"max_norm is negative" in err()
        for kw in ("lr", "b1", "b2", "eps", "mn", "tau"):
            for bad in (float("nan"), float("inf")):
                assert step(h[s], **{kw: bad}) == ERR and b"not finite" in err(), (kw, bad)
    # parameters / gradients / state not bound; tau > 0 with no target bound
    fresh = ctypes.c_void_p()
    assert L.sgrl_mlp_create(ctypes.byref(fresh)) == 0
    try:
        assert step(fresh) == ERR and b"parameters not set" in err()
        assert L.sgrl_mlp_bind_optim(fresh, null, null, 0, null, 0, null, 0, null, 0) == ERR
    finally:
        L.sgrl_mlp_destroy(fresh)
    pol = tw.net["actor"]
    other = HipMlpActor(pol)
    other.sync_weights()
    assert step(other.h) == ERR and b"gradients not bound" in err()
    ps = other._params()
    cast = lambda ptrs: ctypes.cast((ctypes.c_void_p * len(ptrs))(*ptrs), ctypes.c_void_p)
    g_arr = cast([p.grad.data_ptr() for p in ps])
    m_arr = cast([tw.opt["actor"].state[p]["exp_avg"].data_ptr() for p in ps])
    v_arr = cast([tw.opt["actor"].state[p]["exp_avg_sq"].data_ptr() for p in ps])
    s_arr = cast([tw.opt["actor"].state[p]["step"].data_ptr() for p in ps])
    t_arr = cast([p.data_ptr() for p in tw.target["actor"].actor.parameters()])
    partials = torch.full((512,), 7.0, device="cuda:0")
    pp = ctypes.c_void_p(partials.data_ptr())
    n = len(ps)
    assert L.sgrl_mlp_bind_optim(other.h, m_arr, v_arr, n, s_arr, n, null, 0, pp, 512) == ERR and b"gradients not bound" in err()
    assert L.sgrl_mlp_bind_grads(other.h, g_arr, n) == 0
    assert step(other.h) == ERR and b"state not bound" in err()
    assert L.sgrl_mlp_bind_optim(other.h, m_arr, v_arr, n - 1, s_arr, n, null, 0, pp, 512) == ERR and b"expected" in err()
    assert L.sgrl_mlp_bind_optim(other.h, m_arr, v_arr, n, s_arr, 0, null, 0, pp, 512) == ERR and b"step counters" in err()
    assert L.sgrl_mlp_bind_optim(other.h, m_arr, v_arr, n, s_arr, n, t_arr, n - 1, pp, 512) == ERR and b"target addresses" in err()
    assert L.sgrl_mlp_bind_optim(other.h, m_arr, v_arr, n, s_arr, n, null, 0, pp, 3) == ERR and b"partials" in err()
    assert L.sgrl_mlp_bind_optim(other.h, m_arr, v_arr, n, s_arr, n, null, 0, pp, 512) == 0 and L.sgrl_mlp_optim_bound(other.h) == 1
    assert step(other.h, tau=0.005) == ERR and b"no target bound" in err()
    # a later parameter bind drops the gradient bind and the state bind; binding the gradients again does not bring the state back
    other.sync_weights(force=True)
    assert L.sgrl_mlp_optim_bound(other.h) == 0
    assert step(other.h, tau=0.0) == ERR and b"gradients not bound" in err()
    assert L.sgrl_mlp_bind_grads(other.h, g_arr, n) == 0
    assert step(other.h, tau=0.0) == ERR and b"state not bound" in err()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in everything) and bool((partials == 7).all())      # none of the refused calls wrote anything
    # and the well-formed calls go through
    assert L.sgrl_mlp_bind_optim(other.h, m_arr, v_arr, n, s_arr, n, t_arr, n, pp, 512) == 0
    assert step(other.h, tau=1.0) == 0 and step(h["critic"]) == 0
    torch.cuda.synchronize()
    for s in SIDES:
        for p, t in zip(tw.params(s), tw.tparams(s)):
            assert float(tw.opt[s].state[p]["step"]) == 8.0 and not bool((p == 7).all())
            assert bool((tw.opt[s].state[p]["exp_avg_sq"] < 49.0).all())
    assert _equal(tw.params("actor"), tw.tparams("actor"))                                     # tau = 1


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def _seeded_agent(optim, L=7, seed=3):
    from sgrl_amd.td3 import Agent
    torch.manual_seed(seed)
    a = Agent(_args(L), device=torch.device("cuda:0"), mlp_hip_grads=True, mlp_hip_optim=optim)
    for mod, sd in ((a.actor, 3), (a.critic, 4), (a.actor_target, 5), (a.critic_target, 6)):
        apply_seeded_(mod, sd)
    a.change_morphology(_graph(L))
    a.models2train()
    return a


def _update_batch(g, n=64):
    batch = {"obs": torch.randn((n, 287), generator=g), "next_obs": torch.randn((n, 287), generator=g),
             "action": torch.rand((n, 21), generator=g) * 2 - 1, "reward": torch.randn((n, 1), generator=g),
             "done": (torch.rand((n, 1), generator=g) < 0.2).float()}
    return {k: v.cuda() for k, v in batch.items()}, (torch.randn((n, 21), generator=g) * 0.2).cuda()


def test_twenty_updates_against_the_parent_path():
    """From one seeded state, twenty updates (ten with the actor step) with and without the optimizer half on HIP: every parameter
    tensor of the four networks within the step-norm tolerance of test_twenty_updates_against_the_pytorch_gradient_half (2e-3 of the
    step's norm plus sqrt(numel) * max|p| * 1.2e-7), accumulated over the updates; Adam's step counts agree."""
    from sgrl_amd.mlp_hip import HipMlpOptim
    new, old = _seeded_agent(True), _seeded_agent(None)
    assert new.use_mlp_hip_optim and not old.use_mlp_hip_optim
    old.load_state_dict(new.state_dict())
    nets = ("actor", "critic", "actor_target", "critic_target")
    tol = {nm: [0.0] * len(list(getattr(old, nm).parameters())) for nm in nets}
    g = torch.Generator().manual_seed(77)
    for it in range(20):
        batch, noise = _update_batch(g)
        before = {nm: [p.detach().double().clone() for p in getattr(old, nm).parameters()] for nm in nets}
        la, lb = new.update(batch, it, noise=noise), old.update(batch, it, noise=noise)
        assert sorted(la) == sorted(lb) and all(np.isfinite(float(v)) for v in la.values())
        for nm in nets:
            for i, (p, q) in enumerate(zip(getattr(old, nm).parameters(), before[nm])):
                tol[nm][i] += 2e-3 * float((p.detach().double() - q).norm()) + np.sqrt(p.numel()) * float(q.abs().max()) * 1.2e-7
    assert isinstance(new._mlp_optim, HipMlpOptim) and new.mlp_hip_optim_refusal is None and old._mlp_optim is None
    for nm in nets:
        for i, ((name, p), q) in enumerate(zip(getattr(new, nm).named_parameters(), getattr(old, nm).parameters())):
            d = float((p.detach().double() - q.detach().double()).norm())
            print("20 updates %s %s: |new - parent| %.3g  tolerance %.3g" % (nm, name, d, tol[nm][i]))
            assert d <= tol[nm][i], (nm, name, d, tol[nm][i])
    for a in (new, old):
        assert [float(a.critic_optimizer.state[p]["step"]) for p in a.critic.parameters()] == [20.0] * 12
        assert [float(a.actor_optimizer.state[p]["step"]) for p in a.actor.parameters()] == [10.0] * 6
    # the state_dicts are interchangeable: the parent path continues from the new path's optimizer state
    old.load_state_dict(new.state_dict())
    old.critic_optimizer.load_state_dict(new.critic_optimizer.state_dict())
    batch, noise = _update_batch(g)
    out = old.update(batch, 21, noise=noise)
    assert np.isfinite(float(out["loss/critic_loss"])) and float(old.critic_optimizer.state[next(old.critic.parameters())]["step"]) == 21.0


def test_unserved_optimizers_keep_the_parent_path():
    a = _seeded_agent(True)
    a.critic_optimizer = torch.optim.Adam(a.critic.parameters(), lr=1e-4, weight_decay=1e-2)
    g = torch.Generator().manual_seed(5)
    batch, noise = _update_batch(g, 9)
    out = a.update(batch, 0, noise=noise)
    assert all(np.isfinite(float(v)) for v in out.values()) and "loss/actor_loss" in out
    assert a._mlp_optim is None and "weight decay" in a.mlp_hip_optim_refusal and a.use_mlp_hip_optim
    a.critic_optimizer = torch.optim.Adam(a.critic.parameters(), lr=1e-4)
    a.update(batch, 1, noise=noise)
    assert a._mlp_optim is not None and a.mlp_hip_optim_refusal is None


def test_new_path_replays_the_reference_update(golden_dir):
    """tests/golden/td3_update_mlp.npz (the executed reference's Agent.update) through the new path: losses, step norms and the
    parameter sums of all four networks at the tolerances of test_mlp_grads_gpu's replay."""
    from sgrl_amd import td3
    from sgrl_amd.td3 import Agent, default_train_args
    z = np.load(os.path.join(golden_dir, "td3_update_mlp.npz"))
    hyper = dict(zip([str(k) for k in z["hyper_keys"]], z["hyper_vals"]))
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=7, lr=hyper["lr"], policy_noise=hyper["policy_noise"],
                              noise_clip=hyper["noise_clip"], discount=hyper["discount"], policy_freq=int(hyper["policy_freq"]),
                              grad_clipping_value=hyper["grad_clipping_value"], max_action=hyper["max_action"])
    args.agent.target_smoothing_tau, args.agent.reward_scale = hyper["target_smoothing_tau"], hyper["reward_scale"]
    agent = Agent(args, device=torch.device("cuda:0"), mlp_hip_grads=True, mlp_hip_optim=True)
    assert agent.use_mlp_hip_optim
    apply_seeded_(agent.actor, int(z["seed"]))
    apply_seeded_(agent.critic, int(z["seed"]))
    with torch.no_grad():
        for tgt, src in ((agent.actor_target, agent.actor), (agent.critic_target, agent.critic)):
            for tp, sp in zip(tgt.parameters(), src.parameters()):
                tp.copy_(0.97 * sp)
    agent.change_morphology(_graph(7))
    agent.models2train()
    called = []
    real = td3.clip_and_step
    td3.clip_and_step = lambda opt, max_norm: called.append(opt) or real(opt, max_norm)
    try:
        for it in range(2):
            tag = "it%d/" % it
            batch = {k: torch.from_numpy(z[tag + k]).cuda() for k in ("obs", "action", "next_obs", "reward", "done")}
            before = {nm: [p.detach().double().clone() for p in getattr(agent, nm).parameters()] for nm in ("actor", "critic")}
            loss = agent.update(batch, it, noise=torch.from_numpy(z[tag + "noise"]).cuda())
            ref_cl = float(z[tag + "critic_loss"])
            print("reference update %d: critic_loss %.9g  reference %.9g" % (it, float(loss["loss/critic_loss"]), ref_cl))
            assert abs(float(loss["loss/critic_loss"]) - ref_cl) < 1e-4 * abs(ref_cl), it
            ref_al = float(z[tag + "actor_loss"])
            assert np.isnan(ref_al) == ("loss/actor_loss" not in loss)
            if not np.isnan(ref_al):
                assert abs(float(loss["loss/actor_loss"]) - ref_al) < 1e-4 * abs(ref_al) + 2e-6
            assert abs(loss["misc/train_reward_mean"] - float(z[tag + "train_reward_mean"])) < 1e-6
            for nm in ("critic", "actor"):
                st = np.array([float((p.detach().double() - q).norm()) for p, q in zip(getattr(agent, nm).parameters(), before[nm])])
                st64 = z[tag + nm + "_step_norms_f64"]
                ulp_floor = np.sqrt(z[nm + "_numel"]) * np.array([float(q.abs().max()) for q in before[nm]]) * 1.2e-7
                print("reference update %d %s: |step - step64| / tolerance %s" % (it, nm, np.array2string(np.abs(st - st64) / (2e-3 * st64 + ulp_floor), precision=3)))
                assert (np.abs(st - st64) <= 2e-3 * st64 + ulp_floor).all(), (it, nm)
                if tag + nm + "_grad_norms" not in z.files:
                    assert st.max() == 0.0
            for nm in ("actor", "critic", "actor_target", "critic_target"):
                got = np.array([float(p.detach().double().sum()) for p in getattr(agent, nm).parameters()])
                ref = z[tag + nm + "_param_sums"]
                numel = np.array([p.numel() for p in getattr(agent, nm).parameters()])
                assert (np.abs(got - ref) <= 2e-3 * hyper["lr"] * numel + 1e-6 * np.abs(ref) + 1e-7).all(), (it, nm)
    finally:
        td3.clip_and_step = real
    assert called == [] and agent._mlp_optim is not None       # the whole optimizer side ran on the new path


def test_device_trainer_trains_on_the_optimizer_path():
    from sgrl_amd.mlp_hip import HipMlpOptim
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_hip_grads=True)
    args.mlp_hip_optim = True
    tr = DeviceTrainer(["3d_hopper_3_shin"], 4, args=args, seed=2, device="cuda:0", max_buffer_size=4096, batch_size=64)
    assert tr.agent.use_mlp_hip_optim and tr.agent._mlp_optim is None
    tr.warmup(8)
    s = tr.train_round(max_steps=40, max_iters=2)
    assert s["per_morph_iter"] == 2
    assert isinstance(tr.agent._mlp_optim, HipMlpOptim)
    losses = tr.last_losses["3d_hopper_3_shin"]
    assert all(np.isfinite(float(v)) for v in losses.values())
    assert float(tr.agent.critic_optimizer.state[next(tr.agent.critic.parameters())]["step"]) == 2.0


@pytest.mark.parametrize("capturable", [False, True], ids=["plain", "capturable"])
def test_binds_again_when_a_tensor_has_moved(capturable):
    """A gradient, a state tensor, a target parameter and a parameter replaced by copies between two steps: the second step reads and
    writes the new tensors and ends with the bits of the undisturbed run."""
    tw = _twin(3, (40, 72))
    for s in SIDES:
        g1, g2 = tw.gradients(s, 41, 10 * MAX_NORM), tw.gradients(s, 42, 10 * MAX_NORM)
        outs = []
        for move in (False, True):
            tw.reset({s: tw.state(s)}, capturable=capturable, hip=True)
            tw.set_grads(s, g1)
            tw.step(s, MAX_NORM, 0.005)
            old = None
            if move:
                p0, p1 = tw.params(s)[0], tw.params(s)[1]
                t0 = tw.tparams(s)[0]
                st = tw.opt[s].state[p0]
                old = (p0.grad, st["exp_avg"], st["exp_avg_sq"], t0.data, p1.data)
                p0.grad = p0.grad.clone()
                st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
                t0.data = t0.data.clone()
                p1.data = p1.data.clone()
                kept = [x.clone() for x in old]
            tw.set_grads(s, g2)
            tw.step(s, MAX_NORM, 0.005)
            outs.append(tw.read(s))
            if move:
                assert all(torch.equal(x, y) for x, y in zip(old, kept))             # the tensors left behind were not touched
                tw.params(s)[0].grad = old[0]                                         # the twin's persistent tensors back in place
                tw.tparams(s)[0].data, tw.params(s)[1].data = old[3], old[4]
        assert all(_equal(outs[0][k], outs[1][k]) for k in ("p", "g", "m", "v", "t")) and outs[0]["steps"] == outs[1]["steps"] == [2.0] * len(g1)


def test_a_second_step_allocates_nothing_and_launch_counts():
    tw = _twin(3, (40, 72))
    for capturable in (False, True):
        tw.reset({s: tw.state(s) for s in SIDES}, capturable=capturable, hip=True)
        assert tw.optim.launches() == 2
        for s in SIDES:
            tw.set_grads(s, tw.gradients(s, 2, 1.0))
        for s in SIDES:
            tw.step(s, MAX_NORM, 0.005)
        torch.cuda.synchronize()
        mem, gen = torch.cuda.memory_allocated(), (tw.grads.actor.generation(), tw.grads.critic.generation())
        keys = (tw.optim._actor.key, tw.optim._critic.key)
        versions = [p._version for s in SIDES for p in tw.params(s) + tw.tparams(s)]
        for s in SIDES:
            tw.step(s, MAX_NORM, 0.005)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == mem
        assert gen == (tw.grads.actor.generation(), tw.grads.critic.generation())
        assert keys == (tw.optim._actor.key, tw.optim._critic.key)                     # nothing was bound again
        assert all(p._version > v for p, v in zip([p for s in SIDES for p in tw.params(s) + tw.tparams(s)], versions))
    p = tw.optim.plan()
    assert p["actor"]["chunks"] >= p["actor"]["tensors"] == 6 and p["critic"]["tensors"] == 12
