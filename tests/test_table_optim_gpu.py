"""The table optimizer (csrc/train_gemm.hip k_opt_sqnorm / k_opt_total / k_opt_adam / k_opt_lerp over include/sgrl_train.h
sgrl_optim_clip_adam / sgrl_optim_lerp; td3.clip_and_step, td3.soft_update_network) against float64 on the MI355X, where Adam's eps
decides the step as well as where it does not.  The yardstick and the inputs are tests/optim_restate.py, qualified on the CPU by
tests/test_table_optim.py.

THE TABLE: optim_restate.table_shapes(), 300 tensors -- 1, 1023, 1024, 1025 and 2049 elements (the edges of the 1024-element chunk
cut), (3, 3, 3), (30, 128), one tensor of 300 x 1024 (more partial sums than k_opt_total has threads), the rest 1 to 7 elements; rows
256, 257 and 290 hold real work past the stride of k_opt_total's counter loop.  Every field (p, g, m, v) lives in ONE flat buffer
the tensors are views of, at 4-byte granularity: a write past a tensor's end lands in its neighbour and is seen.

THREE IMPLEMENTATIONS on identical state, each against the float64 restatement: the table path (_TABLE_OPT = True, capturable
group), torch's own (_TABLE_OPT = False, plain group: clip_grad_norm_ + torch.optim.Adam.step -- "parent32"), and the adam_step
fall-through (a plain group with _TABLE_OPT = True; a capturable group with _TABLE_OPT = False and either _FUSED_ADAM arm).

BARS, per tensor in the max-norm, for g, m and v:     |got - f64| <= 10 |parent32 - f64| + 1e-5 max|x64|
parameters from zero: the same with max|x64| replaced by the tensor's largest accumulated |step64| (sum over the steps so far of
|step64| per element: steps of alternating sign cancel, their rounding does not); parameters from randn: the project's step bar in
the 2-norm, 2e-3 |step64| + sqrt(numel) max|p| 1.2e-7, accumulated over the steps.  Tensors that had no gradient are held to
equality with their state.

1  seven regimes (optim_restate.REGIMES), five steps each, from zero and from randn parameters
2  counts 0, 1, 1000 and 100000 in one table, m and v at the tensors' own scales, some gradients None on the second of three
   steps: every counter reads back exactly, every tensor moves by the bias corrections of its OWN count
3  the soft update against float64 for tau in {0, 0.005, 1}, and 200 successive updates toward a fixed source
4  one NaN / one inf element in one small tensor: the NaN pattern of torch's own path in g, m, v and p of EVERY tensor
5  the same state and gradients twice give the same bits

MEASURED on the MI355X (the printed lines of a run; 22 tests in 8 s).  Worst error / bar over the five steps and all of g, m, v, p,
from zero | from randn parameters; "ceiling": parent32's own worst error over the 1e-5 floor (what the factor 10 multiplies):
    regime          table            fall-fused       fall-foreach     parent32         ceiling
    unit-clip       0.271 | 0.271    0.162 | 0.211    0.829 | 0.211    0.099 | 0.211    13.7
    tiny-eps        0.052 | 0.445    0.052 | 0.445    0.094 | 0.445    0.094 | 0.445    1.51
    mixed-clip      0.201 | 0.436    0.201 | 0.436    0.824 | 0.436    0.063 | 0.436    0.174
    mixed-noclip    0.097 | 0.386    0.097 | 0.386    0.833 | 0.386    0.076 | 0.386    0.312
    mixed-maxnorm0  0.064 | 0.403    0.064 | 0.403    0.820 | 0.403    0.091 | 0.403    1.00
    just-under      0.124 | 0.211    0.124 | 0.211    0.830 | 0.211    0.086 | 0.211    0.622
    just-over       0.263 | 0.263    0.097 | 0.217    0.827 | 0.217    0.100 | 0.217    121
    mixed counts    0.019 | 0.382    0.024 | 0.382    0.979 | 0.382    0.054 | 0.382    0.118
fall-plain is parent32 to the digit.  From randn the figure is the parameters' own rounding (half an ulp of p per step, the same
on every path) under the step bar: at 1e-11 the whole step is one ulp of a parameter of magnitude 1, which is why only the zero
start and the m, v state see it.  The ceilings of 13.7 and 121 are m of one-element tensors whose five gradients cancel; the table
path stays at 0.27 of its bar there.  fall-foreach at 0.82 ... 0.98 is torch's capturable arithmetic, which that arm copies bit for
bit: 1 - beta2 ** step is formed in float32 from 0.999 rounded to 0.99900001287, and sqrt(1 - b2^t) is off by 6.4e-6, 9.8e-6, 3.3e-6,
9.4e-6, 8.8e-6 at t = 1 ... 5 and 3.7e-6 at t = 1001 (the table kernel and torch's fused kernel form it in double: 2e-7).  It is a
function of the count alone, so the margin does not move with the data; wherever eps decides ('tiny-eps') it drops out.
Soft update: one update, max error 2.6e-7 against the foreach path's 3.6e-7; 200 updates 3.3e-6 against 1.7e-5; worst per tensor error / bar 0.098.  Non-finite: NaN with the clip, 317 365 of 317 365
elements of each of g, m, v, p on all three of table, parent32 and float64; NaN without the clip and inf with it, the element alone;
inf without the clip, NaN in p alone (inf / inf) and inf in g, m, v.

TEETH: four wrong builds of the kernels (scratch copies, not committed) against this file and against the older kernel-level test,
tests/test_train_ops_gpu.py::test_table_optimizer_steps_match_torch:
    eps added before the division by bc2_sqrt    fails all 14 regime cases, both mixed-count cases and inf-clip here; the old test
                                                 already caught it (all three of its cases: its gradients of 0.01 leave eps visible)
    bias correction at t - 1                     fails 20 of the 22 tests here (1 - b1^0 = 0 at the first step); the old test
                                                 already caught it (all three cases)
    every row reading row 0's step counter       passes the old test (every tensor on one count) and every single-count test here;
                                                 fails test_every_tensor_steps_by_its_own_count, both starts
    fminf for the clip factor (the code before)  passes the old test; fails test_non_finite_gradients_spread_as_in_torch[nan-clip]
                                                 here and both NaN cases of test_mlp_optim_gpu.py
"""
import functools

import numpy as np
import pytest
import torch

import optim_restate as R

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 1e-4, (0.9, 0.999), 1e-8
DEV = "cuda:0"
FIELDS = ("p", "g", "m", "v")
# name -> (_TABLE_OPT, capturable group, _FUSED_ADAM or None: as the module has it)
IMPLS = {"table": (True, True, None), "parent32": (False, False, None), "fall-plain": (True, False, None),
         "fall-fused": (False, True, True), "fall-foreach": (False, True, False)}


class Table(object):
    """The tensors of optim_restate.table_shapes() as views of one flat device buffer per field, the capturable step counters as
    views of one more, and `run`: an implementation over a start state and a list of gradient sets, everything read back flat."""

    def __init__(self, shapes):
        self.shapes, self.sizes = shapes, R.sizes_of(shapes)
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.total = int(self.offs[-1])
        self.flat = {k: torch.zeros(self.total, dtype=torch.float32, device=DEV) for k in FIELDS + ("dst",)}
        self.steps = torch.zeros(len(shapes), dtype=torch.float32, device=DEV)
        view = lambda k: [self.flat[k][a:a + n].view(s) for a, n, s in zip(self.offs[:-1].tolist(), self.sizes, shapes)]
        self.params = [torch.nn.Parameter(x) for x in view("p")]
        self.views = {k: view(k) for k in ("g", "m", "v")}
        self.dst = [torch.nn.Parameter(x) for x in view("dst")]
        assert all(p.data_ptr() == self.flat["p"].data_ptr() + 4 * int(a) for p, a in zip(self.params, self.offs))

    def flatten(self, xs, dtype=np.float64):
        return np.concatenate([np.asarray(x, dtype=dtype).ravel() for x in xs])

    def put(self, key, xs):
        self.flat[key].copy_(torch.from_numpy(self.flatten(xs, np.float32)))

    def get(self, key):
        return self.flat[key].double().cpu().numpy()

    def permax(self, flat):
        return np.maximum.reduceat(np.abs(flat), self.offs[:-1])

    def per2(self, flat):
        return np.sqrt(np.add.reduceat(flat * flat, self.offs[:-1]))

    def run(self, impl, p0, grad_steps, max_norm, counts=None, m0=None, v0=None):
        """-> per step {"p", "g", "m", "v": flat float64 arrays, "t": the counters}.  grad_steps[k][i] may be None."""
        from sgrl_amd import td3
        table_opt, capturable, fused = IMPLS[impl]
        n = len(self.shapes)
        self.put("p", p0)
        self.put("m", m0 if m0 is not None else [np.zeros(s) for s in self.shapes])
        self.put("v", v0 if v0 is not None else [np.zeros(s) for s in self.shapes])
        counts = [0] * n if counts is None else counts
        self.steps.copy_(torch.tensor(counts, dtype=torch.float32))
        opt = torch.optim.Adam(self.params, lr=LR, betas=BETAS, eps=EPS, capturable=capturable)
        for i, p in enumerate(self.params):
            step = self.steps[i] if capturable else torch.tensor(float(counts[i]), dtype=torch.float32)
            opt.state[p] = {"step": step, "exp_avg": self.views["m"][i], "exp_avg_sq": self.views["v"][i]}
        keep = (td3._TABLE_OPT, td3._FUSED_ADAM)
        outs = []
        try:
            td3._TABLE_OPT = table_opt
            if fused is not None:
                td3._FUSED_ADAM = fused
            for gs in grad_steps:
                self.put("g", [np.zeros(s) if g is None else g for g, s in zip(gs, self.shapes)])
                for p, g, view in zip(self.params, gs, self.views["g"]):
                    p.grad = None if g is None else view
                td3.clip_and_step(opt, max_norm)
                out = {k: self.get(k) for k in FIELDS}
                out["t"] = self.steps.cpu().tolist() if capturable else [float(opt.state[p]["step"]) for p in self.params]
                outs.append(out)
        finally:
            td3._TABLE_OPT, td3._FUSED_ADAM = keep
            for p in self.params:
                p.grad = None
        return outs


@functools.lru_cache(maxsize=None)
def _table():
    return Table(R.table_shapes())


def _impls():
    return [k for k, v in IMPLS.items() if not (v[2] is True and not hasattr(torch, "_fused_adam_"))]


def _reference(tab, p0, grad_steps, max_norm, counts=None, m0=None, v0=None):
    """The float64 restatement over the same inputs -> per step flat arrays p, g, m, v, step and the counts; g of a tensor without
    a gradient reads 0 (what Table.run uploads)."""
    n = len(tab.shapes)
    p = [np.asarray(x, dtype=np.float64) for x in p0]
    m = [np.zeros(s) for s in tab.shapes] if m0 is None else [x.astype(np.float64) for x in m0]
    v = [np.zeros(s) for s in tab.shapes] if v0 is None else [x.astype(np.float64) for x in v0]
    t = [0] * n if counts is None else list(counts)
    outs = []
    for gs in grad_steps:
        p, g, m, v, t, _, step = R.step_restated(p, gs, m, v, t, LR, BETAS[0], BETAS[1], EPS, max_norm, 0.0)
        g = [np.zeros(s) if x is None else x for x, s in zip(g, tab.shapes)]
        out = {k: tab.flatten(x) for k, x in (("p", p), ("g", g), ("m", m), ("v", v), ("step", step))}
        out["t"] = [float(x) for x in t]
        outs.append(out)
    return outs


def _hold(tab, what, runs, ref, p0, zero_start):
    """Every implementation of `runs` against `ref` under the bars of the module docstring, after every step.  Prints, per
    implementation, the worst error / bar, and for parent32 its worst error / floor (the part of the bar that is not its own
    error); returns {implementation: worst}."""
    worst = {k: 0.0 for k in runs}
    ceiling = 0.0
    fails = []
    acc = np.zeros(tab.total)
    bar2 = np.zeros(len(tab.shapes))
    before = tab.flatten(p0)
    for k, r in enumerate(ref):
        acc = acc + np.abs(r["step"])
        floors = {key: 1e-5 * tab.permax(r[key]) for key in ("g", "m", "v")}
        floors["p"] = 1e-5 * tab.permax(acc)
        bar2 = bar2 + 2e-3 * tab.per2(r["step"]) + np.sqrt(np.asarray(tab.sizes)) * tab.permax(before) * 1.2e-7
        before = r["p"]
        par = runs["parent32"][k]
        for impl, outs in runs.items():
            got = outs[k]
            if got["t"] != r["t"]:
                fails.append((what, impl, k + 1, "counters", [(i, a, b) for i, (a, b) in enumerate(zip(got["t"], r["t"])) if a != b][:8]))
            for key in FIELDS:
                if key == "p" and not zero_start:
                    err, bar = tab.per2(got["p"] - r["p"]), bar2
                else:
                    e_par = tab.permax(par[key] - r[key])
                    err, bar = tab.permax(got[key] - r[key]), 10.0 * e_par + floors[key]
                    if impl == "parent32":
                        ceiling = max(ceiling, float(np.where(floors[key] > 0, e_par / np.where(floors[key] > 0, floors[key], 1.0), 0.0).max()))
                ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
                ratio = np.where(np.isnan(err), np.inf, ratio)
                worst[impl] = max(worst[impl], float(ratio.max()))
                bad = np.nonzero(ratio > 1.0)[0]
                if bad.size:
                    fails.append((what, impl, k + 1, key, [(int(j), tab.sizes[j], float(err[j]), float(bar[j])) for j in bad[:6]], int(bad.size)))
    print("%s: worst error / bar %s; parent32 error / floor %.3g" % (what, ", ".join("%s %.3g" % (k, v) for k, v in worst.items()), ceiling))
    assert not fails, fails[:6]
    return worst


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["zero", "randn"])
@pytest.mark.parametrize("regime", sorted(R.REGIMES))
def test_five_steps_against_float64(regime, start):
    tab = _table()
    max_norm, gsteps = R.regime_gradients(regime, tab.shapes)
    p0 = R.start_parameters(tab.shapes, zero=(start == "zero"))
    ref = _reference(tab, p0, gsteps, max_norm)
    runs = {impl: tab.run(impl, p0, gsteps, max_norm) for impl in _impls()}
    _hold(tab, "%s from %s" % (regime, start), runs, ref, p0, start == "zero")
    clipped = not np.array_equal(runs["table"][0]["g"], tab.flatten(gsteps[0]))
    assert clipped == R.REGIMES[regime][3]                          # .grad is written exactly where the clip binds
    if start == "zero":
        assert np.abs(runs["table"][-1]["p"]).min() > 0            # parameters that start at zero resolve every step


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
NO_GRAD_ON_STEP_2 = (0, 5, 200, 255, 256, 257, 290, 299)


@pytest.mark.parametrize("start", ["zero", "randn"])
def test_every_tensor_steps_by_its_own_count(start):
    tab = _table()
    scales = R.tensor_scales("mixed", tab.shapes)
    counts, m0, v0 = R.mixed_count_state(tab.shapes, scales)
    max_norm = R.MAX_NORM
    gsteps = [R.draw_gradients(tab.shapes, scales, 900 + k) for k in range(3)]
    for i in NO_GRAD_ON_STEP_2:
        gsteps[1][i] = None
    p0 = R.start_parameters(tab.shapes, zero=(start == "zero"))
    ref = _reference(tab, p0, gsteps, max_norm, counts, m0, v0)
    want = [float(c + 3 - (i in NO_GRAD_ON_STEP_2)) for i, c in enumerate(counts)]
    assert ref[-1]["t"] == want and len(set(want[256:])) > 4
    runs = {impl: tab.run(impl, p0, gsteps, max_norm, counts, m0, v0) for impl in _impls()}
    for impl, outs in runs.items():
        assert outs[-1]["t"] == want, impl                          # every counter exactly
        for i in NO_GRAD_ON_STEP_2:                                # and a tensor without a gradient did not move
            a, b = int(tab.offs[i]), int(tab.offs[i + 1])
            assert all(np.array_equal(outs[1][key][a:b], outs[0][key][a:b]) for key in ("p", "m", "v")), (impl, i)
    _hold(tab, "mixed counts from %s" % start, runs, ref, p0, start == "zero")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self, ps):
        super().__init__()
        self.ps = torch.nn.ParameterList(ps)


def _soft(tab, table_opt, src, dst, tau, times=1):
    from sgrl_amd import td3
    tab.put("p", [src]), tab.put("dst", [dst])
    keep = td3._TABLE_OPT
    try:
        td3._TABLE_OPT = table_opt
        for _ in range(times):
            td3.soft_update_network(_Net(tab.params), _Net(tab.dst), tau)
    finally:
        td3._TABLE_OPT = keep
    assert np.array_equal(tab.get("p"), src.astype(np.float64))    # the source is only read
    return tab.get("dst")


def test_soft_update_against_float64():
    tab = _table()
    rng = np.random.default_rng(21)
    src, dst = rng.standard_normal(tab.total).astype(np.float32), rng.standard_normal(tab.total).astype(np.float32)
    assert np.array_equal(_soft(tab, True, src, dst, 1.0), src.astype(np.float64))        # tau = 1: the source, bit for bit
    assert np.array_equal(_soft(tab, True, src, dst, 0.0), dst.astype(np.float64))        # tau = 0: left alone
    for times in (1, 200):
        want = dst.astype(np.float64)
        for _ in range(times):
            want = want * (1 - 0.005) + 0.005 * src.astype(np.float64)
        e_tab = np.abs(_soft(tab, True, src, dst, 0.005, times) - want)
        e_par = np.abs(_soft(tab, False, src, dst, 0.005, times) - want)
        per = tab.permax(e_tab) / (10.0 * tab.permax(e_par) + 1e-5 * tab.permax(want))
        print("soft update x %d: max error table %.3g, foreach %.3g (ratio %.3g); worst per tensor error / bar %.3g"
              % (times, e_tab.max(), e_par.max(), e_tab.max() / e_par.max(), per.max()))
        assert e_tab.max() <= 10.0 * e_par.max()                    # over the table, no floor
        assert per.max() <= 1.0                                    # per tensor, the convention's bar


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [R.MAX_NORM, 0.0], ids=["clip", "max-norm-0"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradients_spread_as_in_torch(bad, max_norm):
    """Ordinary floats in ordinary launches: a NaN total gives a NaN clip coefficient (torch.clamp propagates it) and with it NaN in
    g, m, v and p of every tensor of the table; an infinite total gives coef = 0 and a NaN in the element alone."""
    tab = _table()
    scales = R.tensor_scales("unit", tab.shapes)
    gsteps = [R.draw_gradients(tab.shapes, scales, 700 + k) for k in range(2)]
    gsteps[1][5] = gsteps[1][5].copy()
    gsteps[1][5].ravel()[-1] = bad
    p0 = R.start_parameters(tab.shapes, zero=True)
    ref = _reference(tab, p0, gsteps, max_norm)
    runs = {impl: tab.run(impl, p0, gsteps, max_norm) for impl in ("table", "parent32")}
    got, par = runs["table"][1], runs["parent32"][1]
    assert got["t"] == par["t"] == [2.0] * len(tab.shapes)
    at = int(tab.offs[6]) - 1
    for key in FIELDS:
        nan_t, nan_p, nan_r = np.isnan(got[key]), np.isnan(par[key]), np.isnan(ref[1][key])
        print("%s max_norm %g %s: NaN in %d (table) / %d (parent32) / %d (float64) of %d elements" % (bad, max_norm, key, nan_t.sum(), nan_p.sum(), nan_r.sum(), tab.total))
        assert np.array_equal(nan_t, nan_p) and np.array_equal(nan_t, nan_r), key
        if max_norm > 0 and np.isnan(bad):
            assert nan_t.all(), key                                # the whole table
        elif np.isinf(bad) and max_norm == 0 and key != "p":
            assert not nan_t.any() and np.isinf(got[key][at])      # no clip: inf stays inf in g, m and v; p gets inf / inf
        else:
            assert nan_t.sum() == 1 and nan_t[at], key             # the element alone
        inf_t, inf_p = np.isinf(got[key]), np.isinf(par[key])
        assert np.array_equal(inf_t, inf_p) and np.array_equal(got[key][inf_t], par[key][inf_t]), key
    # the finite values under the bars (NaN and inf taken out of all three on the same elements)
    fin = np.isfinite(ref[1]["p"]) & np.isfinite(ref[1]["g"]) & np.isfinite(ref[1]["m"]) & np.isfinite(ref[1]["v"])
    if fin.any():
        clean = lambda out: dict({k: np.where(fin, out[k], 0.0) for k in out if k != "t"}, t=out["t"])
        _hold(tab, "%s max_norm %g, finite part" % (bad, max_norm), {k: [v[0], clean(v[1])] for k, v in runs.items()},
              [ref[0], clean(ref[1])], p0, True)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_the_same_state_twice_gives_the_same_bits():
    tab = _table()
    for regime in ("unit-clip", "mixed-maxnorm0"):
        max_norm, gsteps = R.regime_gradients(regime, tab.shapes, steps=2)
        p0 = R.start_parameters(tab.shapes, zero=False)
        a, b = tab.run("table", p0, gsteps, max_norm), tab.run("table", p0, gsteps, max_norm)
        for x, y in zip(a, b):
            assert all(np.array_equal(x[k], y[k]) for k in FIELDS) and x["t"] == y["t"]
