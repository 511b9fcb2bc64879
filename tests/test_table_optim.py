"""The yardstick and the inputs of tests/test_table_optim_gpu.py, qualified on the CPU (no GPU needed).

1  tests/optim_restate.step_restated against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64: a step count per tensor
   (0, 1, 1000, 100000 in one group), a gradient that is None on one step, the clip active and inactive, max_norm = 0, and a NaN
   and an infinite total (the same NaN pattern, the finite values equal); mlp_optim_restate.step_restated is the same arithmetic
2  the regimes of optim_restate.REGIMES are what their names say: which way the clip goes, and where Adam's eps decides the step.
   'tiny-eps': every element has sqrt(v_hat) < eps (asserted: >= 99 %; the generator gives |g| <= 2e-11 against eps = 1e-8).  The
   mixed sets: the tensors whose elements all lie below eps are 45 % (no clip) and 55 % (clip, coef ~ 0.1) in expectation over
   10^U(-13, -2) scales; asserted >= 30 %, five standard deviations of a 300-tensor draw below that.  The unit-scale sets: none
3  torch's own float32 path on the CPU stays within the FLOOR of the GPU tests' bars, the part that does not depend on a measured
   parent: per tensor in the max-norm 1e-5 max|x64| for g and v, 1e-5 of the largest accumulated |step64| for parameters that start
   at zero, the step bar for parameters that start at randn.  So a correct float32 implementation fits with room, and the factor
   10 on the parent's error is not what lets one pass.  m is a signed sum: in a one-element tensor five gradients of alternating
   sign can cancel to 3e-4 of their magnitudes (measured, 'just-over'), and the 1e-6 relative error the float32 total leaves in
   every clipped gradient is then 3e-3 of m; here m is therefore held to 1e-5 of the same sum taken without the signs
   (M := b1 M + (1 - b1) |g|), the accumulated magnitude, as the parameters are.  Worst ratios are printed (pytest -s)
4  sgrl_optim_clip_adam / sgrl_optim_lerp return their argument errors without a device
"""
import ctypes

import numpy as np
import pytest
import torch

import mlp_optim_restate
import optim_restate as R

LR, BETAS, EPS = 1e-4, (0.9, 0.999), 1e-8


def torch_steps(p0, grad_steps, max_norm, dtype, counts=None, m0=None, v0=None, device="cpu", step=None):
    """clip_grad_norm_ + torch.optim.Adam.step over the gradients of grad_steps (entries may be None) in `dtype` -> per step a dict
    of lists of float64 arrays p, g, m, v and the counts t.  `step(opt, max_norm)` replaces the two calls when given."""
    params = [torch.nn.Parameter(torch.tensor(x, dtype=dtype, device=device)) for x in p0]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS)
    if counts is not None:
        for p, c, m, v in zip(params, counts, m0, v0):
            opt.state[p] = {"step": torch.tensor(float(c)), "exp_avg": torch.tensor(m, dtype=dtype, device=device),
                            "exp_avg_sq": torch.tensor(v, dtype=dtype, device=device)}
    outs = []
    for gs in grad_steps:
        for p, g in zip(params, gs):
            p.grad = None if g is None else torch.tensor(g, dtype=dtype, device=device)
        if step is not None:
            step(opt, max_norm)
        else:
            if max_norm > 0:
                torch.nn.utils.clip_grad_norm_(params, max_norm)
            opt.step()
        f64 = lambda x: x.detach().double().cpu().numpy().copy()
        st = [opt.state[p] for p in params]
        outs.append({"p": [f64(p) for p in params], "g": [None if p.grad is None else f64(p.grad) for p in params],
                     "m": [f64(s["exp_avg"]) if s else np.zeros(p.shape) for s, p in zip(st, params)],
                     "v": [f64(s["exp_avg_sq"]) if s else np.zeros(p.shape) for s, p in zip(st, params)],
                     "t": [int(s["step"]) if s else 0 for s in st]})
    return outs


def restated_steps(p0, grad_steps, max_norm, counts=None, m0=None, v0=None):
    """The same over optim_restate.step_restated; each step's dict also carries `step` (p_new - p_old)."""
    p = [np.asarray(x, dtype=np.float64) for x in p0]
    m = [np.zeros_like(x) for x in p] if m0 is None else m0
    v = [np.zeros_like(x) for x in p] if v0 is None else v0
    t = [0] * len(p) if counts is None else counts
    outs = []
    for gs in grad_steps:
        p, g, m, v, t, _, step = R.step_restated(p, gs, m, v, t, LR, BETAS[0], BETAS[1], EPS, max_norm, 0.0)
        outs.append({"p": p, "g": g, "m": m, "v": v, "t": list(t), "step": step})
    return outs


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
SHAPES_SMALL = [(7, 5), (7,), (3, 7), (3,), (1, 3), (1,), (2, 2, 2), (1,)]


def _same(got, want, what):
    """The same NaN pattern; the finite values within 1e-12 of the tensor's maximum (infinities equal)."""
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, (what, i)
            continue
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, i, a, b)
        fin = np.isfinite(b)
        assert np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), (what, i)
        if fin.any():
            assert np.abs(a[fin] - b[fin]).max() <= 1e-12 * max(np.abs(b[fin]).max(), 1e-300), (what, i, a, b)


@pytest.mark.parametrize("max_norm,scale", [(0.1, 1.0), (0.1, 1e-3), (0.0, 1.0), (0.1, 1e-11)],
                         ids=["clip-active", "clip-inactive", "max-norm-0", "eps-decides"])
def test_restatement_matches_torch_in_float64_with_a_count_per_tensor(max_norm, scale):
    scales = np.full(len(SHAPES_SMALL), scale)
    counts, m0, v0 = R.mixed_count_state(SHAPES_SMALL, scales)
    assert sorted(set(counts)) == sorted(R.MIXED_COUNTS)
    p0 = R.start_parameters(SHAPES_SMALL, zero=False)
    gsteps = [R.draw_gradients(SHAPES_SMALL, scales, 50 + k) for k in range(3)]
    gsteps[1][2] = None                                   # one tensor without a gradient on the second step: its count falls behind
    m0, v0 = [x.astype(np.float64) for x in m0], [x.astype(np.float64) for x in v0]
    want = torch_steps(p0, gsteps, max_norm, torch.float64, counts, m0, v0)
    got = restated_steps(p0, gsteps, max_norm, counts, m0, v0)
    active = [R.total_norm(g) > max_norm > 0 for g in gsteps]
    assert all(active) == (max_norm > 0 and scale == 1.0) and any(active) == all(active)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a["t"] == b["t"] == [c + k + 1 - (1 if (i == 2 and k >= 1) else 0) for i, c in enumerate(counts)]
        for key in ("p", "g", "m", "v"):
            _same(a[key], b[key], (k, key))
        assert all(np.array_equal(s, pn - po) for s, pn, po in zip(a["step"], a["p"], (got[k - 1]["p"] if k else [x.astype(np.float64) for x in p0])))
    assert np.array_equal(got[1]["p"][2], got[0]["p"][2]) and np.array_equal(got[1]["m"][2], got[0]["m"][2])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")], ids=["nan", "inf", "-inf"])
def test_restatement_follows_torch_on_a_non_finite_total(bad):
    """A NaN gradient: coef is NaN (torch.clamp propagates it) and every gradient, moment and parameter of the group becomes NaN.
    An infinite one: coef = 0, every other gradient becomes 0 and only the element itself NaN (inf * 0)."""
    scales = np.ones(len(SHAPES_SMALL))
    p0 = R.start_parameters(SHAPES_SMALL, zero=False)
    g0 = R.draw_gradients(SHAPES_SMALL, scales, 3)
    g1 = [x.copy() for x in R.draw_gradients(SHAPES_SMALL, scales, 4)]
    g1[3][1] = bad
    for max_norm in (0.1, 0.0):
        want = torch_steps(p0, [g0, g1], max_norm, torch.float64)
        got = restated_steps(p0, [g0, g1], max_norm)
        for key in ("p", "g", "m", "v"):
            _same(got[1][key], want[1][key], (max_norm, key))
        nans = [bool(np.isnan(x).all()) for key in ("p", "g", "m", "v") for x in got[1][key]]
        if max_norm > 0 and np.isnan(bad):
            assert all(nans)                              # the whole group
        else:
            hit = [int(np.isnan(x).sum()) for x in got[1]["p"]]
            assert hit == [0, 0, 0, 1, 0, 0, 0, 0], hit    # the element alone
            if max_norm > 0:
                assert all(float(np.abs(x).max()) == 0.0 for i, x in enumerate(got[1]["g"]) if i != 3)


def test_the_mlp_restatement_is_the_same_arithmetic():
    """mlp_optim_restate.step_restated, now a call into optim_restate, returns for finite input the bits of the lines it used to hold."""
    rng = np.random.default_rng(2)
    shapes = [(7, 5), (7,), (1,)]
    p, m, tg = ([rng.standard_normal(s) for s in shapes] for _ in range(3))
    v = [rng.standard_normal(s) ** 2 for s in shapes]
    for scale, max_norm, tau, t in ((10.0, 0.1, 0.005, 0), (1e-3, 0.1, 1.0, 1000), (1.0, 0.0, 0.0, 3)):
        g = [rng.standard_normal(s) * scale for s in shapes]
        got = mlp_optim_restate.step_restated(p, g, m, v, t, LR, BETAS[0], BETAS[1], EPS, max_norm, tau, tg)
        gc = g
        if max_norm > 0:
            total = sum(float((x * x).sum()) for x in g)
            gc = [x * min(1.0, max_norm / (np.sqrt(total) + 1e-6)) for x in g]
        m1 = [BETAS[0] * a + (1 - BETAS[0]) * x for a, x in zip(m, gc)]
        v1 = [BETAS[1] * a + (1 - BETAS[1]) * x * x for a, x in zip(v, gc)]
        p1 = [w - (LR / (1 - BETAS[0] ** (t + 1))) * a / (np.sqrt(b) / np.sqrt(1 - BETAS[1] ** (t + 1)) + EPS) for w, a, b in zip(p, m1, v1)]
        t1 = [x * (1 - tau) + tau * w for x, w in zip(tg, p1)] if tau > 0 else tg
        assert got[4] == t + 1 and len(got) == 6
        for a, b in zip(got[:4] + (got[5],), (p1, gc, m1, v1, t1)):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 2 and 3 ----------------------------------------------------------------------------------------------------------------
def test_table_shapes_are_what_the_kernels_need():
    shapes = R.table_shapes()
    sizes = R.sizes_of(shapes)
    assert len(shapes) == 300 and {1, 1023, 1024, 1025, 2049, 27, 30 * 128, 300 * 1024} <= set(sizes)
    assert sum(-(-n // R.CHUNK) for n in sizes) > 256 + 256                   # k_opt_total: strided sum and tree
    assert sizes[256] == 1025 and sizes[290] == 2049 and len(sizes) > 256     # rows past the counter loop's stride
    small = [n for i, n in enumerate(sizes) if i not in R.SPECIAL]
    assert set(small) == set(range(1, 8))
    counts, _, _ = R.mixed_count_state(shapes, R.tensor_scales("mixed", shapes))
    assert set(counts[:256]) == set(counts[256:]) == set(R.MIXED_COUNTS)
    for kind in ("unit", "tiny", "mixed"):
        s = R.tensor_scales(kind, shapes)
        assert s.min() >= 1e-13 and s.max() <= 1.0
        g = R.draw_gradients(shapes, s, 1)
        assert all(x.dtype == np.float32 and np.abs(x).min() >= 0.5 * sc * (1 - 1e-6) and np.abs(x).max() <= 2 * sc * (1 + 1e-6) for x, sc in zip(g, s))
        assert min((1 - BETAS[1]) * float(np.abs(x).min()) ** 2 for x in g) > 1.18e-38        # (1 - b2) g^2 a normal float32
    s = R.tensor_scales("mixed", shapes)
    assert s.min() == 1e-13 and s.max() == 1e-2 and 3 < np.log10(s).std() < 4


@pytest.mark.parametrize("regime", sorted(R.REGIMES))
@pytest.mark.parametrize("start", ["zero", "randn"])
def test_regimes_are_what_they_say_and_float32_stays_within_the_floor_of_the_bars(regime, start):
    shapes = R.table_shapes()
    max_norm, gsteps = R.regime_gradients(regime, shapes)
    kind, _, _, binds = R.REGIMES[regime]
    p0 = R.start_parameters(shapes, zero=(start == "zero"))
    ref = restated_steps(p0, gsteps, max_norm)
    # the clip goes the way the regime says, on every step, in float64 and at float32's resolution of the total (1e-5 is ample)
    for g in gsteps:
        tn = R.total_norm(g)
        assert (tn > max_norm * (1 + 2e-5) and max_norm > 0) if binds else (max_norm == 0 or tn < max_norm * (1 - 2e-5)), (regime, tn)
    # where eps decides
    last = ref[-1]
    share = R.eps_share(last["v"], last["t"])
    below = [bool((np.sqrt(v / (1 - BETAS[1] ** t)) < EPS).all()) for v, t in zip(last["v"], last["t"])]
    print("%s: elements with sqrt(v_hat) < eps %.4f, tensors wholly below %.3f" % (regime, share, np.mean(below)))
    if kind == "tiny":
        assert share >= 0.99
    elif kind == "mixed":
        assert np.mean(below) >= 0.30 and not all(below)
    else:
        assert share == 0.0
    # torch's float32 path on the CPU against the floor of the GPU bars
    f32 = torch_steps(p0, gsteps, max_norm, torch.float32)
    acc = [np.zeros_like(x, dtype=np.float64) for x in p0]
    mag_m = [np.zeros_like(x, dtype=np.float64) for x in p0]       # m with |g| in place of g: what m's terms add up to without their signs
    bar_p = np.zeros(len(shapes))
    before = [x.astype(np.float64) for x in p0]
    worst = {}
    for k in range(len(gsteps)):
        assert f32[k]["t"] == ref[k]["t"] == [k + 1] * len(shapes)
        acc = [a + np.abs(s) for a, s in zip(acc, ref[k]["step"])]
        mag_m = [BETAS[0] * a + (1 - BETAS[0]) * np.abs(g) for a, g in zip(mag_m, ref[k]["g"])]
        for key in ("g", "m", "v"):
            mags = mag_m if key == "m" else [np.abs(b) for b in ref[k][key]]
            ratio = max(np.abs(a - b).max() / (1e-5 * c.max()) for a, b, c in zip(f32[k][key], ref[k][key], mags))
            worst[key] = max(worst.get(key, 0.0), ratio)
        if start == "zero":
            ratio = max(np.abs(a - b).max() / (1e-5 * c.max()) for a, b, c in zip(f32[k]["p"], ref[k]["p"], acc))
        else:
            bar_p += np.array([2e-3 * np.sqrt((s ** 2).sum()) + np.sqrt(b.size) * np.abs(b).max() * 1.2e-7 for s, b in zip(ref[k]["step"], before)])
            err = np.array([np.sqrt(((a - b) ** 2).sum()) for a, b in zip(f32[k]["p"], ref[k]["p"])])
            ratio = float((err / bar_p).max())
        before = ref[k]["p"]
        worst["p"] = max(worst.get("p", 0.0), ratio)
    print("%s from %s: float32 on the CPU, worst error / floor of the bar: %s" % (regime, start, {k: "%.3g" % v for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_returned_without_a_device():
    from sgrl_amd import td3
    L = td3._optim_lib()
    assert L.sgrl_optim_chunk() == R.CHUNK
    buf = np.zeros(64, dtype=np.int64)                    # stands in for every pointer: a refused call reads and launches nothing
    ok, null = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(None)
    hyper = (1e-4, 0.9, 0.999, 1e-8)
    err = lambda: L.sgrl_train_last_error()
    for table, n, chunks, nc, max_norm, scratch in ((null, 1, ok, 1, 0.1, ok), (ok, 1, null, 1, 0.1, ok), (ok, 0, ok, 1, 0.1, ok), (ok, -3, ok, 1, 0.1, ok),
                                                    (ok, 1, ok, 0, 0.1, ok), (ok, 1, ok, -1, 0.1, ok), (ok, 1, ok, 1, 0.1, null), (null, 1, ok, 1, 0.0, null)):
        assert L.sgrl_optim_clip_adam(table, n, chunks, nc, *hyper, max_norm, scratch, null) == -1
        assert b"sgrl_optim_clip_adam: bad argument" in err()
    for table, chunks, nc in ((null, ok, 1), (ok, null, 1), (ok, ok, 0), (ok, ok, -1)):
        assert L.sgrl_optim_lerp(table, chunks, nc, 0.005, null) == -1
        assert b"sgrl_optim_lerp: bad argument" in err()
    assert not buf.any()
