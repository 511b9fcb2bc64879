"""Host side of the graphed TD3 update of the MLP agent (td3.GraphedMlpUpdates, mlp_hip.batch_stats over include/sgrl_mlp.h
sgrl_mlp_batch_stats; no GPU needed): the NumPy restatement of the batch prologue (tests/mlp_batch_restate.py, the kernel's fixed
order in float32) against float64 and against torch on the CPU, the refusals of the class, its launch bookkeeping, and the stamp --
what a captured graph has baked -- over stub objects.

The bars are worst-case summation bounds, not measurements: a sum of n float32 terms in any order is within (n - 1) u sum|x| of the
exact one (u = 2^-24), the division by n adds one rounding: mean bar (n + 2) u mean|x|.  The variance adds, per term, the rounding of
the difference, of the square and of the sum, and the mean's own error e shifts every deviation: the sum of squares moves by at most
n e^2 (the cross term vanishes to first order around the exact mean): (n + 8) 2^-23 var64 + 2 (mean bar)^2.  Printed by a run here:
the restatement reaches at most 0.24 of the mean bar and 0.09 of the variance bar on these inputs (both at B = 2; 5e-3 and 3e-3 at
B = 256)."""
import types

import numpy as np
import pytest
import torch

from mlp_batch_restate import bars, batch_stats_f64, batch_stats_restated
from sgrl_amd import _lib, mlp_hip, td3

BS = [1, 2, 31, 33, 66, 256, 1024, 4096]
SEEDS = range(20)
SCALE = 0.3


def rewards(B, seed):
    return np.random.RandomState(1000 * B + seed).normal(1.0, 0.5, B).astype(np.float32)


@pytest.mark.parametrize("B", BS)
def test_restatement_against_float64(B):
    worst = [0.0, 0.0]
    for seed in SEEDS:
        r = rewards(B, seed)
        _, mean, var = batch_stats_restated(r, SCALE)
        mean64, var64 = batch_stats_f64(r, SCALE)
        mean_bar, var_bar = bars(r, SCALE)
        assert mean.dtype == np.float32 and var.dtype == np.float32
        assert abs(float(mean) - mean64) <= mean_bar, (B, seed, float(mean), mean64, mean_bar)
        worst[0] = max(worst[0], abs(float(mean) - mean64) / mean_bar)
        if B == 1:
            assert np.isnan(var) and np.isnan(var64)
            continue
        assert abs(float(var) - var64) <= var_bar, (B, seed, float(var), var64, var_bar)
        worst[1] = max(worst[1], abs(float(var) - var64) / var_bar)
    print("B %d: worst error / bar: mean %.3g, variance %.3g" % (B, worst[0], worst[1]))


@pytest.mark.parametrize("B", BS)
def test_restated_reward_and_statistics_against_torch_on_the_cpu(B):
    for seed in (0, 7):
        r = rewards(B, seed)
        out, mean, var = batch_stats_restated(r, SCALE)
        t = torch.from_numpy(r).reshape(B, 1) * SCALE            # the statement it replaces: float32 tensor * Python float
        assert t.dtype == torch.float32 and np.array_equal(out.view(np.uint32), t.reshape(-1).numpy().view(np.uint32))
        mean_bar, var_bar = bars(r, SCALE)
        assert abs(float(mean) - float(torch.mean(t))) <= 2 * mean_bar
        if B > 1:
            assert abs(float(var) - float(torch.var(t))) <= 2 * var_bar
        else:
            assert np.isnan(var) and bool(torch.isnan(torch.var(t)))


def test_launch_count_and_argument_errors_need_no_device():
    import ctypes
    L = _lib.lib()
    mlp_hip._bind(L)
    assert mlp_hip.batch_stats_launches() == L.sgrl_mlp_batch_stats_launches() == 1
    buf = np.zeros(8, dtype=np.float32)
    p, null = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(None)
    odd = ctypes.c_void_p(buf.ctypes.data + 2)
    cf = ctypes.c_float
    for args, what in (((null, 4, cf(1.0), p, p), b"null"), ((p, 4, cf(1.0), null, p), b"null"), ((p, 4, cf(1.0), p, null), b"null"),
                       ((p, 0, cf(1.0), p, p), b"n outside"), ((p, -3, cf(1.0), p, p), b"n outside"), ((p, (1 << 24) + 1, cf(1.0), p, p), b"n outside"),
                       ((p, 4, cf(float("nan")), p, p), b"not finite"), ((p, 4, cf(float("inf")), p, p), b"not finite"),
                       ((odd, 4, cf(1.0), p, p), b"aligned")):
        assert L.sgrl_mlp_batch_stats(*args, null) == -1, what          # SGRL_ERR_ARG, before any launch
        assert b"sgrl_mlp_batch_stats" in L.sgrl_mlp_last_error() and what in L.sgrl_mlp_last_error(), L.sgrl_mlp_last_error()
    assert not buf.any()
    with pytest.raises(_lib.SgrlError, match="float32 tensor on the reward's GPU"):
        mlp_hip.batch_stats(torch.zeros(4), 1.0, torch.zeros(4), torch.zeros(2))


def _args(atype, **over):
    a = td3.default_train_args(actor_type=atype, critic_type=atype, **over)
    if atype == "mlp":
        a.mlp_num_limbs = 3
        a.agent.policy_network = {"hidden_dims": [8, 8]}
        a.agent.q_network = {"hidden_dims": [8, 8]}
    return a


def test_refuses_a_cpu_agent_and_a_set_agent_with_the_reason():
    cpu = td3.Agent(_args("mlp"), device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="needs the agent on the GPU"):
        td3.GraphedMlpUpdates(cpu, 16)
    assert not cpu.use_mlp_hip_optim                                 # a refused construction leaves the agent as it was
    with pytest.raises(NotImplementedError, match="serves 'mlp' \\+ 'mlp' agents only"):
        td3.GraphedMlpUpdates(td3.Agent(_args("set"), device=torch.device("cpu")), 16)
    with pytest.raises(NotImplementedError, match="GraphedUpdates is not built for 'mlp'"):     # and the other class keeps refusing
        td3.GraphedUpdates(cpu, 16)


def test_launch_bookkeeping_restated_from_constants():
    g = td3.GraphedMlpUpdates.__new__(td3.GraphedMlpUpdates)          # launches() reads the ABI only
    g._mlp_hip = mlp_hip
    prologue, packs, chain, critic_grads, actor_grads, optim = 1, 2, 1, 3, 4, 2
    assert g.launches(1) == prologue + packs + chain + critic_grads + optim == 9
    assert g.launches(0) == g.launches(1) + actor_grads + optim == 15


# ---- the stamp over stubs -------------------------------------------------------------------------------------------------------
class _T(object):
    """A tensor as far as the stamp looks: an address and, for a parameter, a .grad."""

    def __init__(self, addr, grad=None):
        self.addr, self.grad = addr, grad

    def data_ptr(self):
        return self.addr


class _H(object):
    def __init__(self, gen, bound):
        self.gen, self._bound = gen, bound

    def generation(self):
        return self.gen


def _world():
    """Stub handles, parameters, optimizers and sides with distinct addresses everywhere."""
    nxt = iter(range(0x1000, 0x100000, 0x40))
    nets = [[_T(next(nxt), _T(next(nxt))) for _ in range(n)] for n in (2, 4, 2, 4)]     # target actor / critic, online actor / critic
    handles = [_H(0, tuple(p.addr for p in ps)) for ps in nets]
    opts = []
    for ps in (nets[2], nets[3]):
        state = {p: {"exp_avg": _T(next(nxt)), "exp_avg_sq": _T(next(nxt)), "step": _T(next(nxt))} for p in ps}
        opts.append((types.SimpleNamespace(state=state, param_groups=[{"lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8}]), ps))
    sides = [types.SimpleNamespace(partials=_T(next(nxt)), counter=_T(next(nxt))) for _ in range(2)]
    scalars = [0.1, 0.005, 0.5, 0.99, 1.0, 0.3]          # grad_clipping_value, tau, noise_clip, discount, max_action, reward_scale
    return handles, nets, opts, sides, scalars


def _stamp(w):
    return td3.mlp_update_stamp(w[0], w[1], w[2], w[3], w[4])


def _changes():
    """(name, function that changes ONE listed field of a world)"""
    out = []
    for i, who in enumerate(("target actor", "target critic", "grads actor", "grads critic")):
        out.append((who + " generation", lambda w, i=i: setattr(w[0][i], "gen", 1)))
        out.append((who + " bound addresses", lambda w, i=i: setattr(w[0][i], "_bound", w[0][i]._bound[:-1] + (0x7,))))
        out.append((who + " parameter address", lambda w, i=i: setattr(w[1][i][-1], "addr", 0x9)))
    for i in (2, 3):
        out.append(("online .grad address %d" % i, lambda w, i=i: setattr(w[1][i][0], "grad", _T(0xB))))
        out.append(("online .grad missing %d" % i, lambda w, i=i: setattr(w[1][i][0], "grad", None)))
    for k, who in enumerate(("actor", "critic")):
        for key in ("exp_avg", "exp_avg_sq", "step"):
            out.append(("%s optimizer %s address" % (who, key), lambda w, k=k, key=key: w[2][k][0].state[w[2][k][1][0]].__setitem__(key, _T(0xD))))
        out.append((who + " optimizer state missing", lambda w, k=k: w[2][k][0].state.pop(w[2][k][1][-1])))
        out.append((who + " lr", lambda w, k=k: w[2][k][0].param_groups[0].__setitem__("lr", 3e-4)))
        out.append((who + " beta1", lambda w, k=k: w[2][k][0].param_groups[0].__setitem__("betas", (0.8, 0.999))))
        out.append((who + " beta2", lambda w, k=k: w[2][k][0].param_groups[0].__setitem__("betas", (0.9, 0.99))))
        out.append((who + " eps", lambda w, k=k: w[2][k][0].param_groups[0].__setitem__("eps", 1e-7)))
        out.append((who + " partials", lambda w, k=k: setattr(w[3][k], "partials", _T(0xF))))
        out.append((who + " counter", lambda w, k=k: setattr(w[3][k], "counter", _T(0x11))))
        out.append((who + " counter missing", lambda w, k=k: setattr(w[3][k], "counter", None)))
    for j, who in enumerate(("grad_clipping_value", "tau", "noise_clip", "discount", "max_action", "reward_scale")):
        out.append((who, lambda w, j=j: w[4].__setitem__(j, w[4][j] * 0.5)))
    out.append(("grad_clipping_value off", lambda w: w[4].__setitem__(0, None)))
    return out


@pytest.mark.parametrize("name,change", _changes(), ids=[n for n, _ in _changes()])
def test_stamp_changes_when_one_listed_field_changes(name, change):
    w = _world()
    before = _stamp(w)
    assert before == _stamp(_world()) and hash(before) == hash(_stamp(w))        # plain values: comparable, repeatable
    change(w)
    assert _stamp(w) != before, name


def test_stamp_reads_no_values():
    """An in-place write into a parameter changes no address: the stamp is the same, the next replay reads the new value."""
    w = _world()
    before = _stamp(w)
    w[1][1][0].value = 42.0
    assert _stamp(w) == before
