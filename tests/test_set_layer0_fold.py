"""The layer-0 fold of the SET forward (include/sgrl_set.h, csrc/set_actor.hip k_fold_l0) on the CPU, in float64.

At layer 0 the vector stream is g0 = sqrt(128) Wge v: rank 8.  sgrl_amd.set_hip.layer0_fold states the fold matrices the device builds
behind every pack (Mt, W1p, Q, Wu); here each identity the device path rests on is held to 1e-12 relative against the unfolded
quantities of the float64 module at FULL-RANK weights (oracle.formula.full_rank_values), the folded attention block is run end to end
against the module's hooked layer-0 outputs, and a census shows that a wrong fold (two columns of Wge or two rows of W1p exchanged)
moves those outputs by more than the bound tests/test_set_layer0_fold_gpu.py holds the device to."""
import numpy as np
import pytest
import torch

import set_full_rank_ref as R
from oracle import set_ref
from oracle.formula import apply_full_rank_, synth_obs
from sgrl_amd import set_hip

SEED, OBS_SEED, B = 8, 108, 3          # the weight seed qualified by tests/test_set_full_rank.py
NAMES = ["3d_walker_7_full", "3d_cheetah_14_full"]
RTOL = 1e-12
AT = "transformer_encoder.layers.0.self_attn."


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


class Case(object):
    def __init__(self, name):
        self.name, self.L = name, R.num_limbs(name)
        self.pol = R.cpu_modules("actor", lambda m: apply_full_rank_(m, SEED), torch.float64)
        self.obs = synth_obs(self.L, B, OBS_SEED + self.L)
        _, self.stages = R.actor_forward(self.pol, name, self.obs)
        self.sd = {k[len("actor."):]: v.numpy() for k, v in self.pol.state_dict().items()}
        self.fold = set_hip.layer0_fold(self.pol.actor)
        gd = R.graph_dict(name, f64=True)
        self.trav, self.relation = [np.asarray(t) for t in gd["traversals"]], gd["relation"].numpy()
        x = self.obs.reshape(B, self.L, 41)
        self.V = np.swapaxes(x[..., :24].reshape(B, self.L, 8, 3), -1, -2)          # [B, L, 3, 8]
        self.n0 = x[..., 24:]
        # the unfolded quantities (oracle/set_ref.py)
        self.g0 = (self.V @ self.sd["g_encoder.weight"].T) * np.sqrt(128.0)
        self.Z0 = np.concatenate([self.g0 @ self.sd[AT + "g_proj.weight"].T, self.V[..., 1:3]], -1)      # [B, L, 3, 32]
        self.G = np.einsum("blsa,blsc->blac", self.Z0, self.Z0)
        self.C = np.einsum("blsa,blsc->blac", self.V, self.V)

    def folded_attention(self, fold):
        """(vector output [B L, 384], scalar output [B L, 128]) of layer 0's attention block through the fold matrices, as the device
        runs it: Z0 and the row divisor from V, linear_g1 on the blocks of C, values mixed 8 wide and taken through Wu."""
        sd, V, L = self.sd, self.V, self.L
        S = np.einsum("blsa,ac,bltc->blst", V, fold["Q"], V)
        fn = np.sqrt((S ** 2).sum((-2, -1)))[..., None] + 1.0
        h = np.maximum(set_hip.blocks48(self.C) @ fold["W1p"].T + sd[AT + "linear_g1.bias"], 0)
        inv = h @ sd[AT + "linear_g2.weight"].T + sd[AT + "linear_g2.bias"]
        ng = (self.n0 @ sd["encoder.weight"].T + sd["encoder.bias"]) * np.sqrt(128.0)
        ng = ng + np.concatenate([sd["pos_encoder.embeddings.%d.weight" % i][t] for i, t in enumerate(self.trav)], 1)[None]
        c = np.concatenate([inv, ng], -1)
        lin = lambda n: c @ sd[AT + n + ".weight"].T + sd[AT + n + ".bias"]
        q = (lin("q_proj") / fn * 128.0 ** -0.5).reshape(B, L, 2, 128)
        k = (lin("k_proj") / fn).reshape(B, L, 2, 128)
        v = (lin("v_proj") / fn).reshape(B, L, 2, 128)
        rel = self.relation @ sd["transformer_encoder.rel_encoder.weight"].T + sd["transformer_encoder.rel_encoder.bias"]
        s = np.einsum("bihd,bjhd->bhij", q, k) + np.transpose(rel, (2, 0, 1))[None]
        w = np.exp(s - s.max(-1, keepdims=True))
        w = w / w.sum(-1, keepdims=True)
        o = np.einsum("bhij,bjhd->bihd", w, v).reshape(B, L, 256) @ sd[AT + "ng_out.weight"].T + sd[AT + "ng_out.bias"]
        mixed = np.einsum("bhij,bjsp->bhisp", w, V)
        g1 = np.einsum("chp,bhisp->bisc", fold["Wu"], mixed)
        return {"layer0/attn/out0": g1.reshape(B * L, 384), "layer0/attn/out1": o.reshape(B * L, 128)}


@pytest.fixture(scope="module", params=NAMES)
def case(request):
    return Case(request.param)


def test_the_fold_identities_hold_in_float64(case):
    f, V = case.fold, case.V
    ia, ib, ok = (t.numpy() for t in set_hip.gram_order())
    w1 = set_hip.fold_gram_weight(torch.from_numpy(case.sd[AT + "linear_g1.weight"])).numpy()
    S = np.einsum("blsa,ac,bltc->blst", V, f["Q"], V)
    rows = [("V Mt = Z0", V @ f["Mt"], case.Z0),
            ("Mt' (V'V) Mt = Z0'Z0", np.einsum("ax,blac,cy->blxy", f["Mt"], case.C, f["Mt"]), case.G),
            ("W1p blocks(C) = W1 blocks576(Z0'Z0)", set_hip.blocks48(case.C) @ f["W1p"].T, case.G[..., ia, ib] @ w1.T),
            ("||V Q V'||_F = ||Z0'Z0||_F", np.sqrt((S ** 2).sum((-2, -1))), np.sqrt((case.G ** 2).sum((-2, -1))))]
    got = case.folded_attention(f)
    rows += [("Wu form of attention-0's vector output", got["layer0/attn/out0"], case.stages["layer0/attn/out0"]),
             ("attention-0's scalar output behind the folded site", got["layer0/attn/out1"], case.stages["layer0/attn/out1"])]
    bad = []
    for what, a, b in rows:
        e = _rel(a, b)
        print("L0FOLD %s | %s | relative %.3e" % (case.name, what, e))
        if not e < RTOL:
            bad.append((what, e))
    assert not bad, bad
    assert (f["W1p"] != 0).all() and f["W1p"].shape == (256, 48) and f["Wu"].shape == (128, 2, 8)


def test_a_wrong_fold_is_visible_to_the_device_test(case):
    """Two columns of Wge exchanged before the fold is taken, or two rows of W1p afterwards: each moves a layer-0 attention output the
    device test compares by more than its bound there (2e-5 (1 + max |ref|), tests/set_full_rank_ref.py)."""
    base = case.folded_attention(case.fold)
    bounds = {k: R.TOL_STAGE * (1.0 + np.abs(case.stages[k]).max()) for k in base}
    wge = case.pol.actor.g_encoder.weight
    wrong = []
    for c0, c1 in ((0, 3), (1, 2), (4, 7)):
        R._swap(wge, c0, c1)
        try:
            wrong.append(("Wge[:, %d<->%d]" % (c0, c1), set_hip.layer0_fold(case.pol.actor)))
        finally:
            R._swap(wge, c0, c1)
    for r0, r1 in ((3, 11), (5, 133)):
        f = dict(case.fold, W1p=case.fold["W1p"].copy())
        f["W1p"][[r0, r1]] = f["W1p"][[r1, r0]]
        wrong.append(("W1p rows %d<->%d" % (r0, r1), f))
    weak = []
    for label, f in wrong:
        got = case.folded_attention(f)
        ratio = max(np.abs(got[k] - base[k]).max() / bounds[k] for k in base)
        print("L0FOLD census %s | %s | largest shift %.3g x bound" % (case.name, label, ratio))
        if not ratio > 1.0:
            weak.append((label, ratio))
    assert not weak, weak


@pytest.mark.parametrize("critic", [False, True])
def test_the_plan_reserves_the_fold_block(critic):
    from sgrl_amd.set_policy import make_critic, make_policy
    net = make_critic(use_hip=False).critic1 if critic else make_policy(use_hip=False).actor
    segs, offs, total, _ = set_hip.plan_segments(net, critic=critic)
    o = int(offs[set_hip.NW + set_hip.NSITES + 2])
    assert len(offs) == set_hip.NW + set_hip.NSITES + set_hip.NEXTRA and o % 64 == 0 and o + set_hip.L0F_FLOATS == total
    assert set_hip.L0F_FLOATS == 256 * 48 + 8 * 32 + 8 * 8 + 128 * 2 * 8
