#!/usr/bin/env python3
"""Golden vectors for the SWAT networks' dropout: executes the reference StructurePolicy and one Q network of its
CriticStructurePolicy (reference src/StructureActor.py, src/StructureCritic.py) in train() mode with dropout_rate 0.1, the
formula weights of oracle/formula.py, ONE walker_7 row (B = 1) on the CPU, torch.manual_seed(SEED_*) right before each forward.
The reference's modules are run in FLOAT64 (module.double(); F.dropout draws the same masks for either dtype -- asserted below
against a float32 run), so that the fixture carries no float32 rounding of the machine it was captured on: two float32 runs of this
network on different hosts differ by up to 1.3e-6, more than the 1e-6 the test allows for a mask to be called the same.
At B = 1 the reference's (N, B, d) layout and this repository's [B, L, E] number the elements of every dropped tensor alike, so
F.dropout consumes torch's generator in the same order on both sides (tests/test_swat_dropout.py (d)).  Build container only;
numbers only."""
import os, sys
HERE = os.path.dirname(os.path.abspath(__file__)); REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO); sys.path.insert(0, HERE)
import numpy as np, torch
import refstub
refstub.install()
import utils as ref_utils
from StructureActor import StructurePolicy
from StructureCritic import CriticStructurePolicy
from capture_golden import _args_ns
from oracle.formula import apply_formula_, synth_obs

NAME, P, SEED_ACTOR, SEED_CRITIC = "3d_walker_7_full", 0.1, 1234, 1235
a = _args_ns()
a.dropout_rate = P
pol = StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False, a).train()
crit = CriticStructurePolicy(41, 3, 32, 1, 3, True, False, False, a).train()
apply_formula_(pol); apply_formula_(crit)
parents = ref_utils.getGraphStructure(refstub.all_xmls()[NAME])
gd = ref_utils.getGraphDict(parents, ["pre", "inlcrs", "postlcrs"], [], device=torch.device("cpu"))
pol.change_morphology(gd); crit.change_morphology(gd)
L = len(parents)
obs = synth_obs(L, 1, 31 + L).astype(np.float32)
act = np.random.RandomState(100 + L).uniform(-1, 1, size=(1, 3 * L)).astype(np.float32)
res = {"obs": obs, "act_in": act, "p": np.float32(P), "seed_actor": np.int64(SEED_ACTOR), "seed_critic": np.int64(SEED_CRITIC)}


def run(dtype):
    o, a_in = torch.from_numpy(obs).to(dtype), torch.from_numpy(act).to(dtype)
    pol.to(dtype).train(); crit.to(dtype).train()
    gd_t = dict(gd); gd_t["relation"] = gd["relation"].to(dtype)
    pol.change_morphology(gd_t); crit.change_morphology(gd_t)
    out = {}
    with torch.no_grad():
        torch.manual_seed(SEED_ACTOR)
        out["action"] = pol(o).numpy()
        torch.manual_seed(SEED_CRITIC)
        out["q1"] = crit.Q1(o, a_in).numpy()
        pol.eval(); crit.eval()
        out["action_eval"] = pol(o).numpy()
        out["q1_eval"] = crit.Q1(o, a_in).numpy()
    return out


f32 = run(torch.float32)
pol.double(); crit.double()
apply_formula_(pol); apply_formula_(crit)           # the formula weights again, at float64's precision
res.update(run(torch.float64))
for k, v in f32.items():                            # the same masks in both dtypes: dropout moves the outputs by 0.3 .. 0.9
    assert res[k].dtype == np.float64 and np.abs(res[k] - v).max() < 1e-5, (k, np.abs(res[k] - v).max())
    print("%s: |float32 - float64| max %.3g" % (k, np.abs(res[k] - v).max()))
assert np.abs(res["action"] - res["action_eval"]).max() > 1e-4 and np.abs(res["q1"] - res["q1_eval"]).max() > 1e-4      # dropout did act
np.savez_compressed(os.path.join(REPO, "tests", "golden", "swat_dropout.npz"), **res)
print("swat dropout golden written: |action - eval| max %.3g, |q1 - eval| max %.3g"
      % (np.abs(res["action"] - res["action_eval"]).max(), np.abs(res["q1"] - res["q1_eval"]).max()))
