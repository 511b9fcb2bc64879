"""Host side of the batched HIP SWAT actor forward (sgrl_amd/swat_hip.py, include/sgrl_swat.h): the parameter plan the C ABI
binds, the exported symbols, no CPU fallback, and the rollout's choice of HIP forward by policy type."""
import ctypes
import json
import os
import re

import pytest
import torch

from sgrl_amd import _lib
from sgrl_amd.set_policy import default_args

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _swat(**over):
    from sgrl_amd.swat_policy import StructurePolicy
    return StructurePolicy(41, 3, 32, 1, 1.0, 3, True, False, False, default_args(**over))


@pytest.mark.parametrize("tnorm", [1, 0])
@pytest.mark.parametrize("cond", [0, 1])
def test_plan_covers_every_actor_parameter_once(cond, tnorm, golden_dir):
    from sgrl_amd.swat_hip import plan_params
    pol = _swat(condition_decoder_on_features=cond, transformer_norm=tnorm)
    plan = plan_params(pol.actor)
    names = [n for n, _ in plan]
    assert len(names) == len(set(names))
    params = dict(pol.actor.named_parameters())
    assert sorted(names) == sorted(params)
    for n, shape in plan:
        assert tuple(params[n].shape) == tuple(shape), n
    # the ABI's slot count (include/sgrl_swat.h SGRL_SWAT_NW): 9 globals + 3 x 12 per layer (+ 2 for the final norm)
    assert len(plan) == 9 + 3 * 12 + (2 if tnorm else 0)
    if tnorm:        # the fixtures of the executed reference are for its default transformer_norm = 1
        with open(os.path.join(golden_dir, "swat_state_dict_keys.json")) as f:
            gold = json.load(f)["actor_cond%d" % cond]
        assert {"actor." + n: list(s) for n, s in plan} == gold


def test_plan_order_matches_the_slot_enums_of_the_header():
    from sgrl_amd.swat_hip import plan_params
    text = open(os.path.join(REPO, "include", "sgrl_swat.h")).read()
    glob = re.search(r"enum \{\s*SGRL_SWAT_EMB0 = 0,(.*?)SGRL_SWAT_NGLOBAL", text, re.S).group(0)
    layer = re.search(r"enum \{\s*SGRL_SWAT_IN_W = 0,(.*?)SGRL_SWAT_NLAYER", text, re.S).group(0)
    # every slot is documented with the state_dict name it takes: the plan must list the same names in the same order
    gnames = re.findall(r"/\* ([a-z_.0-9]+) \[", glob)
    lnames = re.findall(r"/\* ([a-z_.0-9]+) \[", layer)
    plan = [n for n, _ in plan_params(_swat().actor)]
    assert len(gnames) == 9 and len(lnames) == 12
    assert plan[:9] == gnames
    assert [p.split(".", 3)[3] for p in plan[9:21]] == lnames
    assert plan[-2:] == ["transformer_encoder.norm.weight", "transformer_encoder.norm.bias"]


def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sgrl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_swat_symbol():
    so = ctypes.CDLL(_lib.build())
    names = _declared("sgrl_swat.h")
    assert {"sgrl_swat_create", "sgrl_swat_destroy", "sgrl_swat_bind_params", "sgrl_swat_graph", "sgrl_swat_forward",
            "sgrl_swat_last_error"} <= set(names)
    for n in names:
        assert hasattr(so, n), n
    assert os.path.basename(_lib.CSRC) and "swat_actor.hip" in _lib.SOURCES


def test_no_cpu_fallback_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from sgrl_amd.swat_hip import HipSwatActor
    with pytest.raises(_lib.SgrlError):
        HipSwatActor(_swat())
    # and the raw ABI refuses too
    from sgrl_amd.swat_hip import _bind
    L = _lib.lib()
    _bind(L)
    h = ctypes.c_void_p()
    assert L.sgrl_swat_create(ctypes.byref(h)) == -3 and not h.value
    assert b"no CPU fallback" in L.sgrl_swat_last_error()


def test_rollout_picks_the_hip_forward_by_policy_type():
    from sgrl_amd.rollout import hip_actor_class
    from sgrl_amd.set_hip import HipSetActor
    from sgrl_amd.set_policy import SEPolicy
    from sgrl_amd.smp_policy import ActorGraphPolicy
    from sgrl_amd.swat_hip import HipSwatActor
    args = default_args()
    se = SEPolicy(41, 3, 32, 1, 1.0, 3, True, False, False, args, use_hip=False)
    assert hip_actor_class(se) is HipSetActor
    assert hip_actor_class(_swat()) is HipSwatActor
    smp = ActorGraphPolicy(41, 3, 32, 1, 1.0, 3, True, True, False, args)
    with pytest.raises(NotImplementedError, match="StructurePolicy"):
        hip_actor_class(smp)
