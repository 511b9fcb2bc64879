"""Host side of the MLP HIP forward (sgrl_amd/mlp_hip.py `plan` over include/sgrl_mlp.h sgrl_mlp_plan; no GPU needed): padded widths,
packed-buffer offsets, kernel variant, LDS bytes and tile counts against a NumPy restatement (tests/mlp_restate.py), and the
argument errors of the plan."""
import pytest

from mlp_restate import plan_restated
from sgrl_amd import _lib, mlp_hip

CASES = [([123, 256, 256, 9], 1), ([287, 256, 256, 21], 8192), ([574, 256, 256, 42], 65), ([123, 40, 72, 9], 63), ([287, 40, 72, 21], 130),
         ([287, 256, 21], 31), ([287, 64, 48, 80, 32, 21], 33), ([574, 1024, 1024, 42], 64), ([41, 1, 3], 1), ([1024, 512, 3], 7),
         ([574, 257, 513, 42], 2), ([16, 32, 1024, 1024, 1024, 1024], 100)]


@pytest.mark.parametrize("dims,n_env", CASES)
def test_plan_matches_the_restatement(dims, n_env):
    got, want = mlp_hip.plan(dims, n_env), plan_restated(dims, n_env)
    assert got == want
    nl = len(dims) - 1
    assert got["kpad"][0] % 16 == 0 and got["kpad"][0] >= dims[0] and all(n % 32 == 0 for n in got["npad"])
    assert all(got["npad"][l] >= dims[l + 1] and got["kpad"][l] % got["bk"] == 0 for l in range(nl))
    assert got["kpad"][1:] == got["npad"][:-1]
    assert got["lds_bytes"] <= 160 * 1024 and 256 * got["chunks"] >= max(got["npad"])
    assert got["tiles"] * got["tile_rows"] >= n_env > (got["tiles"] - 1) * got["tile_rows"]
    # regions of the packed buffer tile it without overlap
    spans = sorted([(got["w_off"][l], got["npad"][l] * got["kpad"][l]) for l in range(nl)] + [(got["b_off"][l], got["npad"][l]) for l in range(nl)])
    pos = 0
    for off, size in spans:
        assert off == pos
        pos += size
    assert pos == got["total"]


@pytest.mark.parametrize("dims", [[287, 21], [287, 8, 8, 8, 8, 8, 21], [287, 1025, 21], [1025, 256, 21], [287, 256, 0], [287, 256, 1025]])
def test_plan_refuses_what_the_kernel_is_not_built_for(dims):
    with pytest.raises(_lib.SgrlError):
        mlp_hip.plan(dims)


def test_net_dims_of_a_policy():
    from sgrl_amd.mlp_policy import MlpPolicy
    from sgrl_amd.td3 import default_train_args
    args = default_train_args(mlp_num_limbs=14)
    args.agent.policy_network = {"hidden_dims": [40, 72]}
    pol = MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, args)
    assert mlp_hip.net_dims(pol.actor) == [574, 40, 72, 42]
