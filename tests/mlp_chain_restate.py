"""NumPy restatement of include/sgrl_mlp.h sgrl_mlp_chain_plan (what the fused TD3 target-chain kernel uses for an actor / critic
pair), on top of mlp_restate.plan_restated."""
from mlp_restate import plan_restated


def chain_plan_restated(actor_dims, critic_dims, tile_rows=32, lds_limit=160 * 1024):
    """Column chunks: the larger of the two networks' plans.  Activation row stride: the widest padded input of either network + 4.
    Weight panels 16 deep unless LDS only has room for 8 beside the activation tile; LDS = the tile + two panels of 256 rows."""
    pa, pc = plan_restated(actor_dims), plan_restated(critic_dims)
    assert critic_dims[-1] == 1 and critic_dims[0] == actor_dims[0] + actor_dims[-1]
    sx = max(max(pa["kpad"]), max(pc["kpad"])) + 4
    lds = lambda bk: 4 * (tile_rows * sx + 2 * 256 * (bk + 4))
    bk = 16 if lds(16) <= lds_limit else 8
    return {"chunks": max(pa["chunks"], pc["chunks"]), "bk": bk, "lds_bytes": lds(bk), "sx": sx, "tile_rows": tile_rows}
