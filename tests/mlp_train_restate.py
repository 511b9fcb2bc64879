"""NumPy restatement of include/sgrl_mlp.h sgrl_mlp_train_plan (what the gradient half of an MLP agent's TD3 update uses for an
actor / critic pair at a batch size), on top of mlp_restate.plan_restated."""
from mlp_restate import plan_restated

TRAIN_MAX_WIDTH = 512


def _wgrad_tiles(dims):
    """One workgroup per 32 x 32 tile of every UNPADDED dW_l [dims[l + 1]][dims[l]]."""
    return sum(-(-dims[l + 1] // 32) * -(-dims[l] // 32) for l in range(len(dims) - 1))


def _ws_floats(p, dims, stacks, batch, tile_rows):
    """Input tile [B, kpad_0]; per stack the hidden activations [B, npad_l] and every G_l [B, npad_l]; an actor adds tanh(z)
    [B, npad_last] and the action rows [B, out]; two loss partials per row tile and stack."""
    hidden, every = sum(p["npad"][:-1]), sum(p["npad"])
    n = batch * p["kpad"][0] + stacks * batch * (hidden + every)
    if stacks == 1:
        n += batch * (p["npad"][-1] + dims[-1])
    return n + 2 * stacks * (-(-batch // tile_rows))


def train_plan_restated(actor_dims, critic_dims, batch, tile_rows=32, lds_limit=160 * 1024):
    """Column chunks from the widest padded layer OUTPUT of either network (at most 512: two chunks).  Activation row stride: the
    widest padded width of either network, input or output, + 4 (the backward pass keeps G of the last layer in the tile too).
    Panels and LDS as the chain's."""
    pa, pc = plan_restated(actor_dims), plan_restated(critic_dims)
    assert critic_dims[-1] == 1 and critic_dims[0] == actor_dims[0] + actor_dims[-1]
    nmax = max(pa["npad"] + pc["npad"])
    assert nmax <= TRAIN_MAX_WIDTH
    sx = max(pa["kpad"] + pa["npad"] + pc["kpad"] + pc["npad"]) + 4
    lds = lambda bk: 4 * (tile_rows * sx + 2 * 256 * (bk + 4))
    bk = 16 if lds(16) <= lds_limit else 8
    return {"chunks": 1 if nmax <= 256 else 2, "bk": bk, "lds_bytes": lds(bk), "sx": sx, "critic_wgrad_tiles": 2 * _wgrad_tiles(critic_dims),
            "actor_wgrad_tiles": _wgrad_tiles(actor_dims), "row_tiles": -(-batch // tile_rows),
            "critic_ws_floats": _ws_floats(pc, critic_dims, 2, batch, tile_rows), "actor_ws_floats": _ws_floats(pa, actor_dims, 1, batch, tile_rows),
            "tile_rows": tile_rows}
