"""The two-half SET forward (include/sgrl_set.h, sgrl_set_last_split) against the single pass.

A batch on the fused tile-kernel path is cut at an environment boundary and its halves run as two staggered chains of the same
kernels on the handle's two streams.  Per row neither the kernels nor their order nor their arithmetic change, so the actions
must be BIT-IDENTICAL to those of the single pass (SGRL_SET_SPLIT=0): no tolerance.  The switch is read once per process, so
each arm is a child process (this file run as a script), as tests/test_set_gpu.py does for its A/B product forms."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WALKERS = ["3d_walker_2_right_leg_left_knee", "3d_walker_3_left_knee_right_knee", "3d_walker_3_left_leg_right_foot",
           "3d_walker_4_right_knee_left_foot", "3d_walker_5_foot", "3d_walker_5_left_knee", "3d_walker_6_right_foot",
           "3d_walker_7_full"]
CASES = {
    "walker8x1024": (WALKERS, [1024] * 8),                                            # the benchmark's batch: 35 840 nodes
    "uneven3x700": ([WALKERS[7], WALKERS[0], WALKERS[4]], [700] * 3),                  # 9 800 nodes, halves of different make-up
    "small": ([WALKERS[7], WALKERS[0]], [100, 100]),                                   # 900 nodes: below the small-batch threshold
}


def _child(case, out_path):
    sys.path.insert(0, REPO)
    import torch
    from oracle.formula import apply_formula_
    from sgrl_amd import graph as G, mjcf
    from sgrl_amd.set_hip import HipSetActor
    from sgrl_amd.set_policy import make_policy
    names, counts = CASES[case]
    torch.manual_seed(0)
    pol = make_policy(device="cuda:0").eval()
    apply_formula_(pol)
    gds = [G.getGraphDict(mjcf.load_asset(n).parents, ["pre", "inlcrs", "postlcrs"], [], device=torch.device("cuda:0")) for n in names]
    act = HipSetActor(pol)
    act.configure(gds, counts)
    gen = torch.Generator().manual_seed(7)
    obs = (torch.randn((sum(counts), 287), generator=gen) * 0.5).cuda()
    a1 = act.forward_batch(obs).clone()
    split1 = act.last_split()
    act.hold_weights(True)                      # the rollout's way: packed once, then reused
    a2 = act.forward_batch(obs).clone()
    a3 = act.forward_batch(obs).clone()
    ms = act.time_forward(obs, torch.empty_like(a1), 3)      # back-to-back forwards on one stream
    a4 = act.forward_batch(obs).clone()
    torch.cuda.synchronize()
    np.save(out_path, a1.cpu().numpy())
    print(json.dumps({"nodes": act.num_nodes, "split": split1, "split_after": act.last_split(),
                      "repeatable": bool(torch.equal(a1, a2) and torch.equal(a1, a3) and torch.equal(a1, a4)),
                      "finite": bool(torch.isfinite(a1).all()), "nonzero": bool((a1 != 0).any()), "ms": ms,
                      "redos": act.scale_redos()}))


def _run(case, tmp_path, split_env):
    out = os.path.join(str(tmp_path), "%s_%s.npy" % (case, split_env if split_env is not None else "default"))
    env = dict(os.environ)
    env.pop("SGRL_SET_SPLIT", None)
    if split_env is not None:
        env["SGRL_SET_SPLIT"] = split_env
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert info["finite"] and info["nonzero"] and info["repeatable"], info
    assert info["redos"] == 0, info
    return info, np.load(out)


@pytest.mark.parametrize("case", ["walker8x1024", "uneven3x700"])
def test_two_halves_give_the_single_pass_bit_for_bit(case, tmp_path):
    import torch
    single_info, single = _run(case, tmp_path, "0")
    assert single_info["split"] == 0 and single_info["split_after"] == 0, single_info
    for mode in (None, "2", "3"):               # the default form and the two kept for comparison (include/sgrl_set.h)
        info, got = _run(case, tmp_path, mode)
        print(case, mode, info)
        assert info["nodes"] >= 2048 and 0 < info["split"] < info["nodes"], info
        assert abs(2 * info["split"] - info["nodes"]) <= info["nodes"] // 16, info       # near the middle
        assert info["split_after"] == info["split"], info
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(single)), (case, mode)


def test_small_batches_keep_the_single_pass(tmp_path):
    import torch
    info, got = _run("small", tmp_path, None)
    assert info["nodes"] < 2048 and info["split"] == 0 and info["split_after"] == 0, info
    _, single = _run("small", tmp_path, "0")
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(single))


def test_tile_kernels_below_the_size_keep_the_single_pass():
    """sgrl_set_debug_small_nodes(0) puts a tiny batch on the tile kernels (what smoke() and the parity tests do): still one pass."""
    import torch
    from sgrl_amd import graph as G, mjcf
    from sgrl_amd.set_hip import HipSetActor
    from sgrl_amd.set_policy import make_policy
    pol = make_policy(device="cuda:0").eval()
    act = HipSetActor(pol)
    names = [WALKERS[7], WALKERS[0]]
    act.configure([G.getGraphDict(mjcf.load_asset(n).parents, ["pre", "inlcrs", "postlcrs"], [], device=torch.device("cuda:0")) for n in names], [4, 4])
    obs = torch.randn((8, 287), device="cuda:0") * 0.5
    base = act.forward_batch(obs).clone()
    act.debug_small_nodes(0)
    tile = act.forward_batch(obs)
    assert act.last_split() == 0
    assert float((tile - base).abs().max()) < 2e-5


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
