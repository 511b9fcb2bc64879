"""BatchedModularVecEnv.get_images() through the ray caster (sgrl_amd/render.py, csrc/render.hip): geometric property tests, and the
kernel's bytes against the float64 restatement of its own definition (tests/render_restate.py, qualified on the CPU by
tests/test_render_restate.py) -- MuJoCo's renderer is a third-party dependency, pixel parity with it is neither claimed nor pinned."""
import ctypes

import numpy as np
import pytest
import torch

import render_restate as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_a_single_sphere_projects_where_geometry_says():
    from sgrl_amd import render
    geoms = np.zeros((2, render.GEOM_FLOATS), dtype=np.float32)
    geoms[0, 0], geoms[0, 9:12] = 0, [0.7, 0.7, 0.7]                                  # ground plane z = 0
    geoms[1, 0], geoms[1, 1:4], geoms[1, 7], geoms[1, 9:12] = 2, [0.0, 5.0, 1.0], 0.5, [1.0, 0.0, 0.0]   # red sphere
    cam = np.array([0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 1, np.tan(np.deg2rad(45.0) / 2)], dtype=np.float32)     # at (0,0,1) looking along +y
    img = render.render([(geoms, cam)], width=200, height=200)[0].cpu().numpy()
    red = (img[..., 0] > 100) & (img[..., 1] < 60) & (img[..., 2] < 60)
    ys, xs = np.nonzero(red)
    assert abs(xs.mean() - 99.5) < 1.0 and abs(ys.mean() - 99.5) < 1.0                 # dead centre
    # silhouette radius: tan(asin(r / d)) / tan(fovy / 2) * (height / 2)
    expect = np.tan(np.arcsin(0.5 / 5.0)) / np.tan(np.deg2rad(22.5)) * 100
    assert abs((xs.max() - xs.min() + 1) / 2 - expect) < 1.5 and abs((ys.max() - ys.min() + 1) / 2 - expect) < 1.5
    assert (img[:90] .astype(int).sum(-1) > 0).all()                                   # sky above the horizon is painted too
    # row 150 meets the floor at y = 1 / (0.505 tan(fovy / 2)) = 4.78; column 120 at x = 0.41, column 160 at x = 1.20: cells (0, 4), (1, 4)
    cell = lambda col: int(np.floor((2 * (col + 0.5) / 200 - 1) / 0.505)) + int(np.floor(1 / (0.505 * np.tan(np.deg2rad(22.5)))))
    assert (cell(120) + cell(160)) % 2 == 1
    assert not np.array_equal(img[150, 120], img[150, 160])                            # opposite checker parity, different shade
    floor = img[160:, :, :]
    assert floor.std() > 5                                                             # the checker pattern is visible


def test_get_images_shows_the_robot_and_follows_it():
    from sgrl_amd.vec_env import BatchedModularVecEnv
    env = BatchedModularVecEnv(["3d_walker_7_full", "3d_humanoid_9_full"], 2, seed=2, device="cuda:0")
    env.reset()
    a = env.get_images(width=160, height=120)
    assert a.shape == (4, 120, 160, 3) and a.dtype == np.uint8
    b = env.get_images(width=160, height=120)
    assert np.array_equal(a, b)                                                        # deterministic
    sky = np.array([0.55, 0.7, 0.9]) * 255
    for img in a:
        body = (np.abs(img[30:100, 50:110].astype(float) - sky).sum(-1) > 60) & (img[30:100, 50:110].astype(int).std(-1) > 8)
        assert body.mean() > 0.02                                                      # something that is neither sky nor grey floor near the centre
    assert not np.array_equal(a[0], a[2])                                              # different morphologies look different
    sub = env.get_images(env_ids=[3], width=160, height=120)
    assert np.array_equal(sub[0], a[3])
    for _ in range(30):
        env.step([np.random.RandomState(1).uniform(-1, 1, size=env.action_max_len) for _ in range(env.num_envs)])
    c = env.get_images(width=160, height=120)
    assert not np.array_equal(a[0], c[0])                                              # the pose changed, so did the frame
    env.close()


def _through_both_paths(s):
    """The frames of a scene through render.render_device (the arrays as they are, records beyond the counts included) and
    through render.render (host lists cut at the counts)."""
    from sgrl_amd import render
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared scenes are read-only
    dev = render.render_device(up(s.geoms), up(s.n_geoms), up(s.cams), width=s.width, height=s.height)
    lists = [(s.geoms[i, :s.n_geoms[i]], s.cams[i]) for i in range(s.geoms.shape[0])]
    host = render.render(lists, width=s.width, height=s.height, device=DEV)
    torch.cuda.synchronize()
    return dev.cpu().numpy(), host.cpu().numpy()


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_frames_equal_the_float64_restatement(name):
    """Measured on an MI355X (largest difference in levels, largest share of differing non-fragile pixels over the images): see
    DESIGN, the paragraph on the ray caster's parity with its own definition."""
    s, ref = R.scene(name)
    assert (s.width, s.height) in ((1, 1), (17, 33), (33, 17), (48, 40), (96, 64), (64, 48)) and s.geoms.shape[0] <= 6
    for path, got in zip(("render_device", "render"), _through_both_paths(s)):
        v = R.compare(got, ref)
        print("%s via %s: max difference %d level(s), share of differing pixels %.4f, fragile share %.4f"
              % (name, path, v.max_diff, v.share, v.fragile_share))
        assert v.ok, (name, path, v)


def test_a_count_above_max_geoms_is_bounded_by_it():
    from sgrl_amd import render
    s = R.bounded_counts()
    assert s.geoms.shape == (3, 4, 16) and s.n_geoms.tolist() == [9, 4, 0] and not s.geoms[2].any()
    geoms = torch.from_numpy(s.geoms).to(DEV)                          # three images' worth of records; two are rendered
    got = render.render_device(geoms[:2], torch.from_numpy(s.n_geoms[:2]).to(DEV), torch.from_numpy(s.cams[:2]).to(DEV),
                               width=s.width, height=s.height).cpu().numpy()
    ref = R.render_ref(s.geoms[:2], [4, 4], s.cams[:2], s.width, s.height)
    leaked = R.render_ref(s.geoms.reshape(1, 12, 16), [9], s.cams[:1], s.width, s.height)      # what reading on would show
    assert not R.compare(leaked.bytes, R.render_ref(s.geoms[:1], [4], s.cams[:1], s.width, s.height)).ok
    v = R.compare(got, ref)
    print("bounded counts: max difference %d level(s), share %.4f, fragile share %.4f" % (v.max_diff, v.share, v.fragile_share))
    assert v.ok, v
    assert v.fragile_share <= R.MAX_FRAGILE


def test_render_argument_errors_launch_nothing():
    from sgrl_amd import render
    L = render._bind(render._lib.lib())
    s, _ = R.scene("occlusion")
    n, mg = s.geoms.shape[0], s.geoms.shape[1]
    geoms, counts, cams = (torch.from_numpy(np.array(a)).to(DEV) for a in (s.geoms, s.n_geoms, s.cams))
    wide = torch.zeros((n, 65, 16), dtype=torch.float32, device=DEV)   # backs the max_geoms = 65 call, should it ever launch
    out = torch.full((n, s.height, s.width, 3), 7, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = [p(geoms), p(counts), mg, p(cams), n, s.width, s.height, p(out), None]
    ERR_ARG = -1
    for slot in (0, 1, 3, 7):                                          # null geoms, counts, cameras, output
        bad = list(good)
        bad[slot] = None
        assert L.sgrl_render(*bad) == ERR_ARG, slot
    for slot, value in ((2, 0), (2, -1), (4, 0), (4, -2), (5, 0), (5, -1), (6, 0), (6, -1)):
        bad = list(good)
        bad[slot] = value
        assert L.sgrl_render(*bad) == ERR_ARG, (slot, value)
    bad = list(good)
    bad[0], bad[2] = p(wide), 65                                       # one record more than the kernel stages
    assert L.sgrl_render(*bad) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                      # nothing was launched
    assert L.sgrl_render(*good) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7).all())
