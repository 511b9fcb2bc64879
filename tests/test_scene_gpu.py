"""Render scenes assembled on the device (csrc/scene.hip, include/sgrl_render.h sgrl_scene) and what is built on them: the scenes
against their definition `render.scene_of` on the records read back, the launch count and the argument errors, the frames of
`get_images_device` against the ray caster fed the same scenes, the policy video demo (evaluate.VideoDemo) against the NumPy
restatement of the evaluation rule (tests/eval_restate.py), and DeviceTrainer.save_video_demo, which must leave the training state
alone."""
import ctypes
import os

import numpy as np
import pytest

from eval_restate import GroupedEval

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ["3d_walker_7_full", "3d_humanoid_9_full", "3d_cheetah_14_full", "3d_hopper_3_shin"]      # deepest chains, most geoms, a light one
IDS = [11, 0, 5, 5, 7, 3]            # unordered, a repeat, the last environment, all four morphologies
# both sides compute in float64 and round once to float32: they differ only where the float64 results straddle a rounding boundary
RTOL, ATOL = 2.4e-7, 1e-9            # two float32 ulps


@pytest.fixture(scope="module")
def env():
    from sgrl_amd.vec_env import BatchedModularVecEnv
    e = BatchedModularVecEnv(NAMES, 3, seed=2, device=DEV)
    yield e
    e.close()


def _walk(env, steps, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        a = torch.rand((env.num_envs, env.action_max_len), generator=g) * 2.0 - 1.0
        env.step_device(a.to(env.device).contiguous())
    torch.cuda.synchronize()


def _check_scenes(env, where):
    from sgrl_amd import render
    geoms, counts, cams = [t.cpu().numpy() for t in render.device_scenes(env, IDS)]
    rec, _ = env.get_records()
    mg = max(m.ngeom for m in env.models)
    assert geoms.shape == (len(IDS), mg, 16) and counts.shape == (len(IDS),) and cams.shape == (len(IDS), 13)
    assert geoms.dtype == np.float32 and counts.dtype == np.int32 and cams.dtype == np.float32
    worst = -np.inf                  # largest |difference| minus its bound: negative = inside
    for k, i in enumerate(IDS):
        m = env.models[env.env_morph[i]]
        want_g, want_c = render.scene_of(m, rec[i, :m.nq])
        n = m.ngeom
        assert counts[k] == n, (where, k)
        assert np.array_equal(geoms[k, :n, 0], want_g[:, 0]), (where, k, "type")
        assert np.array_equal(geoms[k, :n, 9:], want_g[:, 9:]), (where, k, "rgb and the unused tail")
        assert not geoms[k, n:].any(), (where, k, "padding")
        for got, want in ((geoms[k, :n, 1:9], want_g[:, 1:9]), (cams[k], want_c)):
            err = np.abs(got.astype(np.float64) - want) - (ATOL + RTOL * np.abs(want))
            worst = max(worst, float(err.max()))
            assert np.allclose(got, want, rtol=RTOL, atol=ATOL), (where, k, float(np.abs(got - want).max()))
    print(where, "largest |difference| - bound:", worst)


def test_scenes_equal_scene_of_on_the_records(env):
    env.reset_device()
    _check_scenes(env, "after reset")
    _walk(env, 25, seed=7)
    _check_scenes(env, "after 25 steps")


def test_one_launch_and_argument_errors(env):
    import torch
    from sgrl_amd import render
    L = render._bind(env._L)
    assert L.sgrl_scene_launches() == 1
    mg = max(m.ngeom for m in env.models)
    assert L.sgrl_max_geoms(env._h) == mg
    assert L.sgrl_max_geoms(None) == -1
    n = len(IDS)
    ids = torch.tensor(IDS, dtype=torch.int32, device=DEV)
    geoms = torch.full((n, mg, 16), 7.0, dtype=torch.float32, device=DEV)
    counts = torch.full((n,), 7, dtype=torch.int32, device=DEV)
    cams = torch.full((n, 13), 7.0, dtype=torch.float32, device=DEV)
    dist = render.camera_distances(env)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = [env._h, p(ids), n, ctypes.c_void_p(dist.ctypes.data), mg, p(geoms), p(counts), p(cams), None]
    ERR_ARG = -1
    for slot in (0, 1, 3, 5, 6, 7):                                # a null engine, ids, distances, geoms, counts, cameras
        bad = list(good)
        bad[slot] = None
        assert L.sgrl_scene(*bad) == ERR_ARG, slot
    for slot, value in ((2, 0), (2, -3), (4, mg - 1)):              # no image; one geom record too few
        bad = list(good)
        bad[slot] = value
        assert L.sgrl_scene(*bad) == ERR_ARG, (slot, value)
    torch.cuda.synchronize()
    assert bool((geoms == 7.0).all()) and bool((counts == 7).all()) and bool((cams == 7.0).all())      # nothing was launched
    assert L.sgrl_scene(*good) == 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [env.models[env.env_morph[i]].ngeom for i in IDS]
    for bad_ids in ([0, env.num_envs], [-1], []):
        with pytest.raises(ValueError):
            render.device_scenes(env, bad_ids)
    with pytest.raises(ValueError):
        env.get_images_device([env.num_envs], 8, 8)


def test_frames_are_the_ray_caster_on_the_device_scenes(env):
    import torch
    from sgrl_amd import render
    env.reset_device()
    a = env.get_images_device(IDS, 96, 64)
    assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == (len(IDS), 64, 96, 3)
    geoms, counts, cams = [t.cpu().numpy() for t in render.device_scenes(env, IDS)]
    scenes = [(geoms[k, :counts[k]], cams[k]) for k in range(len(IDS))]
    want = render.render(scenes, width=96, height=64, device=DEV)
    assert torch.equal(a, want)                                     # same input, same ray caster
    assert torch.equal(a[2], a[3])                                  # the repeated id
    assert torch.equal(env.get_images_device(IDS, 96, 64), a)       # deterministic
    out = torch.zeros_like(a)
    assert env.get_images_device(IDS, 96, 64, out=out) is out and torch.equal(out, a)
    assert len(torch.unique(a.reshape(-1, 3), dim=0)) > 8           # a picture, not a constant
    _walk(env, 30, seed=8)
    assert not torch.equal(env.get_images_device(IDS, 96, 64), a)


DEMO_NAMES = ["3d_walker_7_full", "3d_hopper_3_shin"]


def _demo(max_len, max_ep, chunk_frames):
    import torch
    from sgrl_amd.evaluate import VideoDemo
    from sgrl_amd.rollout import Rollout
    from sgrl_amd.set_policy import make_policy
    torch.manual_seed(4)
    ro = Rollout(DEMO_NAMES, 1, policy=make_policy(device=DEV).eval(), seed=5, device=DEV, max_episode_steps=max_ep)
    demo = VideoDemo(ro, width=64, height=48, max_trajectory_length=max_len, max_episode_steps=max_ep, chunk_frames=chunk_frames)
    out = demo.run()
    return ro, demo, out


def test_demo_frames_and_overlay_follow_the_reference_rule():
    import torch
    from sgrl_amd.vec_env import BatchedModularVecEnv
    ro, demo, (frames, overlay, close_step) = _demo(12, 8, chunk_frames=4)     # several chunks, the last one partial
    assert 1 <= close_step <= 8                                      # the time limit closes every episode by step 8
    assert isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.shape == (close_step + 1, 2, 48, 64, 3)
    assert overlay.shape == (close_step, 2, 4) and demo.last_dones.shape == (close_step, 2)
    assert close_step <= demo.last_steps <= min(12, close_step + 2)  # the stop flag is read a step late
    twin = BatchedModularVecEnv(DEMO_NAMES, 1, seed=5, device=DEV, max_episode_steps=8)
    twin.reset_device()
    assert np.array_equal(frames[0], twin.get_images_device(None, 64, 48).cpu().numpy())
    twin.close()
    for t in range(1, close_step + 1):
        assert not np.array_equal(frames[t], frames[t - 1]), t        # the bodies move
    ref = GroupedEval(np.zeros(2, dtype=np.int64), 1, 8)
    for t in range(close_step):
        ref.record(overlay[t, :, 1], demo.last_dones[t], t)
        assert np.array_equal(overlay[t, :, 2], ref.acc), t
        assert np.array_equal(overlay[t, :, 3], ref.ep_steps.astype(np.float64)), t
        assert np.isfinite(overlay[t]).all() and (overlay[t, :, 0] > 0).all()
    assert ref.close_step[0] == close_step and ref.open[0] == 0
    ro.env.close()


def test_demo_that_never_closes_has_every_frame():
    ro, demo, (frames, overlay, close_step) = _demo(5, 1000, chunk_frames=None)
    assert close_step == 0
    assert frames.shape == (6, 2, 48, 64, 3) and overlay.shape == (5, 2, 4) and demo.last_steps == 5
    assert not demo.last_dones.any()
    assert np.array_equal(overlay[:, :, 3], np.repeat(np.arange(1.0, 6.0)[:, None], 2, axis=1))
    assert np.array_equal(overlay[:, :, 2], np.cumsum(overlay[:, :, 1], axis=0))
    ro.env.close()


def test_trainer_demo_leaves_the_training_state_alone(tmp_path):
    import torch
    from PIL import Image
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_hopper_5_full", "3d_walker_7_full"]
    tr = DeviceTrainer(names, 2, args=default_train_args(max_episode_steps=20, batch_size=16), seed=3, device=DEV, max_buffer_size=256)
    tr.warmup(6)
    col = tr.sink.collector

    def snapshot():
        torch.cuda.synchronize()
        return ([t.clone() for t in (tr.ro.env.obs, col.done_list, col.episode_timesteps, col.episode_reward, col._reward_buf)],
                (tr.sink.stored, tr.tot_env_steps, tr.ro.env.get_counters().tolist()))
    before = snapshot()
    paths = tr.save_video_demo(tmp_path / "demos", width=48, height=48, max_trajectory_length=6)
    assert [os.path.basename(p) for p in paths] == ["0.gif", "1.gif"] and all(os.path.exists(p) for p in paths)
    for p in paths:
        with Image.open(p) as im:
            assert im.size == (48, 48) and 2 <= im.n_frames <= 7
    ro_demo = tr.demo_rollouts[tuple(names)][1]
    assert ro_demo is not tr.ro and ro_demo.env is not tr.ro.env and ro_demo.policy is tr.agent.actor and not ro_demo.holds_weights
    assert ro_demo.env.num_envs == 2                                 # one environment per morphology
    held_out = ["3d_hopper_3_shin"]
    zero_shot = tr.save_video_demo(tmp_path / "zero_shot", width=48, height=48, max_trajectory_length=6, env_names=held_out)
    assert [os.path.basename(p) for p in zero_shot] == ["0.gif"]
    assert tr.demo_rollouts[tuple(names)][1] is ro_demo              # cached
    after = snapshot()
    assert after[1] == before[1]
    for a, b in zip(before[0], after[0]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    tr.collect_step(random_actions=True)                             # the training loop goes on
    torch.cuda.synchronize()
