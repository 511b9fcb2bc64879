"""The host half of the policy video demo (sgrl_amd/evaluate.py write_demo_gifs): one GIF per environment, the frames kept as they
are, the reference's four text lines inside the top band of every frame but the first; and the demo itself refuses to run without
a device (no CPU fallback)."""
import os

import numpy as np
import pytest

from sgrl_amd import _lib
from sgrl_amd.evaluate import write_demo_gifs

T, N, H, W = 4, 3, 120, 420


def _frames():
    """uint8 [T + 1, N, H, W, 3]: 10 x 10 blocks of 8 colours below row 100 and ONE colour per frame above it, where the text goes
    -- so that a frame still has fewer than 256 colours with the anti-aliased text on it (8 + the blends of yellow with one
    colour) and the GIF palette holds every one of them exactly.  Every frame of every environment differs."""
    rng = np.random.RandomState(5)
    levels = np.array([20, 200], dtype=np.uint8)
    blocks = levels[rng.randint(0, 2, size=(T + 1, N, H // 10, W // 10, 3))]
    out = np.ascontiguousarray(blocks.repeat(10, axis=2).repeat(10, axis=3))
    out[:, :, :100] = levels[rng.randint(0, 2, size=(T + 1, N, 1, 1, 3))]
    out[:, :, :100, :, 2] = 20                                      # never the text's own yellow ... nor white
    return out


def _overlay():
    rng = np.random.RandomState(6)
    ov = rng.normal(size=(T, N, 4))
    ov[:, :, 3] = np.arange(1, T + 1)[:, None]
    return ov


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        n = im.n_frames
        out = []
        for k in range(n):
            im.seek(k)
            out.append(np.asarray(im.convert("RGB")))
    return n, np.stack(out)


def test_one_gif_per_environment_with_every_frame_and_the_right_size(tmp_path):
    frames = _frames()
    paths = write_demo_gifs(frames, _overlay(), str(tmp_path / "demos"), fps=60, text=True)
    assert [os.path.basename(p) for p in paths] == ["%d.gif" % i for i in range(N)]
    assert sorted(os.listdir(str(tmp_path / "demos"))) == ["%d.gif" % i for i in range(N)]
    for p in paths:
        n, dec = _decode(p)
        assert n == T + 1 and dec.shape == (T + 1, H, W, 3)


def test_without_text_the_frames_decode_to_the_input(tmp_path):
    frames = _frames()
    paths = write_demo_gifs(frames, _overlay(), str(tmp_path), text=False)
    for i, p in enumerate(paths):
        n, dec = _decode(p)
        assert n == T + 1
        assert np.array_equal(dec[0], frames[0, i])
        assert np.array_equal(dec, frames[:, i])


def test_text_stays_inside_the_top_band_and_off_the_first_frame(tmp_path):
    frames = _frames()
    paths = write_demo_gifs(frames, _overlay(), str(tmp_path), text=True)
    for i, p in enumerate(paths):
        _, dec = _decode(p)
        assert np.array_equal(dec[0], frames[0, i])
        for t in range(1, T + 1):
            diff = (dec[t] != frames[t, i]).any(axis=-1)
            assert diff.any(), "no text on frame %d" % t
            assert not diff[100:].any()
            assert not diff[:, :100].any()                          # the lines start at x = 100
            changed = dec[t][diff]
            # the reference's yellow (255, 255, 0), blended into the band's colour by the font's anti-aliasing
            assert ((changed[:, 0] >= 240) & (changed[:, 1] >= 240) & (changed[:, 2] <= 20)).any()


def test_shapes_are_checked(tmp_path):
    frames = _frames()
    with pytest.raises(ValueError):
        write_demo_gifs(frames, _overlay()[:-1], str(tmp_path))
    with pytest.raises(ValueError):
        write_demo_gifs(frames.astype(np.float32), _overlay(), str(tmp_path))


def test_the_demo_needs_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from sgrl_amd.rollout import Rollout
    with pytest.raises(_lib.SgrlError):
        Rollout(["3d_hopper_3_shin"], 1)                            # what a VideoDemo runs over
    from sgrl_amd import render
    with pytest.raises(_lib.SgrlError):
        render.render_device(torch.zeros((1, 4, 16)), torch.zeros(1, dtype=torch.int32), torch.zeros((1, 13)), 8, 8)
