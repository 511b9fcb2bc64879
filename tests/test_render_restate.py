"""The float64 restatement of the ray caster (tests/render_restate.py) and the comparison the GPU tests use, qualified before any
kernel is involved: the reported hits against signed distance functions (independence), the comparison against deliberately wrong
restatements (sensitivity), and the share of pixels the comparison leaves out (condition)."""
from fractions import Fraction

import numpy as np
import pytest

import render_restate as R

NAMES = sorted(R.SCENES)


def _bodies(recs, o):
    """The sphere and capsule records that can be drawn from eye o: a geom that contains the eye is not."""
    return [r for r in recs if int(r[0]) != 0 and R.signed_distance(r, o) >= 0.0]


def _scene_distance(bodies, p):
    if not bodies:
        return np.full(p.shape[:-1], np.inf)
    return np.min([R.signed_distance(r, p) for r in bodies], axis=0)


def test_sky_bytes_in_exact_arithmetic():
    want = [int(Fraction(c) * 255 + Fraction(1, 2)) for c in ("0.55", "0.7", "0.9")]
    assert want == [140, 179, 230]
    s, ref = R.scene("batch")
    assert s.n_geoms[0] == 0 and (ref.hit[0] == -1).all()               # an image with no geoms is pure sky
    assert (ref.bytes[0] == np.array(want, dtype=np.uint8)).all()


@pytest.mark.parametrize("name", NAMES)
def test_hits_lie_on_the_surfaces_and_nothing_lies_before_them(name):
    s, ref = R.scene(name)
    for i in range(s.geoms.shape[0]):
        recs = s.geoms[i, :s.n_geoms[i]].astype(np.float64)
        o, d, t, hit = ref.o[i], ref.d[i].reshape(-1, 3), ref.t[i].reshape(-1), ref.hit[i].reshape(-1)
        bodies = _bodies(recs, o)
        planes = [r for r in recs if int(r[0]) == 0]
        # every reported hit point lies on the surface of the geom it names
        for g in np.unique(hit[hit >= 0]):
            sel = hit == g
            p = o + t[sel, None] * d[sel]
            if int(recs[g, 0]) == 0:
                assert np.abs(p[:, 2] - recs[g, 3]).max() < 1e-9, (name, i, g)
            else:
                assert R.signed_distance(recs[g], o) >= 0.0, (name, i, g)
                assert np.abs(R.signed_distance(recs[g], p)).max() < 1e-9, (name, i, g)
        # and the ray is outside every drawable body (and above every plane it looks down on) at 32 evenly spaced points before it
        sel = hit >= 0
        frac = np.arange(1, 33) / 33.0
        p = o + (t[sel, None] * frac)[..., None] * d[sel, None, :]
        assert (_scene_distance(bodies, p) > 0.0).all(), (name, i)
        for r in planes:
            assert (p[..., 2] - r[3] > 0.0)[d[sel, 2] < R.PLANE_DZ].all(), (name, i)
        # sky: no plane is reached, and sphere tracing finds no body along the ray
        sky = d[hit < 0]
        for r in planes:
            assert ((sky[:, 2] >= R.PLANE_DZ) | ((r[3] - o[2]) / sky[:, 2] <= 0.0)).all(), (name, i)
        if bodies and len(sky):
            far = np.linalg.norm(recs[:, 1:4] - o, axis=1).max() + 4.0
            tt, low, at = np.zeros(len(sky)), np.full(len(sky), np.inf), np.zeros(len(sky))
            for _ in range(400):
                dist = _scene_distance(bodies, o + tt[:, None] * sky)
                at, low = np.where(dist < low, tt, at), np.minimum(low, dist)
                tt = np.minimum(tt + np.maximum(dist, 1e-3), far)
                if (tt >= far).all():
                    break
            assert (tt >= far).all(), (name, i)
            lo, hi = np.maximum(at - 2e-3, 0.0), at + 2e-3              # the closest approach to within the tracer's smallest step
            for _ in range(60):
                m1, m2 = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
                left = _scene_distance(bodies, o + m1[:, None] * sky) < _scene_distance(bodies, o + m2[:, None] * sky)
                lo, hi = np.where(left, lo, m1), np.where(left, m2, hi)
            low = np.minimum(low, _scene_distance(bodies, o + (0.5 * (lo + hi))[:, None] * sky))
            assert (low > 0.0).all(), (name, i, float(low.min()))


def test_scenes_show_what_they_are_meant_to():
    s, ref = R.scene("occlusion")
    alone = lambda i, g: int((R.cast(s.geoms[i, g:g + 1], s.cams[i], s.width, s.height)["hit"] == 0).sum())
    seen = lambda i, g: int((ref.hit[i] == g).sum())
    assert 0 < seen(0, 2) < alone(0, 2) and 0 < seen(0, 3) < alone(0, 3)       # the capsule is partly hidden and partly hides
    assert seen(0, 1) == alone(0, 1) > 0
    assert seen(1, 0) > 0 and seen(1, 1) > 0 and seen(2, 0) > 0 and seen(2, 1) > 0
    assert seen(3, 0) == 0 and seen(3, 1) > 0 and seen(3, 2) > 0 and (ref.hit[3] == -1).any()     # looking upward: no plane
    assert seen(4, 1) == 0 and seen(4, 2) == 0 and seen(4, 3) > 0               # behind the camera
    assert seen(5, 1) == 0 and seen(5, 2) == 0 and seen(5, 3) > 0               # the eye is inside both
    neg = ref.o[0] + ref.t[0][..., None] * ref.d[0]
    floor = ref.hit[0] == 0
    assert (floor & (neg[..., 0] < -1.0) & (neg[..., 1] < -1.0)).any() and (floor & (neg[..., 0] > 1.0) & (neg[..., 1] > 1.0)).any()
    for name in ("axis_parallel_1x1", "axis_parallel_17x33", "axis_parallel_33x17"):
        s, ref = R.scene(name)
        for i in range(2):
            pa, pb = R.segment(s.geoms[i, 1].astype(np.float64))
            d = ref.d[i, s.height // 2, s.width // 2]
            assert (pb - pa) @ (pb - pa) - ((pb - pa) @ d) ** 2 <= 1e-12         # the central ray is parallel to the axis
            assert ref.hit[i, s.height // 2, s.width // 2] == 1
            assert abs(ref.t[i, s.height // 2, s.width // 2] - 2.4) < 1e-6       # and meets the near cap (float32 records)
    s, ref = R.scene("batch")
    assert s.n_geoms.tolist() == [0, 1, 64, 3, 64] and s.geoms.shape[1] == 64
    filler = R.to_bytes(np.array(R.FILLER))
    assert not (ref.bytes.reshape(-1, 3) == filler).all(-1).any()
    assert all((ref.hit[i] == 63).any() for i in (2, 4))
    s, ref = R.scene("real")
    assert all(len(np.unique(ref.hit[i])) > 3 for i in range(6))


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_passes_its_own_comparison_and_few_pixels_are_fragile(name):
    s, ref = R.scene(name)
    v = R.compare(ref.bytes, ref)
    print(name, "fragile share per image:", [round(float(f.mean()), 5) for f in ref.fragile])
    assert v.ok and v.max_diff == 0 and v.share == 0.0
    assert v.fragile_share <= R.MAX_FRAGILE, (name, v.fragile_share)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_comparison_rejects_every_mutant(mutant):
    rejected = []
    for name in NAMES:
        s, ref = R.scene(name)
        v = R.compare(R.render_mutant(s.geoms, s.n_geoms, s.cams, s.width, s.height, mutant), ref)
        if not v.ok:
            rejected.append((name, v.max_diff, round(v.share, 4)))
    print(mutant, "rejected on:", rejected)
    assert rejected, mutant


def test_a_single_level_everywhere_is_rejected_and_a_few_are_not():
    s, ref = R.scene("capsule_views")
    got = ref.bytes.copy()
    got[:, ::7, ::9, 1] ^= 1                                             # one level on 1 pixel in 63: inside both bars
    assert R.compare(got, ref).ok
    got = ref.bytes.copy()
    got[:, ::5, ::5, 1] ^= 1                                             # one level on 4 %
    v = R.compare(got, ref)
    assert not v.ok and v.max_diff == 1
    got = ref.bytes.copy()
    keep = np.argwhere(~ref.fragile[3])[0]
    got[3, keep[0], keep[1], 2] ^= 2                                     # two levels on one pixel
    v = R.compare(got, ref)
    assert not v.ok and v.max_diff == 2
