"""Float64 NumPy restatement of the ray caster (sgrl_amd/csrc/render.hip, include/sgrl_render.h), the comparison its tests share and
the scenes they render.  Deliberately plainer than the kernel and NOT a transliteration of it:

  * a capsule is the union of a finite cylinder and two spheres.  Its entry point is the smallest positive entry root of the three,
    where the root of the (infinite) cylinder counts only between the end planes, 0 < y < |ba|^2; the cylinder is intersected in the
    components perpendicular to the unit axis, not in the kernel's |ba|^2-scaled closed form; there is no branch for a ray parallel
    to the axis (the cylinder's quadratic degenerates, its root is not finite and does not count; the two spheres cover the case);
  * the normal is the hit point minus the closest point of the segment, divided by r;
  * "entry points only" is stated once: a sphere or capsule whose signed distance at the eye is negative is not drawn.

What is the same is the definition: the ray through the pixel centre, the record layout of include/sgrl_render.h, the nearest hit with
t > 1e-4 (the plane: t > 0, as the kernel has it; the two differ only for an eye within 1e-4 of the plane, which no scene has), the
plane only for d.z < -1e-6, colour * (0.35 + 0.45 max(-n.d, 0) + 0.2 max(n.z, 0)), the sky unshaded,
byte = floor(clip(c * 255 + 0.5, 0, 255)).  The sky is the decimal colour (0.55, 0.7, 0.9): 0.7 * 255 + 0.5 and 0.9 * 255 + 0.5 are the
integers 179 and 230 (test_render_restate.py checks the bytes in exact rational arithmetic).

A pixel is FRAGILE when this reference's own answer is not stable under float32-sized perturbation:
  * the hit id differs when every radius is scaled by 1 + 1e-4 or by 1 - 1e-4 (silhouettes and the curves where two geoms meet);
  * the checker parity differs when the floor hit point moves by +-8 * 2^-24 * (|o| + t) in x or in y;
  * |d.z + 1e-6| < 1e-6 (the plane's own threshold).
Fragile pixels are the only ones `compare` leaves out.
"""
import collections
import functools

import numpy as np

GEOM_FLOATS, CAM_FLOATS, MAX_GEOMS = 16, 13, 64
SKY = np.array([0.55, 0.7, 0.9])
T_MIN, PLANE_DZ = 1e-4, -1e-6
RADIUS_EPS, FLOOR_EPS = 1e-4, 8.0 * 2.0 ** -24
MAX_LEVELS, MAX_SHARE, MAX_FRAGILE = 1, 0.02, 0.01          # the bars of `compare`, and the cap on the fragile share per image

MUTANTS = ("wrong_cap", "no_clamp", "no_parallel", "short_loop", "next_camera", "trunc_checker", "no_l2", "half_segment")


# ---------------------------------------------------------------------------------------------------------------- geometry
def rays(cam, width, height):
    """(eye [3], unit directions [height, width, 3]) through the pixel centres."""
    cam = np.asarray(cam, dtype=np.float64)
    o, fwd, right, up, th = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12]
    px, py = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    u = (2.0 * (px + 0.5) / width - 1.0) * th * (float(width) / float(height))
    v = (1.0 - 2.0 * (py + 0.5) / height) * th
    d = fwd + u[..., None] * right + v[..., None] * up
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


def is_capsule(rec):
    return int(rec[0]) == 3 and rec[8] > 0.0


def segment(rec, mutant=None):
    """End points of a capsule's segment (a sphere: both are its centre)."""
    c, ax, hl = rec[1:4], rec[4:7], rec[8]
    if not is_capsule(rec):
        return c, c
    return c - hl * ax, (c if mutant == "half_segment" else c + hl * ax)


def closest_on_segment(p, pa, pb, clamp=True):
    ba = pb - pa
    l2 = ba @ ba
    if l2 == 0.0:
        return np.broadcast_to(pa, p.shape)
    f = ((p - pa) @ ba) / l2
    if clamp:
        f = np.clip(f, 0.0, 1.0)
    return pa + f[..., None] * ba


def signed_distance(rec, p):
    """dist(point, segment) - r of a sphere or capsule record at points p [..., 3]."""
    rec = np.asarray(rec, dtype=np.float64)
    pa, pb = segment(rec)
    return np.linalg.norm(p - closest_on_segment(p, pa, pb), axis=-1) - rec[7]


def _sphere_entry(o, d, c, r):
    oc = o - c
    b = d @ oc
    h = b * b - (oc @ oc - r * r)
    return np.where(h > 0.0, -b - np.sqrt(np.maximum(h, 0.0)), np.inf)


def _body_hit(rec, o, d, mutant):
    """(t [h, w], inf where the sphere or capsule is not hit; normal [h, w, 3])."""
    r = rec[7]
    pa, pb = segment(rec, mutant)
    if signed_distance(rec, o) < 0.0:                                   # the eye is inside: entry points only, nothing is drawn
        return np.full(d.shape[:-1], np.inf), np.zeros_like(d)
    which = None
    if not is_capsule(rec):
        t = _sphere_entry(o, d, pa, r)
        t = np.where(t > 0.0, t, np.inf)
    else:
        ba = pb - pa
        l2 = ba @ ba
        e = ba / np.sqrt(l2)
        oa = o - pa
        dp, op = d - (d @ e)[..., None] * e, oa - (oa @ e) * e            # components perpendicular to the axis
        with np.errstate(all="ignore"):
            qa, qb, qc = (dp * dp).sum(-1), dp @ op, op @ op - r * r
            tc = (-qb - np.sqrt(qb * qb - qa * qc)) / qa
            y = (oa + tc[..., None] * d) @ ba
            tc = np.where(np.isfinite(tc) & (y > 0.0) & (y < l2), tc, np.inf)
        cand = np.stack([_sphere_entry(o, d, pa, r), _sphere_entry(o, d, pb, r), tc])
        cand = np.where(cand > 0.0, cand, np.inf)
        which, t = cand.argmin(0), cand.min(0)
        if mutant == "wrong_cap":                                        # a cap hit takes the sphere at the other end
            t = np.where(which == 0, cand[1], np.where(which == 1, cand[0], t))
        if mutant == "no_parallel":
            t = np.where(l2 - (d @ ba) ** 2 <= 1e-12, np.inf, t)
    p = o + np.where(np.isfinite(t), t, 0.0)[..., None] * d
    foot = closest_on_segment(p, pa, pb, clamp=mutant != "no_clamp")
    if mutant == "wrong_cap" and which is not None:
        foot = np.where((which == 0)[..., None], pb, np.where((which == 1)[..., None], pa, foot))
    return t, (p - foot) / r


def _plane_hit(rec, o, d, mutant):
    """(t, checker parity) of the horizontal plane at the record's centre z."""
    dz = d[..., 2]
    ok = dz < PLANE_DZ
    t = np.where(ok, (rec[3] - o[2]) / np.where(ok, dz, 1.0), np.inf)
    t = np.where(t > 0.0, t, np.inf)
    tt = np.where(np.isfinite(t), t, 0.0)
    return t, checker(o[0] + tt * d[..., 0], o[1] + tt * d[..., 1], mutant)


def checker(x, y, mutant=None):
    cell = np.trunc if mutant == "trunc_checker" else np.floor
    return ((cell(x).astype(np.int64) + cell(y).astype(np.int64)) & 1).astype(bool)


def cast(recs, cam, width, height, radius_scale=1.0, mutant=None):
    """One image: dict of o, d, t (inf for sky), hit (-1 for sky), colour [h, w, 3] before quantisation."""
    recs = np.array(recs, dtype=np.float64).reshape(-1, GEOM_FLOATS)
    recs[:, 7] *= radius_scale
    o, d = rays(cam, width, height)
    best = np.full((height, width), np.inf)
    hit = np.full((height, width), -1, dtype=np.int64)
    nrm = np.zeros((height, width, 3))
    col = np.broadcast_to(SKY, (height, width, 3)).copy()
    for g in range(recs.shape[0] - (1 if mutant == "short_loop" else 0)):
        rec = recs[g]
        if int(rec[0]) == 0:
            t, par = _plane_hit(rec, o, d, mutant)
            n = np.broadcast_to(np.array([0.0, 0.0, 1.0]), d.shape)
            c = rec[9:12] * np.where(par, 0.9, 0.6)[..., None]
            new = t < best
        else:
            t, n = _body_hit(rec, o, d, mutant)
            c = np.broadcast_to(rec[9:12], d.shape)
            new = (t > T_MIN) & (t < best)
        best, hit = np.where(new, t, best), np.where(new, g, hit)
        nrm, col = np.where(new[..., None], n, nrm), np.where(new[..., None], c, col)
    l1 = np.maximum(-(nrm * d).sum(-1), 0.0)
    l2 = 0.0 if mutant == "no_l2" else np.maximum(nrm[..., 2], 0.0)
    shade = np.where(hit >= 0, 0.35 + 0.45 * l1 + 0.2 * l2, 1.0)
    return {"o": o, "d": d, "t": best, "hit": hit, "colour": col * shade[..., None]}


def to_bytes(colour):
    return np.floor(np.clip(colour * 255.0 + 0.5, 0.0, 255.0)).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------- reference
class Ref(object):
    """colour float64 [n, h, w, 3] before quantisation, hit int [n, h, w] (-1 sky), fragile bool [n, h, w]; for the tests of the
    reference itself also the eyes o [n, 3], the directions d [n, h, w, 3] and the hit distances t [n, h, w] (inf for sky)."""

    def __init__(self, images, fragile):
        self.colour = np.stack([im["colour"] for im in images])
        self.hit = np.stack([im["hit"] for im in images])
        self.t = np.stack([im["t"] for im in images])
        self.o = np.stack([im["o"] for im in images])
        self.d = np.stack([im["d"] for im in images])
        self.fragile = fragile

    @property
    def bytes(self):
        return to_bytes(self.colour)


def _counts(geoms, n_geoms):
    return [max(0, min(int(k), geoms.shape[1], MAX_GEOMS)) for k in n_geoms]


def render_ref(geoms, n_geoms, cams, width, height):
    """geoms [n, max_geoms, 16], n_geoms [n], cams [n, 13] -> Ref.  Image i draws its first min(n_geoms[i], max_geoms, 64) records."""
    geoms, cams = np.asarray(geoms, dtype=np.float64), np.asarray(cams, dtype=np.float64)
    images, fragile = [], []
    for i, ng in enumerate(_counts(geoms, n_geoms)):
        im = cast(geoms[i, :ng], cams[i], width, height)
        frag = np.abs(im["d"][..., 2] + 1e-6) < 1e-6
        for s in (1.0 + RADIUS_EPS, 1.0 - RADIUS_EPS):
            frag |= cast(geoms[i, :ng], cams[i], width, height, radius_scale=s)["hit"] != im["hit"]
        floor = np.zeros_like(frag)
        floor[im["hit"] >= 0] = geoms[i, im["hit"][im["hit"] >= 0], 0].astype(np.int64) == 0
        t = np.where(floor, im["t"], 0.0)
        x, y = im["o"][0] + t * im["d"][..., 0], im["o"][1] + t * im["d"][..., 1]
        e = FLOOR_EPS * (np.linalg.norm(im["o"]) + t)
        par = checker(x, y)
        for dx, dy in ((e, 0.0), (-e, 0.0), (0.0, e), (0.0, -e)):
            frag |= floor & (checker(x + dx, y + dy) != par)
        images.append(im)
        fragile.append(frag)
    return Ref(images, np.stack(fragile))


def render_mutant(geoms, n_geoms, cams, width, height, mutant):
    """The bytes of a deliberately wrong restatement (MUTANTS): what `compare` has to reject."""
    assert mutant in MUTANTS
    geoms, cams = np.asarray(geoms, dtype=np.float64), np.asarray(cams, dtype=np.float64)
    n = geoms.shape[0]
    return np.stack([to_bytes(cast(geoms[i, :ng], cams[(i + 1) % n if mutant == "next_camera" else i], width, height,
                                   mutant=mutant)["colour"]) for i, ng in enumerate(_counts(geoms, n_geoms))])


Verdict = collections.namedtuple("Verdict", "ok max_diff share fragile_share")


def compare(got_bytes, ref):
    """The bars on the non-fragile pixels of every image: the bytes differ from the reference's by at most MAX_LEVELS per channel,
    and at most MAX_SHARE of them differ at all.  Returns Verdict(ok, largest difference, largest share of differing pixels over the
    images, largest fragile share over the images)."""
    got, want = np.asarray(got_bytes), ref.bytes
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64)).max(-1)
    max_diff, share, frag = 0, 0.0, 0.0
    for i in range(diff.shape[0]):
        keep = ~ref.fragile[i]
        frag = max(frag, 1.0 - float(keep.mean()))
        if keep.any():
            max_diff = max(max_diff, int(diff[i][keep].max()))
            share = max(share, float((diff[i][keep] > 0).mean()))
    return Verdict(max_diff <= MAX_LEVELS and share <= MAX_SHARE, max_diff, share, frag)


# ------------------------------------------------------------------------------------------------------------------ scenes
def plane(z, rgb):
    rec = np.zeros(GEOM_FLOATS)
    rec[3], rec[6], rec[9:12] = z, 1.0, rgb
    return rec


def sphere(c, r, rgb, gtype=2):
    rec = np.zeros(GEOM_FLOATS)
    rec[0], rec[1:4], rec[6], rec[7], rec[9:12] = gtype, c, 1.0, r, rgb
    return rec


def capsule(c, axis, r, hl, rgb):
    rec = np.zeros(GEOM_FLOATS)
    axis = np.asarray(axis, dtype=np.float64)
    rec[0], rec[1:4], rec[4:7], rec[7], rec[8], rec[9:12] = 3, c, axis / np.linalg.norm(axis), r, hl, rgb
    return rec


def look_at(eye, target, fovy_deg=45.0, up_hint=(0.0, 0.0, 1.0)):
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up_hint)
    right /= np.linalg.norm(right)
    return np.concatenate([eye, fwd, right, np.cross(right, fwd), [np.tan(np.deg2rad(fovy_deg) / 2.0)]])


Scene = collections.namedtuple("Scene", "geoms n_geoms cams width height")
FLOOR, RED, GREEN, BLUE, OCHRE, FILLER = (0.75, 0.8, 0.7), (0.83, 0.31, 0.22), (0.27, 0.72, 0.33), (0.24, 0.41, 0.87), \
    (0.81, 0.66, 0.29), (0.93, 0.07, 0.91)


def pack(images, width, height, max_geoms=None, filler=False):
    """images: list of (records, camera) -> Scene of float32 / int32 arrays, as the kernel reads them.  With `filler` the records
    beyond each image's count hold a huge sphere right in front of that image's camera, which must not appear."""
    n = len(images)
    mg = max_geoms or max(1, max(len(r) for r, _ in images))
    geoms = np.zeros((n, mg, GEOM_FLOATS), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    cams = np.zeros((n, CAM_FLOATS), dtype=np.float32)
    for i, (recs, cam) in enumerate(images):
        cams[i] = cam
        if filler:
            geoms[i, :] = sphere(cam[0:3] + 2.0 * cam[3:6], 1.0, FILLER)
        if len(recs):
            geoms[i, :len(recs)] = np.asarray(recs)
        counts[i] = len(recs)
    return Scene(geoms, counts, cams, width, height)


def _capsule_views():
    eye = (0.0, 0.0, 1.2)
    cam = look_at(eye, (0.0, 4.0, 0.9))
    pitched = look_at((0.0, 0.0, 2.5), (0.0, 4.0, 1.5))
    near_axis = pitched[3:6] + 1e-3 * pitched[6:9]                      # 1e-3 rad off the view direction
    floor = plane(0.0, FLOOR)
    return pack([
        ([floor, capsule((0.0, 4.0, 1.0), (1.0, 0.0, 0.0), 0.3, 0.8, RED)], cam),                      # side on
        ([floor, capsule((0.2, 4.0, 1.2), (1.0, 1.0, 0.5), 0.3, 0.7, GREEN)], cam),                    # oblique
        ([floor, capsule((0.0, 4.0, 1.5), near_axis, 0.4, 0.7, BLUE)], pitched),                       # nearly parallel
        ([floor, capsule((0.0, 3.5, 1.0), (0.0, 0.0, 1.0), 0.5, 0.0, OCHRE)], cam),                    # hl = 0 with type 3: a sphere
        ([floor, capsule((0.0, 3.5, 1.0), (1.0, 0.0, 0.0), 0.5, 1e-3, RED)], cam),                     # hl much smaller than r
        ([floor, capsule((0.0, 3.5, 0.2), (0.3, 0.0, 1.0), 0.3, 0.8, GREEN)], cam),                    # piercing the floor
    ], 96, 64)


def _axis_parallel(width, height):
    """Looking straight down a vertical capsule centred on an odd-sized image: the central pixel's ray is exactly parallel to the
    axis.  Two images, so that the near cap is once the segment's end and once its start; the floor below has negative x and y."""
    eye = np.array([0.25, -0.3, 5.0])
    cam = look_at(eye, eye - [0.0, 0.0, 1.0], up_hint=(0.0, 1.0, 0.0))
    floor = plane(0.0, FLOOR)
    return pack([([floor, capsule((0.25, -0.3, 1.5), (0.0, 0.0, s), 0.5, 0.6, RED)], cam) for s in (1.0, -1.0)], width, height)


def _occlusion():
    cam = look_at((3.0, -3.0, 2.5), (0.0, 0.0, 0.5))                   # the floor around the origin: x and y of both signs
    floor = plane(0.0, FLOOR)
    up = look_at((0.0, 0.0, 0.5), (0.3, 2.0, 3.0))
    behind = look_at((0.13, 0.0, 1.07), (0.2, 4.0, 0.8), fovy_deg=50.0)
    return pack([
        ([floor, sphere((1.5, -1.3, 1.6), 0.3, BLUE), capsule((0.0, 0.0, 0.9), (1.0, 1.0, 0.2), 0.3, 0.9, RED),
          sphere((-1.4, 1.5, 0.8), 0.6, GREEN)], cam),                                                  # hidden by / hiding
        ([plane(0.7, FLOOR), sphere((0.0, 0.0, 0.9), 0.5, OCHRE)], cam),                                # plane at z != 0
        ([plane(-1.25, FLOOR), capsule((0.0, 0.0, 0.0), (1.0, -1.0, 0.0), 0.25, 0.6, BLUE)], cam),
        ([floor, sphere((0.3, 2.0, 3.0), 0.5, RED), capsule((-0.4, 2.2, 3.2), (1.0, 0.0, 1.0), 0.2, 0.5, GREEN)], up),   # no plane
        ([floor, capsule((0.1, -3.0, 1.1), (0.0, 1.0, 0.1), 0.4, 0.8, RED), sphere((0.13, -2.0, 1.1), 0.5, BLUE),
          sphere((0.3, 4.0, 1.0), 0.5, GREEN)], behind),                                                # behind the camera
        ([floor, sphere((3.2, -3.1, 2.4), 1.0, RED), capsule((3.0, -3.0, 2.0), (0.0, 0.0, 1.0), 0.6, 0.8, BLUE),
          capsule((0.0, 0.0, 0.8), (1.0, 1.0, 0.0), 0.3, 0.7, GREEN)], cam),                           # eye inside: not drawn
    ], 48, 40)


def _batch():
    """5 images in one call, counts 0, 1, 64, 3, 64 of max_geoms 64, a camera each; the records beyond a count hold the filler."""
    rng = np.random.RandomState(11)

    def crowd():
        recs = [plane(0.0, FLOOR)]
        for _ in range(62):
            c = rng.uniform([-2.0, 3.0, 0.2], [2.0, 7.0, 2.5])
            rgb = rng.uniform(0.2, 0.95, size=3)
            if rng.rand() < 0.5:
                recs.append(sphere(c, rng.uniform(0.12, 0.3), rgb))
            else:
                recs.append(capsule(c, rng.normal(size=3), rng.uniform(0.12, 0.3), rng.uniform(0.1, 0.5), rgb))
        recs.append(sphere((0.1, 2.2, 1.1), 0.3, OCHRE))                # the last record, near and in plain view
        return recs
    cams = [look_at((0.0, -1.0 - 0.3 * k, 1.3 + 0.2 * k), (0.2 * k - 0.4, 5.0, 1.0)) for k in range(5)]
    few = [plane(0.0, FLOOR), sphere((0.4, 4.0, 1.0), 0.5, BLUE), capsule((-0.5, 3.5, 0.9), (1.0, 0.2, 0.6), 0.25, 0.6, RED)]
    return pack([([], cams[0]), ([plane(0.0, FLOOR)], cams[1]), (crowd(), cams[2]), (few, cams[3]), (crowd(), cams[4])],
                96, 64, max_geoms=64, filler=True)


REAL = ("3d_cheetah_14_full", "3d_humanoid_9_full", "3d_hopper_3_shin")


def _real():
    """render.scene_of of three shipped morphologies at qpos0 and at one tilted root pose."""
    from sgrl_amd import mjcf, render
    images = []
    for name in REAL:
        m = mjcf.load_asset(name)
        tilted = np.array(m.qpos0, dtype=np.float64)
        half = 0.5 * 0.6                                                # 0.6 rad about a skew axis, lifted clear of the floor
        tilted[2] += 0.3
        tilted[3:7] = np.concatenate([[np.cos(half)], np.sin(half) * np.array([0.6, 0.64, 0.48])])
        for qpos in (m.qpos0, tilted):
            recs, cam = render.scene_of(m, qpos)
            images.append((list(recs), cam))
    return pack(images, 64, 48)


SCENES = {
    "capsule_views": _capsule_views,
    "axis_parallel_1x1": lambda: _axis_parallel(1, 1),
    "axis_parallel_17x33": lambda: _axis_parallel(17, 33),
    "axis_parallel_33x17": lambda: _axis_parallel(33, 17),
    "occlusion": _occlusion,
    "batch": _batch,
    "real": _real,
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """(Scene, Ref) of a named scene: computed once, shared by the tests, never written to."""
    s = SCENES[name]()
    ref = render_ref(s.geoms, s.n_geoms, s.cams, s.width, s.height)
    for a in (s.geoms, s.n_geoms, s.cams, ref.colour, ref.hit, ref.fragile, ref.t, ref.o, ref.d):
        a.setflags(write=False)
    return s, ref


def bounded_counts():
    """max_geoms = 4: image 0 claims 9 records, image 1 holds a distinctive sphere that image 0's camera would see, and a third
    image's worth of zero records pads the buffer so that 9 records from image 0's start stay inside it."""
    cam = look_at((0.0, 0.0, 1.2), (0.0, 4.0, 0.9))
    first = [plane(0.0, FLOOR), sphere((-0.8, 4.0, 0.9), 0.4, BLUE), capsule((0.6, 4.0, 0.8), (0.2, 0.0, 1.0), 0.25, 0.5, RED),
             sphere((0.0, 6.0, 1.5), 0.5, GREEN)]
    second = [sphere((0.0, 2.5, 1.2), 0.6, FILLER), plane(0.0, FLOOR), sphere((1.0, 3.0, 0.5), 0.3, OCHRE),
              sphere((-1.0, 3.0, 0.5), 0.3, OCHRE)]
    s = pack([(first, cam), (second, cam), ([], cam)], 48, 40, max_geoms=4)
    counts = s.n_geoms.copy()
    counts[0] = 9
    return s._replace(n_geoms=counts)
