"""Off-screen rendering for `BatchedModularVecEnv.get_images()` (reference src/subproc_vec_env.py:70-73 -> every worker's
`env.render(mode='rgb_array')`, MuJoCo's OpenGL renderer through gym / mujoco-py: third-party, absent here).

A ray caster (csrc/render.hip, C ABI include/sgrl_render.h) over the morphology's own geoms -- ground plane, spheres,
capsules at the bodies' world poses -- seen through the reference's camera (`viewer_setup`, <env>.py:166-170: track body 2,
distance = half the model extent, look-at height 1.15, elevation -20 degrees; MuJoCo's default azimuth 90 and fovy 45).
Pixel parity with MuJoCo's rasteriser is neither claimed nor pinned: it shows what the engine simulates.  The scene
(forward kinematics of the requested environments) is assembled on the host from the engine's state records: this is a
visualisation path, not part of the rollout.

`device_scenes` / `render_device` are the same two stages without the host: the scenes of any number of environments come from ONE
launch over the engine's records where they lie (csrc/scene.hip, `sgrl_scene` of include/sgrl_render.h: `scene_of` restated on the
device), and the ray caster reads them there.  This is what the policy video demo (evaluate.VideoDemo) renders its frames with.
"""
import ctypes

import numpy as np
import torch

from . import _lib, mjcf

GEOM_FLOATS, CAM_FLOATS = 16, 13
_PALETTE = np.array([[0.8, 0.6, 0.4], [0.85, 0.45, 0.35], [0.4, 0.6, 0.85], [0.45, 0.75, 0.5], [0.8, 0.75, 0.4]])


def model_extent(m):
    """Radius-like size of the model at qpos0 (stand-in for MuJoCo's model.stat.extent): the largest distance between the
    bounding spheres of two of its non-plane geoms."""
    xpos, xquat, _, _ = mjcf.kinematics_np(m, m.qpos0)
    pts, rad = [], []
    for g in range(m.ngeom):
        if m.geom_type[g] == 0:
            continue
        b = m.geom_body[g]
        pts.append(xpos[b] + mjcf.quat_to_mat(xquat[b]) @ m.geom_pos[g])
        rad.append(m.geom_size[g][0] + (m.geom_size[g][1] if m.geom_type[g] == 3 else 0.0))
    pts, rad = np.array(pts), np.array(rad)
    d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + rad[:, None] + rad[None]
    return float(max(d.max(), 2 * rad.max()))


def scene_of(m, qpos):
    """(geom records [ngeom, 16], camera record [13]) of morphology `m` at configuration `qpos`."""
    xpos, xquat, _, _ = mjcf.kinematics_np(m, qpos)
    recs = np.zeros((m.ngeom, GEOM_FLOATS), dtype=np.float32)
    for g in range(m.ngeom):
        b = m.geom_body[g]
        rb = mjcf.quat_to_mat(xquat[b])
        pos = xpos[b] + rb @ m.geom_pos[g]
        axis = rb @ mjcf.quat_to_mat(m.geom_quat[g])[:, 2]
        t = int(m.geom_type[g])
        recs[g, 0] = t
        recs[g, 1:4] = pos
        recs[g, 4:7] = axis
        recs[g, 7] = 0.0 if t == 0 else m.geom_size[g][0]
        recs[g, 8] = m.geom_size[g][1] if t == 3 else 0.0
        recs[g, 9:12] = [0.75, 0.8, 0.7] if t == 0 else _PALETTE[b % len(_PALETTE)]
    # camera: reference viewer_setup (<env>.py:166-170) on MuJoCo's tracking camera (azimuth 90, fovy 45)
    track = min(2, m.nbody - 1)
    lookat = np.array([xpos[track][0], xpos[track][1], 1.15])
    dist, el, az = 0.5 * model_extent(m) * 2.2, np.deg2rad(-20.0), np.deg2rad(90.0)
    fwd = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    eye = lookat - dist * fwd
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    cam = np.concatenate([eye, fwd, right, up, [np.tan(np.deg2rad(45.0) / 2)]]).astype(np.float32)
    return recs, cam


def render(scenes, width=256, height=256, device="cuda:0"):
    """scenes: list of (geom records, camera record) -> uint8 [n, height, width, 3] (a CUDA tensor)."""
    if not torch.cuda.is_available():
        raise _lib.SgrlError("rendering needs an MI355X (no CPU fallback)")
    L = _lib.lib()
    L.sgrl_render.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                              ctypes.c_void_p, ctypes.c_void_p]
    n = len(scenes)
    mg = max(s[0].shape[0] for s in scenes)
    geoms = np.zeros((n, mg, GEOM_FLOATS), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    cams = np.zeros((n, CAM_FLOATS), dtype=np.float32)
    for i, (g, c) in enumerate(scenes):
        geoms[i, :g.shape[0]] = g
        counts[i] = g.shape[0]
        cams[i] = c
    dev = torch.device(device)
    gd, cd, kd = torch.from_numpy(geoms).to(dev), torch.from_numpy(cams).to(dev), torch.from_numpy(counts).to(dev)
    out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev)
    rc = L.sgrl_render(ctypes.c_void_p(gd.data_ptr()), ctypes.c_void_p(kd.data_ptr()), mg, ctypes.c_void_p(cd.data_ptr()), n, int(width),
                       int(height), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise _lib.SgrlError("sgrl_render failed (%d)" % rc)
    return out


def _bind(L):
    """The scene entry points of include/sgrl_render.h."""
    if getattr(L, "_scene_bound", False):
        return L
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.sgrl_max_geoms.argtypes = [vp]
    L.sgrl_max_geoms.restype = ci
    L.sgrl_scene_launches.argtypes = []
    L.sgrl_scene_launches.restype = ci
    L.sgrl_scene.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp]
    L.sgrl_scene.restype = ci
    L.sgrl_render.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp]
    L.sgrl_render.restype = ci
    L._scene_bound = True
    return L


def camera_distances(env):
    """float64 [n_morph]: the camera distance of `scene_of` per morphology of `env` (a host constant: computed once per
    environment object)."""
    d = getattr(env, "_cam_dist", None)
    if d is None:
        d = env._cam_dist = np.ascontiguousarray([0.5 * model_extent(m) * 2.2 for m in env.models], dtype=np.float64)
    return d


def _device_ids(env, env_ids):
    """int32 device tensor of the requested environment ids, validated on the host (the library cannot look at them without a
    synchronisation); the upload of the list used last is kept, so that a frame loop over the same environments uploads once."""
    ids = np.arange(env.num_envs, dtype=np.int64) if env_ids is None else np.asarray(
        env_ids.detach().cpu().numpy() if torch.is_tensor(env_ids) else env_ids)
    if ids.ndim != 1 or ids.size == 0 or ids.dtype.kind not in "iu":
        raise ValueError("env_ids must be a non-empty 1-d list of integers")
    if ids.min() < 0 or ids.max() >= env.num_envs:
        raise ValueError("env_ids must lie in 0 .. %d (num_envs - 1), got %d .. %d" % (env.num_envs - 1, ids.min(), ids.max()))
    key = ids.astype(np.int32).tobytes()
    cached = getattr(env, "_scene_ids", None)
    if cached is None or cached[0] != key:
        cached = env._scene_ids = (key, torch.from_numpy(ids.astype(np.int32)).to(env.device))
    return cached[1]


def device_scenes(env, env_ids=None):
    """The scenes of environments `env_ids` (default: all) of a BatchedModularVecEnv as device tensors
    (geoms float32 [n, max_geoms, 16], n_geoms int32 [n], cams float32 [n, 13]): `scene_of` of every requested environment's
    current qpos in one launch, nothing copied to the host."""
    L = _bind(_lib.lib())
    ids = _device_ids(env, env_ids)
    n, mg = int(ids.numel()), int(L.sgrl_max_geoms(env._h))
    dev = env.device
    geoms = torch.empty((n, mg, GEOM_FLOATS), dtype=torch.float32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    cams = torch.empty((n, CAM_FLOATS), dtype=torch.float32, device=dev)
    dist = camera_distances(env)
    rc = L.sgrl_scene(env._h, ctypes.c_void_p(ids.data_ptr()), n, ctypes.c_void_p(dist.ctypes.data), mg, ctypes.c_void_p(geoms.data_ptr()),
                      ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(cams.data_ptr()),
                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise _lib.SgrlError("sgrl_scene failed (%d)" % rc)
    return geoms, counts, cams


def render_device(geoms, n_geoms, cams, width=256, height=256, out=None):
    """`sgrl_render` on scenes that are already on the device (device_scenes) -> uint8 [n, height, width, 3] on the same device,
    written into `out` when given."""
    L = _bind(_lib.lib())
    dev, n = geoms.device, int(geoms.shape[0])
    if dev.type != "cuda":
        raise _lib.SgrlError("rendering needs an MI355X (no CPU fallback)")
    for t, dtype, shape in ((geoms, torch.float32, (n, geoms.shape[1], GEOM_FLOATS)), (n_geoms, torch.int32, (n,)),
                            (cams, torch.float32, (n, CAM_FLOATS))):
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
            raise _lib.SgrlError("render_device: scenes must be the contiguous tensors of device_scenes on one device")
    shape = (n, int(height), int(width), 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != dev or not out.is_contiguous():
        raise _lib.SgrlError("render_device: out must be a contiguous uint8 tensor of shape %s on %s" % (shape, dev))
    rc = L.sgrl_render(ctypes.c_void_p(geoms.data_ptr()), ctypes.c_void_p(n_geoms.data_ptr()), int(geoms.shape[1]),
                       ctypes.c_void_p(cams.data_ptr()), n, int(width), int(height), ctypes.c_void_p(out.data_ptr()),
                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise _lib.SgrlError("sgrl_render failed (%d)" % rc)
    return out
