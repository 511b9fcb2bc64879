/* sgrl_render.h -- C ABI of the off-screen renderer behind BatchedModularVecEnv.get_images() (gfx950).
 *
 * What it replaces: `SubprocVecEnv.get_images()` (reference src/subproc_vec_env.py:70-73), i.e. every worker's
 * `env.render(mode='rgb_array')` = MuJoCo's OpenGL off-screen renderer through gym 0.17.2 / mujoco-py (third-party, absent here).
 * This is a ray caster over the same scene description (ground plane, spheres, capsules at the bodies' world poses) with the
 * reference's camera set-up (`viewer_setup`, <env>.py:166-170: tracked body, distance, look-at height, elevation -20 deg).
 * PIXEL PARITY WITH MuJoCo's RASTERISER IS NEITHER CLAIMED NOR PINNED: it is a visualisation aid.  What IS held is parity with the
 * renderer's own definition: tests/render_restate.py restates it in float64 NumPy (a capsule as the union of a cylinder and two
 * spheres), tests/test_render_restate.py qualifies that restatement without a GPU (signed distances at the hit points, mutants that
 * the comparison must reject), and tests/test_render_gpu.py holds the kernel's bytes to it within one level per channel on every
 * pixel whose float64 answer is stable under float32-sized perturbation.
 *
 * The definition: the ray through the pixel centre; the nearest hit over the image's geoms (t > 1e-4 for spheres and capsules, t > 0
 * for the plane, which is tested only where the ray's d.z < -1e-6; entry points only, so a geom that contains the eye is not drawn);
 * colour * (0.35 + 0.45 max(-n.d, 0) + 0.2 max(n.z, 0)), the plane's colour times 0.9 / 0.6 by the parity of floor(x) + floor(y) of
 * the hit point; sky (0.55, 0.7, 0.9) unshaded; byte = floor(clip(c * 255 + 0.5, 0, 255)).
 *
 * One image = one camera + a list of geoms in world coordinates.  All pointers are DEVICE pointers owned by the caller.
 */
#ifndef SGRL_RENDER_H
#define SGRL_RENDER_H

#include <stdint.h>

#include "sgrl.h"   /* sgrl_engine */

#ifdef __cplusplus
extern "C" {
#endif

/* geom record, 16 floats: type (0 horizontal plane with a checker pattern, at its record's centre z; 2 sphere; 3 capsule, drawn as
 * a sphere when its half length is 0) | centre xyz | unit axis xyz (capsule) | radius | half length | rgb | 3 unused */
#define SGRL_RENDER_GEOM_FLOATS 16
/* camera record, 13 floats: eye xyz | forward xyz | right xyz | up xyz | tan(fovy / 2) */
#define SGRL_RENDER_CAM_FLOATS 13

/* rgb[n_img][height][width][3] (uint8).  geoms[n_img][max_geoms][16], n_geoms[n_img], cams[n_img][13].  Image i draws its first
 * min(n_geoms[i], max_geoms) records: the counts live on the device, where the entry point cannot look at them, so a count above
 * max_geoms is bounded by the kernel and never reaches the next image's records.  SGRL_ERR_ARG (nothing launched) for a null
 * pointer, n_img, width or height <= 0, max_geoms <= 0 or max_geoms > 64. */
int sgrl_render(const float* geoms, const int32_t* n_geoms, int max_geoms, const float* cams, int n_img, int width, int height,
                uint8_t* rgb, void* stream);

/* ---- scene assembly on the device -------------------------------------------------------------------------------------------
 * What it replaces: the state hand-over of `SubprocVecEnv.get_images()` (reference src/subproc_vec_env.py:70-73: every worker
 * renders its own MuJoCo state) and the tracking camera of `viewer_setup` (<env>.py:166-170).  sgrl_scene turns the engine's state
 * records into the geom / camera records above without leaving the device: forward kinematics of the requested environments from
 * the qpos in their records and the geoms of their morphology blobs, ONE launch, one 64-thread workgroup per image.  Its definition
 * is `render.scene_of` (sgrl_amd/render.py): float64 arithmetic, one rounding to float32 at the store.  Geom records g >= ngeom of
 * an image are written as zeros.  An id outside [0, n_env) gives an empty scene (n_geoms = 0, zero records) and reads nothing: the
 * ids live on the device, so the caller validates them before the upload. */
int sgrl_max_geoms(const sgrl_engine* e);     /* largest ngeom over the engine's morphologies */
int sgrl_scene_launches(void);                /* kernel launches per sgrl_scene call: 1 */
/* env_ids DEV int32[n_img]; cam_dist HOST double[n_morph]: camera distance per morphology (0.5 * model extent * 2.2, a constant of
 * the environment object; float64 because the eye is computed in float64 and rounded once); it is uploaded when it differs from
 * the previous call's, in stream order.  geoms DEV float[n_img][max_geoms][16]; n_geoms DEV int32[n_img]; cams DEV float[n_img][13].
 * SGRL_ERR_ARG (nothing launched) for a null pointer, n_img <= 0 or max_geoms < sgrl_max_geoms(e). */
int sgrl_scene(sgrl_engine* e, const int32_t* env_ids, int n_img, const double* cam_dist, int max_geoms, float* geoms,
               int32_t* n_geoms, float* cams, void* stream);

#ifdef __cplusplus
}
#endif
#endif
