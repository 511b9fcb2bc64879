// scene.hip -- state records -> render scenes on the device, ONE launch (C ABI: include/sgrl_render.h sgrl_scene).  gfx950 only.
//
// What it replaces: the host half of `SubprocVecEnv.get_images()` (reference src/subproc_vec_env.py:70-73) -- every worker hands its
// MuJoCo state to the renderer, whose tracking camera `viewer_setup` (<env>.py:166-170) sets up.  Here the state is the engine's
// record and the scene description is the geom / camera records of sgrl_render; `render.scene_of` (sgrl_amd/render.py) is the
// definition, restated below term for term in float64 with one rounding to float32 at the store.
//
// Launch geometry: one workgroup of 64 threads (one wavefront) per image.  Thread b walks body b's chain from the torso down
// (`body_path`, depth <= SGRL_MAXDEPTH) exactly as mjcf.kinematics_np composes it parent by parent, the poses go through LDS,
// thread g writes geom g's record (four 16-byte stores), thread 0 the camera and the count.  Plain loads and stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/sgrl.h"
#include "../../include/sgrl_model.h"
#include "../../include/sgrl_render.h"
#include "engine_view.h"

namespace {

constexpr int kThreads = 64;
constexpr int kMaxBodies = 64;      // sgrl_engine_create admits no more

struct SceneArgs {
  const sgrl_engine_dev::MorphDev* morphs;
  const int32_t* env_morph;
  const double* rec;
  const double* cam_dist;           // [n_morph]
  const int32_t* env_ids;           // [n_img]
  float* geoms;                     // [n_img][max_geoms][16]
  int32_t* n_geoms;                 // [n_img]
  float* cams;                      // [n_img][13]
  int n_env, stride, max_geoms;
  // the state-independent part of the camera record (host, float64): forward | right | up | tan(fovy / 2)
  double fwd[3], right[3], up[3], tan_half;
};

__device__ __forceinline__ void quat_mul(double* r, const double* a, const double* b) {
  const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  const double z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}

// mjcf.quat_to_mat, row major
__device__ __forceinline__ void quat_to_mat(double* m, const double* q) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}

__device__ __forceinline__ void mat_vec(double* r, const double* m, const double* v) {
  const double x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
  const double y = m[3] * v[0] + m[4] * v[1] + m[5] * v[2];
  const double z = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}

// mjcf.normalize_quat: q / |q|
__device__ __forceinline__ void quat_normalize(double* q) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

// mjcf.axisangle_to_quat
__device__ __forceinline__ void axisangle_to_quat(double* q, const double* axis, double angle) {
  const double n = sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
  if (angle == 0.0 || n < 1e-15) { q[0] = 1; q[1] = 0; q[2] = 0; q[3] = 0; return; }
  double s, c;
  sincos(0.5 * angle, &s, &c);
  q[0] = c; q[1] = axis[0] / n * s; q[2] = axis[1] / n * s; q[3] = axis[2] / n * s;
}

// render._PALETTE[body % 5] (float64 literals, rounded once to float32)
__device__ __forceinline__ void palette(int k, float* rgb) {
  double r, g, b;
  switch (k) {
    case 0: r = 0.8; g = 0.6; b = 0.4; break;
    case 1: r = 0.85; g = 0.45; b = 0.35; break;
    case 2: r = 0.4; g = 0.6; b = 0.85; break;
    case 3: r = 0.45; g = 0.75; b = 0.5; break;
    default: r = 0.8; g = 0.75; b = 0.4; break;
  }
  rgb[0] = (float)r; rgb[1] = (float)g; rgb[2] = (float)b;
}

__global__ __launch_bounds__(kThreads) void k_scene(SceneArgs a) {
  __shared__ double xpos[kMaxBodies * 3];
  __shared__ double xquat[kMaxBodies * 4];
  const int img = blockIdx.x, t = threadIdx.x;
  float4* const grec = reinterpret_cast<float4*>(a.geoms + (size_t)img * a.max_geoms * SGRL_RENDER_GEOM_FLOATS);
  float* const cam = a.cams + (size_t)img * SGRL_RENDER_CAM_FLOATS;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int env = __builtin_amdgcn_readfirstlane(a.env_ids[img]);
  if (env < 0 || env >= a.n_env) {                        // an id outside the engine: an empty scene, nothing read for it
    for (int g = t; g < a.max_geoms; g += kThreads)
      for (int k = 0; k < 4; k++) grec[4 * g + k] = zero4;
    if (t < SGRL_RENDER_CAM_FLOATS) cam[t] = 0.f;
    if (t == 0) a.n_geoms[img] = 0;
    return;
  }
  const int mi = __builtin_amdgcn_readfirstlane(a.env_morph[env]);
  const sgrl_engine_dev::MorphDev md = a.morphs[mi];
  int32_t hdr[SGRL_NHDR];
#pragma unroll
  for (int k = 0; k < SGRL_NHDR; k++) hdr[k] = __builtin_amdgcn_readfirstlane(md.ib[k]);   // wave-uniform: the view lives in scalar registers
  SgrlModelView m;
  sgrl_model_view_dims(hdr, md.ib, md.fb, md.ib, md.fb, &m);
  const int nbody = min(m.nbody, kMaxBodies);
  const double* const qpos = a.rec + (size_t)env * a.stride;

  // ---- body poses: mjcf.kinematics_np along the chain torso .. b ------------------------------------------------------------
  if (t < nbody) {
    double pos[3] = {0.0, 0.0, 0.0}, quat[4] = {1.0, 0.0, 0.0, 0.0};        // the world body
    const int depth = t == 0 ? 0 : min(m.body_depth[t], SGRL_MAXDEPTH);
    for (int lvl = 0; lvl < depth; lvl++) {
      const int c = m.body_path[8 * t + lvl];
      if (c < 1 || c >= nbody) break;
      const int j0 = m.body_jntadr[c], jn = m.body_jntnum[c];
      if (jn == 1 && m.jnt_type[j0] == SGRL_JNT_FREE) {
        const int qa = m.jnt_qposadr[j0];
        for (int k = 0; k < 3; k++) pos[k] = qpos[qa + k];
        for (int k = 0; k < 4; k++) quat[k] = qpos[qa + 3 + k];
      } else {
        double mat[9], bp[3], bq[4], v[3], qn[4];
        for (int k = 0; k < 3; k++) bp[k] = m.body_pos[3 * c + k];
        for (int k = 0; k < 4; k++) bq[k] = m.body_quat[4 * c + k];
        quat_to_mat(mat, quat);
        mat_vec(v, mat, bp);
        for (int k = 0; k < 3; k++) pos[k] += v[k];
        quat_mul(qn, quat, bq);
        for (int k = 0; k < 4; k++) quat[k] = qn[k];
        for (int j = j0; j < j0 + jn; j++) {
          double jp[3], ja[3], anchor[3], ql[4];
          for (int k = 0; k < 3; k++) { jp[k] = m.jnt_pos[3 * j + k]; ja[k] = m.jnt_axis[3 * j + k]; }
          quat_to_mat(mat, quat);
          mat_vec(v, mat, jp);
          for (int k = 0; k < 3; k++) anchor[k] = pos[k] + v[k];
          const int qa = m.jnt_qposadr[j];
          axisangle_to_quat(ql, ja, qpos[qa] - m.qpos0[qa]);
          quat_mul(qn, quat, ql);
          for (int k = 0; k < 4; k++) quat[k] = qn[k];
          quat_to_mat(mat, quat);
          mat_vec(v, mat, jp);
          for (int k = 0; k < 3; k++) pos[k] = anchor[k] - v[k];
        }
      }
      quat_normalize(quat);
    }
    for (int k = 0; k < 3; k++) xpos[3 * t + k] = pos[k];
    for (int k = 0; k < 4; k++) xquat[4 * t + k] = quat[k];
  }
  __syncthreads();

  // ---- geom records ---------------------------------------------------------------------------------------------------------------
  for (int g = t; g < a.max_geoms; g += kThreads) {
    if (g >= m.ngeom) {
      for (int k = 0; k < 4; k++) grec[4 * g + k] = zero4;
      continue;
    }
    const int b = min(max(m.geom_body[g], 0), nbody - 1), type = m.geom_type[g];
    double bq[4], rb[9], gp[3], gq[4], rg[9], v[3], axis[3];
    for (int k = 0; k < 4; k++) { bq[k] = xquat[4 * b + k]; gq[k] = m.geom_quat[4 * g + k]; }
    for (int k = 0; k < 3; k++) gp[k] = m.geom_pos[3 * g + k];
    quat_to_mat(rb, bq);
    mat_vec(v, rb, gp);
    quat_to_mat(rg, gq);
    const double col2[3] = {rg[2], rg[5], rg[8]};
    mat_vec(axis, rb, col2);
    float rgb[3];
    if (type == SGRL_GEOM_PLANE) { rgb[0] = (float)0.75; rgb[1] = (float)0.8; rgb[2] = (float)0.7; }
    else palette(b % 5, rgb);
    const double radius = type == SGRL_GEOM_PLANE ? 0.0 : m.geom_size[3 * g];
    const double half = type == SGRL_GEOM_CAPSULE ? m.geom_size[3 * g + 1] : 0.0;
    grec[4 * g + 0] = make_float4((float)type, (float)(xpos[3 * b] + v[0]), (float)(xpos[3 * b + 1] + v[1]), (float)(xpos[3 * b + 2] + v[2]));
    grec[4 * g + 1] = make_float4((float)axis[0], (float)axis[1], (float)axis[2], (float)radius);
    grec[4 * g + 2] = make_float4((float)half, rgb[0], rgb[1], rgb[2]);
    grec[4 * g + 3] = zero4;
  }

  // ---- camera: viewer_setup on the tracking camera ------------------------------------------------------------------------------
  if (t == 0) {
    const int track = min(2, nbody - 1);
    const double dist = a.cam_dist[mi];
    const double lookat[3] = {xpos[3 * track], xpos[3 * track + 1], 1.15};
    for (int k = 0; k < 3; k++) {
      cam[k] = (float)(lookat[k] - dist * a.fwd[k]);
      cam[3 + k] = (float)a.fwd[k];
      cam[6 + k] = (float)a.right[k];
      cam[9 + k] = (float)a.up[k];
    }
    cam[12] = (float)a.tan_half;
    a.n_geoms[img] = m.ngeom;
  }
}

// elevation -20 degrees, azimuth 90 degrees, fovy 45 degrees: the lines of render.scene_of
void camera_frame(SceneArgs* a) {
  const double el = -20.0 * (M_PI / 180.0), az = 90.0 * (M_PI / 180.0);
  a->fwd[0] = std::cos(el) * std::cos(az); a->fwd[1] = std::cos(el) * std::sin(az); a->fwd[2] = std::sin(el);
  const double* f = a->fwd;
  double r[3] = {f[1] * 1.0 - f[2] * 0.0, f[2] * 0.0 - f[0] * 1.0, f[0] * 0.0 - f[1] * 0.0};      // fwd x (0, 0, 1)
  const double n = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (int k = 0; k < 3; k++) a->right[k] = r[k] / n;
  r[0] = a->right[0]; r[1] = a->right[1]; r[2] = a->right[2];
  a->up[0] = r[1] * f[2] - r[2] * f[1]; a->up[1] = r[2] * f[0] - r[0] * f[2]; a->up[2] = r[0] * f[1] - r[1] * f[0];   // right x fwd
  a->tan_half = std::tan(45.0 * (M_PI / 180.0) / 2);
}

}  // namespace

extern "C" {

int sgrl_max_geoms(const sgrl_engine* e) {
  sgrl_engine_view v;
  if (sgrl_engine_view_of(const_cast<sgrl_engine*>(e), &v) != SGRL_OK) return SGRL_ERR_ARG;
  return v.max_geoms;
}

int sgrl_scene_launches(void) { return 1; }

int sgrl_scene(sgrl_engine* e, const int32_t* env_ids, int n_img, const double* cam_dist, int max_geoms, float* geoms,
               int32_t* n_geoms, float* cams, void* stream) {
  sgrl_engine_view v;
  if (!e || !env_ids || !cam_dist || !geoms || !n_geoms || !cams || n_img <= 0) return SGRL_ERR_ARG;
  if (sgrl_engine_view_of(e, &v) != SGRL_OK || max_geoms < v.max_geoms) return SGRL_ERR_ARG;
  // the camera distances are constants of an environment object: they cross to the device when they change, i.e. once
  if (std::memcmp(v.cam_dist_host, cam_dist, sizeof(double) * v.n_morph) != 0) {
    std::memcpy(v.cam_dist_host, cam_dist, sizeof(double) * v.n_morph);
    if (hipMemcpyAsync(v.cam_dist_dev, v.cam_dist_host, sizeof(double) * v.n_morph, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) {
      for (int k = 0; k < v.n_morph; k++) v.cam_dist_host[k] = std::nan("");
      return SGRL_ERR_HIP;
    }
  }
  SceneArgs a;
  a.morphs = v.morphs; a.env_morph = v.env_morph; a.rec = v.rec; a.cam_dist = v.cam_dist_dev;
  a.env_ids = env_ids; a.geoms = geoms; a.n_geoms = n_geoms; a.cams = cams;
  a.n_env = v.n_env; a.stride = v.stride; a.max_geoms = max_geoms;
  camera_frame(&a);
  hipLaunchKernelGGL(k_scene, dim3(n_img), dim3(kThreads), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? SGRL_OK : SGRL_ERR_HIP;
}

}  // extern "C"
