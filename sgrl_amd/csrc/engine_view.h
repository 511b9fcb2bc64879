// engine_view.h -- what a translation unit other than engine.hip may see of an engine handle (the struct itself stays private to
// engine.hip): where the morphology blobs and the state records lie on the device.  Used by scene.hip, which reads an
// environment's qpos from its record where it lies.
#pragma once
#include <stdint.h>

struct sgrl_engine;

namespace sgrl_engine_dev {

struct MorphDev {
  const int32_t* ib;
  const double* fb;
  int32_t slot;      // which instance of its family's fixed-dimension kernel serves this morphology (-1: generic kernel only)
  int32_t pad_;
};

}  // namespace sgrl_engine_dev

struct sgrl_engine_view {
  const sgrl_engine_dev::MorphDev* morphs;   // DEV [n_morph]
  const int32_t* env_morph;                  // DEV [n_env]
  const double* rec;                         // DEV [n_env * stride]: qpos[nq] | qvel[nv] | torso_xy_stale[2] | target[2]
  int n_morph, n_env, stride;
  int max_geoms;                             // largest ngeom over the morphologies
  double* cam_dist_dev;                      // DEV [n_morph], owned by the engine: the camera distances of the last sgrl_scene ...
  double* cam_dist_host;                     // ... and the host copy they were uploaded from [n_morph] (NaN until the first call)
};

// 0, or SGRL_ERR_ARG for a null argument (defined in engine.hip)
int sgrl_engine_view_of(sgrl_engine* e, sgrl_engine_view* v);
