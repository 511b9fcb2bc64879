// dropout.hip -- counter-RNG dropout of the SWAT networks' differentiable passes, for gfx950 (C ABI: include/sgrl_train.h; Python:
// train_ops.dropout; user: swat_policy with dropout_rate > 0).
//
//   k_dropout   y[i] = keep(i) ? x[i] * scale : 0,   keep(i) = word(seed, step, 0x100 + site, i) >= thr
// The mask is a FUNCTION of (seed, step, site, i) -- Philox4x32-10 as the replay draw uses it (replay_rng.h) -- so nothing is stored
// between the passes: the backward is the same kernel applied to dy with the forward's (step, site).  `step` is read from DEVICE
// memory: the host never has to know it.  One thread per four consecutive elements: ONE Philox block serves the quad, which moves
// as one 16-byte load and one 16-byte store when both base pointers are 16-byte aligned and as four scalar accesses otherwise;
// the last, partial quad is always scalar.  A capped grid with a grid-stride loop over 64-bit quad numbers; every element is
// written exactly once: the same input gives the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/sgrl.h"
#include "../../include/sgrl_train.h"
#include "dropout_rng.h"
#include "train_internal.h"

namespace {

using sgrl_train_detail::fail;
using sgrl_train_detail::launched;

constexpr int DT = 256;           // threads per workgroup
constexpr int64_t DG = 4096;      // grid cap: beyond 4 Mi elements every thread loops

__global__ __launch_bounds__(DT) void k_dropout(const float* __restrict__ x, float* __restrict__ y, int64_t n, uint64_t thr, float scale,
                                                uint64_t seed, const uint64_t* __restrict__ step_dev, uint32_t stream_id, int vec) {
  const uint64_t step = step_dev[0];
  const int64_t quads = (n + 3) >> 2, stride = (int64_t)gridDim.x * DT;
  for (int64_t q = (int64_t)blockIdx.x * DT + threadIdx.x; q < quads; q += stride) {
    const int64_t i0 = q << 2;
    if (vec && i0 + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(x + i0);
      const sgrl_replay::Words4 o = sgrl_replay::replay_block(seed, step, stream_id, (uint32_t)q);
      float4 r;
      r.x = sgrl_dropout::apply(v.x, o.w[0], thr, scale);
      r.y = sgrl_dropout::apply(v.y, o.w[1], thr, scale);
      r.z = sgrl_dropout::apply(v.z, o.w[2], thr, scale);
      r.w = sgrl_dropout::apply(v.w, o.w[3], thr, scale);
      *reinterpret_cast<float4*>(y + i0) = r;
    } else {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = i0 + u < n ? x[i0 + u] : 0.f;
      const sgrl_replay::Words4 o = sgrl_replay::replay_block(seed, step, stream_id, (uint32_t)q);
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (i0 + u < n) y[i0 + u] = sgrl_dropout::apply(v[u], o.w[u], thr, scale);
    }
  }
}

int run(const char* name, const float* x, float* y, int64_t n, float p, uint64_t seed, const uint64_t* step_dev, int site, void* stream) {
  if (!x || !y || !step_dev) return fail(SGRL_ERR_ARG, std::string(name) + ": null pointer");
  if (n <= 0) return fail(SGRL_ERR_ARG, std::string(name) + ": n <= 0");
  {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y, bytes = (uintptr_t)n * sizeof(float);
    if (a < b ? b - a < bytes : a - b < bytes) return fail(SGRL_ERR_ARG, std::string(name) + ": input and output overlap (out of place only)");
  }
  if (!sgrl_dropout::valid(p, site)) return fail(SGRL_ERR_ARG, std::string(name) + ": p outside [0, 1] or site outside 0 .. 2^24 - 1");
  const int64_t quads = (n + 3) >> 2, blocks = (quads + DT - 1) / DT;
  const int vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0 ? 1 : 0;
  hipLaunchKernelGGL(k_dropout, dim3((unsigned)(blocks < DG ? blocks : DG)), dim3(DT), 0, (hipStream_t)stream, x, y, n,
                     sgrl_dropout::threshold(p), sgrl_dropout::scale(p), seed, step_dev, sgrl_dropout::stream_of(site), vec);
  { int lrc = SGRL_OK; if (!launched("k_dropout launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

}  // namespace

extern "C" {

int sgrl_dropout_forward(const float* x, float* y, int64_t n, float p, uint64_t seed, const uint64_t* step_dev, int site, void* stream) {
  return run("sgrl_dropout_forward", x, y, n, p, seed, step_dev, site, stream);
}

int sgrl_dropout_backward(const float* dy, float* dx, int64_t n, float p, uint64_t seed, const uint64_t* step_dev, int site, void* stream) {
  return run("sgrl_dropout_backward", dy, dx, n, p, seed, step_dev, site, stream);
}

}  // extern "C"
