// td3_loss.hip -- the two losses of a TD3 update and their gradients, for gfx950 (C ABI: include/sgrl_train.h; Python:
// train_ops.twin_mse / neg_mean; user: td3.Agent `loss_kernels`).
//
//   k_twin_mse_fwd   loss = (sum (q1 - t)^2 + sum (q2 - t)^2) / n        F.mse_loss(q1, t) + F.mse_loss(q2, t)
//   k_twin_mse_bwd   dq_k[i] = g 2 (q_k[i] - t[i]) / n
//   k_neg_mean_fwd   loss = -sum q / n                                  -q.mean()
//   k_neg_mean_bwd   dq[i] = -g / n
// n is a few thousand at training shapes (batch x limbs): what these calls cost is their launch, so each is ONE launch.  The
// forward reductions are ONE workgroup of 256 threads: thread t sums the elements i = t, t + 256, ... in ascending order in float64,
// the 256 partial sums meet in a fixed-shape tree in LDS (128, 64, ..., 1 pairs) -- no atomics, no second launch, and the same
// input gives the same bits.  The backward kernels are element-wise over a capped grid (a grid-stride loop, 64-bit indices) and
// read the upstream gradient g from DEVICE memory: the host never sees it, so the calls can be recorded into a hipGraph.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sgrl.h"
#include "../../include/sgrl_train.h"
#include "train_internal.h"

namespace {

using sgrl_train_detail::fail;
using sgrl_train_detail::launched;

constexpr int RT = 256;           // threads of the reduction workgroup
constexpr int ET = 256;           // threads per workgroup of the element-wise kernels
constexpr int64_t EG = 256;       // their grid cap: beyond 65 536 elements every thread loops

// the sum over the workgroup of one double per thread: lds[t] += lds[t + s] for s = 128, 64, ..., 1; the total is lds[0]
__device__ __forceinline__ void tree_sum(double* lds, int t) {
#pragma unroll
  for (int s = RT / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (t < s) lds[t] += lds[t + s];
  }
  __syncthreads();
}

__global__ __launch_bounds__(RT) void k_twin_mse_fwd(const float* __restrict__ q1, const float* __restrict__ q2,
                                                     const float* __restrict__ tg, int64_t n, float* __restrict__ loss) {
  __shared__ double s1[RT], s2[RT];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int64_t i = t; i < n; i += RT) {
    const double y = (double)tg[i];
    const double d1 = (double)q1[i] - y, d2 = (double)q2[i] - y;
    a += d1 * d1;
    b += d2 * d2;
  }
  s1[t] = a;
  s2[t] = b;
  tree_sum(s1, t);
  tree_sum(s2, t);
  if (t == 0) loss[0] = (float)((s1[0] + s2[0]) / (double)n);
}

__global__ __launch_bounds__(ET) void k_twin_mse_bwd(const float* __restrict__ q1, const float* __restrict__ q2,
                                                     const float* __restrict__ tg, int64_t n, const float* __restrict__ g,
                                                     float* __restrict__ dq1, float* __restrict__ dq2) {
  const double up = (double)g[0], dn = (double)n;
  const int64_t step = (int64_t)gridDim.x * ET;
  for (int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x; i < n; i += step) {
    const double y = (double)tg[i];
    dq1[i] = (float)(up * (2.0 * ((double)q1[i] - y)) / dn);
    dq2[i] = (float)(up * (2.0 * ((double)q2[i] - y)) / dn);
  }
}

__global__ __launch_bounds__(RT) void k_neg_mean_fwd(const float* __restrict__ q, int64_t n, float* __restrict__ loss) {
  __shared__ double s[RT];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int64_t i = t; i < n; i += RT) a += (double)q[i];
  s[t] = a;
  tree_sum(s, t);
  if (t == 0) loss[0] = (float)(-s[0] / (double)n);
}

__global__ __launch_bounds__(ET) void k_neg_mean_bwd(int64_t n, const float* __restrict__ g, float* __restrict__ dq) {
  const float v = (float)(-(double)g[0] / (double)n);
  const int64_t step = (int64_t)gridDim.x * ET;
  for (int64_t i = (int64_t)blockIdx.x * ET + threadIdx.x; i < n; i += step) dq[i] = v;
}

unsigned elem_blocks(int64_t n) {
  const int64_t b = (n + ET - 1) / ET;
  return (unsigned)(b < EG ? b : EG);
}

// [a, a + n) and [b, b + n) floats share an element
bool overlap(const float* a, const float* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  return x < y ? y - x < bytes : x - y < bytes;
}

}  // namespace

extern "C" {

int sgrl_td3_twin_mse_forward(const float* q1, const float* q2, const float* target, int64_t n, float* loss, void* stream) {
  if (!q1 || !q2 || !target || !loss) return fail(SGRL_ERR_ARG, "sgrl_td3_twin_mse_forward: null pointer");
  if (n <= 0) return fail(SGRL_ERR_ARG, "sgrl_td3_twin_mse_forward: n <= 0");
  if (overlap(q1, target, n) || overlap(q2, target, n)) return fail(SGRL_ERR_ARG, "sgrl_td3_twin_mse_forward: q1 / q2 alias target");
  hipLaunchKernelGGL(k_twin_mse_fwd, dim3(1), dim3(RT), 0, (hipStream_t)stream, q1, q2, target, n, loss);
  { int lrc = SGRL_OK; if (!launched("k_twin_mse_fwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_td3_twin_mse_backward(const float* q1, const float* q2, const float* target, int64_t n, const float* g, float* dq1, float* dq2,
                               void* stream) {
  if (!q1 || !q2 || !target || !g || !dq1 || !dq2) return fail(SGRL_ERR_ARG, "sgrl_td3_twin_mse_backward: null pointer");
  if (n <= 0) return fail(SGRL_ERR_ARG, "sgrl_td3_twin_mse_backward: n <= 0");
  if (overlap(q1, target, n) || overlap(q2, target, n) || overlap(dq1, target, n) || overlap(dq2, target, n))
    return fail(SGRL_ERR_ARG, "sgrl_td3_twin_mse_backward: q1 / q2 / dq1 / dq2 alias target");
  hipLaunchKernelGGL(k_twin_mse_bwd, dim3(elem_blocks(n)), dim3(ET), 0, (hipStream_t)stream, q1, q2, target, n, g, dq1, dq2);
  { int lrc = SGRL_OK; if (!launched("k_twin_mse_bwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_td3_neg_mean_forward(const float* q, int64_t n, float* loss, void* stream) {
  if (!q || !loss) return fail(SGRL_ERR_ARG, "sgrl_td3_neg_mean_forward: null pointer");
  if (n <= 0) return fail(SGRL_ERR_ARG, "sgrl_td3_neg_mean_forward: n <= 0");
  hipLaunchKernelGGL(k_neg_mean_fwd, dim3(1), dim3(RT), 0, (hipStream_t)stream, q, n, loss);
  { int lrc = SGRL_OK; if (!launched("k_neg_mean_fwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_td3_neg_mean_backward(int64_t n, const float* g, float* dq, void* stream) {
  if (!g || !dq) return fail(SGRL_ERR_ARG, "sgrl_td3_neg_mean_backward: null pointer");
  if (n <= 0) return fail(SGRL_ERR_ARG, "sgrl_td3_neg_mean_backward: n <= 0");
  hipLaunchKernelGGL(k_neg_mean_bwd, dim3(elem_blocks(n)), dim3(ET), 0, (hipStream_t)stream, n, g, dq);
  { int lrc = SGRL_OK; if (!launched("k_neg_mean_bwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_td3_loss_launches(void) { return 1; }

}  // extern "C"
