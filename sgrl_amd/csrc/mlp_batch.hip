// mlp_batch.hip -- the batch prologue of the MLP agent's TD3 update (C ABI: include/sgrl_mlp.h, "batch prologue"): the reward scaling
// and the two train_reward statistics (reference src/agent.py:124, 160-161) in ONE launch of ONE workgroup, so that an update is this
// library's launches from its first to its last and a hipGraph of it holds kernel nodes only.
//
//   k_mlp_batch_stats   out[i] = reward[i] * scale;  stats[0] = mean(out);  stats[1] = sum((out - mean)^2) / (n - 1)
//
// Two passes, as torch.var: the mean first, then the squared deviations from it.  A thread reads in the second pass exactly the
// elements of `out` it wrote in the first (program order within a thread: no fence needed), which is what makes out == reward legal.
//
// ORDER OF THE SUMS (fixed, so a call is bit-repeatable; no atomics, no scratch), that of mlp_optim.hip's apply launch.  Thread t of
// 256 adds elements t, t + 256, t + 512, ... serially (ceil(n / 256) additions from 0); a wave adds its 64 lanes by a butterfly (xor
// 32, 16, 8, 4, 2, 1: 6 additions); the four waves' sums are added in wave order ((w0 + w1) + w2) + w3 (3 additions).  The longest
// chain of float additions into either sum is 9 + ceil(n / 256): 10 at the trainer's 256 rows, 65 545 at the largest n served.
// Every product, sum and quotient is ONE correctly rounded float32 operation (no fused multiply-add), so tests/mlp_batch_restate.py
// restates the bits in NumPy.  n = 1: 0 / 0, NaN, as torch.var gives.
#include "mlp_internal.h"

#include <cmath>

using namespace sgrl_mlp_detail;

// Left alone the compiler contracts s + r * scale and q + d * d into fused multiply-adds (one rounding instead of two: another last
// bit now and then; the *_rn intrinsics do not help, they are plain operators compiled under the headers' own setting).  Contraction
// is off for the arithmetic written in this file; the division stays the correctly rounded one.
#pragma clang fp contract(off)

namespace {

constexpr int kMaxN = 1 << 24;          // every count up to here is a float32

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// the sum over the workgroup's 256 threads, in every thread: butterfly per wave, then the four waves in order
__device__ __forceinline__ float group_sum(float s, float* red) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_mlp_batch_stats(const float* reward, int n, float scale, float* out, float* stats) {
  __shared__ float red[2][4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float x = reward[i] * scale;
    out[i] = x;
    s = s + x;
  }
  const float mean = group_sum(s, red[0]) / (float)n;
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = out[i] - mean;
    q = q + d * d;
  }
  const float var = group_sum(q, red[1]) / (float)(n - 1);
  if (threadIdx.x == 0) {
    stats[0] = mean;
    stats[1] = var;
  }
}

}  // namespace

extern "C" {

int sgrl_mlp_batch_stats_launches(void) { return 1; }

int sgrl_mlp_batch_stats(const float* reward, int n, float reward_scale, float* reward_out, float* stats, void* stream) {
  const char* who = "sgrl_mlp_batch_stats";
  if (!reward || !reward_out || !stats) return mfail(SGRL_ERR_ARG, std::string(who) + ": null argument");
  if (n < 1 || n > kMaxN) return mfail(SGRL_ERR_ARG, std::string(who) + ": n outside 1 .. 2^24, got " + std::to_string(n));
  if (!std::isfinite(reward_scale)) return mfail(SGRL_ERR_ARG, std::string(who) + ": reward_scale is not finite");
  const void* ptrs[3] = {reward, reward_out, stats};
  const int rc = check_addresses(ptrs, 3, who, "address");
  if (rc != SGRL_OK) return rc;
  hipLaunchKernelGGL(k_mlp_batch_stats, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), reward, n, reward_scale, reward_out, stats);
  return launched("k_mlp_batch_stats");
}

}  // extern "C"
