// explore_actions.hip -- the behaviour policy's action choice (include/sgrl_explore.h): exploration noise on the actor's output, or
// the warm-up's uniform actions, clamped and zero-padded, in ONE launch.  gfx950 only.
//
// Launch geometry: kThreads = 256 threads per workgroup, one thread per element, whole rows per workgroup: 256 / act_max rows
// (six at act_max = 42; a row wider than 256 slots is one workgroup's, its threads striding over it), so a thread finds its row and
// slot with one 32-bit division of its own number.  Every thread computes the Philox block of its element and takes its half of it,
// as the replay's noise does (replay_sample.hip): the ten integer rounds are small beside the float64 log and cos that follow, and
// sharing a block between the two threads that own its halves would tie the lane pairing to the parity of env_id_base * act_max.
// No LDS, no atomics; an element is read and written by the same thread, so `out` may be `policy_act`.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sgrl.h"
#include "../../include/sgrl_explore.h"
#include "replay_rng.h"

namespace {

thread_local std::string g_explore_err;

int fail(int code, const std::string& msg) {
  g_explore_err = msg;
  return code;
}

constexpr int kThreads = 256;
constexpr uint32_t kStreamGauss = 2u, kStreamUniform = 3u;      // 0 and 1 are the replay's (sgrl_replay.h)

struct ExploreArgs {
  const float* policy_act;
  float* out;
  const int32_t* act_len;
  int ld_in, ld_out, n_env, act_max, rows_per_group, mode;
  uint64_t env_id_base, seed, step;
  float std, lo, hi;
};

__global__ __launch_bounds__(kThreads) void k_explore_actions(ExploreArgs a) {
  const int r = (int)threadIdx.x / a.act_max;
  if (r >= a.rows_per_group) return;
  const int64_t i = (int64_t)blockIdx.x * a.rows_per_group + r;      // local row
  if (i >= (int64_t)a.n_env) return;
  const int live = a.act_len[i];
  const uint32_t tag = a.mode == SGRL_EXPLORE_UNIFORM ? kStreamUniform : kStreamGauss;
  for (int c = (int)threadIdx.x - r * a.act_max; c < a.act_max; c += kThreads) {
    float v = 0.0f;                                                  // the padding slots
    if (c < live) {
      const uint64_t e = (a.env_id_base + (uint64_t)i) * (uint64_t)a.act_max + (uint64_t)c;      // words 2 e and 2 e + 1: one half of block e >> 1
      const sgrl_replay::Words4 o = sgrl_replay::replay_block(a.seed, a.step, tag, (uint32_t)(e >> 1));
      const uint32_t x1 = (e & 1u) ? o.w[2] : o.w[0], x2 = (e & 1u) ? o.w[3] : o.w[1];
      const double u1 = ((double)x1 + 0.5) * (1.0 / 4294967296.0);
      // __fmul_rn / __fadd_rn: every operation rounds to float32 by itself (no fused multiply-add), as the definition says
      if (a.mode == SGRL_EXPLORE_UNIFORM) {
        v = __fadd_rn(a.lo, __fmul_rn(a.hi - a.lo, (float)u1));
      } else {
        const double u2 = ((double)x2 + 0.5) * (1.0 / 4294967296.0);
        const double z = sqrt(-2.0 * log(u1)) * cos(2.0 * 3.14159265358979323846 * u2);
        v = __fadd_rn(a.policy_act[(size_t)i * a.ld_in + c], __fmul_rn((float)z, a.std));
        v = v < a.lo ? a.lo : v;
        v = v > a.hi ? a.hi : v;
      }
    }
    a.out[(size_t)i * a.ld_out + c] = v;
  }
}

}  // namespace

extern "C" {

int sgrl_explore_actions(const float* policy_act, int ld_in, float* out, int ld_out, const int32_t* act_len, int n_env, int act_max,
                         int64_t env_id_base, uint64_t seed, uint64_t step, int mode, float std, float lo, float hi, void* stream) {
  if (!out || !act_len) return fail(SGRL_ERR_ARG, "sgrl_explore_actions: null out or act_len");
  if (mode != SGRL_EXPLORE_GAUSS && mode != SGRL_EXPLORE_UNIFORM) return fail(SGRL_ERR_ARG, "sgrl_explore_actions: unknown mode");
  if (mode == SGRL_EXPLORE_GAUSS && !policy_act) return fail(SGRL_ERR_ARG, "sgrl_explore_actions: null policy_act in GAUSS mode");
  if (n_env < 0 || act_max <= 0) return fail(SGRL_ERR_ARG, "sgrl_explore_actions: n_env below 0 or act_max below 1");
  if (ld_out < act_max || (mode == SGRL_EXPLORE_GAUSS && ld_in < act_max))
    return fail(SGRL_ERR_ARG, "sgrl_explore_actions: a row stride is smaller than act_max");
  if (!(std >= 0.0f)) return fail(SGRL_ERR_ARG, "sgrl_explore_actions: std below 0");
  if (!(lo <= hi)) return fail(SGRL_ERR_ARG, "sgrl_explore_actions: lo above hi");
  const int64_t elem_limit = (int64_t)1 << 33;                       // element e lies in block e >> 1, a 32-bit number
  if (env_id_base < 0 || env_id_base >= elem_limit || env_id_base + n_env > (elem_limit - 1) / act_max)
    return fail(SGRL_ERR_ARG, "sgrl_explore_actions: env_id_base below 0, or (env_id_base + n_env) * act_max at or above 2^33");
  if (n_env == 0) return SGRL_OK;
  ExploreArgs a;
  a.policy_act = policy_act; a.out = out; a.act_len = act_len;
  a.ld_in = ld_in; a.ld_out = ld_out; a.n_env = n_env; a.act_max = act_max;
  a.rows_per_group = act_max >= kThreads ? 1 : kThreads / act_max;
  a.mode = mode;
  a.env_id_base = (uint64_t)env_id_base; a.seed = seed; a.step = step;
  a.std = std; a.lo = lo; a.hi = hi;
  const unsigned groups = (unsigned)(((int64_t)n_env + a.rows_per_group - 1) / a.rows_per_group);
  hipLaunchKernelGGL(k_explore_actions, dim3(groups), dim3(kThreads), 0, (hipStream_t)stream, a);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(SGRL_ERR_HIP, std::string("k_explore_actions launch failed (") + hipGetErrorName(le) + "); there is no CPU fallback");
  return SGRL_OK;
}

int sgrl_explore_actions_launches(void) { return 1; }

const char* sgrl_explore_last_error(void) { return g_explore_err.c_str(); }

}  // extern "C"
