// eval_record.hip -- the evaluation bookkeeping (include/sgrl_eval.h): the per-environment rule of the reference's evaluate loop
// for every trajectory of an evaluation at once, ONE launch per time step.  gfx950 only.
//
// Launch geometry: kThreads = 256 threads per workgroup, one thread per environment.  The only traffic between threads is integer
// atomics on the per-group member count and the open-group count, and one plain 32-bit store of a group's closing step by the
// member that took the count to zero.  A member of the same group in the same launch may read that word before or after the store
// (0 or step + 1); the freeze test `!= 0 && <= step` answers "not frozen" to both, so no ordering between them is needed.  Across
// launches the stream orders everything.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sgrl.h"
#include "../../include/sgrl_eval.h"

namespace {

thread_local std::string g_eval_err;

int fail(int code, const std::string& msg) {
  g_eval_err = msg;
  return code;
}

constexpr int kThreads = 256;

// device-side copy of the state descriptor (plain pointers: no member is read through the constant path except `group`)
struct EvalArgs {
  const int32_t* group;
  uint8_t* done_ever;
  long long* ep_steps;
  double* ep_reward;
  double* acc;
  int* remaining;
  int* close_step;
  int* open;
};

__global__ __launch_bounds__(kThreads) void k_eval_clear(EvalArgs s, int n_env, int n_groups) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n_env) {
    s.done_ever[i] = 0;
    s.ep_steps[i] = 0;
    s.ep_reward[i] = 0.0;
    s.acc[i] = 0.0;
  }
  if (i < n_groups) {
    s.remaining[i] = 0;
    s.close_step[i] = 0;
  }
  if (i == 0) *s.open = n_groups;
}

__global__ __launch_bounds__(kThreads) void k_eval_count(EvalArgs s, int n_env, int n_groups) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_env) return;
  const int g = s.group[i];
  if (g < 0 || g >= n_groups) return;
  atomicAdd(&s.remaining[g], 1);
}

template <typename R>
__global__ __launch_bounds__(kThreads) void k_eval_record(EvalArgs s, const R* __restrict__ reward, const uint8_t* __restrict__ done,
                                                          int n_env, int n_groups, int step, int max_steps) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_env) return;
  const int g = s.group[i];
  if (g < 0 || g >= n_groups) return;
  const int closed = s.close_step[g];
  if (closed != 0 && closed <= step) return;             // the group completed in an earlier launch: frozen
  double acc = s.acc[i] + (double)reward[i];
  double er = s.ep_reward[i];
  const long long st = s.ep_steps[i];
  const bool cur = done[i] != 0 || st + 1 == (long long)max_steps;
  if (cur && er == 0.0) { er = acc; acc = 0.0; }         // latched while still exactly 0 (later dones re-latch a zero return)
  s.ep_reward[i] = er;
  s.acc[i] = acc;
  const bool was = s.done_ever[i] != 0;
  if (!was) s.ep_steps[i] = st + 1;
  if (cur && !was) {
    s.done_ever[i] = 1;
    if (atomicSub(&s.remaining[g], 1) == 1) {            // the last member of its group to finish once
      s.close_step[g] = step + 1;
      atomicSub(s.open, 1);
    }
  }
}

const char* check_state(const sgrl_eval_state* st) {
  if (!st) return "null state";
  if (!st->group || !st->done_ever || !st->ep_steps || !st->ep_reward || !st->acc || !st->remaining || !st->close_step || !st->open)
    return "null state member";
  return nullptr;
}

EvalArgs device_args(const sgrl_eval_state* st) {
  EvalArgs a;
  a.group = st->group;
  a.done_ever = st->done_ever;
  a.ep_steps = reinterpret_cast<long long*>(st->ep_steps);
  a.ep_reward = st->ep_reward;
  a.acc = st->acc;
  a.remaining = reinterpret_cast<int*>(st->remaining);
  a.close_step = reinterpret_cast<int*>(st->close_step);
  a.open = reinterpret_cast<int*>(st->open);
  return a;
}

int launched(const char* what) {
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(SGRL_ERR_HIP, std::string(what) + " launch failed (" + hipGetErrorName(le) + "); there is no CPU fallback");
  return SGRL_OK;
}

}  // namespace

extern "C" {

int sgrl_eval_begin(const sgrl_eval_state* state, int n_env, int n_groups, void* stream) {
  if (const char* why = check_state(state)) return fail(SGRL_ERR_ARG, std::string("sgrl_eval_begin: ") + why);
  if (n_env <= 0 || n_groups <= 0) return fail(SGRL_ERR_ARG, "sgrl_eval_begin: n_env or n_groups below 1");
  const EvalArgs a = device_args(state);
  const int n = n_env > n_groups ? n_env : n_groups;
  hipLaunchKernelGGL(k_eval_clear, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, a, n_env, n_groups);
  hipLaunchKernelGGL(k_eval_count, dim3((n_env + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, a, n_env, n_groups);
  return launched("k_eval_clear / k_eval_count");
}

int sgrl_eval_record(const sgrl_eval_state* state, const float* reward_f32, const double* reward_f64, const uint8_t* done_u8,
                     int n_env, int n_groups, int step, int max_episode_steps, void* stream) {
  if (const char* why = check_state(state)) return fail(SGRL_ERR_ARG, std::string("sgrl_eval_record: ") + why);
  if (!done_u8) return fail(SGRL_ERR_ARG, "sgrl_eval_record: null done");
  if (n_env <= 0 || n_groups <= 0) return fail(SGRL_ERR_ARG, "sgrl_eval_record: n_env or n_groups below 1");
  if (step < 0 || step == INT32_MAX) return fail(SGRL_ERR_ARG, "sgrl_eval_record: step outside 0 .. 2^31-2");
  if (max_episode_steps <= 0) return fail(SGRL_ERR_ARG, "sgrl_eval_record: max_episode_steps below 1");
  if ((reward_f32 != nullptr) == (reward_f64 != nullptr))
    return fail(SGRL_ERR_ARG, "sgrl_eval_record: exactly one of reward_f32 / reward_f64 must be given");
  const EvalArgs a = device_args(state);
  const dim3 grid((n_env + kThreads - 1) / kThreads), block(kThreads);
  if (reward_f32)
    hipLaunchKernelGGL(k_eval_record<float>, grid, block, 0, (hipStream_t)stream, a, reward_f32, done_u8, n_env, n_groups, step, max_episode_steps);
  else
    hipLaunchKernelGGL(k_eval_record<double>, grid, block, 0, (hipStream_t)stream, a, reward_f64, done_u8, n_env, n_groups, step, max_episode_steps);
  return launched("k_eval_record");
}

int sgrl_eval_record_launches(void) { return 1; }

const char* sgrl_eval_last_error(void) { return g_eval_err.c_str(); }

}  // extern "C"
