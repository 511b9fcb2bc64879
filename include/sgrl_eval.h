/* sgrl_eval.h -- C ABI of the evaluation bookkeeping in libsgrl_hip.so: the per-environment rule of the reference's
 * BaseTrainer.evaluate (reference src/common/trainer.py:80-146; restated by sgrl_amd/evaluate.py BatchedEvaluator) for ALL
 * trajectories of one evaluation at once, one launch per time step.
 *
 * The reference runs its num_eval_trajectories one after the other.  They do not depend on each other, so here they lie side by
 * side: every environment belongs to a GROUP (one trajectory of the reference = one environment of every morphology), and the
 * reference's `all(done)` test, which ends a trajectory and decides whether it contributes at all, becomes a property of a group.
 *
 * State: caller-owned DEVICE memory, described by a HOST struct of device pointers.
 *   per environment [n_env]   group      int32    id of the trajectory group the environment belongs to (input, 0 .. n_groups-1)
 *                             done_ever  uint8    finished at least once
 *                             ep_steps   int64    steps until the first done                    (episode_timesteps_list)
 *                             ep_reward  float64  return latched at a done while still exactly 0 (episode_reward_list)
 *                             acc        float64  running sum since the last latch              (episode_reward_list_buffer)
 *   per group [n_groups]      remaining  int32    members not yet done once
 *                             close_step int32    0 = open, else the 1-based step at which the group completed
 *   global                    open       int32[1] groups still open
 *
 * The rule of one sgrl_eval_record for environment i, g = group[i], in float64:
 *   if close_step[g] != 0 and close_step[g] <= step: return            the group completed in an EARLIER launch: frozen
 *   acc += reward;  cur = done | (ep_steps + 1 == max_episode_steps)
 *   if cur and ep_reward == 0: ep_reward = acc; acc = 0                the reference's re-latch-while-zero rule
 *   if not done_ever: ep_steps += 1
 *   if cur and not done_ever: done_ever = 1
 *                             if atomicSub(&remaining[g], 1) == 1: close_step[g] = step + 1; atomicSub(open, 1)
 * The member that closes a group writes step + 1; the other members of the group running in the same launch read 0 or step + 1,
 * and neither freezes them: every member completes the closing step's bookkeeping, as the reference does before it tests
 * all(done).  Only integer atomics: every output is bit-reproducible and independent of scheduling.
 *
 * Conventions as in sgrl.h: int return codes, DEV = device pointer owned by the caller, `stream` a hipStream_t as void*.
 */
#ifndef SGRL_EVAL_H
#define SGRL_EVAL_H

#include <stdint.h>

#include "sgrl.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgrl_eval_state {
  const int32_t* group;   /* DEV [n_env] */
  uint8_t* done_ever;     /* DEV [n_env] */
  int64_t* ep_steps;      /* DEV [n_env] */
  double* ep_reward;      /* DEV [n_env] */
  double* acc;            /* DEV [n_env] */
  int32_t* remaining;     /* DEV [n_groups] */
  int32_t* close_step;    /* DEV [n_groups] */
  int32_t* open;          /* DEV [1] */
} sgrl_eval_state;

/* Start an evaluation: zeroes done_ever / ep_steps / ep_reward / acc / close_step, counts `remaining` from `group` (an id outside
 * 0 .. n_groups-1 is counted nowhere, and its environment is never recorded) and sets open = n_groups.  Two launches on `stream`.
 * A group without members never completes: the caller checks that (sgrl_amd/evaluate.py DeviceEvaluator does). */
int sgrl_eval_begin(const sgrl_eval_state* state, int n_env, int n_groups, void* stream);

/* One time step of every environment: reward as DEV float[n_env] (reward_f32: what sgrl_step writes) OR DEV double[n_env]
 * (reward_f64: parity tests), exactly one of the two; done_u8 DEV uint8[n_env]; `step` the caller's 0-based step counter.
 * ONE launch, one thread per environment, on `stream`; allocates nothing, synchronises nothing, can be recorded into a hipGraph.
 * SGRL_ERR_ARG, before any launch, for: a null state or state member or done_u8; n_env <= 0, n_groups <= 0, step < 0,
 * max_episode_steps <= 0; both reward pointers or neither.  SGRL_ERR_HIP with no device: there is no CPU fallback. */
int sgrl_eval_record(const sgrl_eval_state* state, const float* reward_f32, const double* reward_f64, const uint8_t* done_u8,
                     int n_env, int n_groups, int step, int max_episode_steps, void* stream);
/* Launches of one sgrl_eval_record (1). */
int sgrl_eval_record_launches(void);
const char* sgrl_eval_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SGRL_EVAL_H */
