/* sgrl_explore.h -- C ABI of the behaviour policy's action choice in libsgrl_hip.so: the exploration noise and the warm-up actions
 * from the counter RNG, written in ONE launch straight into the tensor the engine reads.
 *
 * Replaces, for one collection step,
 *   the exploration noise        reference src/trainer.py:184-189   (np.random.normal, +, clip) and the zero padding :191-195
 *   the warm-up actions          reference src/trainer.py:95-102    (uniform in the action range)
 *
 * THE NOISE is a function of (seed, step, global environment number, slot) and nothing else, so that any restatement
 * (tests/explore_restate.py has one in NumPy) computes the same values.  For local row i, slot c and g = env_id_base + i:
 *   padding   c >= act_len[i]:  out[i][c] = 0 for c < act_max; columns act_max .. ld_out-1 are not touched
 *   element   e = g * act_max + c takes words 2e and 2e + 1 of its stream: one half of block e >> 1, the layout of the replay's
 *             target-policy noise (sgrl_replay.h)
 *   block     Philox4x32-10 with key (seed lo, seed hi) and counter (block, step lo, step hi, stream tag): replay_block of
 *             sgrl_amd/csrc/replay_rng.h with draw = step
 *   GAUSS, stream tag 2:    u1, u2 = (word + 0.5) / 2^32 and z = sqrt(-2 ln u1) * cos(2 pi u2) in float64, z rounded once to float32;
 *                           out = min(max(policy_act + z * std, lo), hi), each operation rounded to float32, in that order
 *   UNIFORM, stream tag 3:  out = lo + (hi - lo) * (float)u1, each operation rounded to float32; policy_act is not read
 * Stream tags 0 (rows) and 1 (target-policy noise) are the replay's: the four streams of one (seed, counter) share no words.
 * A row's values do not depend on which call, or which rank, computes it: rows [a, b) of a call with env_id_base = 0 are those of
 * a call with env_id_base = a.
 *
 * Conventions as in sgrl.h: int return codes, DEV = device pointer owned by the caller, `stream` a hipStream_t as void*.
 */
#ifndef SGRL_EXPLORE_H
#define SGRL_EXPLORE_H

#include <stdint.h>

#include "sgrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGRL_EXPLORE_GAUSS 0
#define SGRL_EXPLORE_UNIFORM 1

/*   policy_act  DEV float [n_env, ld_in], ld_in >= act_max; NULL allowed in UNIFORM mode (never read there)
 *   out         DEV float [n_env, ld_out], ld_out >= act_max; may be the same memory as policy_act (every element is read and
 *               written by the same thread)
 *   act_len     DEV int32 [n_env]: live slots of each row (3 L), <= act_max
 * Asynchronous on `stream`; reads nothing back to the host, allocates nothing, can be recorded into a hipGraph; ONE launch, one
 * thread per element.  n_env == 0 is success without a launch.
 * SGRL_ERR_ARG, before any launch, for: a null out or act_len; a null policy_act in GAUSS mode; ld_in (GAUSS) or ld_out below
 * act_max; n_env < 0; act_max <= 0; an unknown mode; std < 0; lo > hi; env_id_base < 0; (env_id_base + n_env) * act_max >= 2^33
 * (the block number is 32 bits wide).  SGRL_ERR_HIP with no device: there is no CPU fallback. */
int sgrl_explore_actions(const float* policy_act, int ld_in, float* out, int ld_out, const int32_t* act_len, int n_env, int act_max,
                         int64_t env_id_base, uint64_t seed, uint64_t step, int mode, float std, float lo, float hi, void* stream);
/* Launches of one sgrl_explore_actions (1). */
int sgrl_explore_actions_launches(void);
const char* sgrl_explore_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SGRL_EXPLORE_H */
