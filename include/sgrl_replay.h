/* sgrl_replay.h -- C ABI of the read side of the device replay ring in libsgrl_hip.so: one call draws a batch of distinct rows,
 * gathers them and draws the target-policy noise, straight into tensors the caller owns.
 *
 * Replaces, for one TD3 update,
 *   ReplayBuffer.sample                    reference src/common/buffer.py:87-126
 *                                          (np.random.choice(fill, batch, replace=False) plus five fancy-index reads)
 *   the target-policy noise draw           reference src/agent.py:128
 * The write side of the ring is sgrl_ingest_block (sgrl.h), whose sgrl_ring descriptor this call reads.
 *
 * THE DRAW is defined in integers, so that any restatement (tests/test_replay_sample.py has one in NumPy) computes the same rows
 * bit for bit.  Philox4x32-10 (the round function and constants of rng_uniform01 in sgrl_amd/csrc/step_body.h; here in
 * sgrl_amd/csrc/replay_rng.h) with
 *   key     = (seed lo, seed hi)
 *   counter = (i >> 2, draw lo, draw hi, stream)          word i & 3 of the output is x_i
 * Indices, stream 0:
 *   candidate c_i = (uint64(x_i) * uint64(fill)) >> 32 for i = 0, 1, 2, ...; idx[j] is the j-th DISTINCT value of that sequence in
 *   order of i: sequential rejection of repeats, i.e. a uniform ordered sample without replacement, which is what the reference
 *   draws.  The multiply-shift is biased by less than fill / 2^32 (2.4e-4 at the reference's 1 M-row buffers).  At most
 *   max_candidates candidates are looked at (0 = 64 * k); if fewer than k distinct values have turned up by then, the remaining
 *   positions take the smallest row numbers not yet taken, ascending.  With the default cap that is unreachable in practice
 *   (fill = k = 1024, the worst case, needed at most 16 631 candidates in 200 trials against a cap of 65 536; the tail beyond the
 *   cap is below e^-50): the parameter exists so that a test can reach the fallback on purpose.
 * Noise, stream 1:
 *   element (j, c), c < act_dim, takes words 2e and 2e + 1 with e = j * act_dim + c; u = (x + 0.5) / 2^32 as rng_uniform01 does;
 *   z = sqrt(-2 ln u1) * cos(2 pi u2) evaluated in float64 and rounded once to float32, then multiplied by noise_std in float32.
 *   Unclipped: the TD3 target path clips it.
 *
 * Conventions as in sgrl.h: int return codes, DEV = device pointer owned by the caller, `stream` a hipStream_t as void*.
 */
#ifndef SGRL_REPLAY_H
#define SGRL_REPLAY_H

#include <stdint.h>

#include "sgrl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGRL_REPLAY_MAX_BATCH 1024

/* k = min(fill, batch) rows of `ring` (a HOST struct holding DEVICE pointers and obs_dim / act_dim; `fill` = its filled rows):
 *   output row j = ring row idx[j], cut to obs_dim / act_dim columns; columns beyond those, up to the ld_* stride, and rows
 *   k .. batch-1 of every output are not written.
 *   idx_in   DEV int64[k] or NULL: use these rows instead of drawing (gather only; each must be in 0 .. fill-1)
 *   obs / action / next_obs   DEV float [k, ld_*];  reward / done   DEV float [k]
 *   idx_out  DEV int64[k] or NULL: the rows taken, in draw order
 *   noise    DEV float [k, ld_noise] or NULL: noise_std * N(0, 1) in columns 0 .. act_dim-1
 * Asynchronous on `stream`; reads nothing back to the host, allocates nothing, can be recorded into a hipGraph; ONE launch.
 * SGRL_ERR_ARG, before any launch, for: a null ring, ring array or output; fill < 1 or fill > 2^31; batch outside 1 .. 1024; an
 * ld_* smaller than its dimension; noise with ld_noise < act_dim; max_candidates < 0 or > 2^32.  SGRL_ERR_HIP with no device:
 * there is no CPU fallback. */
int sgrl_replay_sample(const sgrl_ring* ring, int64_t fill, int batch, uint64_t seed, uint64_t draw, int64_t max_candidates,
                       const int64_t* idx_in, float* obs, int ld_obs, float* action, int ld_act, float* next_obs, int ld_next,
                       float* reward, float* done, int64_t* idx_out, float* noise, int ld_noise, float noise_std, void* stream);
/* Launches of one sgrl_replay_sample (1: every workgroup of the gather recomputes the draw instead of waiting for a launch of its own). */
int sgrl_replay_sample_launches(void);
const char* sgrl_replay_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SGRL_REPLAY_H */
