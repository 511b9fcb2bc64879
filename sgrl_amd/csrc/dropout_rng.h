// dropout_rng.h -- the ONE definition of the dropout masks (include/sgrl_train.h "counter-RNG dropout"), shared by the element-wise
// kernel (dropout.hip) and the SWAT attention pair (train_gemm.hip).  Plain C++ on top of replay_rng.h: host and device compile the
// same text; tests/dropout_restate.py restates it in NumPy and train_ops restates it in torch integer arithmetic.
//   word = replay_word(seed, step, 0x100 + site, i)       i: row-major linear index in the tensor the dropout is applied to
//   thr  = (uint64) floor((double) p * 4294967296.0)      p in [0, 1] (a float)
//   keep = (uint64) word >= thr
//   y    = keep ? x * (1.0f / (1.0f - p)) : 0.0f          p == 1: thr = 2^32, nothing kept; p == 0: thr = 0, scale = 1, y = x
// Stream ids 0 and 1 belong to the replay draw (replay_sample.hip); the dropout sites start at 0x100.
#ifndef SGRL_DROPOUT_RNG_H
#define SGRL_DROPOUT_RNG_H

#include <stdint.h>

#include "replay_rng.h"

namespace sgrl_dropout {

constexpr uint32_t kStreamBase = 0x100u;
constexpr int kMaxSite = (1 << 24) - 1;

inline bool valid(float p, int site) { return p >= 0.f && p <= 1.f && site >= 0 && site <= kMaxSite; }      // false for a NaN p
inline uint64_t threshold(float p) { return (uint64_t)((double)p * 4294967296.0); }       // the product is exact: truncation = floor
inline float scale(float p) { return 1.0f / (1.0f - p); }                                 // inf at p == 1: never multiplied with
inline uint32_t stream_of(int site) { return kStreamBase + (uint32_t)site; }

SGRL_RNG_FN bool keep(uint32_t word, uint64_t thr) { return (uint64_t)word >= thr; }
SGRL_RNG_FN float apply(float x, uint32_t word, uint64_t thr, float scale) { return keep(word, thr) ? x * scale : 0.0f; }

}  // namespace sgrl_dropout
#endif
