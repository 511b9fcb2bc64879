// replay_rng.h -- the counter RNG of the replay draw (include/sgrl_replay.h): Philox4x32-10, the round function and constants of
// rng_uniform01 (step_body.h), handing out all four words of a block.  Plain integer C++: host and device compile the same text.
#ifndef SGRL_REPLAY_RNG_H
#define SGRL_REPLAY_RNG_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SGRL_RNG_FN __host__ __device__ inline
#else
#define SGRL_RNG_FN inline
#endif

namespace sgrl_replay {

struct Words4 {
  uint32_t w[4];
};

SGRL_RNG_FN Words4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Words4{{c0, c1, c2, c3}};
}

// the block holding words 4 b .. 4 b + 3 of stream `stream` of (seed, draw): key (seed lo, seed hi), counter (b, draw lo, draw hi, stream)
SGRL_RNG_FN Words4 replay_block(uint64_t seed, uint64_t draw, uint32_t stream, uint32_t b) {
  return philox4x32_10(b, (uint32_t)draw, (uint32_t)(draw >> 32), stream, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// word i of the stream
SGRL_RNG_FN uint32_t replay_word(uint64_t seed, uint64_t draw, uint32_t stream, uint64_t i) {
  const Words4 o = replay_block(seed, draw, stream, (uint32_t)(i >> 2));
  const uint32_t lane = (uint32_t)i & 3u;
  return lane == 0 ? o.w[0] : (lane == 1 ? o.w[1] : (lane == 2 ? o.w[2] : o.w[3]));
}

}  // namespace sgrl_replay
#endif
