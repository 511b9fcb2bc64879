// replay_sample.hip -- the read side of the device replay ring (include/sgrl_replay.h): draw k distinct rows, gather the five arrays
// and draw the target-policy noise in ONE launch.  gfx950 only.
//
// Launch geometry: kThreads = 256 threads (four wavefronts) per workgroup, one workgroup per kRowsPerGroup = 4 output rows, one
// wavefront per row.  Every workgroup first recomputes the WHOLE draw into LDS (a few thousand Philox blocks: cheaper than a
// second launch and a workspace to carry the indices in), then each wavefront copies its row of obs / action / next_obs with
// consecutive lanes on consecutive floats (16 bytes per lane where dimension, strides and addresses allow it, 4 otherwise: the
// ring's rows are 16-byte aligned only when obs_dim % 4 == 0) and writes its row of the noise.
//
// The draw (sequential rejection of repeated candidates, in candidate order) as rounds of one candidate per thread: every candidate
// is entered into an LDS hash table of the values seen so far; the first occurrence of a value within a round is the one with the
// smallest thread number (an atomicMin on the entry's owner word), values of earlier rounds are owned by nobody (owner 0); a
// prefix sum over the first occurrences gives their positions.  The table holds at most the < 1024 accepted values plus one
// round's 256 candidates in 2048 entries.  The result does not depend on the workgroup size.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sgrl.h"
#include "../../include/sgrl_replay.h"
#include "replay_rng.h"

namespace {

thread_local std::string g_replay_err;

int fail(int code, const std::string& msg) {
  g_replay_err = msg;
  return code;
}

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerGroup = kWaves;
constexpr int kMaxBatch = SGRL_REPLAY_MAX_BATCH;
constexpr int kTable = 2048;                 // hash entries: a power of two above kMaxBatch + kThreads
constexpr uint32_t kEmpty = 0xFFFFFFFFu;     // no row number reaches it (fill <= 2^31)

struct SampleArgs {
  const float* r_obs; const float* r_action; const float* r_next; const float* r_reward; const float* r_done;
  int obs_dim, act_dim;
  uint32_t fill;
  int k;
  uint64_t seed, draw, cap;
  const long long* idx_in;
  float* obs; float* action; float* next_obs; float* reward; float* done;
  int ld_obs, ld_act, ld_next;
  long long* idx_out;
  float* noise;
  int ld_noise;
  float noise_std;
  int vec_obs, vec_act, vec_next;            // the row copy may use 16-byte accesses
};

struct DrawLds {
  uint32_t key[kTable];
  uint32_t owner[kTable];
  uint32_t idx[kMaxBatch];
  uint32_t wave_tot[kWaves];
};

// slot of value v in the table, entering it if it is not there
__device__ int table_enter(DrawLds& s, uint32_t v) {
  int h = (int)((v * 2654435761u) >> 21);
  for (;;) {
    const uint32_t old = atomicCAS(&s.key[h], kEmpty, v);
    if (old == kEmpty || old == v) return h;
    h = (h + 1) & (kTable - 1);
  }
}

__device__ bool table_has(const DrawLds& s, uint32_t v) {
  int h = (int)((v * 2654435761u) >> 21);
  for (;;) {
    const uint32_t cur = s.key[h];
    if (cur == v) return true;
    if (cur == kEmpty) return false;
    h = (h + 1) & (kTable - 1);
  }
}

// exclusive prefix sum of `flag` over the workgroup in thread order; *total = the sum.  Two barriers.
__device__ int block_scan(DrawLds& s, bool flag, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();                           // wave_tot of the previous scan has been read by everybody
  if (lane == 0) s.wave_tot[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  int ex = before, tot = 0;
  for (int w = 0; w < kWaves; w++) {
    const int t = (int)s.wave_tot[w];
    ex += w < wave ? t : 0;
    tot += t;
  }
  *total = tot;
  return ex;
}

__device__ void draw_indices(DrawLds& s, const SampleArgs& a) {
  const int tid = threadIdx.x, k = a.k;
  for (int i = tid; i < kTable; i += kThreads) {
    s.key[i] = kEmpty;
    s.owner[i] = kEmpty;
  }
  __syncthreads();
  int n_acc = 0;
  uint64_t base = 0;
  while (n_acc < k && base < a.cap) {
    const uint64_t i = base + (uint64_t)tid;
    const bool active = i < a.cap;
    uint32_t c = 0;
    int slot = 0;
    if (active) {
      c = (uint32_t)(((uint64_t)sgrl_replay::replay_word(a.seed, a.draw, 0u, i) * (uint64_t)a.fill) >> 32);
      slot = table_enter(s, c);
      atomicMin(&s.owner[slot], (uint32_t)tid + 1u);
    }
    __syncthreads();
    const bool first = active && s.owner[slot] == (uint32_t)tid + 1u;
    int total;
    const int pos = n_acc + block_scan(s, first, &total);
    if (first) {
      s.owner[slot] = 0u;                    // a value of an earlier round from now on
      if (pos < k) s.idx[pos] = c;
    }
    n_acc += total;
    base += kThreads;
    __syncthreads();
  }
  // the cap was reached first: the remaining positions take the smallest rows not yet taken, ascending.  Fewer than k rows are
  // taken, so k - n_acc free ones exist below k (<= fill); the table holds exactly the accepted values here
  for (int r0 = 0; n_acc < k && r0 < k; r0 += kThreads) {
    const int r = r0 + tid;
    const bool free_row = r < k && !table_has(s, (uint32_t)r);
    int total;
    const int pos = n_acc + block_scan(s, free_row, &total);
    if (free_row && pos < k) s.idx[pos] = (uint32_t)r;
    n_acc += total;
  }
  __syncthreads();
}

// one wavefront copies n floats of a row
__device__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, int n, int vec, int lane) {
  if (vec) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int e = lane; e < (n >> 2); e += 64) d4[e] = s4[e];
  } else {
    for (int e = lane; e < n; e += 64) dst[e] = src[e];
  }
}

__global__ __launch_bounds__(kThreads) void k_replay_sample(SampleArgs a) {
  __shared__ DrawLds s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = (int)blockIdx.x * kRowsPerGroup + wave;      // this wavefront's output row
  if (a.idx_in == nullptr) draw_indices(s, a);               // uniform over the workgroup: barriers inside
  if (j >= a.k) return;
  size_t r;
  if (a.idx_in != nullptr) {
    const long long v = a.idx_in[j];
    if (v < 0 || v >= (long long)a.fill) return;             // a row outside the filled part is never read (its output row stays as it was)
    r = (size_t)v;
  } else {
    r = (size_t)s.idx[j];
  }
  copy_row(a.r_obs + r * (size_t)a.obs_dim, a.obs + (size_t)j * a.ld_obs, a.obs_dim, a.vec_obs, lane);
  copy_row(a.r_next + r * (size_t)a.obs_dim, a.next_obs + (size_t)j * a.ld_next, a.obs_dim, a.vec_next, lane);
  copy_row(a.r_action + r * (size_t)a.act_dim, a.action + (size_t)j * a.ld_act, a.act_dim, a.vec_act, lane);
  if (lane == 0) a.reward[j] = a.r_reward[r];
  if (lane == 1) a.done[j] = a.r_done[r];
  if (lane == 2 && a.idx_out != nullptr) a.idx_out[j] = (long long)r;
  if (a.noise != nullptr) {
    for (int c = lane; c < a.act_dim; c += 64) {
      const uint64_t e = (uint64_t)j * (uint64_t)a.act_dim + (uint64_t)c;      // words 2 e and 2 e + 1: one half of block e >> 1
      const sgrl_replay::Words4 o = sgrl_replay::replay_block(a.seed, a.draw, 1u, (uint32_t)(e >> 1));
      const uint32_t x1 = (e & 1u) ? o.w[2] : o.w[0], x2 = (e & 1u) ? o.w[3] : o.w[1];
      const double u1 = ((double)x1 + 0.5) * (1.0 / 4294967296.0), u2 = ((double)x2 + 0.5) * (1.0 / 4294967296.0);
      const double z = sqrt(-2.0 * log(u1)) * cos(2.0 * 3.14159265358979323846 * u2);
      a.noise[(size_t)j * a.ld_noise + c] = (float)z * a.noise_std;
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int sgrl_replay_sample(const sgrl_ring* ring, int64_t fill, int batch, uint64_t seed, uint64_t draw, int64_t max_candidates,
                       const int64_t* idx_in, float* obs, int ld_obs, float* action, int ld_act, float* next_obs, int ld_next,
                       float* reward, float* done, int64_t* idx_out, float* noise, int ld_noise, float noise_std, void* stream) {
  if (!ring || !ring->obs || !ring->action || !ring->next_obs || !ring->reward || !ring->done || ring->obs_dim < 1 || ring->act_dim < 1)
    return fail(SGRL_ERR_ARG, "sgrl_replay_sample: null ring or ring array, or a dimension below 1");
  if (!obs || !action || !next_obs || !reward || !done) return fail(SGRL_ERR_ARG, "sgrl_replay_sample: null output");
  if (fill < 1 || fill > ((int64_t)1 << 31)) return fail(SGRL_ERR_ARG, "sgrl_replay_sample: fill outside 1 .. 2^31");
  if (batch < 1 || batch > kMaxBatch) return fail(SGRL_ERR_ARG, "sgrl_replay_sample: batch outside 1 .. 1024");
  if (ld_obs < ring->obs_dim || ld_next < ring->obs_dim || ld_act < ring->act_dim)
    return fail(SGRL_ERR_ARG, "sgrl_replay_sample: a row stride is smaller than its dimension");
  if (noise && ld_noise < ring->act_dim) return fail(SGRL_ERR_ARG, "sgrl_replay_sample: ld_noise is smaller than act_dim");
  if (max_candidates < 0 || max_candidates > ((int64_t)1 << 32))
    return fail(SGRL_ERR_ARG, "sgrl_replay_sample: max_candidates outside 0 .. 2^32");
  const int k = (int)(fill < (int64_t)batch ? fill : (int64_t)batch);
  SampleArgs a;
  a.r_obs = ring->obs; a.r_action = ring->action; a.r_next = ring->next_obs; a.r_reward = ring->reward; a.r_done = ring->done;
  a.obs_dim = ring->obs_dim; a.act_dim = ring->act_dim;
  a.fill = (uint32_t)fill;
  a.k = k;
  a.seed = seed; a.draw = draw;
  a.cap = max_candidates == 0 ? (uint64_t)64 * (uint64_t)k : (uint64_t)max_candidates;
  a.idx_in = reinterpret_cast<const long long*>(idx_in);
  a.obs = obs; a.action = action; a.next_obs = next_obs; a.reward = reward; a.done = done;
  a.ld_obs = ld_obs; a.ld_act = ld_act; a.ld_next = ld_next;
  a.idx_out = reinterpret_cast<long long*>(idx_out);
  a.noise = noise; a.ld_noise = ld_noise; a.noise_std = noise_std;
  // 16 bytes per lane needs every row of source and destination on a 16-byte boundary
  a.vec_obs = a.obs_dim % 4 == 0 && ld_obs % 4 == 0 && aligned16(ring->obs) && aligned16(obs);
  a.vec_next = a.obs_dim % 4 == 0 && ld_next % 4 == 0 && aligned16(ring->next_obs) && aligned16(next_obs);
  a.vec_act = a.act_dim % 4 == 0 && ld_act % 4 == 0 && aligned16(ring->action) && aligned16(action);
  hipLaunchKernelGGL(k_replay_sample, dim3((k + kRowsPerGroup - 1) / kRowsPerGroup), dim3(kThreads), 0, (hipStream_t)stream, a);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(SGRL_ERR_HIP, std::string("k_replay_sample launch failed (") + hipGetErrorName(le) + "); there is no CPU fallback");
  return SGRL_OK;
}

int sgrl_replay_sample_launches(void) { return 1; }

const char* sgrl_replay_last_error(void) { return g_replay_err.c_str(); }

}  // extern "C"
