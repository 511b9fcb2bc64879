// engine.hip -- HIP kernels + C ABI (include/sgrl.h) of the batched rollout engine.  gfx950 only.
//
// Launch geometry: one 64-thread workgroup (= one wavefront) per environment; dynamic LDS = the largest
// per-environment slab over the morphologies in the batch (step_body.h Layout).  Per-environment persistent
// state is an array of records in HBM: one wave reads and writes one contiguous record (coalesced), the
// observation row [env][obs_max_len] is written once with consecutive lanes on consecutive floats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine_kernel.h"
#include "stream_pick.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(SGRL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                \
  } while (0)

using namespace sgrl_engine_dev;

// generic instances: dimensions from the morphology header at run time (any morphology the limits of sgrl_engine_create admit)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_env_step(BatchArgs a, StepOut out) {
  env_step_wave<DimsAny, sgrl::HipWave>(a, out, __builtin_amdgcn_readfirstlane(a.block_env[blockIdx.x]));
}

// The step kernel for the LIGHT morphologies (nv <= kLightNv: walker_2/3/4, hopper_3/4): the same source with the register
// solvers of the larger dof counts compiled out and a 168-register budget, i.e. three waves per SIMD = 12 workgroups per CU
// instead of 8.  Their slabs (7..13 KB) leave the LDS half empty at 8 per CU, and the kernel is bound by the latency of its
// dependent chains: throughput follows the number of resident environments.
constexpr int kLightNv = 15;
constexpr int kLightPerCu = 12;
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_env_step_light(BatchArgs a, StepOut out) {
  env_step_wave<DimsAny, sgrl::HipWaveT<kLightNv>>(a, out, __builtin_amdgcn_readfirstlane(a.block_env[blockIdx.x]));
}

// sgrl_reset: every environment.  sgrl_reset_where: `out.done` carries the caller's mask [n_env] (the reset writes no `done`, so the
// field is free here); a workgroup whose environment is not selected leaves before it reads or writes anything of that environment.
__global__ __launch_bounds__(64) void k_env_reset(BatchArgs a, StepOut out) {
  const int env = __builtin_amdgcn_readfirstlane(a.block_env[blockIdx.x]);
  if (out.done && !__builtin_amdgcn_readfirstlane((int)out.done[env])) return;
  SgrlModelView m; sgrl::Layout o; double* S; int32_t* I;
  setup<DimsAny>(a, env, &m, &o, &S, &I);
  sgrl::HipWave w;
  const sgrl::StepIO io = make_io(a, out, env);
  sgrl::env_reset(w, m, o, S, I, io, true);
}

__global__ __launch_bounds__(64) void k_env_refresh(BatchArgs a, StepOut out) {
  const int env = __builtin_amdgcn_readfirstlane(a.block_env[blockIdx.x]);
  SgrlModelView m; sgrl::Layout o; double* S; int32_t* I;
  setup<DimsAny>(a, env, &m, &o, &S, &I);
  sgrl::HipWave w;
  const sgrl::StepIO io = make_io(a, out, env);
  sgrl::env_refresh(w, m, o, S, I, io);
}

// ---- test hooks (sgrl_debug_chol_solve, sgrl_debug_chol_inv): the register solvers on either wave policy, one workgroup.  FORM 1 is
// what the step kernels run (broadcast inside the FMA instruction), FORM 0 the lane-read form it replaced: only these hooks build it.
template <int FORM, class Wv>
__device__ __forceinline__ void debug_chol_solve(Wv& w, int n, double* C, double* x, double* wv, bool inverse, bool inverse_only, int32_t* ok) {
  bool done;
  if (inverse_only) {
    done = w.template chol_inv_packed<FORM>(n, C, sgrl::kMinVal);
  } else if (!inverse) {
    done = w.template chol_solve_packed<FORM>(n, C, x, sgrl::kMinVal);
  } else {                     // the explicit-inverse path as lcp_block_pivot ran it: x = T'(T rhs), two lane-per-entry products
    done = w.template chol_inv_packed<FORM>(n, C, sgrl::kMinVal);
    if (done) {
      w.lanes(n, [&](int i) {
        double z = 0;
        for (int c = 0; c <= i; c++) z += C[i * (i + 1) / 2 + c] * x[c];
        wv[i] = z;
      });
      w.lanes(n, [&](int k) {
        double s = 0;
        for (int i = k; i < n; i++) s += C[i * (i + 1) / 2 + k] * wv[i];
        x[k] = s;
      });
    }
  }
  if (w.lane == 0) *ok = done ? 1 : 0;
}
__global__ __launch_bounds__(64) void k_debug_chol_solve(int flags, const int32_t* n, const double* C, const double* rhs, double* C_out,
                                                         double* x_out, int32_t* ok) {
  constexpr int LD = SGRL_DEBUG_CHOL_LD;
  __shared__ double sC[2 * LD], sx[64], swv[64];
  const int t = threadIdx.x;
  for (int i = t; i < 2 * LD; i += 64) sC[i] = C[i];
  sx[t] = rhs[t];
  swv[t] = 0.0;
  __syncthreads();
  const bool inv = (flags & 2) != 0, inv_only = (flags & 8) != 0;
  if (flags & 1) {
    sgrl::HalfWaveT<15, sgrl::HipHalfPrim<sgrl::DimsAny>> w;
    const int h = w.half;
    if (flags & 4) debug_chol_solve<0>(w, n[h], sC + h * LD, sx + h * 32, swv + h * 32, inv, inv_only, ok + h);
    else debug_chol_solve<1>(w, n[h], sC + h * LD, sx + h * 32, swv + h * 32, inv, inv_only, ok + h);
  } else {
    sgrl::HipWave w;
    if (flags & 4) debug_chol_solve<0>(w, n[0], sC, sx, swv, inv, inv_only, ok);
    else debug_chol_solve<1>(w, n[0], sC, sx, swv, inv, inv_only, ok);
  }
  __syncthreads();
  for (int i = t; i < 2 * LD; i += 64) C_out[i] = sC[i];
  x_out[t] = sx[t];
}

// ---- fixed-dimension kernels of the step (step_spec.hip; table generated by sgrl_amd/_lib.py build()) ------------------------
typedef int (*SpecLaunch)(int, int, void*, const void*, const void*);
struct SpecFamily { int waves; int n; SpecLaunch launch; int itab_global; };      // itab_global: the kernel reads the int tables from global memory (no LDS copy)
struct SpecMember { int family, slot; int dims[12]; };      // 11 header fields + "has a two-environments-per-wavefront instance"
}  // namespace
#ifndef SGRL_NO_SPECS
#define SGRL_FAMILY(id, waves, n, itab) extern "C" int sgrl_spec_launch_##id(int, int, void*, const void*, const void*);
#define SGRL_MEMBER(...)
#include "spec_table.inc"
#undef SGRL_FAMILY
#undef SGRL_MEMBER
namespace {
const SpecFamily kFamilies[] = {
#define SGRL_FAMILY(id, waves, n, itab) {waves, n, sgrl_spec_launch_##id, itab},
#define SGRL_MEMBER(...)
#include "spec_table.inc"
#undef SGRL_FAMILY
#undef SGRL_MEMBER
};
const SpecMember kMembers[] = {
#define SGRL_FAMILY(id, waves, n, itab)
#define SGRL_MEMBER(fam, slot, ...) {fam, slot, {__VA_ARGS__}},
#include "spec_table.inc"
#undef SGRL_FAMILY
#undef SGRL_MEMBER
};
constexpr int kNumMembers = (int)(sizeof(kMembers) / sizeof(kMembers[0]));
}  // namespace
#else
namespace {
const SpecFamily kFamilies[1] = {{0, 0, nullptr, 0}};
const SpecMember kMembers[1] = {{-1, -1, {0}}};
constexpr int kNumMembers = 0;
}  // namespace
#endif
namespace {
// the instance built for exactly this header's dimension set (index into kMembers) in a kernel of `waves` waves per SIMD, or -1
int spec_for(const int32_t* hdr, int waves) {
  static const int fields[11] = {SGRL_H_NBODY, SGRL_H_NJNT, SGRL_H_NQ, SGRL_H_NV, SGRL_H_NU, SGRL_H_NGEOM, SGRL_H_NPAIR,
                                 SGRL_H_INTEGRATOR, SGRL_H_FRAME_SKIP, SGRL_H_MAX_ROWS, SGRL_H_SOLVER};
  for (int k = 0; k < kNumMembers; k++) {
    if (kFamilies[kMembers[k].family].waves != waves) continue;
    bool same = true;
    for (int f = 0; f < 11 && same; f++) same = kMembers[k].dims[f] == hdr[fields[f]];
    if (same) return k;
  }
  return -1;
}
}  // namespace

struct sgrl_engine {
  int n_morph = 0, n_env = 0, stride = 0, lds_bytes = 0, scratch_stride = 0;
  int obs_max_len = 0, action_max_len = 0;
  std::vector<int32_t*> d_ib;
  std::vector<double*> d_fb;
  MorphDev* d_morphs = nullptr;
  int32_t* d_env_morph = nullptr;
  int32_t* d_block_env = nullptr;
  int32_t* d_step_env = nullptr;     // fixed-dimension step kernels: workgroup -> first environment ...
  int32_t* d_step_mate = nullptr;    // ... and its wave mate (-1: one environment per workgroup)
  int n_paired = 0;                  // environments that step two to a wavefront
  double* d_rec = nullptr;
  int32_t* d_cnt = nullptr;
  double* d_scratch = nullptr;
  int max_geoms = 0;                 // largest ngeom over the morphologies (sgrl_max_geoms)
  double* d_cam_dist = nullptr;      // [n_morph] camera distance per morphology as sgrl_scene last uploaded it (engine_view.h)
  std::vector<double> cam_dist;      // its host copy
  BatchArgs args{};
  // Launch groups: morphologies whose LDS slab admits the same number of workgroups per CU share one launch (its
  // dynamic LDS = the group's largest slab), so a 23-morphology mix is not dragged to the occupancy of its biggest
  // member.  Groups run concurrently on their own streams, forked from / joined to the caller's stream by events.
  struct Group {
    int first = 0, count = 0, lds = 0; bool light = false; int spec = -1; hipStream_t stream = nullptr; hipEvent_t done = nullptr;
    int step_first = 0, step_count = 0, step_lds = 0;     // the group's workgroups on its fixed-dimension step kernel (spec >= 0)
  };
  std::vector<Group> groups;
  bool groups_checked = false;     // group streams measured to sit on distinct hardware queues (stream_pick.h)
  hipEvent_t fork = nullptr;
  std::vector<int> morph_lds;
};

namespace {
template <class K>
int launch_groups(sgrl_engine* e, K kernel_in, const StepOut& out, hipStream_t user, bool is_step = false) {
  auto pick = [&](const sgrl_engine::Group& g) { return (is_step && g.light) ? k_env_step_light : kernel_in; };
  // a group of one dimension set steps on the kernel instance built for it
  auto launch = [&](const sgrl_engine::Group& g, const BatchArgs& a_in, hipStream_t st) -> int {
    const BatchArgs& a = a_in;
    if (is_step && g.spec >= 0) {
      BatchArgs b = a_in;       // the step kernels walk the workgroup list (one or two environments each), not the environment list
      b.block_env = e->d_step_env + g.step_first;
      b.block_mate = e->d_step_mate + g.step_first;
      const int rc = kFamilies[g.spec].launch(g.step_count, g.step_lds, st, &b, &out);
      return rc == 0 ? SGRL_OK : fail(SGRL_ERR_HIP, std::string("fixed-dimension step kernel launch failed: ") + hipGetErrorString((hipError_t)rc));
    }
    hipLaunchKernelGGL(pick(g), dim3(g.count), dim3(64), g.lds, st, a, out);
    return SGRL_OK;
  };
  if (e->groups.size() == 1) {
    const int rc = launch(e->groups[0], e->args, user);
    if (rc != SGRL_OK) return rc;
  } else {
    if (!e->groups_checked && sgrl_streams::enabled()) {
      // first multi-group launch: every group's stream on its own hardware queue, as far as the runtime has them
      // (stream_pick.h; the caller's stream only waits meanwhile, so it may share a queue with a group)
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(user, &cap);
      if (cap == hipStreamCaptureStatusNone) {
        std::vector<hipStream_t> taken;
        for (auto& g : e->groups) {
          if (!taken.empty()) g.stream = sgrl_streams::pick(taken, g.stream, 6);
          taken.push_back(g.stream);
        }
        e->groups_checked = true;
      }
    }
    if (hipEventRecord(e->fork, user) != hipSuccess) return fail(SGRL_ERR_HIP, "hipEventRecord(fork) failed");
    for (auto& g : e->groups) {
      BatchArgs a = e->args;
      a.block_env = e->args.block_env + g.first;
      if (hipStreamWaitEvent(g.stream, e->fork, 0) != hipSuccess) return fail(SGRL_ERR_HIP, "hipStreamWaitEvent(fork) failed");
      const int rc = launch(g, a, g.stream);
      if (rc != SGRL_OK) return rc;
      if (hipEventRecord(g.done, g.stream) != hipSuccess || hipStreamWaitEvent(user, g.done, 0) != hipSuccess)
        return fail(SGRL_ERR_HIP, "cannot join a launch group back to the caller's stream");
    }
  }
  {
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(SGRL_ERR_HIP, std::string("kernel launch failed (") + hipGetErrorName(le) + ": " + hipGetErrorString(le) + ")");
  }
  return SGRL_OK;
}
}  // namespace


// ---- replay push: the rows of ReplayBuffer.add_transition, one launch -----------------------------------------------------
// block[e] = obs[o] | action[a] | next_obs[o] | reward | done | store | morph_id (floats; sgrl.h sgrl_pack_transitions).  A null
// source leaves its columns as they are (the observation half is written before the step overwrites the observation buffer, the
// rest after it).  HBM-bound copy: one workgroup per environment, consecutive lanes on consecutive floats of the row.
struct PackArgs {
  const float* obs; const float* act; const float* nxt; const float* rew; const float* done_f; const uint8_t* done_u8;
  const uint8_t* store; const int64_t* morph; float* block;
  int ld_obs, ld_act, ld_nxt, o, a;
};
__global__ __launch_bounds__(256) void k_pack_transitions(PackArgs p) {
  const size_t e = blockIdx.x;
  const int row = 2 * p.o + p.a + 4;
  float* b = p.block + e * row;
  for (int c = threadIdx.x; c < row; c += 256) {
    if (c < p.o) {
      if (p.obs) b[c] = p.obs[e * p.ld_obs + c];
    } else if (c < p.o + p.a) {
      if (p.act) b[c] = p.act[e * p.ld_act + (c - p.o)];
    } else if (c < 2 * p.o + p.a) {
      if (p.nxt) b[c] = p.nxt[e * p.ld_nxt + (c - p.o - p.a)];
    } else {
      const int k = c - 2 * p.o - p.a;
      if (k == 0) { if (p.rew) b[c] = p.rew[e]; }
      else if (k == 1) { if (p.done_f) b[c] = p.done_f[e]; else if (p.done_u8) b[c] = p.done_u8[e] ? 1.f : 0.f; }
      else if (k == 2) { if (p.store) b[c] = p.store[e] ? 1.f : 0.f; }
      else if (p.morph) b[c] = (float)p.morph[e];
    }
  }
}

// Collection-round bookkeeping of the reference's loop for all environments of a rank in ONE launch (reference src/trainer.py:205-232;
// sgrl_amd/rollout.py RoundCollector.record, which states the rule and keeps the tensor form for CPU ranks): per environment
//   done_bool = done;  if steps + 1 == max_steps: done_bool = 0, done = true            (the time limit is not a terminal state)
//   reward_buf += reward;  the FIRST finished episode's return is latched into ep_reward
//   store = !done_list;  steps += store;  done_list |= store && done
// and `all_done` (set to 1 by a one-thread launch just before) is cleared by every environment still collecting.
// One 32-bit word set from the device, on the caller's stream.  (Round 6: `hipMemsetAsync` of 4 / 8 bytes in the per-step calls below
// cost the config-5 collection step about 1 ms -- tools/diag/train_bench_ab.sh: 10.7-11.0 ms against 9.85 -- a plain launch does not.)
__global__ void k_set_word(unsigned* p, unsigned v, int n) { if ((int)threadIdx.x < n) p[threadIdx.x] = v; }

__global__ __launch_bounds__(256) void k_round_record(const float* __restrict__ reward, const uint8_t* __restrict__ done, uint8_t* done_list,
                                                      long long* ep_steps, float* ep_reward, float* reward_buf, uint8_t* store, float* done_bool,
                                                      int* all_done, int n, int max_steps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool d = done[i] != 0;
  float db = d ? 1.f : 0.f;
  const long long st = ep_steps[i];
  if (st + 1 == (long long)max_steps) { db = 0.f; d = true; }
  float rb = reward_buf[i] + reward[i];
  float er = ep_reward[i];
  if (d && er == 0.f) { er = rb; rb = 0.f; }
  ep_reward[i] = er;
  reward_buf[i] = rb;
  const bool was = done_list[i] != 0;
  store[i] = was ? 0 : 1;
  done_bool[i] = db;
  if (!was) ep_steps[i] = st + 1;
  const bool now = was || d;
  done_list[i] = now ? 1 : 0;
  if (!now) *all_done = 0;
}

// The round record that keeps EVERY episode (sgrl.h sgrl_round_record_all).  The first-episode block is k_round_record's, on the same
// state, so the episode statistics, the update count and the round end do not move; what is stored does:
//   timeout = cur_steps + 1 == max_steps;  done_bool = done && !timeout;  cur_steps = (done || timeout) ? 0 : cur_steps + 1
//   store = 1, except in a step taken after the round was already complete (`was_complete`: the `all_done` of the previous step of the
//   round, moved over by k_round_carry before this kernel clears `all_done` again)
__global__ void k_round_carry(int* all_done, int* was_complete) {
  if (threadIdx.x == 0) { *was_complete = *all_done; *all_done = 1; }
}

__global__ __launch_bounds__(256) void k_round_record_all(const float* __restrict__ reward, const uint8_t* __restrict__ done, uint8_t* done_list,
                                                          long long* ep_steps, float* ep_reward, float* reward_buf, long long* cur_steps,
                                                          uint8_t* store, float* done_bool, int* all_done, const int* was_complete, int n,
                                                          int max_steps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool raw = done[i] != 0;
  bool d = raw;
  const long long st = ep_steps[i];
  if (st + 1 == (long long)max_steps) d = true;
  float rb = reward_buf[i] + reward[i];
  float er = ep_reward[i];
  if (d && er == 0.f) { er = rb; rb = 0.f; }
  ep_reward[i] = er;
  reward_buf[i] = rb;
  const bool was = done_list[i] != 0;
  if (!was) ep_steps[i] = st + 1;
  const bool now = was || d;
  done_list[i] = now ? 1 : 0;
  if (!now) *all_done = 0;
  const long long cs = cur_steps[i];
  const bool timeout = cs + 1 == (long long)max_steps;
  done_bool[i] = (raw && !timeout) ? 1.f : 0.f;
  cur_steps[i] = (raw || timeout) ? 0 : cs + 1;
  store[i] = *was_complete ? 0 : 1;
}

// replay ingest: one workgroup per row of the gathered block; the row's morphology picks the ring, slot[] the place in it
__global__ __launch_bounds__(256) void k_ingest_rows(const float* __restrict__ block, int o, int a, const int64_t* __restrict__ slot,
                                                     const sgrl_ring* __restrict__ rings, int n_rings) {
  const size_t r = blockIdx.x;
  const long long sl = slot[r];
  if (sl < 0) return;
  const int row = 2 * o + a + 4;
  const float* b = block + r * row;
  const int k = (int)b[2 * o + a + 3];
  if (k < 0 || k >= n_rings) return;
  const sgrl_ring g = rings[k];
  for (int c = threadIdx.x; c < g.obs_dim; c += 256) {
    g.obs[(size_t)sl * g.obs_dim + c] = b[c];
    g.next_obs[(size_t)sl * g.obs_dim + c] = b[o + a + c];
  }
  for (int c = threadIdx.x; c < g.act_dim; c += 256) g.action[(size_t)sl * g.act_dim + c] = b[o + c];
  if (threadIdx.x == 0) { g.reward[sl] = b[2 * o + a]; g.done[sl] = b[2 * o + a + 1]; }
}

// Slots of a gathered block's rows in their morphologies' rings, on the device, for ANY number of rows (one rank's block or the
// learner's whole gather of N ranks: one pair of launches per step whatever N).  slot[r] = (pos[m] + rank of row r among the stored
// rows of morphology m, in row order) % cap[m]; then pos[m] advances and pending[m] grows by the rows stored.
//   k_ingest_keys: one thread per row -- key[r] = ring of a stored row, -1 otherwise (4 bytes per row, read back coalesced) and
//                  the per-ring counts of every 256-row chunk; the LAST chunk to finish (a ticket over the chunks, not the
//                  rows: a ticket every row's workgroup takes serialises 8192 atomics on one address, 0.37 ms) copies the
//                  rings' write pointers into the workspace (`base`) and advances pos[] / pending[] by the totals;
//   k_ingest_slots: one workgroup per chunk -- a row's slot = `base` of its ring + stored rows of that ring in the chunks before
//                  (the chunk counts) + in its chunk before it (the chunk's keys in LDS);
//   k_ingest_rows: one workgroup per row copies it into its ring (the copy kernel of sgrl_ingest_rows: 3.9 TB/s).
// (Round 5 first fused slots and copy into one kernel, one workgroup and then one wave per row: 0.23 / 0.14 ms for 65 536 rows --
// every row's copy waited for two dependent rounds of count loads; apart they take 0.09.)
constexpr int kIngestThreads = 256, kIngestMaxRings = 32, kIngestChunk = 256;
struct IngestWs { unsigned* ticket; long long* base; int* chunk_hist; int* key; };
__host__ __device__ inline IngestWs ingest_ws(long long* ws, int n_rows) {       // inside the caller's int64 workspace (include/sgrl.h)
  const int n_chunks = (n_rows + kIngestChunk - 1) / kIngestChunk;
  IngestWs w;
  w.ticket = reinterpret_cast<unsigned*>(ws);
  w.base = ws + 1;                                                 // [32] write pointers before this block
  w.chunk_hist = reinterpret_cast<int*>(ws + 1 + kIngestMaxRings);  // [n_chunks][32]
  w.key = w.chunk_hist + n_chunks * kIngestMaxRings;               // [n_rows]
  return w;
}
__host__ __device__ inline int ingest_ws_words(int n_rows) {      // int64 words of ticket + base + counts + keys (the slots follow)
  const int n_chunks = (n_rows + kIngestChunk - 1) / kIngestChunk;
  return 1 + kIngestMaxRings + (n_chunks * kIngestMaxRings + n_rows + 1) / 2;
}
__global__ __launch_bounds__(kIngestThreads) void k_ingest_keys(const float* __restrict__ block, int n_rows, int o, int a, int n_rings,
                                                                long long* pos, const long long* __restrict__ cap, long long* pending,
                                                                long long* ws) {
  __shared__ int hist[kIngestMaxRings];
  __shared__ unsigned last_sh;
  const IngestWs w = ingest_ws(ws, n_rows);
  const int t = threadIdx.x, r = blockIdx.x * kIngestChunk + t;
  if (t < kIngestMaxRings) hist[t] = 0;
  __syncthreads();
  if (r < n_rows) {
    const float* b = block + (size_t)r * (2 * o + a + 4) + 2 * o + a;
    const int m = (int)b[3];
    const int k = (b[2] > 0.5f && m >= 0 && m < n_rings) ? m : -1;
    w.key[r] = k;
    if (k >= 0) atomicAdd(&hist[k], 1);
  }
  __syncthreads();
  if (t < kIngestMaxRings) w.chunk_hist[blockIdx.x * kIngestMaxRings + t] = hist[t];
  __syncthreads();
  if (t == 0) { __threadfence(); last_sh = atomicAdd(w.ticket, 1u) == gridDim.x - 1 ? 1u : 0u; }
  __syncthreads();
  if (last_sh) {                                   // every chunk's counts are in memory
    __threadfence();
    // totals per ring: thread (ring t & 31, group t >> 5) sums every eighth chunk, the eight partial sums meet in LDS (one thread
    // per ring walking all chunks was a chain of 256 dependent-latency loads for the 65 536 rows of an N = 8 step)
    __shared__ int part[kIngestThreads / kIngestMaxRings][kIngestMaxRings];
    {
      const int ring = t & (kIngestMaxRings - 1), grp = t / kIngestMaxRings;
      int p = 0;
      for (int g = grp; g < (int)gridDim.x; g += kIngestThreads / kIngestMaxRings) p += w.chunk_hist[g * kIngestMaxRings + ring];
      part[grp][ring] = p;
    }
    __syncthreads();
    if (t < n_rings) {
      long long total = 0;
#pragma unroll
      for (int g = 0; g < kIngestThreads / kIngestMaxRings; g++) total += part[g][t];
      const long long p0 = pos[t];
      w.base[t] = p0;
      pos[t] = (p0 + total) % cap[t];
      pending[t] += total;
    }
    if (t == 0) *w.ticket = 0u;                    // the workspace is ready for the next call (zeroed once by the host side)
  }
}
// slots of the rows of one 256-row chunk: prefix of the chunk counts before it (per ring) + the row's rank inside the chunk
__global__ __launch_bounds__(kIngestThreads) void k_ingest_slots(int n_rows, const long long* __restrict__ cap, long long* ws, long long* __restrict__ slot) {
  __shared__ int keys[kIngestChunk];
  __shared__ int part[8][kIngestMaxRings];
  const IngestWs w = ingest_ws(ws, n_rows);
  const int t = threadIdx.x, c = blockIdx.x, r = c * kIngestChunk + t;
  const int k = r < n_rows ? w.key[r] : -1;
  keys[t] = k;
  {     // thread (ring t & 31, lane group t >> 5) sums its share of the chunks before c
    const int ring = t & 31, grp = t >> 5;
    int p = 0;
    for (int g = grp; g < c; g += 8) p += w.chunk_hist[g * kIngestMaxRings + ring];
    part[grp][ring] = p;
  }
  __syncthreads();
  long long sl = -1;
  if (k >= 0) {
    int rank = 0;
#pragma unroll
    for (int g = 0; g < 8; g++) rank += part[g][k];
    for (int j = 0; j < t; j++) rank += keys[j] == k ? 1 : 0;
    sl = (w.base[k] + rank) % cap[k];
  }
  if (r < n_rows) slot[r] = sl;
}

extern "C" {

const char* sgrl_last_error(void) { return g_err.c_str(); }
const char* sgrl_version(void) { return "sgrl-hip 0.2.0 (gfx950)"; }     // 0.2.0: sgrl_ingest_ws_words; sgrl_ingest_block zeroes its ticket itself
#ifdef SGRL_PHASE_PROF
int sgrl_phase_prof(unsigned long long* host, int n_env, int reset) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (host && hipMemcpyFromSymbol(host, HIP_SYMBOL(sgrl_engine_dev::g_phase_prof), sizeof(unsigned long long) * 16 * (size_t)n_env) != hipSuccess) return -2;
  if (reset) { static unsigned long long z[16 * 65536]; if (hipMemcpyToSymbol(HIP_SYMBOL(sgrl_engine_dev::g_phase_prof), z, sizeof(z)) != hipSuccess) return -3; }
  return 0;
}
#endif

// kflags: bit 0 half-wave policy, bit 1 explicit-inverse path, bit 2 lane-read form, bit 3 chol_inv_packed alone
static int debug_chol_run(const char* who, int kflags, const int32_t* n, const double* C, const double* rhs, double* C_out, double* x_out, int32_t* ok) {
  constexpr int LD = SGRL_DEBUG_CHOL_LD;
  const std::string name(who);
  if (!n || !C || !rhs || !C_out || !x_out || !ok) return fail(SGRL_ERR_ARG, name + ": null pointer");
  for (int p = 0; p < ((kflags & 1) ? 2 : 1); p++)
    if (n[p] < 0 || n[p] * (n[p] + 1) / 2 > LD) return fail(SGRL_ERR_ARG, name + ": n out of range");
  const size_t bytes = sizeof(double) * (4 * LD + 128) + sizeof(int32_t) * 4;
  char* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, bytes));
  double* dC = (double*)d; double* dCo = dC + 2 * LD; double* dr = dCo + 2 * LD; double* dx = dr + 64;
  int32_t* dn = (int32_t*)(dx + 64); int32_t* dok = dn + 2;
  const int32_t n2[2] = {n[0], (kflags & 1) ? n[1] : 0};
  hipError_t e = hipMemset(d, 0, bytes);
  if (e == hipSuccess) e = hipMemcpy(dC, C, sizeof(double) * 2 * LD, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dr, rhs, sizeof(double) * 64, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dn, n2, sizeof(n2), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    k_debug_chol_solve<<<1, 64>>>(kflags, dn, dC, dr, dCo, dx, dok);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(C_out, dCo, sizeof(double) * 2 * LD, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(x_out, dx, sizeof(double) * 64, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ok, dok, sizeof(int32_t) * 2, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(SGRL_ERR_HIP, name + ": " + hipGetErrorString(e));
  return SGRL_OK;
}

int sgrl_debug_chol_solve(int flags, const int32_t* n, const double* C, const double* rhs, double* C_out, double* x_out, int32_t* ok) {
  return debug_chol_run("sgrl_debug_chol_solve", flags & 3, n, C, rhs, C_out, x_out, ok);
}
int sgrl_debug_chol_solve_form(int form, int flags, const int32_t* n, const double* C, const double* rhs, double* C_out, double* x_out, int32_t* ok) {
  if (form != 0 && form != 1) return fail(SGRL_ERR_ARG, "sgrl_debug_chol_solve_form: form must be 0 or 1");
  return debug_chol_run("sgrl_debug_chol_solve_form", (flags & 3) | (form ? 0 : 4), n, C, rhs, C_out, x_out, ok);
}
int sgrl_debug_chol_inv(int form, int policy, const int32_t* n, const double* C, double* C_out, int32_t* ok) {
  if (form != 0 && form != 1) return fail(SGRL_ERR_ARG, "sgrl_debug_chol_inv: form must be 0 or 1");
  const double rhs[64] = {0};
  double x_out[64];
  return debug_chol_run("sgrl_debug_chol_inv", (policy & 1) | 8 | (form ? 0 : 4), n, C, rhs, C_out, x_out, ok);
}

void sgrl_engine_destroy(sgrl_engine* e) {
  if (!e) return;
  for (auto p : e->d_ib) if (p) (void)hipFree(p);
  for (auto p : e->d_fb) if (p) (void)hipFree(p);
  if (e->d_morphs) (void)hipFree(e->d_morphs);
  if (e->d_env_morph) (void)hipFree(e->d_env_morph);
  if (e->d_block_env) (void)hipFree(e->d_block_env);
  if (e->d_step_env) (void)hipFree(e->d_step_env);
  if (e->d_step_mate) (void)hipFree(e->d_step_mate);
  if (e->d_rec) (void)hipFree(e->d_rec);
  if (e->d_cnt) (void)hipFree(e->d_cnt);
  if (e->d_scratch) (void)hipFree(e->d_scratch);
  if (e->d_cam_dist) (void)hipFree(e->d_cam_dist);
  for (auto& g : e->groups) { if (g.stream) (void)hipStreamDestroy(g.stream); if (g.done) (void)hipEventDestroy(g.done); }
  if (e->fork) (void)hipEventDestroy(e->fork);
  delete e;
}

int sgrl_engine_create(int n_morph, const int32_t* const* ib, const int32_t* ib_len, const double* const* fb,
                       const int32_t* fb_len, const int32_t* morph_count, int obs_max_len, int action_max_len,
                       uint64_t seed, uint32_t env_id_base, int max_episode_steps, sgrl_engine** out) {
  if (!out) return fail(SGRL_ERR_ARG, "out is null");
  *out = nullptr;
  if (n_morph <= 0 || !ib || !ib_len || !fb || !fb_len || !morph_count) return fail(SGRL_ERR_ARG, "null or empty morphology list");
  int ndev = 0;
  (void)hipGetLastError();
  const hipError_t dev_err = hipGetDeviceCount(&ndev);
  if (dev_err != hipSuccess || ndev == 0)
    return fail(SGRL_ERR_HIP, std::string("no HIP device visible: libsgrl_hip.so needs an MI355X (there is no CPU fallback) [") +
                                  hipGetErrorString(dev_err) + ", " + std::to_string(ndev) + " devices]");
  sgrl_engine* e = new sgrl_engine();
  e->n_morph = n_morph;
  e->obs_max_len = obs_max_len;
  e->action_max_len = action_max_len;
  std::vector<int32_t> env_morph;
  std::vector<MorphDev> morphs(n_morph);
  e->d_ib.assign(n_morph, nullptr);
  e->d_fb.assign(n_morph, nullptr);
  int rc = SGRL_OK;
  for (int k = 0; k < n_morph && rc == SGRL_OK; k++) {
    SgrlModelView v;
    if (!ib[k] || !fb[k] || ib_len[k] < SGRL_NHDR || sgrl_model_view(ib[k], fb[k], &v) != 0) { rc = fail(SGRL_ERR_MODEL, "bad magic in model blob " + std::to_string(k)); break; }
    if (v.n_int != ib_len[k] || v.n_f64 != fb_len[k]) { rc = fail(SGRL_ERR_MODEL, "model blob " + std::to_string(k) + " has unexpected length"); break; }
    if (v.nv > 64 || v.nbody > 64 || v.npair > 64) { rc = fail(SGRL_ERR_LIMIT, "morphology exceeds 64 dofs/bodies/pairs"); break; }
    if ((v.nv | 1) > sgrl::kSlabLdy || ib[k][SGRL_H_MAX_ROWS] > sgrl::kSlabRows) { rc = fail(SGRL_ERR_LIMIT, "morphology exceeds the HBM constraint slab (nv <= 46, max_rows <= 256)"); break; }
    e->scratch_stride = std::max(e->scratch_stride, sgrl::slab_doubles(ib[k][SGRL_H_MAX_ROWS], v.nv | 1));
    e->max_geoms = std::max(e->max_geoms, v.ngeom);
    const int L = v.nbody - 1;
    if (41 * L > obs_max_len || 3 * L > action_max_len) { rc = fail(SGRL_ERR_ARG, "obs_max_len/action_max_len too small for morphology " + std::to_string(k)); break; }
    if (morph_count[k] < 0) { rc = fail(SGRL_ERR_ARG, "negative morph_count"); break; }
    sgrl::Layout o;
    sgrl::make_layout(ib[k], &o, v.n_int, SGRL_STAGE_FLOATS ? v.n_f64 : 0);
    // kinematics and the bias forces park per-joint / per-body / per-dof temporaries in the (then dead) constraint-row block
    if (17 * v.njnt + 7 * v.nbody > (o.lrows + 1) * o.ldy || 6 * v.nv > (o.lrows + 1) * o.ldy) {
      rc = fail(SGRL_ERR_LIMIT, "model " + std::to_string(k) + ": the constraint-row block is too small for the kinematics scratch (17 njnt + 7 nbody doubles)");
      break;
    }
    const int bytes = sgrl::layout_bytes(&o);
    if (bytes > 160 * 1024) { rc = fail(SGRL_ERR_LIMIT, "per-environment LDS slab exceeds 160 KiB"); break; }
    if (bytes > e->lds_bytes) e->lds_bytes = bytes;
    e->morph_lds.push_back(bytes);
    const int need = v.nq + v.nv + 4;
    if (need > e->stride) e->stride = need;
    for (int i = 0; i < morph_count[k]; i++) env_morph.push_back(k);
    if (hipMalloc(&e->d_ib[k], sizeof(int32_t) * ib_len[k]) != hipSuccess || hipMalloc(&e->d_fb[k], sizeof(double) * fb_len[k]) != hipSuccess) { rc = fail(SGRL_ERR_HIP, "hipMalloc(model) failed"); break; }
    (void)hipMemcpy(e->d_ib[k], ib[k], sizeof(int32_t) * ib_len[k], hipMemcpyHostToDevice);
    (void)hipMemcpy(e->d_fb[k], fb[k], sizeof(double) * fb_len[k], hipMemcpyHostToDevice);
    morphs[k].ib = e->d_ib[k];
    morphs[k].fb = e->d_fb[k];
    morphs[k].slot = -1;
    morphs[k].pad_ = 0;
  }
  if (rc == SGRL_OK && env_morph.empty()) rc = fail(SGRL_ERR_ARG, "no environments requested");
  if (rc != SGRL_OK) { sgrl_engine_destroy(e); return rc; }
  e->n_env = (int)env_morph.size();
  e->stride = (e->stride + 1) & ~1;
  bool ok = hipMalloc(&e->d_morphs, sizeof(MorphDev) * n_morph) == hipSuccess &&
            hipMalloc(&e->d_env_morph, sizeof(int32_t) * e->n_env) == hipSuccess &&
            hipMalloc(&e->d_block_env, sizeof(int32_t) * e->n_env) == hipSuccess &&
            hipMalloc(&e->d_step_env, sizeof(int32_t) * e->n_env) == hipSuccess &&
            hipMalloc(&e->d_step_mate, sizeof(int32_t) * e->n_env) == hipSuccess &&
            hipMalloc(&e->d_rec, sizeof(double) * (size_t)e->n_env * e->stride) == hipSuccess &&
            hipMalloc(&e->d_cnt, sizeof(int32_t) * (size_t)e->n_env * 4) == hipSuccess &&
            hipMalloc(&e->d_scratch, sizeof(double) * (size_t)e->n_env * e->scratch_stride) == hipSuccess &&
            hipMalloc(&e->d_cam_dist, sizeof(double) * n_morph) == hipSuccess;
  if (!ok) { sgrl_engine_destroy(e); return fail(SGRL_ERR_HIP, "hipMalloc(state) failed"); }
  e->cam_dist.assign(n_morph, std::nan(""));
  (void)hipMemset(e->d_cam_dist, 0, sizeof(double) * n_morph);
  // a record is stride doubles for every morphology, a lighter one uses fewer: the padding is defined (sgrl_get_records copies it out)
  (void)hipMemset(e->d_rec, 0, sizeof(double) * (size_t)e->n_env * e->stride);
  (void)hipMemcpy(e->d_morphs, morphs.data(), sizeof(MorphDev) * n_morph, hipMemcpyHostToDevice);
  (void)hipMemcpy(e->d_env_morph, env_morph.data(), sizeof(int32_t) * e->n_env, hipMemcpyHostToDevice);
  {
    // dispatch order: group by LDS occupancy class (fewest workgroups per CU first = costliest), inside a group the
    // morphologies with the most dofs first -- workgroups are handed out by index, this balances the tail
    std::vector<int32_t> order(e->n_env);
    for (int i = 0; i < e->n_env; i++) order[i] = i;
    // Fixed-dimension kernels (step_spec.hip): when every morphology of the batch has an instance and the batch spans few
    // families, each family present becomes ONE launch group on its kernel -- layout offsets as immediates (8192 x walker_7:
    // 4.5-4.8 -> 4.0-4.3 ms), and the light families (nv <= 12) at the register budget of four waves per SIMD (8192 x
    // walker_3: 1.73-1.83 -> 1.40-1.49 ms; profiles/r3_variant_probe_specs.log).  SGRL_SPECS=0: never, =1: whenever every
    // morphology has an instance.
    std::vector<int> spec(n_morph, -1);       // family of the morphology
    std::vector<int> pair_lds(n_morph, 0);    // > 0: the morphology's environments step two to a wavefront on a slab pair of this size
    std::vector<int> spec_lds(n_morph, 0);    // the slab on the morphology's fixed-dimension step kernel (smaller where the family reads the int tables from global memory)
    bool use_specs = false;
    {
      const char* sm = getenv("SGRL_SPECS");
      constexpr int kMaxSpecGroups = 4;
      if (!(sm && sm[0] == '0') && kNumMembers > 0) {
        // a batch made of light dimension sets only runs on the light kernels (four waves per SIMD), any other on the kernels
        // that hold every dimension set of a family (two waves per SIMD): one launch per family present
        bool all_light = true, all = true;
        // (in a MIXED batch the light dimension sets stay on the family kernel: as a second, concurrent dispatch on their four-waves-
        // per-SIMD kernel they measured 4-9 % slower, with and without stream priorities -- profiles/r4_mix_light_probe.txt,
        // r5_mix_prio_probe.txt)
        for (int k = 0; k < n_morph; k++) if (morph_count[k] > 0) all_light = all_light && spec_for(ib[k], 4) >= 0;
        // Two environments per wavefront (wave_half.h) where the family kernel holds the set's half-wave instance AND the slab pair
        // still fits eight workgroups per CU (the register budget's count): walker_2 / walker_3 / hopper_3.  SGRL_PAIR=0: never.
        const char* pe = getenv("SGRL_PAIR");
        auto pair_bytes = [&](int k) -> int {
          const int m2 = spec_for(ib[k], 2);
          if (m2 < 0 || !kMembers[m2].dims[11] || (pe && pe[0] == '0')) return 0;
          SgrlModelView v;
          (void)sgrl_model_view(ib[k], fb[k], &v);
          sgrl::Layout po;
          sgrl::make_layout(ib[k], &po, v.n_int, 0, true);
          const int pb = sgrl::layout_bytes(&po);
          // what lives in the Y block before the rows are built: kinematics scratch, and crb (10 doubles per body, pair layouts only)
          const bool scratch_ok = 17 * v.njnt + 7 * v.nbody <= (po.lrows + 1) * po.ldy && 6 * v.nv <= (po.lrows + 1) * po.ldy &&
                                  10 * v.nbody <= (po.lrows + 1) * po.ldy && v.nv <= 15;
          return (sgrl::workgroups_per_cu(pb) >= 8 && scratch_ok) ? pb : 0;
        };
        // An all-light batch whose every morphology pairs (and has at least two environments) takes the FAMILY kernels too: eight
        // wavefronts of two environments per CU beat sixteen wavefronts of one on the four-waves-per-SIMD light kernel (8192 x
        // walker_3 1.44 -> 1.14 ms, walker_2 1.32 -> 0.99, hopper_3 1.73 -> 1.25: profiles/r5_light_pair_probe.txt).
        // (SGRL_PAIR=0 keeps such a batch on the light kernels.)
        if (all_light) {
          bool all_pair = true;
          for (int k = 0; k < n_morph; k++) if (morph_count[k] > 0) all_pair = all_pair && morph_count[k] >= 2 && pair_bytes(k) > 0;
          if (all_pair) all_light = false;
        }
        std::vector<int> distinct;
        for (int k = 0; k < n_morph; k++) {
          if (morph_count[k] == 0) continue;
          int mb = spec_for(ib[k], all_light ? 4 : 2);
          all = all && mb >= 0;
          if (mb < 0) continue;
          spec[k] = kMembers[mb].family;
          morphs[k].slot = kMembers[mb].slot;
          spec_lds[k] = e->morph_lds[k];
          if (kFamilies[spec[k]].itab_global) {
            SgrlModelView v;
            (void)sgrl_model_view(ib[k], fb[k], &v);
            sgrl::Layout so;
            sgrl::make_layout(ib[k], &so, 0, SGRL_STAGE_FLOATS ? v.n_f64 : 0);      // what setup<D>() of that kernel computes
            if (17 * v.njnt + 7 * v.nbody <= (so.lrows + 1) * so.ldy && 6 * v.nv <= (so.lrows + 1) * so.ldy) spec_lds[k] = sgrl::layout_bytes(&so);
            else all = false;                                                       // (never on the shipped assets)
          }
          if (kMembers[mb].dims[11]) pair_lds[k] = pair_bytes(k);      // (the light kernels hold no half-wave instances: flag 0)
          if (std::find(distinct.begin(), distinct.end(), spec[k]) == distinct.end()) distinct.push_back(spec[k]);
        }
        use_specs = all && ((sm && sm[0] == '1') || (int)distinct.size() <= kMaxSpecGroups);
      }
      (void)hipMemcpy(e->d_morphs, morphs.data(), sizeof(MorphDev) * n_morph, hipMemcpyHostToDevice);    // with the slots
    }
    if (use_specs) {
      // heavy families first; inside a family the costliest dimension set (most dofs) first (interleaved sets and lightest-first were
      // measured: walker mix 2.20 -> 2.71-2.87 ms, profiles/r4_order_probe.txt and LAB_LOG round 5)
      std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        const int mx = env_morph[x], my = env_morph[y];
        if (spec[mx] != spec[my]) {
          const int wx = kFamilies[spec[mx]].waves, wy = kFamilies[spec[my]].waves;
          return wx != wy ? wx < wy : spec[mx] < spec[my];
        }
        return ib[mx][SGRL_H_NV] > ib[my][SGRL_H_NV];
      });
      (void)hipMemcpy(e->d_block_env, order.data(), sizeof(int32_t) * e->n_env, hipMemcpyHostToDevice);
      std::vector<int32_t> step_env, step_mate;
      // (Launching a family's LDS classes as separate dispatches of the same kernel -- so that the lighter sets are not dragged to the
      // heaviest member's residency -- loses 15-20 % like every two-queue form: profiles/r5_split_class_probe.txt.)
      constexpr bool split_class = false;
      auto cls_of = [&](int k) { return sgrl::workgroups_per_cu(std::max(spec_lds[k], pair_lds[k])); };
      for (int i = 0; i < e->n_env;) {
        sgrl_engine::Group g;
        g.first = i;
        g.spec = spec[env_morph[order[i]]];
        g.step_first = (int)step_env.size();
        const int g_cls = cls_of(env_morph[order[i]]);
        while (i < e->n_env && spec[env_morph[order[i]]] == g.spec && (!split_class || cls_of(env_morph[order[i]]) == g_cls)) {
          const int k = env_morph[order[i]];
          g.lds = std::max(g.lds, e->morph_lds[k]);
          g.step_lds = std::max(g.step_lds, spec_lds[k]);
          // consecutive environments of a pairable morphology share a workgroup; an odd one out steps alone
          if (pair_lds[k] > 0 && i + 1 < e->n_env && env_morph[order[i + 1]] == k) {
            step_env.push_back(order[i]); step_mate.push_back(order[i + 1]);
            g.step_lds = std::max(g.step_lds, pair_lds[k]);
            e->n_paired += 2;
            i += 2;
          } else {
            step_env.push_back(order[i]); step_mate.push_back(-1);
            i++;
          }
        }
        // diagnostics only (tools/occupancy_sweep.py): SGRL_LDS_PAD=<bytes> inflates the dynamic LDS requests to force fewer residents
        if (const char* pad = getenv("SGRL_LDS_PAD")) { g.lds += atoi(pad); g.step_lds += atoi(pad); e->lds_bytes = std::max(e->lds_bytes, g.lds); }
        g.count = i - g.first;
        g.step_count = (int)step_env.size() - g.step_first;
        e->lds_bytes = std::max(e->lds_bytes, std::max(g.step_lds, g.lds));
        e->groups.push_back(g);
      }
      (void)hipMemcpy(e->d_step_env, step_env.data(), sizeof(int32_t) * step_env.size(), hipMemcpyHostToDevice);
      (void)hipMemcpy(e->d_step_mate, step_mate.data(), sizeof(int32_t) * step_mate.size(), hipMemcpyHostToDevice);
    } else {
      std::vector<int> cost(n_morph), cls(n_morph);
      // A batch made of light morphologies ONLY (few dofs, small slabs: walker_2/3/4, hopper_3/4) runs on k_env_step_light, three
      // waves per SIMD: measured -20 % (8192 x walker_2: 1.96 -> 1.57 ms, walker_4: 2.74 -> 2.20 ms).  In a MIXED batch the light
      // class as a second concurrent dispatch LOSES (walker mix 2.84 -> 3.18 ms, hopper++ 1.59 -> 1.78 ms): 168- and 235-register
      // waves fragment the register file of a SIMD (1 heavy + 1 light instead of 3 light), so the light waves pay for their 31
      // spilled registers without getting the occupancy -- mixed batches therefore stay on the one kernel.  SGRL_LIGHT=0: never.
      bool light_batch = true;
      for (int k = 0; k < n_morph; k++) {
        cost[k] = ib[k][SGRL_H_NV];
        // LDS is handed out in 1280-byte granules (measured with tools/occupancy_probe.py: a 27 064-byte slab fits five
        // times into the 160 KB of a CU, not six)
        const int granule = 1280;
        int per_cu = (160 * 1024) / (((e->morph_lds[k] + granule - 1) / granule) * granule);
        cls[k] = per_cu > 8 ? 8 : per_cu;   // register budget (<= 256 VGPRs): two waves per SIMD = 8 workgroups per CU at most
        light_batch = light_batch && ib[k][SGRL_H_NV] <= kLightNv && per_cu >= kLightPerCu;
      }
      if (light_batch) for (int k = 0; k < n_morph; k++) cls[k] = kLightPerCu;
      std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        const int mx = env_morph[x], my = env_morph[y];
        if (cls[mx] != cls[my]) return cls[mx] < cls[my];
        return cost[mx] > cost[my];
      });
      (void)hipMemcpy(e->d_block_env, order.data(), sizeof(int32_t) * e->n_env, hipMemcpyHostToDevice);
      for (int i = 0; i < e->n_env;) {
        sgrl_engine::Group g;
        g.first = i;
        // A batch whose costliest class already has 6+ workgroups per CU runs that class and the next as ONE dispatch:
        // losing one of seven or eight workgroups on the lighter morphologies costs nothing measurable (walker mix: one
        // dispatch at 7 per CU is as fast as two at 7 and 8).  Batches with heavier members (humanoid 5-6, cheetah 3-4 per
        // CU) keep one dispatch per class: measured 7 % faster on the 23-morphology cwhh batch.
        const int c = cls[env_morph[order[i]]];
        const int c_min = cls[env_morph[order[0]]];
        int top = (c == c_min && c >= 6) ? c + 1 : c;
        if (top >= kLightPerCu) top = kLightPerCu;            // the light class never merges with a heavier one ...
        else if (top > 8) top = 8;                            // ... nor a heavier one with it
        g.light = c == kLightPerCu;
        while (i < e->n_env && cls[env_morph[order[i]]] <= top) { g.lds = std::max(g.lds, e->morph_lds[env_morph[order[i]]]); i++; }
        // diagnostics only (tools/occupancy_sweep.py): SGRL_LDS_PAD=<bytes> inflates the dynamic LDS request to force fewer
        // resident workgroups per CU
        if (const char* pad = getenv("SGRL_LDS_PAD")) { g.lds += atoi(pad); e->lds_bytes = std::max(e->lds_bytes, g.lds); }
        g.count = i - g.first;
        e->groups.push_back(g);
      }
    }
    if (e->groups.size() > 1) {
      bool sok = hipEventCreateWithFlags(&e->fork, hipEventDisableTiming) == hipSuccess;
      // The group streams are PLAIN non-blocking streams.  Round 1 gave the heavy groups higher stream priorities (their
      // workgroups then all start at once and the light ones fill the gaps: k_env_step alone 5..10 % faster on mixed
      // batches), but on this ROCm (7.2) the mere existence of hipStreamCreateWithPriority streams in a process corrupts
      // LATER hipGraph captures -- work enqueued shortly before a capture is recorded into the graph a second time (the TD3
      // update graphs of train_loop.py replayed at 45..60 ms instead of 13..24 ms; tools/diag/train_time_probe3.py) -- and
      // the priorities also slowed the SET forward that follows the step (humanoid mix: step + forward 7.4 ms with, 6.1 ms
      // without).  SGRL_GROUP_PRIO=1 restores them for engine-only experiments.
      int prio_least = 0, prio_greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);   // numerically lower = higher priority
      constexpr bool use_prio = false;
      int gi = 0;
      for (auto& g : e->groups) {
        int prio = prio_greatest + gi++;
        if (prio > prio_least) prio = prio_least;
        const hipError_t se = use_prio ? hipStreamCreateWithPriority(&g.stream, hipStreamNonBlocking, prio)
                                       : hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking);
        sok = sok && se == hipSuccess && hipEventCreateWithFlags(&g.done, hipEventDisableTiming) == hipSuccess;
      }
      if (!sok) { sgrl_engine_destroy(e); return fail(SGRL_ERR_HIP, "cannot create launch-group streams"); }
    }
  }
  {
    std::vector<int32_t> cnt0((size_t)e->n_env * 4, 0);
    for (int i = 0; i < e->n_env; i++) cnt0[4 * (size_t)i + 1] = -1;  // episode = -1: the first reset bumps it to 0
    (void)hipMemcpy(e->d_cnt, cnt0.data(), sizeof(int32_t) * cnt0.size(), hipMemcpyHostToDevice);
  }
  {
    // hipFuncAttributeMaxDynamicSharedMemorySize is kept per kernel AND per device: only ever RAISE it (a second engine with a
    // smaller slab must not lower the limit under the first one's launches), and remember what was raised on WHICH device
    static int g_lds_limit[64];
    static bool g_lds_init = false;
    if (!g_lds_init) { for (int& v : g_lds_limit) v = 48 * 1024; g_lds_init = true; }
    int dev = 0;
    (void)hipGetDevice(&dev);
    int& limit = g_lds_limit[dev >= 0 && dev < 64 ? dev : 0];
    if (e->lds_bytes > limit) {
      hipError_t a1 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_env_step), hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes);
      hipError_t a2 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_env_reset), hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes);
      hipError_t a3 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_env_refresh), hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes);
      hipError_t a4 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_env_step_light), hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes);
      if (a1 != hipSuccess || a2 != hipSuccess || a3 != hipSuccess || a4 != hipSuccess) { sgrl_engine_destroy(e); return fail(SGRL_ERR_HIP, "cannot raise the dynamic LDS limit"); }
      limit = e->lds_bytes;
    }
  }
  BatchArgs& a = e->args;
  a.morphs = e->d_morphs; a.env_morph = e->d_env_morph; a.block_env = e->d_block_env; a.rec = e->d_rec; a.cnt = e->d_cnt; a.scratch = e->d_scratch;
  a.scratch_stride = e->scratch_stride;
  a.stride = e->stride; a.n_env = e->n_env; a.obs_max_len = obs_max_len; a.action_max_len = action_max_len;
  a.seed = seed; a.env_id_base = env_id_base; a.max_episode_steps = max_episode_steps;
  if (hipDeviceSynchronize() != hipSuccess) { sgrl_engine_destroy(e); return fail(SGRL_ERR_HIP, "device error during engine setup"); }
  *out = e;
  return SGRL_OK;
}

int sgrl_num_envs(const sgrl_engine* e) { return e ? e->n_env : SGRL_ERR_ARG; }
int sgrl_record_stride(const sgrl_engine* e) { return e ? e->stride : SGRL_ERR_ARG; }
// What the STEP kernels are launched with (sgrl.h): a family kernel that reads the int tables from global memory runs on a smaller
// slab than k_env_reset / k_env_refresh of the same engine, whose request e->lds_bytes also covers.
int sgrl_lds_bytes(const sgrl_engine* e) {
  if (!e) return SGRL_ERR_ARG;
  int b = 0;
  for (const auto& g : e->groups) b = std::max(b, g.spec >= 0 ? g.step_lds : g.lds);
  return b;
}
int sgrl_launch_groups(const sgrl_engine* e) { return e ? (int)e->groups.size() : SGRL_ERR_ARG; }
int sgrl_paired_envs(const sgrl_engine* e) { return e ? e->n_paired : SGRL_ERR_ARG; }
int sgrl_fixed_dim_groups(const sgrl_engine* e) {
  if (!e) return SGRL_ERR_ARG;
  int n = 0;
  for (const auto& g : e->groups) n += g.spec >= 0 ? 1 : 0;
  return n;
}

int sgrl_reset(sgrl_engine* e, float* obs, double* obs64, void* stream) {
  if (!e || !obs) return fail(SGRL_ERR_ARG, "sgrl_reset: null engine or obs");
  StepOut out{};
  out.obs32 = obs; out.obs64 = obs64;
  return launch_groups(e, k_env_reset, out, (hipStream_t)stream);
}

int sgrl_reset_where(sgrl_engine* e, const uint8_t* mask, float* obs, double* obs64, void* stream) {
  if (!e || !mask || !obs) return fail(SGRL_ERR_ARG, "sgrl_reset_where: null engine, mask or obs");
  StepOut out{};
  out.obs32 = obs; out.obs64 = obs64;
  out.done = const_cast<uint8_t*>(mask);     // read only: k_env_reset takes its mask here
  return launch_groups(e, k_env_reset, out, (hipStream_t)stream);
}

int sgrl_step(sgrl_engine* e, const float* actions, float* obs, float* reward, uint8_t* done, float* dist,
              uint8_t* truncated, double* obs64, double* reward64, int auto_reset, void* stream) {
  if (!e || !actions || !obs) return fail(SGRL_ERR_ARG, "sgrl_step: null engine, actions or obs");
  StepOut out{};
  out.actions = actions; out.obs32 = obs; out.obs64 = obs64; out.reward = reward; out.reward64 = reward64;
  out.done = done; out.dist = dist; out.truncated = truncated; out.auto_reset = auto_reset;
  return launch_groups(e, k_env_step, out, (hipStream_t)stream, true);
}

int sgrl_refresh(sgrl_engine* e, float* obs, double* obs64, void* stream) {
  if (!e || !obs) return fail(SGRL_ERR_ARG, "sgrl_refresh: null engine or obs");
  StepOut out{};
  out.obs32 = obs; out.obs64 = obs64;
  return launch_groups(e, k_env_refresh, out, (hipStream_t)stream);
}

int sgrl_get_records(sgrl_engine* e, double* rec, int32_t* cnt) {
  if (!e) return fail(SGRL_ERR_ARG, "null engine");
  HIP_TRY(hipDeviceSynchronize());
  if (rec) HIP_TRY(hipMemcpy(rec, e->d_rec, sizeof(double) * (size_t)e->n_env * e->stride, hipMemcpyDeviceToHost));
  if (cnt) HIP_TRY(hipMemcpy(cnt, e->d_cnt, sizeof(int32_t) * (size_t)e->n_env * 4, hipMemcpyDeviceToHost));
  return SGRL_OK;
}

int sgrl_set_records(sgrl_engine* e, const double* rec, const int32_t* cnt) {
  if (!e) return fail(SGRL_ERR_ARG, "null engine");
  HIP_TRY(hipDeviceSynchronize());
  if (rec) HIP_TRY(hipMemcpy(e->d_rec, rec, sizeof(double) * (size_t)e->n_env * e->stride, hipMemcpyHostToDevice));
  if (cnt) HIP_TRY(hipMemcpy(e->d_cnt, cnt, sizeof(int32_t) * (size_t)e->n_env * 4, hipMemcpyHostToDevice));
  return SGRL_OK;
}

int sgrl_time_steps(sgrl_engine* e, const float* actions, float* obs, float* reward, uint8_t* done, int reps,
                    void* stream, float* ms_out) {
  if (!e || !actions || !obs || !ms_out || reps <= 0) return fail(SGRL_ERR_ARG, "sgrl_time_steps: bad argument");
  hipEvent_t t0, t1;
  HIP_TRY(hipEventCreate(&t0));
  HIP_TRY(hipEventCreate(&t1));
  StepOut out{};
  out.actions = actions; out.obs32 = obs; out.reward = reward; out.done = done; out.auto_reset = 1;
  HIP_TRY(hipEventRecord(t0, (hipStream_t)stream));
  for (int r = 0; r < reps; r++) {
    const int rc = launch_groups(e, k_env_step, out, (hipStream_t)stream, true);
    if (rc != SGRL_OK) return rc;
  }
  HIP_TRY(hipEventRecord(t1, (hipStream_t)stream));
  HIP_TRY(hipEventSynchronize(t1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, t0, t1));
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  HIP_TRY(hipGetLastError());
  *ms_out = ms / reps;
  return SGRL_OK;
}

int sgrl_ingest_rows(const float* block, int n_rows, int obs_len, int act_len, const int64_t* slot, const sgrl_ring* rings,
                     int n_rings, void* stream) {
  if (!block || !slot || !rings || n_rows <= 0 || obs_len <= 0 || act_len <= 0 || n_rings <= 0)
    return fail(SGRL_ERR_ARG, "sgrl_ingest_rows: bad argument");
  hipLaunchKernelGGL(k_ingest_rows, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, block, obs_len, act_len, slot, rings, n_rings);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(SGRL_ERR_HIP, std::string("k_ingest_rows launch failed (") + hipGetErrorName(le) + ")");
  return SGRL_OK;
}

int64_t sgrl_ingest_ws_words(int n_rows) { return n_rows <= 0 ? 0 : (int64_t)ingest_ws_words(n_rows) + n_rows; }

int sgrl_ingest_block(const float* block, int n_rows, int obs_len, int act_len, const sgrl_ring* rings, int n_rings, int64_t* pos,
                      const int64_t* cap, int64_t* pending, int64_t* slot_ws, void* stream) {
  if (!block || !rings || !pos || !cap || !pending || !slot_ws || n_rows <= 0 || obs_len <= 0 || act_len <= 0 || n_rings <= 0 ||
      n_rings > kIngestMaxRings)
    return fail(SGRL_ERR_ARG, "sgrl_ingest_block: bad argument (at most 32 rings)");
  // the chunk ticket (word 0) starts every call at zero whatever the caller's workspace held: an uninitialised buffer, a launch that
  // was aborted half way or a workspace another call just used must not leave a block without its "last chunk" 
  hipLaunchKernelGGL(k_set_word, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<unsigned*>(slot_ws), 0u, 2);
  hipLaunchKernelGGL(k_ingest_keys, dim3((n_rows + kIngestChunk - 1) / kIngestChunk), dim3(kIngestThreads), 0, (hipStream_t)stream, block, n_rows,
                     obs_len, act_len, n_rings, reinterpret_cast<long long*>(pos), reinterpret_cast<const long long*>(cap),
                     reinterpret_cast<long long*>(pending), reinterpret_cast<long long*>(slot_ws));
  long long* const slots = reinterpret_cast<long long*>(slot_ws) + ingest_ws_words(n_rows);
  hipLaunchKernelGGL(k_ingest_slots, dim3((n_rows + kIngestChunk - 1) / kIngestChunk), dim3(kIngestThreads), 0, (hipStream_t)stream, n_rows,
                     reinterpret_cast<const long long*>(cap), reinterpret_cast<long long*>(slot_ws), slots);
  hipLaunchKernelGGL(k_ingest_rows, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, block, obs_len, act_len, reinterpret_cast<const int64_t*>(slots), rings, n_rings);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return fail(SGRL_ERR_HIP, std::string("sgrl_ingest_block launch failed (") + hipGetErrorName(le) + ")");
  return SGRL_OK;
}

int sgrl_round_record(const float* reward, const uint8_t* done, uint8_t* done_list, int64_t* ep_steps, float* ep_reward, float* reward_buf,
                      uint8_t* store, float* done_bool, int32_t* all_done, int n_env, int max_episode_steps, void* stream) {
  if (!reward || !done || !done_list || !ep_steps || !ep_reward || !reward_buf || !store || !done_bool || !all_done || n_env <= 0)
    return fail(SGRL_ERR_ARG, "sgrl_round_record: bad argument");
  hipLaunchKernelGGL(k_set_word, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<unsigned*>(all_done), 1u, 1);
  hipLaunchKernelGGL(k_round_record, dim3((n_env + 255) / 256), dim3(256), 0, (hipStream_t)stream, reward, done, done_list,
                     reinterpret_cast<long long*>(ep_steps), ep_reward, reward_buf, store, done_bool, reinterpret_cast<int*>(all_done), n_env,
                     max_episode_steps);
  HIP_TRY(hipGetLastError());
  return SGRL_OK;
}

int sgrl_round_record_all(const float* reward, const uint8_t* done, uint8_t* done_list, int64_t* ep_steps, float* ep_reward, float* reward_buf,
                          int64_t* cur_steps, uint8_t* store, float* done_bool, int32_t* all_done, int32_t* was_complete, int n_env,
                          int max_episode_steps, void* stream) {
  if (!reward || !done || !done_list || !ep_steps || !ep_reward || !reward_buf || !cur_steps || !store || !done_bool || !all_done ||
      !was_complete || n_env <= 0)
    return fail(SGRL_ERR_ARG, "sgrl_round_record_all: bad argument");
  hipLaunchKernelGGL(k_round_carry, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<int*>(all_done), reinterpret_cast<int*>(was_complete));
  hipLaunchKernelGGL(k_round_record_all, dim3((n_env + 255) / 256), dim3(256), 0, (hipStream_t)stream, reward, done, done_list,
                     reinterpret_cast<long long*>(ep_steps), ep_reward, reward_buf, reinterpret_cast<long long*>(cur_steps), store, done_bool,
                     reinterpret_cast<int*>(all_done), reinterpret_cast<const int*>(was_complete), n_env, max_episode_steps);
  HIP_TRY(hipGetLastError());
  return SGRL_OK;
}

int sgrl_pack_transitions(const float* obs, int ld_obs, const float* action, int ld_act, const float* next_obs, int ld_next,
                          const float* reward, const float* done_f32, const uint8_t* done_u8, const uint8_t* store,
                          const int64_t* morph_id, float* block, int n_env, int obs_len, int act_len, void* stream) {
  if (!block || n_env < 0 || obs_len <= 0 || act_len <= 0 || (obs && ld_obs < obs_len) || (action && ld_act < act_len) ||
      (next_obs && ld_next < obs_len) || (done_f32 && done_u8))
    return fail(SGRL_ERR_ARG, "sgrl_pack_transitions: bad argument");
  if (n_env == 0) return SGRL_OK;
  PackArgs p{obs, action, next_obs, reward, done_f32, done_u8, store, morph_id, block, ld_obs, ld_act, ld_next, obs_len, act_len};
  hipLaunchKernelGGL(k_pack_transitions, dim3(n_env), dim3(256), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return SGRL_OK;
}

}  // extern "C"

// scene.hip's window on the handle (engine_view.h)
int sgrl_engine_view_of(sgrl_engine* e, sgrl_engine_view* v) {
  if (!e || !v) return SGRL_ERR_ARG;
  v->morphs = e->d_morphs;
  v->env_morph = e->d_env_morph;
  v->rec = e->d_rec;
  v->n_morph = e->n_morph;
  v->n_env = e->n_env;
  v->stride = e->stride;
  v->max_geoms = e->max_geoms;
  v->cam_dist_dev = e->d_cam_dist;
  v->cam_dist_host = e->cam_dist.data();
  return SGRL_OK;
}
