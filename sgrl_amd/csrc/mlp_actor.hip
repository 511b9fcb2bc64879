// mlp_actor.hip -- the monolithic MLP agent's no-grad forwards for a whole batch of environments, ONE launch each (C ABI:
// include/sgrl_mlp.h): the actor, the twin critic, and the TD3 target chain (target actor -> clipped noise -> clamp -> twin target
// critics -> min -> Bellman target).
//
//   k_mlp_pack      live nn.Linear weights / biases -> the padded packed buffer (kpad, npad of sgrl_mlp_plan; zeros in the padding);
//                   at the top of a forward unless the caller holds the weights
//   k_mlp_forward   one workgroup (4 waves) per 32 environment rows.  The observation tile goes into the LDS activation tile
//                   X[32][sx]; every layer computes its whole output row block into registers -- exact-f32 32x32x2 matrix
//                   instructions, the weights streamed through a double-buffered LDS panel of 256 output columns x BK k values --
//                   and, once the last panel has been consumed, writes relu(. + bias) back over X in place: the hidden
//                   activations never leave the chip.  The last layer's epilogue writes max_action * tanh(. + bias) to the action
//                   rows and exact zeros up to the caller's leading dimension.
//   k_mlp_critic    the same walk (mlp_walk, shared by the three kernels) over cat([obs, action]) rows, once per Q stack; the final
//                   N = 1 layer leaves Q in column 0 of one 32-column tile, the two lanes holding it write q[row].
//   k_mlp_chain     actor walk, its epilogue adds the clipped noise, clamps and stores the target action; the workgroup then builds
//                   the critics' input tile -- observation columns from global again, action columns re-read by the very lanes
//                   that stored them (same-thread program order: no cross-workgroup traffic) -- and walks critic 1 and critic 2;
//                   Q1 waits in 16 registers of the two lanes that hold it, min and the Bellman line are done by those lanes.
//
// Wave w of a workgroup owns the 32-column tiles w and w + 4 of each 256-column chunk (a narrow layer -- the 21 action columns --
// costs one tile on one wave, not a 64-column pair).  MAXCH = chunks a workgroup keeps accumulators for (widths up to 256 MAXCH).
// LDS operand layout as csrc/gemm_f32.h k_gemm2: rows of BK + 4 (panel) / sx = kmax + 4 (activations) floats, a lane (row, half)
// reads the contiguous k range [BK / 2 * half, + BK / 2) of its row with ds_read_b128; both strides are 4 * odd, so the 16 lanes of a
// read group fall on distinct 4-bank groups.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "mlp_internal.h"

using namespace sgrl_mlp_detail;

namespace {
thread_local std::string g_mlp_err;
int round_up(int x, int m) { return (x + m - 1) / m * m; }
}  // namespace

int sgrl_mlp_detail::mfail(int code, const std::string& msg) { g_mlp_err = msg; return code; }

int sgrl_mlp_detail::make_plan(const int32_t* dims, int n_dims, Plan* p, const char* who) {
  if (!dims) return mfail(SGRL_ERR_ARG, std::string(who) + ": dims is null");
  if (n_dims < 3 || n_dims > SGRL_MLP_MAX_HIDDEN + 2)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": need 1 .. 4 hidden layers (3 .. 6 widths), got " + std::to_string(n_dims) + " widths");
  for (int i = 0; i < n_dims; i++)
    if (dims[i] < 1 || dims[i] > SGRL_MLP_MAX_WIDTH)
      return mfail(SGRL_ERR_ARG, std::string(who) + ": width " + std::to_string(dims[i]) + " outside 1 .. " + std::to_string(SGRL_MLP_MAX_WIDTH));
  p->n_layers = n_dims - 1;
  for (int i = 0; i < n_dims; i++) p->dims[i] = dims[i];
  int kmax = 0, nmax = 0;
  int64_t off = 0;
  for (int l = 0; l < p->n_layers; l++) {
    p->kpad[l] = l == 0 ? round_up(dims[0], 16) : p->npad[l - 1];
    p->npad[l] = round_up(dims[l + 1], 32);
    p->w_off[l] = off;
    off += (int64_t)p->npad[l] * p->kpad[l];
    kmax = p->kpad[l] > kmax ? p->kpad[l] : kmax;
    nmax = p->npad[l] > nmax ? p->npad[l] : nmax;
  }
  for (int l = 0; l < p->n_layers; l++) { p->b_off[l] = off; off += p->npad[l]; }
  p->total = off;
  const int chunks = (nmax + CH - 1) / CH;
  p->maxch = chunks <= 1 ? 1 : (chunks == 2 ? 2 : 4);
  p->sx = kmax + 4;
  auto lds_for = [&](int bk) { return (int)sizeof(float) * (BM * p->sx + 2 * CH * (bk + 4)); };
  p->bk = lds_for(16) <= LDS_LIMIT ? 16 : 8;
  p->lds = lds_for(p->bk);
  if (p->lds > LDS_LIMIT) return mfail(SGRL_ERR_LIMIT, std::string(who) + ": the activation tile does not fit in LDS");
  return SGRL_OK;
}

namespace {

struct PackArgs {
  const float* w[2][NL];             // [stack][layer]: an actor packs one stack, a critic its two Q stacks back to back
  const float* b[2][NL];
  int n[NL], k[NL], npad[NL], kpad[NL];
  long long w_off[NL], b_off[NL];
  int n_layers, n_stacks;
  long long total;                   // floats of ONE stack
  float* dst;
};

__global__ __launch_bounds__(256) void k_mlp_pack(PackArgs a) {
  const long long all = a.total * a.n_stacks;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < all; g += (long long)gridDim.x * 256) {
    const int s = g >= a.total ? 1 : 0;
    const long long i = g - (s ? a.total : 0);
    float v = 0.f;
    if (i >= a.b_off[0]) {
#pragma unroll
      for (int l = 0; l < NL; l++)
        if (l < a.n_layers && i >= a.b_off[l] && i < a.b_off[l] + a.npad[l]) {
          const int n = (int)(i - a.b_off[l]);
          if (n < a.n[l]) v = (s ? a.b[1][l] : a.b[0][l])[n];
        }
    } else {
#pragma unroll
      for (int l = 0; l < NL; l++)
        if (l < a.n_layers && i >= a.w_off[l] && i < a.w_off[l] + (long long)a.npad[l] * a.kpad[l]) {
          const long long r = i - a.w_off[l];
          const int n = (int)(r / a.kpad[l]), k = (int)(r - (long long)n * a.kpad[l]);
          if (n < a.n[l] && k < a.k[l]) v = (s ? a.w[1][l] : a.w[0][l])[(size_t)n * a.k[l] + k];
        }
    }
    a.dst[g] = v;
  }
}

// Every layer of `a` over the activation tile X[BM][sx] (input in columns [0, kpad[0]), the caller has put a barrier behind its
// writes): hidden layers write relu(. + bias) back over X; the last layer's accumulators go to epi(n, acc, bias_n) once per
// 32-column tile the wave owns (n = the lane's column; C/D layout: row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)).  Returns behind
// a barrier: X and the panels are free.
template <int MAXCH, int BK, class Epi>
__device__ __forceinline__ void mlp_walk(const Net& a, float* X, float* Ws, int sx, Epi&& epi) {
  constexpr int SK = BK + 4;                   // panel row stride
  constexpr int QPR = BK / 4;                  // float4 per panel row
  constexpr int RPP = 256 / QPR;               // panel rows covered per staging pass
  constexpr int NP = CH / RPP;                 // staging passes per panel
  constexpr int KH = BK / 2;                   // k values per lane half
  constexpr int NQ = KH / 4;                   // float4 per lane per operand row per k block
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
  const int kq = t % QPR, r0 = t / QPR;
  for (int l = 0; l < a.n_layers; l++) {
    const int K = a.kpad[l], N = a.npad[l];
    const float* __restrict__ W = a.wp + a.w_off[l];
    const float* __restrict__ bias = a.wp + a.b_off[l];
    const int nkb = K / BK, nch = (N + CH - 1) / CH;
    f32x16 acc[MAXCH][2];
#pragma unroll
    for (int c = 0; c < MAXCH; c++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[c][j][e] = 0.f;
    float4 rw[NP];
    auto gload = [&](int kb, int c) {
#pragma unroll
      for (int i = 0; i < NP; i++) {
        const int n = CH * c + r0 + RPP * i;
        rw[i] = (n < N) ? *reinterpret_cast<const float4*>(W + (size_t)n * K + kb * BK + 4 * kq) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    auto sstore = [&](int st) {
#pragma unroll
      for (int i = 0; i < NP; i++) *reinterpret_cast<float4*>(Ws + (st * CH + r0 + RPP * i) * SK + 4 * kq) = rw[i];
    };
    gload(0, 0);
    sstore(0);
    __syncthreads();
    int st = 0;
    const float* arow = X + li * sx + KH * lh;
    for (int kb = 0; kb < nkb; kb++) {
#pragma unroll
      for (int c = 0; c < MAXCH; c++) {
        if (c < nch) {
          // the panel after (kb, c): global loads in flight under this panel's matrix instructions, LDS writes into the idle stage
          int nc = c + 1, nk = kb;
          if (nc == nch) { nc = 0; nk = kb + 1; }
          const bool more = nk < nkb;
          if (more) gload(nk, nc);
          float4 av[NQ];
#pragma unroll
          for (int q = 0; q < NQ; q++) av[q] = *reinterpret_cast<const float4*>(arow + kb * BK + 4 * q);
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const int colb = 32 * (wave + 4 * j);
            if (CH * c + colb < N) {          // wave-uniform
              const float* brow = Ws + (st * CH + colb + li) * SK + KH * lh;
              float4 bv[NQ];
#pragma unroll
              for (int q = 0; q < NQ; q++) bv[q] = *reinterpret_cast<const float4*>(brow + 4 * q);
#pragma unroll
              for (int q = 0; q < NQ; q++) {
                acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].x, bv[q].x, acc[c][j], 0, 0, 0);
                acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].y, bv[q].y, acc[c][j], 0, 0, 0);
                acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].z, bv[q].z, acc[c][j], 0, 0, 0);
                acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].w, bv[q].w, acc[c][j], 0, 0, 0);
              }
            }
          }
          if (more) sstore(st ^ 1);
          __syncthreads();
          st ^= 1;
        }
      }
    }
    // every read of X and of the panels is behind the last barrier.  C/D layout of a 32 x 32 tile: col = lane & 31,
    // row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const bool last = l + 1 == a.n_layers;
#pragma unroll
    for (int c = 0; c < MAXCH; c++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int n = CH * c + 32 * (wave + 4 * j) + li;
        if (CH * c + 32 * (wave + 4 * j) >= N) continue;
        const float bvv = bias[n];
        if (!last) {
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const int m = (e & 3) + 8 * (e >> 2) + 4 * lh;
            X[m * sx + n] = fmaxf(acc[c][j][e] + bvv, 0.f);
          }
        } else {
          epi(n, acc[c][j], bvv);
        }
      }
    __syncthreads();
  }
}

struct FwdArgs {
  const float* obs; int obs_ld;
  float* act; int act_ld;
  int n_env, in_dim, out_dim, sx;
  Net net;
  float max_action;
};

template <int MAXCH, int BK>
__global__ __launch_bounds__(256) void k_mlp_forward(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
  float* X = mlp_lds;                          // [BM][sx]
  float* Ws = mlp_lds + BM * a.sx;             // [2][CH][BK + 4]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * BM;
  // observation tile (rows beyond n_env and columns beyond the input width: zeros)
  load_rows(X, a.sx, 0, a.in_dim, a.net.kpad[0], a.obs, a.obs_ld, row0, a.n_env);
  __syncthreads();
  mlp_walk<MAXCH, BK>(a.net, X, Ws, a.sx, [&](int n, const f32x16& acc, float bvv) {
    if (n < a.out_dim) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int row = row0 + tile_row(e);
        if (row < a.n_env) a.act[(size_t)row * a.act_ld + n] = a.max_action * tanhf(acc[e] + bvv);
      }
    }
  });
  // slots beyond the output width, up to the caller's leading dimension: exact zeros
  for (int r = wave; r < BM; r += 4) {
    const int row = row0 + r;
    if (row >= a.n_env) break;
    for (int n = a.out_dim + lane; n < a.act_ld; n += 64) a.act[(size_t)row * a.act_ld + n] = 0.f;
  }
}

struct CriticArgs {
  const float* obs; int obs_ld;
  const float* act; int act_ld;
  float* q1; float* q2;              // q2 null: Q1 only
  int n_env, obs_dim, act_dim, sx;
  Net c1, c2;
};

template <int MAXCH, int BK>
__global__ __launch_bounds__(256) void k_mlp_critic(CriticArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
  float* X = mlp_lds;
  float* Ws = mlp_lds + BM * a.sx;
  const int row0 = blockIdx.x * BM;
  for (int s = 0; s < 2; s++) {
    float* q = s ? a.q2 : a.q1;
    if (!q) break;                             // uniform
    // cat([obs, action]) tile; the first stack's hidden activations have overwritten it: loaded again for the second
    load_rows(X, a.sx, 0, a.obs_dim, a.obs_dim, a.obs, a.obs_ld, row0, a.n_env);
    load_rows(X, a.sx, a.obs_dim, a.act_dim, a.c1.kpad[0] - a.obs_dim, a.act, a.act_ld, row0, a.n_env);
    __syncthreads();
    mlp_walk<MAXCH, BK>(s ? a.c2 : a.c1, X, Ws, a.sx, [&](int n, const f32x16& acc, float bvv) {
      if (n == 0) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int row = row0 + tile_row(e);
          if (row < a.n_env) q[row] = acc[e] + bvv;
        }
      }
    });
  }
}

struct ChainArgs {
  const float* obs; int obs_ld;      // next_obs
  const float* noise; int noise_ld;
  const float* reward; const float* done;
  float* target_q;
  float* abuf; int abuf_ld;          // the target action: the caller's action_out, or the critic handle's workspace
  int zero_pad;                      // 1: abuf is the caller's, columns [out_dim, abuf_ld) get exact zeros
  int n_env, in_dim, out_dim, sx;
  Net actor, c1, c2;
  float max_action, noise_clip, discount;
};

template <int MAXCH, int BK>
__global__ __launch_bounds__(256) void k_mlp_chain(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
  float* X = mlp_lds;
  float* Ws = mlp_lds + BM * a.sx;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31;
  const int row0 = blockIdx.x * BM;
  const int sx = a.sx;
  float* abuf = a.abuf;                        // stored and re-read by the same lanes below: not restrict
  load_rows(X, sx, 0, a.in_dim, a.actor.kpad[0], a.obs, a.obs_ld, row0, a.n_env);
  __syncthreads();
  mlp_walk<MAXCH, BK>(a.actor, X, Ws, sx, [&](int n, const f32x16& acc, float bvv) {
    if (n < a.out_dim) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int row = row0 + tile_row(e);
        if (row < a.n_env) {
          const float nz = fminf(fmaxf(a.noise[(size_t)row * a.noise_ld + n], -a.noise_clip), a.noise_clip);
          const float v = a.max_action * tanhf(acc[e] + bvv) + nz;
          abuf[(size_t)row * a.abuf_ld + n] = fminf(fmaxf(v, -a.max_action), a.max_action);
        }
      }
    }
  });
  if (a.zero_pad)
    for (int r = wave; r < BM; r += 4) {
      const int row = row0 + r;
      if (row >= a.n_env) break;
      for (int n = a.out_dim + lane; n < a.abuf_ld; n += 64) abuf[(size_t)row * a.abuf_ld + n] = 0.f;
    }
  const int n_act_pad = a.actor.npad[a.actor.n_layers - 1];
  f32x16 q1v;
#pragma unroll
  for (int e = 0; e < 16; e++) q1v[e] = 0.f;
  for (int s = 0; s < 2; s++) {
    // the critics' input tile: observation columns from global again, zeros behind the action columns up to the padded width,
    // the action columns by the lanes that stored them (the mapping of the actor's last layer)
    load_rows(X, sx, 0, a.in_dim, a.in_dim, a.obs, a.obs_ld, row0, a.n_env);
    load_rows(X, sx, a.in_dim + a.out_dim, 0, a.c1.kpad[0] - a.in_dim - a.out_dim, a.obs, 0, row0, a.n_env);
#pragma unroll
    for (int c = 0; c < MAXCH; c++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int n = CH * c + 32 * (wave + 4 * j) + li;
        if (CH * c + 32 * (wave + 4 * j) >= n_act_pad || n >= a.out_dim) continue;
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const int m = tile_row(e);
          X[m * sx + a.in_dim + n] = (row0 + m < a.n_env) ? abuf[(size_t)(row0 + m) * a.abuf_ld + n] : 0.f;
        }
      }
    __syncthreads();
    if (s == 0) {
      mlp_walk<MAXCH, BK>(a.c1, X, Ws, sx, [&](int n, const f32x16& acc, float bvv) {
        if (n == 0) {
#pragma unroll
          for (int e = 0; e < 16; e++) q1v[e] = acc[e] + bvv;
        }
      });
    } else {
      mlp_walk<MAXCH, BK>(a.c2, X, Ws, sx, [&](int n, const f32x16& acc, float bvv) {
        if (n == 0) {
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const int row = row0 + tile_row(e);
            if (row < a.n_env) {
              const float q = fminf(q1v[e], acc[e] + bvv);
              a.target_q[row] = a.reward[row] + (1.f - a.done[row]) * a.discount * q;
            }
          }
        }
      });
    }
  }
}

typedef void (*fwd_fn)(FwdArgs);
typedef void (*critic_fn)(CriticArgs);
typedef void (*chain_fn)(ChainArgs);
#define SGRL_MLP_PICK(K, maxch, bk)                                                                      \
  ((bk) == 16 ? ((maxch) == 1 ? K<1, 16> : ((maxch) == 2 ? K<2, 16> : K<4, 16>))                          \
              : ((maxch) == 1 ? K<1, 8> : ((maxch) == 2 ? K<2, 8> : K<4, 8>)))
fwd_fn pick_kernel(int maxch, int bk) { return SGRL_MLP_PICK(k_mlp_forward, maxch, bk); }
critic_fn pick_critic(int maxch, int bk) { return SGRL_MLP_PICK(k_mlp_critic, maxch, bk); }
chain_fn pick_chain(int maxch, int bk) { return SGRL_MLP_PICK(k_mlp_chain, maxch, bk); }
int variant_index(int maxch, int bk) { return (bk == 16 ? 0 : 3) + (maxch == 1 ? 0 : (maxch == 2 ? 1 : 2)); }

// What the fused chain kernel uses for the pair: the larger chunk count, the activation stride of the widest padded input of
// either network, the deepest panel that still fits.
struct ChainPlan { int maxch, bk, lds, sx; };
ChainPlan make_chain_plan(const Plan& pa, const Plan& pc) {
  ChainPlan c;
  c.maxch = pa.maxch > pc.maxch ? pa.maxch : pc.maxch;
  c.sx = pa.sx > pc.sx ? pa.sx : pc.sx;
  auto lds_for = [&](int bk) { return (int)sizeof(float) * (BM * c.sx + 2 * CH * (bk + 4)); };
  c.bk = lds_for(16) <= LDS_LIMIT ? 16 : 8;
  c.lds = lds_for(c.bk);
  return c;
}

}  // namespace

enum { KIND_NONE = SGRL_MLP_KIND_NONE, KIND_ACTOR = SGRL_MLP_KIND_ACTOR, KIND_CRITIC = SGRL_MLP_KIND_CRITIC };   // struct sgrl_mlp: mlp_internal.h

namespace {

// The dynamic-LDS limit of a kernel is a property of the function, process-wide: the largest size asked for so far is kept per
// kernel family and variant, and the attribute only ever goes up (handles of different widths share a variant).
enum { FAM_FORWARD = 0, FAM_CRITIC = 1, FAM_CHAIN = 2 };
int g_lds_raised[3][6] = {{0}};
int raise_lds(const void* fn, int family, int variant, int lds, const char* who) {
  int& raised = g_lds_raised[family][variant];
  if (raised >= lds) return SGRL_OK;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return mfail(SGRL_ERR_HIP, std::string(who) + ": cannot raise the kernel's dynamic LDS limit");
  raised = lds;
  return SGRL_OK;
}

int n_stacks(const sgrl_mlp* s) { return s->kind == KIND_CRITIC ? 2 : 1; }

// The pack launch at the top of a forward, unless the handle holds clean weights (a capture always packs; `always`: the gradient
// half, whose weights have just been stepped).
int pack_if_needed(sgrl_mlp* s, hipStream_t st, bool always = false) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  const bool capturing = cap != hipStreamCaptureStatusNone;
  if (s->hold && !s->dirty && !capturing && !always) return SGRL_OK;
  const Plan& p = s->plan;
  PackArgs pa;
  for (int l = 0; l < NL; l++) {
    const bool on = l < p.n_layers;
    for (int k = 0; k < 2; k++) {
      pa.w[k][l] = on ? s->w[k][l] : nullptr;
      pa.b[k][l] = on ? s->b[k][l] : nullptr;
    }
    pa.n[l] = on ? p.dims[l + 1] : 0;
    pa.k[l] = on ? p.dims[l] : 0;
    pa.npad[l] = on ? p.npad[l] : 0;
    pa.kpad[l] = on ? p.kpad[l] : 0;
    pa.w_off[l] = on ? p.w_off[l] : 0;
    pa.b_off[l] = on ? p.b_off[l] : 0;
  }
  pa.n_layers = p.n_layers;
  pa.n_stacks = n_stacks(s);
  pa.total = p.total;
  pa.dst = s->packed;
  const int blocks = (int)((p.total * pa.n_stacks + 1023) / 1024);
  hipLaunchKernelGGL(k_mlp_pack, dim3(blocks), dim3(256), 0, st, pa);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("MLP pack launch: ") + hipGetErrorString(e));
  if (!capturing) s->dirty = false;
  return SGRL_OK;
}

// Shared by the two binds: plan, packed buffer of `stacks` stacks, addresses.
int bind_common(sgrl_mlp* s, const void* const* ptrs, int n_ptrs, const int32_t* dims, int n_dims, int stacks, const char* who) {
  if (!s || !ptrs) return mfail(SGRL_ERR_ARG, std::string(who) + ": null argument");
  Plan p;
  const int rc = make_plan(dims, n_dims, &p, who);
  if (rc != SGRL_OK) return rc;
  if (stacks == 2 && p.dims[p.n_layers] != 1)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": a critic's last width must be 1, got " + std::to_string(p.dims[p.n_layers]));
  if (n_ptrs != 2 * stacks * p.n_layers)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": expected " + std::to_string(2 * stacks * p.n_layers) + " parameter addresses, got " + std::to_string(n_ptrs));
  for (int i = 0; i < n_ptrs; i++)
    if (!ptrs[i] || (reinterpret_cast<uintptr_t>(ptrs[i]) & 3))
      return mfail(SGRL_ERR_ARG, std::string(who) + ": parameter " + std::to_string(i) + " is null or not 4-byte aligned");
  fwd_fn fn = nullptr;
  critic_fn cfn = nullptr;
  int lrc;
  if (stacks == 1) {
    fn = pick_kernel(p.maxch, p.bk);
    lrc = raise_lds(reinterpret_cast<const void*>(fn), FAM_FORWARD, variant_index(p.maxch, p.bk), p.lds, who);
  } else {
    cfn = pick_critic(p.maxch, p.bk);
    lrc = raise_lds(reinterpret_cast<const void*>(cfn), FAM_CRITIC, variant_index(p.maxch, p.bk), p.lds, who);
  }
  if (lrc != SGRL_OK) return lrc;
  const int64_t need = p.total * stacks;
  if (need != s->packed_floats) {
    float* buf = nullptr;
    if (hipMalloc(&buf, sizeof(float) * (size_t)need) != hipSuccess) return mfail(SGRL_ERR_HIP, "device allocation failed (MLP packed weights)");
    if (s->packed) {
      (void)hipDeviceSynchronize();       // a forward in flight may still read the old buffer
      (void)hipFree(s->packed);
      s->generation++;
    }
    s->packed = buf;
    s->packed_floats = need;
  }
  s->plan = p;
  for (int k = 0; k < stacks; k++)
    for (int l = 0; l < p.n_layers; l++) {
      s->w[k][l] = static_cast<const float*>(ptrs[2 * (k * p.n_layers + l)]);
      s->b[k][l] = static_cast<const float*>(ptrs[2 * (k * p.n_layers + l) + 1]);
    }
  s->kernel = stacks == 1 ? reinterpret_cast<const void*>(fn) : reinterpret_cast<const void*>(cfn);
  s->grads_bound = false;  // the gradient addresses follow the parameter bind: bind them again
  s->kind = stacks == 2 ? KIND_CRITIC : KIND_ACTOR;
  s->dirty = true;
  s->n_env = 0;           // the batch structure is checked against the widths: configure again
  return SGRL_OK;
}

}  // namespace

int sgrl_mlp_detail::pack_now(sgrl_mlp* s, hipStream_t st) { return pack_if_needed(s, st, true); }

extern "C" {

const char* sgrl_mlp_last_error(void) { return g_mlp_err.c_str(); }
int sgrl_mlp_forward_launches(void) { return 1; }
int sgrl_mlp_critic_forward_launches(void) { return 1; }
int sgrl_mlp_td_target_launches(void) { return 1; }
int sgrl_mlp_pack_launches(void) { return 1; }
int sgrl_mlp_num_envs(const sgrl_mlp* s) { return s ? s->n_env : 0; }
int64_t sgrl_mlp_generation(const sgrl_mlp* s) { return s ? s->generation : 0; }

int sgrl_mlp_plan(const int32_t* dims, int n_dims, int32_t* kpad, int32_t* npad, int64_t* w_off, int64_t* b_off, int32_t* info,
                  int64_t* total) {
  if (!kpad || !npad || !w_off || !b_off || !info || !total) return mfail(SGRL_ERR_ARG, "sgrl_mlp_plan: null argument");
  Plan p;
  const int rc = make_plan(dims, n_dims, &p, "sgrl_mlp_plan");
  if (rc != SGRL_OK) return rc;
  for (int l = 0; l < p.n_layers; l++) { kpad[l] = p.kpad[l]; npad[l] = p.npad[l]; w_off[l] = p.w_off[l]; b_off[l] = p.b_off[l]; }
  info[0] = p.maxch; info[1] = p.bk; info[2] = p.lds; info[3] = p.sx;
  *total = p.total;
  return SGRL_OK;
}

int sgrl_mlp_chain_plan(const int32_t* actor_dims, int n_a, const int32_t* critic_dims, int n_c, int32_t* info) {
  if (!info) return mfail(SGRL_ERR_ARG, "sgrl_mlp_chain_plan: null argument");
  Plan pa, pc;
  int rc = make_plan(actor_dims, n_a, &pa, "sgrl_mlp_chain_plan (actor)");
  if (rc != SGRL_OK) return rc;
  rc = make_plan(critic_dims, n_c, &pc, "sgrl_mlp_chain_plan (critic)");
  if (rc != SGRL_OK) return rc;
  if (pc.dims[pc.n_layers] != 1)
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_chain_plan: a critic's last width must be 1, got " + std::to_string(pc.dims[pc.n_layers]));
  if (pc.dims[0] != pa.dims[0] + pa.dims[pa.n_layers])
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_chain_plan: the critic reads " + std::to_string(pc.dims[0]) + " values, not the actor's input + output width " +
                                   std::to_string(pa.dims[0] + pa.dims[pa.n_layers]));
  const ChainPlan c = make_chain_plan(pa, pc);
  info[0] = c.maxch; info[1] = c.bk; info[2] = c.lds; info[3] = c.sx;
  return SGRL_OK;
}

int sgrl_mlp_create(sgrl_mlp** out) {
  if (!out) return mfail(SGRL_ERR_ARG, "out is null");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return mfail(SGRL_ERR_HIP, "no HIP device visible: the MLP forwards need an MI355X (there is no CPU fallback)");
  *out = new sgrl_mlp();
  return SGRL_OK;
}

void sgrl_mlp_destroy(sgrl_mlp* s) {
  if (!s) return;
  if (s->packed) (void)hipFree(s->packed);
  if (s->ws) (void)hipFree(s->ws);
  if (s->tws) (void)hipFree(s->tws);
  delete s;
}

int sgrl_mlp_set_params(sgrl_mlp* s, const void* const* ptrs, int n_ptrs, const int32_t* dims, int n_dims) {
  return bind_common(s, ptrs, n_ptrs, dims, n_dims, 1, "sgrl_mlp_set_params");
}

int sgrl_mlp_set_critic_params(sgrl_mlp* s, const void* const* ptrs, int n_ptrs, const int32_t* dims, int n_dims) {
  return bind_common(s, ptrs, n_ptrs, dims, n_dims, 2, "sgrl_mlp_set_critic_params");
}

int sgrl_mlp_hold_weights(sgrl_mlp* s, int hold) {
  if (!s) return mfail(SGRL_ERR_ARG, "sgrl_mlp_hold_weights: null handle");
  s->hold = hold != 0;
  s->dirty = true;
  return SGRL_OK;
}

int sgrl_mlp_configure(sgrl_mlp* s, int n_morph, const int32_t* morph_L, const int32_t* morph_count, int feature, int out) {
  if (!s || n_morph <= 0 || !morph_L || !morph_count || feature < 1 || out < 1) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: bad argument");
  if (s->kind == KIND_NONE) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: parameters not set (sgrl_mlp_set_params / sgrl_mlp_set_critic_params)");
  int64_t n = 0;
  const int in_dim = s->plan.dims[0], out_dim = s->plan.dims[s->plan.n_layers];
  for (int k = 0; k < n_morph; k++) {
    if (morph_count[k] < 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: negative morph_count");
    if (s->kind == KIND_CRITIC) {
      if ((int64_t)(feature + out) * morph_L[k] != in_dim)
        return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: morphology " + std::to_string(k) + " has " + std::to_string(morph_L[k]) +
                                       " limbs; the critic was built for " + std::to_string(in_dim) + " inputs (" + std::to_string(feature) +
                                       " + " + std::to_string(out) + " per limb)");
    } else if ((int64_t)feature * morph_L[k] != in_dim || (int64_t)out * morph_L[k] != out_dim) {
      return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: morphology " + std::to_string(k) + " has " + std::to_string(morph_L[k]) +
                                     " limbs; the network was built for " + std::to_string(in_dim) + " inputs and " +
                                     std::to_string(out_dim) + " outputs (" + std::to_string(feature) + " / " + std::to_string(out) + " per limb)");
    }
    n += morph_count[k];
  }
  if (n == 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: no environments");
  if (n > ((int64_t)1 << 24)) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: more than 2^24 environments in one batch");
  s->n_env = (int)n;
  s->obs_w = feature * morph_L[0];
  s->act_w = out * morph_L[0];
  return SGRL_OK;
}

int sgrl_mlp_forward(sgrl_mlp* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, void* stream) {
  if (!s || !obs || !act) return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: null argument");
  if (s->kind == KIND_CRITIC) return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: the handle is not bound as an actor");
  if (s->kind == KIND_NONE || s->n_env <= 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: parameters or batch structure not set");
  const Plan& p = s->plan;
  const int in_dim = p.dims[0], out_dim = p.dims[p.n_layers];
  if (obs_ld < in_dim || act_ld < out_dim)
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: obs_ld < input width or act_ld < output width (rows too narrow for the network)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = pack_if_needed(s, st);
  if (rc != SGRL_OK) return rc;
  FwdArgs fa;
  fa.obs = obs; fa.obs_ld = obs_ld; fa.act = act; fa.act_ld = act_ld;
  fa.n_env = s->n_env; fa.in_dim = in_dim; fa.out_dim = out_dim; fa.sx = p.sx;
  fa.net = make_net(p, s->packed);
  fa.max_action = max_action;
  const int grid = (s->n_env + BM - 1) / BM;
  hipLaunchKernelGGL(reinterpret_cast<fwd_fn>(const_cast<void*>(s->kernel)), dim3(grid), dim3(256), p.lds, st, fa);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("MLP forward launch: ") + hipGetErrorString(e));
  return SGRL_OK;
}

int sgrl_mlp_critic_forward(sgrl_mlp* s, const float* obs, int obs_ld, const float* act, int act_ld, float* q1, float* q2, void* stream) {
  if (!s || !obs || !act || !q1) return mfail(SGRL_ERR_ARG, "sgrl_mlp_critic_forward: null argument");
  if (s->kind != KIND_CRITIC) return mfail(SGRL_ERR_ARG, "sgrl_mlp_critic_forward: the handle is not bound as a critic");
  if (s->n_env <= 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_critic_forward: batch structure not set");
  if (obs_ld < s->obs_w || act_ld < s->act_w)
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_critic_forward: obs_ld or act_ld below the columns the critic reads (rows too narrow for the network)");
  const Plan& p = s->plan;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = pack_if_needed(s, st);
  if (rc != SGRL_OK) return rc;
  CriticArgs ca;
  ca.obs = obs; ca.obs_ld = obs_ld; ca.act = act; ca.act_ld = act_ld; ca.q1 = q1; ca.q2 = q2;
  ca.n_env = s->n_env; ca.obs_dim = s->obs_w; ca.act_dim = s->act_w; ca.sx = p.sx;
  ca.c1 = make_net(p, s->packed);
  ca.c2 = make_net(p, s->packed + p.total);
  const int grid = (s->n_env + BM - 1) / BM;
  hipLaunchKernelGGL(reinterpret_cast<critic_fn>(const_cast<void*>(s->kernel)), dim3(grid), dim3(256), p.lds, st, ca);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("MLP critic forward launch: ") + hipGetErrorString(e));
  return SGRL_OK;
}

int sgrl_mlp_td_target(sgrl_mlp* actor_t, sgrl_mlp* critic_t, const float* next_obs, int obs_ld, const float* noise, int noise_ld,
                       const float* reward, const float* done, float max_action, float noise_clip, float discount, float* target_q,
                       float* action_out, int action_ld, void* stream) {
  if (!actor_t || !critic_t || !next_obs || !noise || !reward || !done || !target_q) return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: null argument");
  if (actor_t->kind != KIND_ACTOR) return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: the first handle is not bound as an actor");
  if (critic_t->kind != KIND_CRITIC) return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: the second handle is not bound as a critic");
  if (actor_t->n_env <= 0 || critic_t->n_env <= 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: batch structure not set");
  if (actor_t->n_env != critic_t->n_env)
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: actor and critic are configured for different batch structures (" +
                                   std::to_string(actor_t->n_env) + " / " + std::to_string(critic_t->n_env) + " environments)");
  const Plan& pa = actor_t->plan;
  const Plan& pc = critic_t->plan;
  const int in_dim = pa.dims[0], out_dim = pa.dims[pa.n_layers], n_env = actor_t->n_env;
  if (pc.dims[0] != in_dim + out_dim || critic_t->obs_w != in_dim || critic_t->act_w != out_dim)
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: the critic reads " + std::to_string(pc.dims[0]) + " values, not the actor's input + output width " +
                                   std::to_string(in_dim + out_dim));
  if (obs_ld < in_dim || noise_ld < out_dim || (action_out && action_ld < out_dim))
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: obs_ld, noise_ld or action_ld below the network's width (rows too narrow for the network)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  const bool capturing = cap != hipStreamCaptureStatusNone;
  const ChainPlan c = make_chain_plan(pa, pc);
  chain_fn fn = pick_chain(c.maxch, c.bk);
  const int lrc = raise_lds(reinterpret_cast<const void*>(fn), FAM_CHAIN, variant_index(c.maxch, c.bk), c.lds, "sgrl_mlp_td_target");
  if (lrc != SGRL_OK) return lrc;
  if (!action_out) {
    const int64_t need = (int64_t)n_env * out_dim;
    if (need > critic_t->ws_floats) {
      if (capturing)
        return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: the critic's workspace must grow, which a capture cannot record: run this batch size eagerly first");
      float* buf = nullptr;
      if (hipMalloc(&buf, sizeof(float) * (size_t)need) != hipSuccess) return mfail(SGRL_ERR_HIP, "device allocation failed (MLP chain workspace)");
      if (critic_t->ws) {
        (void)hipDeviceSynchronize();     // a chain in flight may still use the old workspace
        (void)hipFree(critic_t->ws);
        critic_t->generation++;
      }
      critic_t->ws = buf;
      critic_t->ws_floats = need;
    }
  }
  int rc = pack_if_needed(actor_t, st);
  if (rc != SGRL_OK) return rc;
  rc = pack_if_needed(critic_t, st);
  if (rc != SGRL_OK) return rc;
  ChainArgs a;
  a.obs = next_obs; a.obs_ld = obs_ld; a.noise = noise; a.noise_ld = noise_ld; a.reward = reward; a.done = done; a.target_q = target_q;
  a.abuf = action_out ? action_out : critic_t->ws;
  a.abuf_ld = action_out ? action_ld : out_dim;
  a.zero_pad = action_out ? 1 : 0;
  a.n_env = n_env; a.in_dim = in_dim; a.out_dim = out_dim; a.sx = c.sx;
  a.actor = make_net(pa, actor_t->packed);
  a.c1 = make_net(pc, critic_t->packed);
  a.c2 = make_net(pc, critic_t->packed + pc.total);
  a.max_action = max_action; a.noise_clip = noise_clip; a.discount = discount;
  const int grid = (n_env + BM - 1) / BM;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(256), c.lds, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("MLP target chain launch: ") + hipGetErrorString(e));
  return SGRL_OK;
}

}  // extern "C"
