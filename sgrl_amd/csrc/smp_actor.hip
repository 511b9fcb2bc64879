// smp_actor.hip -- batched HIP forward of the SMP actor (shared modular policies, reference src/ModularActor.py:12-384, the
// disable_fold path with bottom-up AND top-down messages) behind the C ABI of include/sgrl_smp.h.
//
// The data dependence of SMP runs along tree depth, so the batch is scheduled by GLOBAL TREE LEVEL: the rows of the workspace are
// the nodes of every environment of every morphology sorted by depth (within a depth: limbs with children first, leaves last), and
// level d of the batch is ONE contiguous row range whatever the morphologies.  One forward of a batch whose deepest tree has D
// levels = 6 D launches on the caller's stream:
//   k_smp_embed                       all nodes: cat[:, 0:64] = tanh(normalize(fc1 x)), cat[:, 64:] = 0, xm[:, 32:64] = 0
//   bottom-up, d = D-1 .. 0 (ActorUp, ModularActor.py:35-47)                                                       2 D launches
//     k_gemm2                         raw2 = cat . fc2^T + b                                   rows of level d, K = 64 + 32 mc
//     k_smp_up                        up = normalize(fc3 tanh(raw2)); tanh(up) goes to xm[:, 0:32] of the node and to the
//                                     node's child slot of its parent's cat row
//   top-down, d = 0 .. D-2, limbs with children only (ActorDownAction.msg_base, ModularActor.py:72-96)         4 (D-1) launches
//     k_gemm2 (ReLU) x 2, k_gemm2     raw3 = l3(relu(l2(relu(l1 xm))))        64 -> 400 -> 300 -> 32 mc (l3 over k < 288)
//     k_smp_down                      adds l3's last 12 k terms, down = normalize(raw3); tanh(down[slot]) goes to xm[:, 32:64]
//                                     of every child
//   actions, all nodes at once (action_base feeds no message)                                                       3 launches
//     k_gemm2 (ReLU) x 2              h2 = relu(l2(relu(l1 xm)))              64 -> 400 -> 300
//     k_smp_action                    act = max_action * tanh(l3 h2), zero padding of the action rows
// A leaf's outgoing message is never read (msg_base skips leaves); the deepest level holds leaves only.  fc3 (64 -> 32) sits in
// the row kernel between two level steps: as a product of its own it would cost two more launches per level on a chain that is
// bound by its 2 D dependent steps.  The two 64 -> 400 first layers of action_base and msg_base are NOT stacked: they are two
// live tensors read where torch keeps them, stacking would need a packed copy.  msg_base.l3 has K = 300, not a multiple of the
// product's k tile (16): the product covers k < 288, k_smp_down the remaining 12 terms.
// Every product is exact f32 (v_mfma_f32_32x32x2_f32 in k_gemm2; the row kernels are plain f32 FMA chains).  The weights are
// read through the addresses bound by sgrl_smp_bind_params on every forward: nothing is packed, nothing is cached.
//
// CRITIC (CriticGraphPolicy with bu and td, reference src/ModularCritic.py; sgrl_smp_bind_critic_params / sgrl_smp_forward_q): the
// same schedule and the same kernels, instantiated with CRITIC = true.  CriticUp.fc1 reads [obs | action] per limb from the two
// buffers where they lie; the bottom-up pass and msg_base are the actor's.  The Q heads read RAW values, xum = [up | action |
// parent message slot] (normalised, no tanh), so the critic instances of k_smp_embed / k_smp_up / k_smp_down also store those,
// from the registers they already hold, into xq [N, 80] (columns 64 + act_feature .. 79 zero).  After the top-down pass, over all
// nodes at once:                                                                                        5 + twin launches
//     k_smp_stage_q                   wq [800, 80] = [baseQ1.l1.weight ; baseQ2.l1.weight] zero padded from 67 to 80 columns,
//                                     bq [800] = the two biases -- copied from the LIVE tensors on every forward (the product
//                                     kernel loads 16-byte groups of k from rows of a stride that is a multiple of 4; a
//                                     [400, 67] tensor offers neither, and its last row must not be read past its end)
//     k_gemm2 (ReLU)                  h1q [N, 800] = relu(xq . wq^T + bq): both heads' first layers as ONE product, K = 80
//     k_gemm2 (ReLU) x (1 + twin)     h2q [N, 300 h .. 300 h + 299] = relu(l2_h(h1q[:, 400 h .. 400 h + 399])), lda = 800
//     k_smp_q3                        l3 (300 -> 1) of both heads, one wave per node; the value goes to qe[h][env][limb]
//     k_smp_qsum                      one thread per environment adds its limbs' values in limb order 0 .. L - 1 (a row's result
//                                     does not depend on what else is in the batch) and writes q1, q2 -- or, for
//                                     sgrl_smp_td_target, reward + (1 - done) * discount * min(q1, q2)
// sgrl_smp_td_target = the target actor's forward with k_smp_action<true> (clipped noise added, clamped, written into the
// critic handle's workspace) followed by the twin critic: 12 D + 3 launches on the caller's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sgrl.h"
#include "../../include/sgrl_smp.h"

// own copies, with internal linkage, of the few non-template kernels and device variables gemm_f32.h defines (see swat_actor.hip)
namespace {
#include "gemm_f32.h"
}

namespace {

thread_local std::string g_smp_err;
int mfail(int code, const std::string& msg) { g_smp_err = msg; return code; }

constexpr int MSG = 32;         // message width
constexpr int HU = 64;          // ActorUp hidden units; also the width of xm = [up | down slot]
constexpr int H1 = 400, H2 = 300;
constexpr int H2G = 288;        // k range of msg_base.l3 covered by the product (multiple of the k tile)
constexpr int QK = 80;          // row stride of xq / wq: [up 32 | action <= 8 | slot 32] padded to a multiple of the k tile
constexpr int AFMAX = 8;        // act_feature of a critic / out of an actor at most
constexpr int LMAX = SGRL_SMP_MAX_LIMBS;
constexpr int DMAX = SGRL_SMP_MAX_LEVELS;
constexpr int MCMAX = SGRL_SMP_MAX_CHILDREN;

using sgrl_gemm::EPI_RELU;
using sgrl_gemm::GemmArgs;
using sgrl_gemm::k_gemm2;

__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// F.normalize's divisor: max(||v||_2, 1e-12)
__device__ __forceinline__ float norm_div(float ss) { return fmaxf(sqrtf(ss), 1e-12f); }

struct RowTab {
  const int32_t* row_env;    // [N] environment of the row
  const int32_t* row_limb;   // [N] limb of the row inside its environment
  const int32_t* par;        // [N] row of the parent, -1 at a root
  const int32_t* cidx;       // [N] position of the node in its parent's children row (the bottom-up message slot)
  const int32_t* slot;       // [N] slot of the parent's outgoing message the node reads (top-down; mirrored at a flipped root)
  const int32_t* ch;         // [N, mc] rows of the children, -1 = empty
};

// first half of ActorUp (ModularActor.py:35-40): h = fc1 x + b over the `F` inputs of every node, normalised over its 64 channels,
// then the tanh that the reference applies to [h | child messages]; the message part of the row and the parent-message half of xm
// start as zeros (empty child slots, roots) and are filled by the scatter of k_smp_up / k_smp_down.  16 nodes per 256-thread
// block, lane = channel, 4 nodes per wave; the block's input rows are staged in LDS and every weight is loaded once per wave.
// CRITIC: the last AF of the F inputs come from the action buffer (CriticUp, ModularCritic.py:11-40: fc1 over [x | u]); the raw
// input row of the Q heads starts here too: xq[:, 32 : 32 + AF] = action, xq[:, 32 + AF : 80] = 0 (the parent message of a root,
// the padding).
constexpr int kEmbedRows = 16;
template <bool CRITIC>
__global__ __launch_bounds__(256) void k_smp_embed(const float* __restrict__ obs, int obs_ld, int F, const float* __restrict__ action,
                                                    int act_ld, int AF, const float* __restrict__ W1, const float* __restrict__ b1,
                                                    RowTab rt, float* __restrict__ cat, int K1, float* __restrict__ xm,
                                                    float* __restrict__ xq, int N) {
  __shared__ float xs[kEmbedRows][64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, rb = blockIdx.x * kEmbedRows;
  for (int i = t; i < kEmbedRows * 64; i += 256) {
    const int r = i >> 6, k = i & 63, n = rb + r;
    float v = 0.f;
    if (CRITIC) {
      const int FO = F - AF;
      if (n < N && k < FO) v = obs[(size_t)rt.row_env[n] * obs_ld + FO * rt.row_limb[n] + k];
      else if (n < N && k < F) v = action[(size_t)rt.row_env[n] * act_ld + AF * rt.row_limb[n] + (k - FO)];
    } else {
      if (n < N && k < F) v = obs[(size_t)rt.row_env[n] * obs_ld + F * rt.row_limb[n] + k];
    }
    xs[r][k] = v;
  }
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < F; k++) {
    const float w = W1[lane * F + k];
#pragma unroll
    for (int p = 0; p < 4; p++) acc[p] = fmaf(xs[4 * wave + p][k], w, acc[p]);
  }
  const float b = b1[lane];
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int n = rb + 4 * wave + p;
    if (n >= N) break;                                        // wave-uniform
    const float v = acc[p] + b;
    const float den = norm_div(wave_sum(v * v));
    float* crow = cat + (size_t)n * K1;
    crow[lane] = tanhf(v / den);
    for (int k = HU + lane; k < K1; k += 64) crow[k] = 0.f;
    if (lane < MSG) xm[(size_t)n * HU + MSG + lane] = 0.f;
    if (CRITIC) {
      float* qrow = xq + (size_t)n * QK;
      if (lane < AF) qrow[MSG + lane] = xs[4 * wave + p][F - AF + lane];
      if (MSG + AF + lane < QK) qrow[MSG + AF + lane] = 0.f;         // QK - MSG - AF <= 47 columns: one pass
    }
  }
}

// second half of ActorUp for the rows [r0, r0 + n) of one level: up = normalize(fc3 tanh(raw2) + b) (ModularActor.py:41-47).  Only
// tanh(up) is ever read again -- by the parent's fc2 input (ModularActor.py:37 applies tanh to the concatenation) and by the
// node's own top-down input (ModularActor.py:84) -- so that is what is stored, in both places.  32 rows per 256-thread block:
// fc3 (8 KB) and the block's tanh(raw2) rows live in LDS, a thread owns output j of rows rr, rr + 8, rr + 16, rr + 24.
// CRITIC: the Q heads read up itself (CriticDownAction, ModularCritic.py:79-140: xum is not passed through tanh): xq[:, 0:32].
constexpr int kUpRows = 32;
template <bool CRITIC>
__global__ __launch_bounds__(256) void k_smp_up(const float* __restrict__ raw2, const float* __restrict__ W3, const float* __restrict__ b3,
                                                 RowTab rt, float* __restrict__ cat, int K1, float* __restrict__ xm,
                                                 float* __restrict__ xq, int r0, int n) {
  __shared__ float w3s[HU][MSG + 1];
  __shared__ float ts[kUpRows][HU];
  const int t = threadIdx.x, rb = r0 + blockIdx.x * kUpRows, rend = r0 + n;
  for (int i = t; i < MSG * HU; i += 256) w3s[i & 63][i >> 6] = W3[i];
  for (int i = t; i < kUpRows * HU; i += 256) {
    const int row = rb + (i >> 6);
    ts[i >> 6][i & 63] = row < rend ? tanhf(raw2[(size_t)row * HU + (i & 63)]) : 0.f;
  }
  __syncthreads();
  const int j = t & 31, rr = t >> 5;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int k = 0; k < HU; k++) {
    const float w = w3s[k][j];
#pragma unroll
    for (int p = 0; p < 4; p++) acc[p] = fmaf(ts[rr + 8 * p][k], w, acc[p]);
  }
  const float b = b3[j];
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int row = rb + rr + 8 * p;
    const float u = acc[p] + b;
    float ss = u * u;
    for (int off = 16; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);        // the 32 outputs of a row sit in one half-wave
    const float un = u / norm_div(ss);
    const float tv = tanhf(un);
    if (row < rend) {
      if (CRITIC) xq[(size_t)row * QK + j] = un;
      xm[(size_t)row * HU + j] = tv;
      const int pr = rt.par[row];
      if (pr >= 0) cat[(size_t)pr * K1 + HU + MSG * rt.cidx[row] + j] = tv;
    }
  }
}

// end of msg_base for the n limbs-with-children of one level (rows r0 .. r0 + n of the batch, rows 0 .. n of raw3 / h2): the last
// 12 k terms of l3, down = normalize(.) over the whole 32 mc vector (ModularActor.py:93-96), and the scatter: child c reads slot
// rt.slot[c] of it, through the tanh of its own top-down input (ModularActor.py:84).  One wave per row, column = lane + 64 q.
// CRITIC: the child's Q heads read its slot of down itself: xq[:, 32 + AF : 64 + AF].
template <bool CRITIC>
__global__ __launch_bounds__(256) void k_smp_down(const float* __restrict__ raw3, const float* __restrict__ h2, const float* __restrict__ W3,
                                                   RowTab rt, int mc, float* __restrict__ xm, float* __restrict__ xq, int AF, int r0,
                                                   int n) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int MC = MSG * mc, row = r0 + i;
  float hk[H2 - H2G];
#pragma unroll
  for (int k = 0; k < H2 - H2G; k++) hk[k] = h2[(size_t)i * H2 + H2G + k];
  float v[4], ss = 0.f;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int col = lane + 64 * q;
    v[q] = 0.f;
    if (col < MC) {
      float s = raw3[(size_t)i * MC + col];
      const float* w = W3 + (size_t)col * H2 + H2G;
#pragma unroll
      for (int k = 0; k < H2 - H2G; k++) s = fmaf(hk[k], w[k], s);
      v[q] = s;
    }
    ss = fmaf(v[q], v[q], ss);
  }
  const float den = norm_div(wave_sum(ss));
  float dn[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    dn[q] = v[q] / den;
    v[q] = tanhf(dn[q]);
  }
  for (int k = 0; k < mc; k++) {
    const int c = rt.ch[(size_t)row * mc + k];
    if (c < 0) continue;                                      // wave-uniform
    const int sc = rt.slot[c], q = sc >> 1;                   // slot sc = columns 32 sc .. 32 sc + 31 = half (sc & 1) of register q
    const float val = q == 0 ? v[0] : (q == 1 ? v[1] : (q == 2 ? v[2] : v[3]));
    if ((lane >> 5) == (sc & 1)) xm[(size_t)c * HU + MSG + (lane & 31)] = val;
    if (CRITIC) {
      const float rv = q == 0 ? dn[0] : (q == 1 ? dn[1] : (q == 2 ? dn[2] : dn[3]));
      if ((lane >> 5) == (sc & 1)) xq[(size_t)c * QK + MSG + AF + (lane & 31)] = rv;
    }
  }
}

// action_base.l3 and max_action * tanh (ModularActor.py:86-92) for every node, one wave per node; the node of limb 0 of every
// environment also writes the zero padding act[e, out * L_e : act_ld].
// TARGET (the target actor of a TD3 update, reference agent.py:126-134): act = clamp(max_action * tanh(.) + clamp(noise,
// +-noise_clip), +-max_action), noise laid out like an action row.
template <bool TARGET>
__global__ __launch_bounds__(256) void k_smp_action(const float* __restrict__ h2, const float* __restrict__ W3, const float* __restrict__ b3,
                                                     int O, RowTab rt, const int32_t* __restrict__ env_L, float* __restrict__ act, int act_ld,
                                                     float max_action, const float* __restrict__ noise, int noise_ld, float noise_clip,
                                                     int N) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  float x[5];
#pragma unroll
  for (int i = 0; i < 5; i++) x[i] = (lane + 64 * i < H2) ? h2[(size_t)row * H2 + lane + 64 * i] : 0.f;
  const int env = rt.row_env[row], limb = rt.row_limb[row];
  float* arow = act + (size_t)env * act_ld;
  for (int j = 0; j < O; j++) {
    const float* w = W3 + (size_t)j * H2;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 5; i++)
      if (lane + 64 * i < H2) s = fmaf(x[i], w[lane + 64 * i], s);
    s = wave_sum(s) + b3[j];
    if (TARGET) {
      const float nz = fminf(fmaxf(noise[(size_t)env * noise_ld + O * limb + j], -noise_clip), noise_clip);
      if (lane == 0) arow[O * limb + j] = fminf(fmaxf(max_action * tanhf(s) + nz, -max_action), max_action);
    } else {
      if (lane == 0) arow[O * limb + j] = max_action * tanhf(s);
    }
  }
  if (limb == 0)
    for (int k = O * env_L[env] + lane; k < act_ld; k += 64) arow[k] = 0.f;
}

// The two live [400, QIN] first-layer weights of the Q heads (QIN = 64 + act_feature = 67) as ONE matrix the product kernel can
// read: wq [400 nh, 80], rows 0 .. 399 baseQ1.l1, rows 400 .. 799 baseQ2.l1, columns QIN .. 79 zero; bq the stacked biases.  Every
// source element is read at its own index: no row is read past its end.
__global__ __launch_bounds__(256) void k_smp_stage_q(const float* __restrict__ Wa, const float* __restrict__ ba, const float* __restrict__ Wb,
                                                      const float* __restrict__ bb, int QIN, int nh, float* __restrict__ wq,
                                                      float* __restrict__ bq) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nh * H1 * QK) return;
  const int r = i / QK, k = i - r * QK, h = r >= H1, rr = r - H1 * h;
  const float* W = h ? Wb : Wa;
  wq[i] = k < QIN ? W[(size_t)rr * QIN + k] : 0.f;
  if (i < nh * H1) bq[i] = i < H1 ? ba[i] : bb[i - H1];
}

// baseQ*.l3 (300 -> 1) of nh heads for every node, one wave per node; head h of limb l of env e goes to qe[h][e][l].
__global__ __launch_bounds__(256) void k_smp_q3(const float* __restrict__ h2q, const float* __restrict__ Wa, const float* __restrict__ ba,
                                                 const float* __restrict__ Wb, const float* __restrict__ bb, int nh, RowTab rt, int Lmax,
                                                 int n_env, float* __restrict__ qe, int N) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const size_t at = (size_t)rt.row_env[row] * Lmax + rt.row_limb[row];
  for (int h = 0; h < nh; h++) {
    const float* x = h2q + (size_t)row * (2 * H2) + H2 * h;
    const float* w = h ? Wb : Wa;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 5; i++)
      if (lane + 64 * i < H2) s = fmaf(x[lane + 64 * i], w[lane + 64 * i], s);
    s = wave_sum(s) + (h ? bb[0] : ba[0]);
    if (lane == 0) qe[(size_t)h * n_env * Lmax + at] = s;
  }
}

// The sum over the limbs of an environment (ModularCritic.py:286-290), one thread per environment, limbs in order 0 .. L - 1.
// TD: out1 = reward + (1 - done) * discount * min(q1, q2) (agent.py:136-148) instead of q1 / q2.
template <bool TD>
__global__ __launch_bounds__(256) void k_smp_qsum(const float* __restrict__ qe, const int32_t* __restrict__ env_L, int Lmax, int n_env,
                                                   int nh, float* __restrict__ out1, float* __restrict__ out2,
                                                   const float* __restrict__ reward, const float* __restrict__ done, float discount) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_env) return;
  const int L = env_L[e];
  float s1 = 0.f, s2 = 0.f;
  for (int l = 0; l < L; l++) s1 += qe[(size_t)e * Lmax + l];
  if (nh > 1)
    for (int l = 0; l < L; l++) s2 += qe[(size_t)(n_env + e) * Lmax + l];
  if (TD) {
    out1[e] = reward[e] + (1.0f - done[e]) * discount * fminf(s1, s2);
  } else {
    out1[e] = s1;
    if (nh > 1) out2[e] = s2;
  }
}

// C[M, N] = epi(A[M, K] . W[N, K]^T + b): 128 x 64 tiles, 4 waves, k-tiles of 16 (the configuration swat_actor.hip uses)
constexpr auto kGemm = k_gemm2<0, 4, 1, 1, 2, 16, 1>;
constexpr auto kGemmRelu = k_gemm2<EPI_RELU, 4, 1, 1, 2, 16, 1>;
constexpr int kGemmLds = sgrl_gemm::TileCfg<4, 1, 1, 2, 16>::kLdsBytes;

// K: multiple of 16 (the k range the product covers); ldw: row stride of W
void launch_gemm(hipStream_t st, bool relu, const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc,
                 int M, int N, int K) {
  GemmArgs a{};
  a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.bias = bias; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
  const dim3 grid(((M + 127) / 128) * ((N + 63) / 64));
  if (relu) hipLaunchKernelGGL(kGemmRelu, grid, dim3(256), kGemmLds, st, a);
  else hipLaunchKernelGGL(kGemm, grid, dim3(256), kGemmLds, st, a);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
struct SmpGraphCfg {
  std::vector<int32_t> key;     // n_morph | mc | L[] | count[] | tree[]
  int n_env = 0, N = 0, Lmax = 0, D = 0, mc = 0;
  int off[DMAX + 1] = {};       // first row of level d
  int nnl[DMAX] = {};           // limbs with children at level d (they come first)
  int32_t *d_row_env = nullptr, *d_row_limb = nullptr, *d_par = nullptr, *d_cidx = nullptr, *d_slot = nullptr, *d_ch = nullptr;
  int32_t* d_env_L = nullptr;
  uint64_t last_use = 0;
  void release() {
    void* ptrs[] = {d_row_env, d_row_limb, d_par, d_cidx, d_slot, d_ch, d_env_L};
    for (void* q : ptrs) if (q) (void)hipFree(q);
  }
};

enum { KIND_NONE = 0, KIND_ACTOR = 1, KIND_CRITIC = 2 };

struct sgrl_smp {
  const float* p[SGRL_SMP_NW] = {};       // KIND_ACTOR
  const float* pc[SGRL_SMPQ_NW] = {};     // KIND_CRITIC
  int kind = KIND_NONE;                   // what the last bind made of the handle
  int F = 41, O = 3, AF = 0, mc = 0;      // actor: F inputs, O outputs per limb; critic: F = obs + action inputs, AF of them action
  SmpGraphCfg* cur = nullptr;
  std::vector<SmpGraphCfg*> cfgs;
  uint64_t use_clock = 0;
  int64_t generation = 0;
  float* ws = nullptr;          // workspace, see ws_floats_for; grows only
  int64_t ws_floats = 0;
};

namespace {

template <class T>
int upload(T** dst, const std::vector<T>& v) {
  if (hipMalloc(dst, sizeof(T) * (v.size() ? v.size() : 1)) != hipSuccess) return -1;
  if (!v.empty() && hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
  return 0;
}

int64_t al64(int64_t n) { return (n + 63) & ~int64_t(63); }

// cat [N, 64 + 32 mc] (after the bottom-up pass: raw3 [<= N, 32 mc]) | raw2 [N, 64] | xm [N, 64] | h1 [N, 400] | h2 [N, 300]
// a critic's handle, behind those: xq [N, 80] | wq [800, 80] | bq [800] | h1q [N, 800] | h2q [N, 600] | qe [2, n_env, Lmax] |
// target action [n_env, 8 Lmax] (sgrl_smp_td_target)
int64_t ws_trunk_floats(int64_t N, int mc) { return al64(N * (HU + MSG * mc)) + 2 * al64(N * HU) + al64(N * H1) + al64(N * H2); }
int64_t ws_floats_for(const SmpGraphCfg* c, bool critic) {
  int64_t n = ws_trunk_floats(c->N, c->mc);
  if (critic)
    n += al64((int64_t)c->N * QK) + al64(2 * H1 * QK) + al64(2 * H1) + al64((int64_t)c->N * 2 * H1) + al64((int64_t)c->N * 2 * H2) +
         al64((int64_t)2 * c->n_env * c->Lmax) + al64((int64_t)c->n_env * AFMAX * c->Lmax);
  return n;
}

int use_cfg(sgrl_smp* s, SmpGraphCfg* c) {
  const int64_t need = ws_floats_for(c, s->kind == KIND_CRITIC);
  if (need > s->ws_floats) {
    if (s->ws) { (void)hipFree(s->ws); s->generation++; }      // hipFree waits for the device: no kernel still reads the old block
    s->ws = nullptr; s->ws_floats = 0;
    if (hipMalloc(&s->ws, sizeof(float) * need) != hipSuccess) { s->cur = nullptr; return mfail(SGRL_ERR_HIP, "device allocation failed (SMP workspace)"); }
    s->ws_floats = need;
  }
  c->last_use = ++s->use_clock;
  s->cur = c;
  return SGRL_OK;
}

struct Trunk {      // the tensors the actor and the critic share by role: ActorUp / CriticUp and msg_base
  const float *fc1w, *fc1b, *fc2w, *fc2b, *fc3w, *fc3b, *m1w, *m1b, *m2w, *m2b, *m3w, *m3b;
};

struct Ws {
  float *cat, *raw2, *xm, *h1, *h2, *raw3, *xq, *wq, *bq, *h1q, *h2q, *qe, *act_t;
};

Ws carve(const sgrl_smp* s) {
  const SmpGraphCfg* c = s->cur;
  const int64_t N = c->N;
  Ws w{};
  w.cat = s->ws;
  w.raw2 = w.cat + al64(N * (HU + MSG * c->mc));
  w.xm = w.raw2 + al64(N * HU);
  w.h1 = w.xm + al64(N * HU);
  w.h2 = w.h1 + al64(N * H1);
  w.raw3 = w.cat;                            // the fc2 inputs are dead once the bottom-up pass is over
  if (s->kind == KIND_CRITIC) {
    w.xq = w.h2 + al64(N * H2);
    w.wq = w.xq + al64(N * QK);
    w.bq = w.wq + al64(2 * H1 * QK);
    w.h1q = w.bq + al64(2 * H1);
    w.h2q = w.h1q + al64(N * 2 * H1);
    w.qe = w.h2q + al64(N * 2 * H2);
    w.act_t = w.qe + al64((int64_t)2 * c->n_env * c->Lmax);
  }
  return w;
}

// embedding, bottom-up and top-down passes: 6 D - 3 launches
template <bool CRITIC>
void run_trunk(const sgrl_smp* s, const Trunk& T, const Ws& w, const float* obs, int obs_ld, const float* action, int act_ld,
               hipStream_t st) {
  const SmpGraphCfg* c = s->cur;
  const int N = c->N, mc = c->mc, K1 = HU + MSG * mc, MC = MSG * mc, D = c->D;
  const RowTab rt{c->d_row_env, c->d_row_limb, c->d_par, c->d_cidx, c->d_slot, c->d_ch};
  hipLaunchKernelGGL(k_smp_embed<CRITIC>, dim3((N + kEmbedRows - 1) / kEmbedRows), dim3(256), 0, st, obs, obs_ld, s->F, action, act_ld,
                     s->AF, T.fc1w, T.fc1b, rt, w.cat, K1, w.xm, w.xq, N);
  for (int d = D - 1; d >= 0; d--) {
    const int r0 = c->off[d], n = c->off[d + 1] - r0;
    launch_gemm(st, false, w.cat + (size_t)r0 * K1, K1, T.fc2w, K1, T.fc2b, w.raw2 + (size_t)r0 * HU, HU, n, HU, K1);
    hipLaunchKernelGGL(k_smp_up<CRITIC>, dim3((n + kUpRows - 1) / kUpRows), dim3(256), 0, st, w.raw2, T.fc3w, T.fc3b, rt, w.cat, K1,
                       w.xm, w.xq, r0, n);
  }
  for (int d = 0; d + 1 < D; d++) {
    const int r0 = c->off[d], n = c->nnl[d];
    launch_gemm(st, true, w.xm + (size_t)r0 * HU, HU, T.m1w, HU, T.m1b, w.h1, H1, n, H1, HU);
    launch_gemm(st, true, w.h1, H1, T.m2w, H1, T.m2b, w.h2, H2, n, H2, H1);
    launch_gemm(st, false, w.h2, H2, T.m3w, H2, T.m3b, w.raw3, MC, n, MC, H2G);
    hipLaunchKernelGGL(k_smp_down<CRITIC>, dim3((n + 3) / 4), dim3(256), 0, st, w.raw3, w.h2, T.m3w, rt, mc, w.xm, w.xq, s->AF, r0, n);
  }
}

// noise == nullptr: the plain forward; else the target actor of a TD3 update
int run_forward(sgrl_smp* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, const float* noise, int noise_ld,
                float noise_clip, hipStream_t st) {
  const SmpGraphCfg* c = s->cur;
  const int N = c->N;
  const Ws w = carve(s);
  const RowTab rt{c->d_row_env, c->d_row_limb, c->d_par, c->d_cidx, c->d_slot, c->d_ch};
  auto W = [&](int slot) { return s->p[slot]; };
  const Trunk T{W(SGRL_SMP_FC1_W), W(SGRL_SMP_FC1_B), W(SGRL_SMP_FC2_W), W(SGRL_SMP_FC2_B), W(SGRL_SMP_FC3_W), W(SGRL_SMP_FC3_B),
                W(SGRL_SMP_MSG1_W), W(SGRL_SMP_MSG1_B), W(SGRL_SMP_MSG2_W), W(SGRL_SMP_MSG2_B), W(SGRL_SMP_MSG3_W), W(SGRL_SMP_MSG3_B)};
  run_trunk<false>(s, T, w, obs, obs_ld, nullptr, 0, st);
  launch_gemm(st, true, w.xm, HU, W(SGRL_SMP_ACT1_W), HU, W(SGRL_SMP_ACT1_B), w.h1, H1, N, H1, HU);
  launch_gemm(st, true, w.h1, H1, W(SGRL_SMP_ACT2_W), H1, W(SGRL_SMP_ACT2_B), w.h2, H2, N, H2, H1);
  if (noise)
    hipLaunchKernelGGL(k_smp_action<true>, dim3((N + 3) / 4), dim3(256), 0, st, w.h2, W(SGRL_SMP_ACT3_W), W(SGRL_SMP_ACT3_B), s->O, rt,
                       c->d_env_L, act, act_ld, max_action, noise, noise_ld, noise_clip, N);
  else
    hipLaunchKernelGGL(k_smp_action<false>, dim3((N + 3) / 4), dim3(256), 0, st, w.h2, W(SGRL_SMP_ACT3_W), W(SGRL_SMP_ACT3_B), s->O, rt,
                       c->d_env_L, act, act_ld, max_action, nullptr, 0, 0.f, N);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("SMP forward launch: ") + hipGetErrorString(e));
  return SGRL_OK;
}

// twin critic: nh = 2 heads, or Q1 only.  reward != nullptr: the Bellman target goes to out1 instead of q1 / q2.
int run_forward_q(sgrl_smp* s, const float* obs, int obs_ld, const float* action, int act_ld, int nh, float* out1, float* out2,
                  const float* reward, const float* done, float discount, hipStream_t st) {
  const SmpGraphCfg* c = s->cur;
  const int N = c->N, QIN = HU + s->AF;
  const Ws w = carve(s);
  const RowTab rt{c->d_row_env, c->d_row_limb, c->d_par, c->d_cidx, c->d_slot, c->d_ch};
  auto W = [&](int slot) { return s->pc[slot]; };
  const Trunk T{W(SGRL_SMPQ_FC1_W), W(SGRL_SMPQ_FC1_B), W(SGRL_SMPQ_FC2_W), W(SGRL_SMPQ_FC2_B), W(SGRL_SMPQ_FC3_W), W(SGRL_SMPQ_FC3_B),
                W(SGRL_SMPQ_MSG1_W), W(SGRL_SMPQ_MSG1_B), W(SGRL_SMPQ_MSG2_W), W(SGRL_SMPQ_MSG2_B), W(SGRL_SMPQ_MSG3_W), W(SGRL_SMPQ_MSG3_B)};
  run_trunk<true>(s, T, w, obs, obs_ld, action, act_ld, st);
  hipLaunchKernelGGL(k_smp_stage_q, dim3((nh * H1 * QK + 255) / 256), dim3(256), 0, st, W(SGRL_SMPQ_Q1L1_W), W(SGRL_SMPQ_Q1L1_B),
                     W(SGRL_SMPQ_Q2L1_W), W(SGRL_SMPQ_Q2L1_B), QIN, nh, w.wq, w.bq);
  launch_gemm(st, true, w.xq, QK, w.wq, QK, w.bq, w.h1q, 2 * H1, N, nh * H1, QK);
  launch_gemm(st, true, w.h1q, 2 * H1, W(SGRL_SMPQ_Q1L2_W), H1, W(SGRL_SMPQ_Q1L2_B), w.h2q, 2 * H2, N, H2, H1);
  if (nh > 1)
    launch_gemm(st, true, w.h1q + H1, 2 * H1, W(SGRL_SMPQ_Q2L2_W), H1, W(SGRL_SMPQ_Q2L2_B), w.h2q + H2, 2 * H2, N, H2, H1);
  hipLaunchKernelGGL(k_smp_q3, dim3((N + 3) / 4), dim3(256), 0, st, w.h2q, W(SGRL_SMPQ_Q1L3_W), W(SGRL_SMPQ_Q1L3_B), W(SGRL_SMPQ_Q2L3_W),
                     W(SGRL_SMPQ_Q2L3_B), nh, rt, c->Lmax, c->n_env, w.qe, N);
  const dim3 ge((c->n_env + 255) / 256);
  if (reward)
    hipLaunchKernelGGL(k_smp_qsum<true>, ge, dim3(256), 0, st, w.qe, c->d_env_L, c->Lmax, c->n_env, nh, out1, out2, reward, done, discount);
  else
    hipLaunchKernelGGL(k_smp_qsum<false>, ge, dim3(256), 0, st, w.qe, c->d_env_L, c->Lmax, c->n_env, nh, out1, out2, nullptr, nullptr, 0.f);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("SMP critic forward launch: ") + hipGetErrorString(e));
  return SGRL_OK;
}

// what every forward checks of a handle before it launches anything
int ready(const sgrl_smp* s, int kind, const char* fn) {
  const std::string f(fn);
  if (s->kind != kind)
    return mfail(SGRL_ERR_ARG, kind == KIND_CRITIC ? f + ": the handle is not bound as a critic (sgrl_smp_bind_critic_params)"
                                                   : f + ": the handle is not bound as an actor (sgrl_smp_bind_params)");
  if (!s->cur) return mfail(SGRL_ERR_ARG, f + ": parameters or batch structure not set");
  if (s->cur->mc != s->mc)
    return mfail(SGRL_ERR_ARG, f + ": the batch structure was built for max_children " + std::to_string(s->cur->mc) +
                                   ", the bound parameters for " + std::to_string(s->mc));
  if (ws_floats_for(s->cur, kind == KIND_CRITIC) > s->ws_floats) return mfail(SGRL_ERR_ARG, f + ": workspace smaller than the batch structure needs");
  return SGRL_OK;
}

}  // namespace

extern "C" {

int sgrl_smp_create(sgrl_smp** out) {
  if (!out) return mfail(SGRL_ERR_ARG, "out is null");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return mfail(SGRL_ERR_HIP, "no HIP device visible: the SMP actor forward needs an MI355X (there is no CPU fallback)");
  *out = new sgrl_smp();
  return SGRL_OK;
}

void sgrl_smp_destroy(sgrl_smp* s) {
  if (!s) return;
  for (SmpGraphCfg* c : s->cfgs) { c->release(); delete c; }
  if (s->ws) (void)hipFree(s->ws);
  delete s;
}

int sgrl_smp_bind_params(sgrl_smp* s, const void* const* ptrs, int n, int max_children, int feature, int out) {
  if (!s || !ptrs) return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_params: null argument");
  if (n != SGRL_SMP_NW)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_params: expected " + std::to_string((int)SGRL_SMP_NW) + " parameter addresses, got " + std::to_string(n));
  if (max_children < 1 || max_children > MCMAX) return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_params: need 1 <= max_children <= 8");
  if (feature < 1 || feature > 64 || out < 1 || out > 8) return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_params: need 1 <= feature <= 64, 1 <= out <= 8");
  for (int i = 0; i < n; i++)
    if (!ptrs[i] || (reinterpret_cast<uintptr_t>(ptrs[i]) & 15))
      return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_params: parameter " + std::to_string(i) + " is null or not 16-byte aligned");
  for (int i = 0; i < n; i++) s->p[i] = static_cast<const float*>(ptrs[i]);
  s->mc = max_children;
  s->F = feature;
  s->O = out;
  s->AF = 0;
  s->kind = KIND_ACTOR;
  return SGRL_OK;
}

int sgrl_smp_bind_critic_params(sgrl_smp* s, const void* const* ptrs, int n, int max_children, int feature, int act_feature) {
  if (!s || !ptrs) return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_critic_params: null argument");
  if (n != SGRL_SMPQ_NW)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_critic_params: expected " + std::to_string((int)SGRL_SMPQ_NW) + " parameter addresses, got " + std::to_string(n));
  if (max_children < 1 || max_children > MCMAX) return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_critic_params: need 1 <= max_children <= 8");
  if (feature < 2 || feature > 64 || act_feature < 1 || act_feature > AFMAX || act_feature >= feature)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_critic_params: need 2 <= feature <= 64, 1 <= act_feature <= 8, act_feature < feature");
  for (int i = 0; i < n; i++)
    if (!ptrs[i] || (reinterpret_cast<uintptr_t>(ptrs[i]) & 15))
      return mfail(SGRL_ERR_ARG, "sgrl_smp_bind_critic_params: parameter " + std::to_string(i) + " is null or not 16-byte aligned");
  for (int i = 0; i < n; i++) s->pc[i] = static_cast<const float*>(ptrs[i]);
  s->mc = max_children;
  s->F = feature;
  s->AF = act_feature;
  s->O = 1;
  s->kind = KIND_CRITIC;
  if (s->cur) return use_cfg(s, s->cur);      // a structure set before the bind: the critic's share of the workspace
  return SGRL_OK;
}

int sgrl_smp_graph(sgrl_smp* s, int n_morph, const int32_t* morph_L, const int32_t* morph_count, int max_children, const int32_t* tree) {
  if (!s || n_morph <= 0 || !morph_L || !morph_count || !tree) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: bad argument");
  const int mc = max_children, W = 3 + mc;
  if (mc < 1 || mc > MCMAX) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: need 1 <= max_children <= 8");
  size_t ntree = 0;
  for (int k = 0; k < n_morph; k++) {
    if (morph_L[k] < 1 || morph_L[k] > LMAX)
      return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: limb count " + std::to_string(morph_L[k]) + " outside [1, 16]");
    if (morph_count[k] < 0) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: negative morph_count");
    ntree += (size_t)morph_L[k] * W;
  }
  std::vector<int32_t> key;
  key.push_back(n_morph);
  key.push_back(mc);
  key.insert(key.end(), morph_L, morph_L + n_morph);
  key.insert(key.end(), morph_count, morph_count + n_morph);
  key.insert(key.end(), tree, tree + ntree);
  for (SmpGraphCfg* c : s->cfgs)
    if (c->key == key) return use_cfg(s, c);        // seen before: no allocation, upload or synchronisation
  // the rows must describe a forest laid out by level: every index the kernels follow is checked here
  int D = 0, Lmax = 0;
  int64_t cnt_nl[DMAX] = {}, cnt_leaf[DMAX] = {};
  std::vector<const int32_t*> mt(n_morph);
  {
    const int32_t* tp = tree;
    for (int k = 0; k < n_morph; k++) {
      const int L = morph_L[k];
      mt[k] = tp;
      tp += (size_t)L * W;
      if (L > Lmax) Lmax = L;
      for (int i = 0; i < L; i++) {
        const int32_t* r = mt[k] + (size_t)i * W;
        const int lev = r[0], par = r[1], slot = r[2];
        if (lev < 0 || lev >= DMAX) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: tree level outside [0, 16)");
        if (par < -1 || par >= L || par == i) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: parent index out of range");
        if (slot < 0 || slot >= mc) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: message slot outside [0, max_children)");
        if (par < 0 ? lev != 0 : lev != mt[k][(size_t)par * W] + 1)
          return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: a limb must sit one level below its parent (roots at level 0)");
        int found = 0, nch = 0;
        for (int q = 0; q < mc; q++) {
          const int ch = r[3 + q];
          if (ch < -1 || ch >= L) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: child index out of range");
          if (ch >= 0) {
            if (mt[k][(size_t)ch * W + 1] != i) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: a children row lists a limb whose parent is another limb");
            nch++;
          }
          if (par >= 0 && mt[k][(size_t)par * W + 3 + q] == i) found++;
        }
        if (par >= 0 && found != 1)
          return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: limb " + std::to_string(i) + " must appear exactly once among its parent's " +
                                         std::to_string(mc) + " children slots (more children than max_children?)");
        (nch ? cnt_nl : cnt_leaf)[lev] += morph_count[k];
        if (morph_count[k] > 0 && lev + 1 > D) D = lev + 1;
      }
    }
  }
  int64_t N64 = 0;
  for (int d = 0; d < D; d++) N64 += cnt_nl[d] + cnt_leaf[d];
  if (N64 == 0) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: no environments");
  if (N64 > (int64_t)1 << 24) return mfail(SGRL_ERR_ARG, "sgrl_smp_graph: more than 2^24 nodes in one batch");
  SmpGraphCfg* c = new SmpGraphCfg();
  int cur_nl[DMAX], cur_leaf[DMAX];
  for (int d = 0; d < D; d++) {
    c->off[d + 1] = c->off[d] + (int)(cnt_nl[d] + cnt_leaf[d]);
    c->nnl[d] = (int)cnt_nl[d];
    cur_nl[d] = c->off[d];
    cur_leaf[d] = c->off[d] + (int)cnt_nl[d];
  }
  const int N = (int)N64;
  std::vector<int32_t> row_env(N), row_limb(N), par(N), cidx(N), slot(N), ch((size_t)N * mc), env_L;
  int env = 0;
  for (int k = 0; k < n_morph; k++) {
    const int L = morph_L[k];
    int rowof[LMAX];
    for (int e = 0; e < morph_count[k]; e++, env++) {
      env_L.push_back(L);
      for (int i = 0; i < L; i++) {
        const int32_t* r = mt[k] + (size_t)i * W;
        bool leaf = true;
        for (int q = 0; q < mc; q++) leaf = leaf && r[3 + q] < 0;
        rowof[i] = leaf ? cur_leaf[r[0]]++ : cur_nl[r[0]]++;
      }
      for (int i = 0; i < L; i++) {
        const int32_t* r = mt[k] + (size_t)i * W;
        const int row = rowof[i];
        row_env[row] = env;
        row_limb[row] = i;
        par[row] = r[1] >= 0 ? rowof[r[1]] : -1;
        slot[row] = r[2];
        int ci = 0;
        if (r[1] >= 0)
          for (int q = 0; q < mc; q++) if (mt[k][(size_t)r[1] * W + 3 + q] == i) ci = q;
        cidx[row] = ci;
        for (int q = 0; q < mc; q++) ch[(size_t)row * mc + q] = r[3 + q] >= 0 ? rowof[r[3 + q]] : -1;
      }
    }
  }
  if ((int)s->cfgs.size() >= SGRL_SMP_GRAPH_CACHE) {      // evict the least recently used structure
    size_t lru = 0;
    for (size_t i = 1; i < s->cfgs.size(); i++) if (s->cfgs[i]->last_use < s->cfgs[lru]->last_use) lru = i;
    if (s->cfgs[lru] == s->cur) s->cur = nullptr;
    s->cfgs[lru]->release();                               // hipFree waits for the device
    s->generation++;
    delete s->cfgs[lru];
    s->cfgs.erase(s->cfgs.begin() + lru);
  }
  c->key = std::move(key);
  c->n_env = env; c->N = N; c->Lmax = Lmax; c->D = D; c->mc = mc;
  const bool ok = upload(&c->d_row_env, row_env) == 0 && upload(&c->d_row_limb, row_limb) == 0 && upload(&c->d_par, par) == 0 &&
                  upload(&c->d_cidx, cidx) == 0 && upload(&c->d_slot, slot) == 0 && upload(&c->d_ch, ch) == 0 &&
                  upload(&c->d_env_L, env_L) == 0;
  if (!ok) { c->release(); delete c; return mfail(SGRL_ERR_HIP, "device allocation failed in sgrl_smp_graph"); }
  s->cfgs.push_back(c);
  return use_cfg(s, c);
}

int sgrl_smp_forward(sgrl_smp* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, void* stream) {
  if (!s || !obs || !act) return mfail(SGRL_ERR_ARG, "sgrl_smp_forward: null argument");
  if (s->kind == KIND_NONE || !s->cur) return mfail(SGRL_ERR_ARG, "sgrl_smp_forward: parameters or batch structure not set");
  if (const int rc = ready(s, KIND_ACTOR, "sgrl_smp_forward")) return rc;
  if (obs_ld < s->F * s->cur->Lmax || act_ld < s->O * s->cur->Lmax)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_forward: obs_ld < feature * Lmax or act_ld < out * Lmax (rows too narrow for the largest morphology)");
  return run_forward(s, obs, obs_ld, act, act_ld, max_action, nullptr, 0, 0.f, (hipStream_t)stream);
}

int sgrl_smp_forward_q(sgrl_smp* s, const float* obs, int obs_ld, const float* action, int act_ld, float* q1, float* q2, void* stream) {
  if (!s || !obs || !action || !q1) return mfail(SGRL_ERR_ARG, "sgrl_smp_forward_q: null argument");
  if (const int rc = ready(s, KIND_CRITIC, "sgrl_smp_forward_q")) return rc;
  if (obs_ld < (s->F - s->AF) * s->cur->Lmax || act_ld < s->AF * s->cur->Lmax)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_forward_q: obs_ld < (feature - act_feature) * Lmax or act_ld < act_feature * Lmax (rows too narrow "
                               "for the largest morphology)");
  return run_forward_q(s, obs, obs_ld, action, act_ld, q2 ? 2 : 1, q1, q2, nullptr, nullptr, 0.f, (hipStream_t)stream);
}

int sgrl_smp_td_target(sgrl_smp* a, sgrl_smp* c, const float* next_obs, int obs_ld, const float* noise, int noise_ld, const float* reward,
                       const float* done, float max_action, float noise_clip, float discount, float* target_q, void* stream) {
  if (!a || !c || !next_obs || !noise || !reward || !done || !target_q) return mfail(SGRL_ERR_ARG, "sgrl_smp_td_target: null argument");
  if (const int rc = ready(a, KIND_ACTOR, "sgrl_smp_td_target (actor_t)")) return rc;
  if (const int rc = ready(c, KIND_CRITIC, "sgrl_smp_td_target (critic_t)")) return rc;
  if (a->cur->key != c->cur->key)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_td_target: the two handles hold different batch structures");
  if (c->F != a->F + a->O || c->AF != a->O)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_td_target: the critic's feature must be the actor's feature + out and its act_feature the actor's out");
  const int Lmax = a->cur->Lmax;
  if (obs_ld < a->F * Lmax || noise_ld < a->O * Lmax)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_td_target: obs_ld < feature * Lmax or noise_ld < out * Lmax (rows too narrow for the largest morphology)");
  float* act_t = carve(c).act_t;
  const int act_ld = a->O * Lmax;
  if (const int rc = run_forward(a, next_obs, obs_ld, act_t, act_ld, max_action, noise, noise_ld, noise_clip, (hipStream_t)stream)) return rc;
  return run_forward_q(c, next_obs, obs_ld, act_t, act_ld, 2, target_q, nullptr, reward, done, discount, (hipStream_t)stream);
}

int sgrl_smp_num_nodes(const sgrl_smp* s) { return (s && s->cur) ? s->cur->N : SGRL_ERR_ARG; }
int sgrl_smp_num_levels(const sgrl_smp* s) { return (s && s->cur) ? s->cur->D : SGRL_ERR_ARG; }
int sgrl_smp_launches(const sgrl_smp* s) { return (s && s->cur) ? 6 * s->cur->D : SGRL_ERR_ARG; }
int sgrl_smp_forward_q_launches(const sgrl_smp* s, int twin) { return (s && s->cur) ? 6 * s->cur->D + 2 + (twin ? 1 : 0) : SGRL_ERR_ARG; }
int sgrl_smp_td_target_launches(const sgrl_smp* s) { return (s && s->cur) ? 12 * s->cur->D + 3 : SGRL_ERR_ARG; }
int64_t sgrl_smp_generation(const sgrl_smp* s) { return s ? s->generation : -1; }
const char* sgrl_smp_last_error(void) { return g_smp_err.c_str(); }

}  // extern "C"
