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
constexpr int kEmbedRows = 16;
__global__ __launch_bounds__(256) void k_smp_embed(const float* __restrict__ obs, int obs_ld, int F, const float* __restrict__ W1,
                                                    const float* __restrict__ b1, RowTab rt, float* __restrict__ cat, int K1,
                                                    float* __restrict__ xm, int N) {
  __shared__ float xs[kEmbedRows][64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, rb = blockIdx.x * kEmbedRows;
  for (int i = t; i < kEmbedRows * 64; i += 256) {
    const int r = i >> 6, k = i & 63, n = rb + r;
    float v = 0.f;
    if (n < N && k < F) v = obs[(size_t)rt.row_env[n] * obs_ld + F * rt.row_limb[n] + k];
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
  }
}

// second half of ActorUp for the rows [r0, r0 + n) of one level: up = normalize(fc3 tanh(raw2) + b) (ModularActor.py:41-47).  Only
// tanh(up) is ever read again -- by the parent's fc2 input (ModularActor.py:37 applies tanh to the concatenation) and by the
// node's own top-down input (ModularActor.py:84) -- so that is what is stored, in both places.  32 rows per 256-thread block:
// fc3 (8 KB) and the block's tanh(raw2) rows live in LDS, a thread owns output j of rows rr, rr + 8, rr + 16, rr + 24.
constexpr int kUpRows = 32;
__global__ __launch_bounds__(256) void k_smp_up(const float* __restrict__ raw2, const float* __restrict__ W3, const float* __restrict__ b3,
                                                 RowTab rt, float* __restrict__ cat, int K1, float* __restrict__ xm, int r0, int n) {
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
    const float tv = tanhf(u / norm_div(ss));
    if (row < rend) {
      xm[(size_t)row * HU + j] = tv;
      const int pr = rt.par[row];
      if (pr >= 0) cat[(size_t)pr * K1 + HU + MSG * rt.cidx[row] + j] = tv;
    }
  }
}

// end of msg_base for the n limbs-with-children of one level (rows r0 .. r0 + n of the batch, rows 0 .. n of raw3 / h2): the last
// 12 k terms of l3, down = normalize(.) over the whole 32 mc vector (ModularActor.py:93-96), and the scatter: child c reads slot
// rt.slot[c] of it, through the tanh of its own top-down input (ModularActor.py:84).  One wave per row, column = lane + 64 q.
__global__ __launch_bounds__(256) void k_smp_down(const float* __restrict__ raw3, const float* __restrict__ h2, const float* __restrict__ W3,
                                                   RowTab rt, int mc, float* __restrict__ xm, int r0, int n) {
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
#pragma unroll
  for (int q = 0; q < 4; q++) v[q] = tanhf(v[q] / den);
  for (int k = 0; k < mc; k++) {
    const int c = rt.ch[(size_t)row * mc + k];
    if (c < 0) continue;                                      // wave-uniform
    const int sc = rt.slot[c], q = sc >> 1;                   // slot sc = columns 32 sc .. 32 sc + 31 = half (sc & 1) of register q
    const float val = q == 0 ? v[0] : (q == 1 ? v[1] : (q == 2 ? v[2] : v[3]));
    if ((lane >> 5) == (sc & 1)) xm[(size_t)c * HU + MSG + (lane & 31)] = val;
  }
}

// action_base.l3 and max_action * tanh (ModularActor.py:86-92) for every node, one wave per node; the node of limb 0 of every
// environment also writes the zero padding act[e, out * L_e : act_ld].
__global__ __launch_bounds__(256) void k_smp_action(const float* __restrict__ h2, const float* __restrict__ W3, const float* __restrict__ b3,
                                                     int O, RowTab rt, const int32_t* __restrict__ env_L, float* __restrict__ act, int act_ld,
                                                     float max_action, int N) {
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
    if (lane == 0) arow[O * limb + j] = max_action * tanhf(s);
  }
  if (limb == 0)
    for (int k = O * env_L[env] + lane; k < act_ld; k += 64) arow[k] = 0.f;
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

struct sgrl_smp {
  const float* p[SGRL_SMP_NW] = {};
  bool have_w = false;
  int F = 41, O = 3, mc = 0;
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
int64_t ws_floats_for(int64_t N, int mc) { return al64(N * (HU + MSG * mc)) + 2 * al64(N * HU) + al64(N * H1) + al64(N * H2); }

int use_cfg(sgrl_smp* s, SmpGraphCfg* c) {
  const int64_t need = ws_floats_for(c->N, c->mc);
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

int run_forward(sgrl_smp* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, hipStream_t st) {
  const SmpGraphCfg* c = s->cur;
  const int N = c->N, mc = c->mc, K1 = HU + MSG * mc, MC = MSG * mc, D = c->D;
  float* cat = s->ws;
  float* raw2 = cat + al64((int64_t)N * K1);
  float* xm = raw2 + al64((int64_t)N * HU);
  float* h1 = xm + al64((int64_t)N * HU);
  float* h2 = h1 + al64((int64_t)N * H1);
  float* raw3 = cat;                         // the fc2 inputs are dead once the bottom-up pass is over
  const RowTab rt{c->d_row_env, c->d_row_limb, c->d_par, c->d_cidx, c->d_slot, c->d_ch};
  auto W = [&](int slot) { return s->p[slot]; };
  hipLaunchKernelGGL(k_smp_embed, dim3((N + kEmbedRows - 1) / kEmbedRows), dim3(256), 0, st, obs, obs_ld, s->F, W(SGRL_SMP_FC1_W),
                     W(SGRL_SMP_FC1_B), rt, cat, K1, xm, N);
  for (int d = D - 1; d >= 0; d--) {
    const int r0 = c->off[d], n = c->off[d + 1] - r0;
    launch_gemm(st, false, cat + (size_t)r0 * K1, K1, W(SGRL_SMP_FC2_W), K1, W(SGRL_SMP_FC2_B), raw2 + (size_t)r0 * HU, HU, n, HU, K1);
    hipLaunchKernelGGL(k_smp_up, dim3((n + kUpRows - 1) / kUpRows), dim3(256), 0, st, raw2, W(SGRL_SMP_FC3_W), W(SGRL_SMP_FC3_B), rt,
                       cat, K1, xm, r0, n);
  }
  for (int d = 0; d + 1 < D; d++) {
    const int r0 = c->off[d], n = c->nnl[d];
    launch_gemm(st, true, xm + (size_t)r0 * HU, HU, W(SGRL_SMP_MSG1_W), HU, W(SGRL_SMP_MSG1_B), h1, H1, n, H1, HU);
    launch_gemm(st, true, h1, H1, W(SGRL_SMP_MSG2_W), H1, W(SGRL_SMP_MSG2_B), h2, H2, n, H2, H1);
    launch_gemm(st, false, h2, H2, W(SGRL_SMP_MSG3_W), H2, W(SGRL_SMP_MSG3_B), raw3, MC, n, MC, H2G);
    hipLaunchKernelGGL(k_smp_down, dim3((n + 3) / 4), dim3(256), 0, st, raw3, h2, W(SGRL_SMP_MSG3_W), rt, mc, xm, r0, n);
  }
  launch_gemm(st, true, xm, HU, W(SGRL_SMP_ACT1_W), HU, W(SGRL_SMP_ACT1_B), h1, H1, N, H1, HU);
  launch_gemm(st, true, h1, H1, W(SGRL_SMP_ACT2_W), H1, W(SGRL_SMP_ACT2_B), h2, H2, N, H2, H1);
  hipLaunchKernelGGL(k_smp_action, dim3((N + 3) / 4), dim3(256), 0, st, h2, W(SGRL_SMP_ACT3_W), W(SGRL_SMP_ACT3_B), s->O, rt, c->d_env_L,
                     act, act_ld, max_action, N);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("SMP forward launch: ") + hipGetErrorString(e));
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
  s->have_w = true;
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
  if (!s->have_w || !s->cur) return mfail(SGRL_ERR_ARG, "sgrl_smp_forward: parameters or batch structure not set");
  if (s->cur->mc != s->mc)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_forward: the batch structure was built for max_children " + std::to_string(s->cur->mc) +
                                   ", the bound parameters for " + std::to_string(s->mc));
  if (obs_ld < s->F * s->cur->Lmax || act_ld < s->O * s->cur->Lmax)
    return mfail(SGRL_ERR_ARG, "sgrl_smp_forward: obs_ld < feature * Lmax or act_ld < out * Lmax (rows too narrow for the largest morphology)");
  return run_forward(s, obs, obs_ld, act, act_ld, max_action, (hipStream_t)stream);
}

int sgrl_smp_num_nodes(const sgrl_smp* s) { return (s && s->cur) ? s->cur->N : SGRL_ERR_ARG; }
int sgrl_smp_num_levels(const sgrl_smp* s) { return (s && s->cur) ? s->cur->D : SGRL_ERR_ARG; }
int sgrl_smp_launches(const sgrl_smp* s) { return (s && s->cur) ? 6 * s->cur->D : SGRL_ERR_ARG; }
int64_t sgrl_smp_generation(const sgrl_smp* s) { return s ? s->generation : -1; }
const char* sgrl_smp_last_error(void) { return g_smp_err.c_str(); }

}  // extern "C"
