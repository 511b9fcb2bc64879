// swat_actor.hip -- batched HIP forward of the SWAT actor (structure-aware transformer, reference src/StructureActor.py:17-273)
// behind the C ABI of include/sgrl_swat.h.
//
// One forward over a batch of mixed morphologies = 22 launches on the caller's stream, whatever the number of morphologies:
//   k_swat_embed                  h = (x . Wenc^T + b) * sqrt(128) + [emb0[pre] | emb1[inlcrs] | emb2[postlcrs]]
//   per layer l = 0, 1, 2 (post-norm, StructureActor.py:52-64):
//     k_gemm2                     qkv = h . in_proj^T + b                                  [N, 384]
//     k_swat_attn                 o = softmax(q k^T / 8 (+ rel . Wrel^T + brel on layer 0)) v, one workgroup per environment
//     k_gemm2                     d = o . out_proj^T + b
//     k_swat_add_ln               h = norm1(h + d)
//     k_gemm2 (ReLU)              f = relu(h . linear1^T + b)                              [N, 256]
//     k_gemm2                     d = f . linear2^T + b
//     k_swat_add_ln / k_swat_tail h = norm2(h + d); after the last layer the tail also applies the final LayerNorm
//                                 (transformer_norm), the decoder over h or [h | x] and max_action * tanh, and zeroes the
//                                 padding slots of the action rows
// Every product is exact f32 (v_mfma_f32_32x32x2_f32 in k_gemm2; the row kernels are plain f32 FMA chains).  The weights are
// read through the addresses bound by sgrl_swat_bind_params on every forward: nothing is packed, nothing is cached.
//
// The same 22 launches serve a CRITIC network (feature = 44, out = 1: sgrl_swat_forward_q): the embedding and the cond_decoder
// branch of the tail read a limb's input row from two buffers, [obs 41 | action 3], where they lie, and the tail stores the
// decoder output as it is.  The twin critic (sgrl_swat_forward_twin) is two such chains, the second on the first handle's side
// stream between a fork and a join event (44 launches); the TD3 target chain (sgrl_swat_td_target, 66 launches) is the target
// actor's chain, whose tail adds the clipped noise and clamps, followed by the twin, whose first tail waits for the second
// network's values and stores reward + (1 - done) * discount * min(Q1, Q2).
//
// Dropout entries (sgrl_swat_forward_dropout / _forward_q_dropout / _td_target_dropout: a network in TRAINING mode, batches of one
// morphology): the row kernels are templates over NoDrop | Drop; the Drop instantiations apply the counter-RNG masks of
// dropout_rng.h at the 13 sites of swat_policy.TransformerModel.forward, in its program order --
//   site 0          pos_encoder output [L, 128]           k_swat_embed, on pos before it is added (one mask for every environment)
//   site 1 + 4 l    softmax weights [B, 2, L, L]          k_swat_attn, on s_p after normalisation
//   site 2 + 4 l    out_proj output [B, L, 128]           k_swat_add_ln, on d before h + d
//   site 3 + 4 l    relu(linear1) [B, L, 256]             k_swat_drop_quads, in place between the two products (gemm_f32.h is shared
//                                                         with the SET forward and stays as it is)
//   site 4 + 4 l    linear2 output [B, L, 128]            k_swat_add_ln / k_swat_tail, on d
// -- each over the row-major index of the tensor the module drops; the step is read from device memory.  25 launches per network,
// 75 per chain.  The NoDrop instantiations are the plain entries' kernels: the same code as before the template.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sgrl.h"
#include "../../include/sgrl_swat.h"
#include "dropout_rng.h"

// gemm_f32.h defines a few non-template kernels and device variables for the SET actor's translation unit; included here in an
// unnamed namespace, this translation unit gets its own copies with internal linkage (no duplicate symbols at link time).
namespace {
#include "gemm_f32.h"
}

namespace {

thread_local std::string g_swat_err;
int wfail(int code, const std::string& msg) { g_swat_err = msg; return code; }

constexpr int E = 128;          // embedding
constexpr int HD = 64;          // head dim (2 heads)
constexpr int FF = 256;         // feed-forward
constexpr int LMAX = SGRL_SWAT_MAX_LIMBS;
constexpr int kLaunches = 1 + SGRL_SWAT_LAYERS * 7;
constexpr int kDropSites = 1 + SGRL_SWAT_LAYERS * 4;           // dropout sites of one network
constexpr int kDropLaunches = kLaunches + SGRL_SWAT_LAYERS;    // + one k_swat_drop_quads per layer

using sgrl_gemm::EPI_RELU;
using sgrl_gemm::GemmArgs;
using sgrl_gemm::k_gemm2;

__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// What a kernel needs to drop at ONE site (dropout_rng.h): word = replay_word(seed, *step, stream, i), keep = word >= thr,
// y = keep ? x * scale : 0.  NoDrop is the empty argument of the plain instantiations.
struct NoDrop {
  static constexpr bool on = false;
};
struct Drop {
  static constexpr bool on = true;
  uint64_t thr, seed;
  const uint64_t* step;   // device
  float scale;
  uint32_t stream;        // 0x100 + site
};
__device__ __forceinline__ uint64_t drop_step(const NoDrop&) { return 0; }
__device__ __forceinline__ uint64_t drop_step(const Drop& d) { return d.step[0]; }
__device__ __forceinline__ float dropped(const Drop& d, uint64_t step, float x, uint64_t i) {
  return sgrl_dropout::apply(x, sgrl_replay::replay_word(d.seed, step, d.stream, i), d.thr, d.scale);
}

struct NodeTab {
  const int32_t* node_env;    // [N]
  const int32_t* node_limb;   // [N]
  const int32_t* node_mnode;  // [N] column of the node in the traversal table
  const int32_t* trav;        // [3][TM]
  int TM;
};

// A limb's input row [x0 (F1 values) | x1 (F - F1 values)] read from two row-major buffers where they lie: the actor has F1 = F
// (observations only), a critic F1 = 41 observation features followed by the limb's 3 action slots
struct Src {
  const float* obs; int obs_ld;
  const float* act; int act_ld;
  int F1;
};
__device__ __forceinline__ float src_at(const Src& s, int F, int env, int limb, int k) {
  return k < s.F1 ? s.obs[(size_t)env * s.obs_ld + s.F1 * limb + k] : s.act[(size_t)env * s.act_ld + (F - s.F1) * limb + (k - s.F1)];
}

// what the tail does with the decoder output s of limb l, output j of environment e
enum { TAIL_ACTION = 0,    // max_action * tanh(s)                                                    (StructureActor.py:221-243)
       TAIL_TARGET_ACTION, // clamp(max_action * tanh(s) + clamp(noise[e, out l + j], +-noise_clip), +-max_action)   (agent.py:128-134)
       TAIL_Q,             // s                                                                        (StructureCritic.py:96-112)
       TAIL_TD_TARGET };   // reward[e] + (1 - done[e]) * discount * min(s, q_other[e, l])             (agent.py:136-148)
struct TailEpi {
  int mode;
  float max_action, noise_clip, discount;
  const float* noise; int noise_ld;
  const float* q_other; int q_other_ld;
  const float* reward; const float* done;
};

// input embedding + position embedding (StructureActor.py:159-164, 16-30): 8 nodes per 128-thread block, thread = channel; the
// block's input rows are staged in LDS and every weight is loaded once per block
constexpr int kEmbedNodes = 8;
template <class D>
__global__ __launch_bounds__(128) void k_swat_embed(Src src, int F, const float* __restrict__ Wenc,
                                                     const float* __restrict__ benc, const float* __restrict__ emb0,
                                                     const float* __restrict__ emb1, const float* __restrict__ emb2, NodeTab nt,
                                                     float* __restrict__ h, int N, float scale, D dr) {
  __shared__ float xs[kEmbedNodes][64];
  [[maybe_unused]] const uint64_t step = drop_step(dr);
  const int c = threadIdx.x, nb = blockIdx.x * kEmbedNodes;
  for (int i = c; i < kEmbedNodes * 64; i += 128) {
    const int r = i / 64, k = i % 64, n = nb + r;
    float v = 0.f;
    if (n < N && k < F) v = src_at(src, F, nt.node_env[n], nt.node_limb[n], k);
    xs[r][k] = v;
  }
  __syncthreads();
  float acc[kEmbedNodes];
#pragma unroll
  for (int r = 0; r < kEmbedNodes; r++) acc[r] = 0.f;
  for (int k = 0; k < F; k++) {
    const float w = Wenc[c * F + k];
#pragma unroll
    for (int r = 0; r < kEmbedNodes; r++) acc[r] = fmaf(xs[r][k], w, acc[r]);
  }
  const float b = benc[c];
#pragma unroll
  for (int r = 0; r < kEmbedNodes; r++) {
    const int n = nb + r;
    if (n >= N) break;
    const int mn = nt.node_mnode[n];
    float pos;
    if (c < 42) pos = emb0[nt.trav[mn] * 42 + c];
    else if (c < 84) pos = emb1[nt.trav[nt.TM + mn] * 42 + (c - 42)];
    else pos = emb2[nt.trav[2 * nt.TM + mn] * 44 + (c - 84)];
    if constexpr (D::on) pos = dropped(dr, step, pos, (uint64_t)nt.node_limb[n] * E + c);      // one morphology: [L, 128]
    h[(size_t)n * E + c] = (acc[r] + b) * scale + pos;
  }
}

struct EnvTab {
  const int32_t* env_off;   // [n_env] first node
  const int32_t* env_L;     // [n_env]
  const int32_t* env_rel;   // [n_env] first float of the morphology's relation tensor [L, L, 3]
};

// attention of one environment (MyMultiheadAttention, StructureActor.py:36-45 over torch's multi_head_attention_forward):
// w_h[i, j] = softmax_j(q_h[i] . k_h[j] / 8 + bias_h[i, j]),  o[i][64 h + d] = sum_j w_h[i, j] v[j][64 h + d].
// Layer 0 adds the relation bias (RepeatTransformerEncoder, StructureActor.py:84-100): bias_h[i, j] = rel[i, j, :] . Wrel[h, :]
// + brel[h], computed here from the live rel_encoder parameters.  One 128-thread workgroup per environment: an environment is
// never split, its q | k | v rows (at most 15 x 384 floats) are staged in LDS.
template <class D>
__global__ __launch_bounds__(128) void k_swat_attn(const float* __restrict__ qkv, float* __restrict__ o, EnvTab et,
                                                    const float* __restrict__ rel, const float* __restrict__ Wrel,
                                                    const float* __restrict__ brel, int use_bias, D dr) {
  __shared__ float s_qkv[LMAX][3 * E + 4];
  __shared__ float s_p[2][LMAX][LMAX + 1];
  const int e = blockIdx.x, t = threadIdx.x;
  const int n0 = et.env_off[e], L = et.env_L[e];
  for (int i = t; i < L * 3 * E; i += 128) s_qkv[i / (3 * E)][i % (3 * E)] = qkv[(size_t)(n0 + i / (3 * E)) * 3 * E + i % (3 * E)];
  __syncthreads();
  const float* r = rel + et.env_rel[e];
  for (int idx = t; idx < 2 * L * L; idx += 128) {
    const int hh = idx / (L * L), ij = idx % (L * L), i = ij / L, j = ij % L;
    float dot = 0.f;
#pragma unroll 8
    for (int d = 0; d < HD; d++) dot = fmaf(s_qkv[i][HD * hh + d] * 0.125f, s_qkv[j][E + HD * hh + d], dot);
    if (use_bias) dot += Wrel[3 * hh] * r[3 * ij] + Wrel[3 * hh + 1] * r[3 * ij + 1] + Wrel[3 * hh + 2] * r[3 * ij + 2] + brel[hh];
    s_p[hh][i][j] = dot;
  }
  __syncthreads();
  if (t < 2 * L) {
    const int hh = t / L, i = t % L;
    float m = -INFINITY;
    for (int j = 0; j < L; j++) m = fmaxf(m, s_p[hh][i][j]);
    float sum = 0.f;
    for (int j = 0; j < L; j++) {
      const float x = expf(s_p[hh][i][j] - m);
      s_p[hh][i][j] = x;
      sum += x;
    }
    const float inv = 1.0f / sum;
    if constexpr (D::on) {
      // the weights of row (e, hh, i) are L consecutive elements of [B, 2, L, L]: one Philox block serves up to four of them
      const uint64_t step = drop_step(dr), base = ((uint64_t)(e * 2 + hh) * L + i) * L;
      sgrl_replay::Words4 blk{};
      uint64_t have = ~uint64_t(0);
      for (int j = 0; j < L; j++) {
        const uint64_t idx = base + j;
        if ((idx >> 2) != have) {
          have = idx >> 2;
          blk = sgrl_replay::replay_block(dr.seed, step, dr.stream, (uint32_t)have);
        }
        const uint32_t u = (uint32_t)idx & 3u;
        const uint32_t word = u == 0 ? blk.w[0] : (u == 1 ? blk.w[1] : (u == 2 ? blk.w[2] : blk.w[3]));
        s_p[hh][i][j] = sgrl_dropout::apply(s_p[hh][i][j] * inv, word, dr.thr, dr.scale);
      }
    } else {
      for (int j = 0; j < L; j++) s_p[hh][i][j] *= inv;
    }
  }
  __syncthreads();
  const int c = t, hh = c / HD;
  for (int i = 0; i < L; i++) {
    float acc = 0.f;
    for (int j = 0; j < L; j++) acc = fmaf(s_p[hh][i][j], s_qkv[j][2 * E + c], acc);
    o[(size_t)(n0 + i) * E + c] = acc;
  }
}

// y = LayerNorm(v) * w + b over the 128 channels of a row held by one wave (2 per lane), eps 1e-5 as nn.LayerNorm
__device__ __forceinline__ void row_ln(float& v0, float& v1, const float* __restrict__ w, const float* __restrict__ b, int lane) {
  const float mu = wave_sum(v0 + v1) * (1.f / 128.f);
  const float d0 = v0 - mu, d1 = v1 - mu;
  const float var = wave_sum(d0 * d0 + d1 * d1) * (1.f / 128.f);
  const float inv = 1.0f / sqrtf(var + 1e-5f);
  v0 = d0 * inv * w[lane] + b[lane];
  v1 = d1 * inv * w[64 + lane] + b[64 + lane];
}

// the row's two values of d, dropped over d's row-major index [N, 128] (the lane holds channels lane and 64 + lane: a Philox block
// per element, which these latency-bound kernels can afford)
__device__ __forceinline__ void row_d(const float* __restrict__ d, int row, int lane, const Drop& dr, float& d0, float& d1) {
  const uint64_t step = dr.step[0];
  d0 = dropped(dr, step, d[(size_t)row * E + lane], (uint64_t)row * E + lane);
  d1 = dropped(dr, step, d[(size_t)row * E + 64 + lane], (uint64_t)row * E + 64 + lane);
}

// h = LayerNorm(h + d), in place; one wave per row
template <class D>
__global__ __launch_bounds__(256) void k_swat_add_ln(float* __restrict__ h, const float* __restrict__ d, const float* __restrict__ w,
                                                      const float* __restrict__ b, int N, D dr) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  float v0, v1;
  if constexpr (D::on) {
    float d0, d1;
    row_d(d, row, lane, dr, d0, d1);
    v0 = h[(size_t)row * E + lane] + d0;
    v1 = h[(size_t)row * E + 64 + lane] + d1;
  } else {
    v0 = h[(size_t)row * E + lane] + d[(size_t)row * E + lane];
    v1 = h[(size_t)row * E + 64 + lane] + d[(size_t)row * E + 64 + lane];
  }
  row_ln(v0, v1, w, b, lane);
  h[(size_t)row * E + lane] = v0;
  h[(size_t)row * E + 64 + lane] = v1;
}

// last layer's norm2, the final LayerNorm (fw != null), the decoder (StructureActor.py:164-170: over h, or [h | x] with
// cond_decoder) and the epilogue of TailEpi (the actor's max_action * tanh, StructureActor.py:221-243, or one of the critic /
// target forms); one wave per node.  The node of limb 0 of every environment also writes the zero padding
// act[e, out * L_e : act_ld].
template <class D>
__global__ __launch_bounds__(256) void k_swat_tail(const float* __restrict__ h, const float* __restrict__ d, const float* __restrict__ n2w,
                                                    const float* __restrict__ n2b, const float* __restrict__ fw, const float* __restrict__ fb,
                                                    const float* __restrict__ Wd, const float* __restrict__ bd, int cond, int F, int O,
                                                    Src src, NodeTab nt, const int32_t* __restrict__ env_L,
                                                    float* __restrict__ act, int act_ld, TailEpi ep, int N, D dr) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  float v0, v1;
  if constexpr (D::on) {
    float d0, d1;
    row_d(d, row, lane, dr, d0, d1);
    v0 = h[(size_t)row * E + lane] + d0;
    v1 = h[(size_t)row * E + 64 + lane] + d1;
  } else {
    v0 = h[(size_t)row * E + lane] + d[(size_t)row * E + lane];
    v1 = h[(size_t)row * E + 64 + lane] + d[(size_t)row * E + 64 + lane];
  }
  row_ln(v0, v1, n2w, n2b, lane);
  if (fw) row_ln(v0, v1, fw, fb, lane);
  const int env = nt.node_env[row], limb = nt.node_limb[row];
  const int ldd = cond ? E + F : E;
  const float x = (cond && lane < F) ? src_at(src, F, env, limb, lane) : 0.f;
  float* arow = act + (size_t)env * act_ld;
  for (int j = 0; j < O; j++) {
    const float* wr = Wd + (size_t)j * ldd;
    float s = fmaf(v0, wr[lane], v1 * wr[64 + lane]);
    if (cond && lane < F) s = fmaf(x, wr[E + lane], s);
    s = wave_sum(s) + bd[j];
    if (lane == 0) {
      float y = s;
      if (ep.mode <= TAIL_TARGET_ACTION) {
        y = ep.max_action * tanhf(s);
        if (ep.mode == TAIL_TARGET_ACTION) {
          const float nz = fminf(fmaxf(ep.noise[(size_t)env * ep.noise_ld + O * limb + j], -ep.noise_clip), ep.noise_clip);
          y = fminf(fmaxf(y + nz, -ep.max_action), ep.max_action);
        }
      } else if (ep.mode == TAIL_TD_TARGET) {
        y = fminf(s, ep.q_other[(size_t)env * ep.q_other_ld + O * limb + j]);
        y = ep.reward[env] + (1.0f - ep.done[env]) * ep.discount * y;
      }
      arow[O * limb + j] = y;
    }
  }
  if (limb == 0)
    for (int k = O * env_L[env] + lane; k < act_ld; k += 64) arow[k] = 0.f;
}

// x = dropout(x) in place over `quads` groups of four consecutive floats (the feed-forward hidden layer [N, 256], 16-byte aligned):
// one thread and ONE Philox block per quad, as k_dropout (dropout.hip)
__global__ __launch_bounds__(256) void k_swat_drop_quads(float* __restrict__ x, int64_t quads, Drop dr) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const uint64_t step = dr.step[0];
  float4 v = reinterpret_cast<const float4*>(x)[q];
  const sgrl_replay::Words4 o = sgrl_replay::replay_block(dr.seed, step, dr.stream, (uint32_t)q);
  v.x = sgrl_dropout::apply(v.x, o.w[0], dr.thr, dr.scale);
  v.y = sgrl_dropout::apply(v.y, o.w[1], dr.thr, dr.scale);
  v.z = sgrl_dropout::apply(v.z, o.w[2], dr.thr, dr.scale);
  v.w = sgrl_dropout::apply(v.w, o.w[3], dr.thr, dr.scale);
  reinterpret_cast<float4*>(x)[q] = v;
}

// C[M, N] = epi(A[M, K] . W[N, K]^T + b): 128 x 64 tiles, 4 waves, k-tiles of 16 (K = 128 | 256, N = 128 | 256 | 384)
constexpr auto kGemm = k_gemm2<0, 4, 1, 1, 2, 16, 1>;
constexpr auto kGemmRelu = k_gemm2<EPI_RELU, 4, 1, 1, 2, 16, 1>;
constexpr int kGemmLds = sgrl_gemm::TileCfg<4, 1, 1, 2, 16>::kLdsBytes;

void launch_gemm(hipStream_t st, bool relu, const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M,
                 int N, int K) {
  GemmArgs a{};
  a.A = A; a.lda = lda; a.W = W; a.ldw = K; a.bias = bias; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
  const dim3 grid(((M + 127) / 128) * ((N + 63) / 64));
  if (relu) hipLaunchKernelGGL(kGemmRelu, grid, dim3(256), kGemmLds, st, a);
  else hipLaunchKernelGGL(kGemm, grid, dim3(256), kGemmLds, st, a);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
struct SwatGraphCfg {
  std::vector<int32_t> key_i;   // n_morph | L[] | count[] | trav[]
  std::vector<float> key_f;     // rel[]
  int n_env = 0, N = 0, TM = 0, Lmax = 0;
  int32_t *d_node_env = nullptr, *d_node_limb = nullptr, *d_node_mnode = nullptr, *d_trav = nullptr;
  int32_t *d_env_off = nullptr, *d_env_L = nullptr, *d_env_rel = nullptr;
  float* d_rel = nullptr;
  uint64_t last_use = 0;
  void release() {
    void* ptrs[] = {d_node_env, d_node_limb, d_node_mnode, d_trav, d_env_off, d_env_L, d_env_rel, d_rel};
    for (void* q : ptrs) if (q) (void)hipFree(q);
  }
};

struct sgrl_swat {
  const float* p[SGRL_SWAT_NW(1)] = {};
  bool have_w = false, cond = false, tnorm = false;
  int F = 41, O = 3;
  SwatGraphCfg* cur = nullptr;
  std::vector<SwatGraphCfg*> cfgs;
  uint64_t use_clock = 0;
  int64_t generation = 0;
  float* ws = nullptr;          // workspace: h [N, 128] | qkv [N, 384] | o [N, 128] | out [n_env, out * Lmax]; grows only
  int64_t ws_floats = 0;
  // twin critic / target chain: the second network's chain runs on `side` of the FIRST handle between ev_fork and ev_join
  // (created by the first twin call, never under a capture)
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  const float* W(int slot) const { return p[slot]; }
  const float* WL(int layer, int k) const { return p[SGRL_SWAT_NGLOBAL + layer * SGRL_SWAT_NLAYER + k]; }
};

namespace {

template <class T>
int upload(T** dst, const std::vector<T>& v) {
  if (hipMalloc(dst, sizeof(T) * (v.size() ? v.size() : 1)) != hipSuccess) return -1;
  if (!v.empty() && hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
  return 0;
}

constexpr int kOutMax = 8 * LMAX;     // bind_params: out <= 8
int64_t ws_floats_for(int64_t N, int64_t n_env) { return (E + 3 * E + E) * N + 3 * 64 + kOutMax * n_env; }

int use_cfg(sgrl_swat* s, SwatGraphCfg* c) {
  const int64_t need = ws_floats_for(c->N, c->n_env);
  if (need > s->ws_floats) {
    if (s->ws) { (void)hipFree(s->ws); s->generation++; }      // hipFree waits for the device: no kernel still reads the old block
    s->ws = nullptr; s->ws_floats = 0;
    if (hipMalloc(&s->ws, sizeof(float) * need) != hipSuccess) { s->cur = nullptr; return wfail(SGRL_ERR_HIP, "device allocation failed (SWAT workspace)"); }
    s->ws_floats = need;
  }
  c->last_use = ++s->use_clock;
  s->cur = c;
  return SGRL_OK;
}

// workspace carve-up (16-byte aligned rows for the GEMM's float4 loads): h [N, 128] | qkv [N, 384] | o [N, 128] | out; the
// out_proj result and the feed-forward hidden layer reuse qkv, linear2's result reuses o; `out` [n_env, out * Lmax] holds what
// the target chain keeps to itself (the target actor's noisy action, the second critic's values)
struct Ws { float *h, *qkv, *o, *out; };
Ws carve(const sgrl_swat* s) {
  auto al = [](int64_t n) { return (n + 63) & ~int64_t(63); };
  const int64_t N = s->cur->N;
  Ws w;
  w.h = s->ws;
  w.qkv = w.h + al((int64_t)E * N);
  w.o = w.qkv + al((int64_t)3 * E * N);
  w.out = w.o + al((int64_t)E * N);
  return w;
}
NodeTab node_tab(const SwatGraphCfg* c) { return NodeTab{c->d_node_env, c->d_node_limb, c->d_node_mnode, c->d_trav, c->TM}; }

// One network's dropout: (thr, scale, seed, step) of the call and the site numbers of its 13 sites in program order.  Every run_*
// below takes one by pointer; null = the plain entry's launches, argument for argument what they were.
struct DropCfg {
  uint64_t thr, seed;
  const uint64_t* step;
  float scale;
  int site[kDropSites];
  Drop at(int k) const { return Drop{thr, seed, step, scale, sgrl_dropout::stream_of(site[k])}; }
};

void run_embed(sgrl_swat* s, const Src& src, hipStream_t st, const DropCfg* dc = nullptr) {
  const SwatGraphCfg* c = s->cur;
  const int N = c->N;
  const dim3 grid((N + kEmbedNodes - 1) / kEmbedNodes);
  if (dc)
    hipLaunchKernelGGL(k_swat_embed<Drop>, grid, dim3(128), 0, st, src, s->F, s->W(SGRL_SWAT_ENC_W), s->W(SGRL_SWAT_ENC_B),
                       s->W(SGRL_SWAT_EMB0), s->W(SGRL_SWAT_EMB1), s->W(SGRL_SWAT_EMB2), node_tab(c), carve(s).h, N, sqrtf((float)E),
                       dc->at(0));
  else
    hipLaunchKernelGGL(k_swat_embed<NoDrop>, grid, dim3(128), 0, st, src, s->F, s->W(SGRL_SWAT_ENC_W), s->W(SGRL_SWAT_ENC_B),
                       s->W(SGRL_SWAT_EMB0), s->W(SGRL_SWAT_EMB1), s->W(SGRL_SWAT_EMB2), node_tab(c), carve(s).h, N, sqrtf((float)E),
                       NoDrop{});
}

void launch_add_ln(hipStream_t st, float* h, const float* d, const float* w, const float* b, int N, const DropCfg* dc, int site) {
  const dim3 grid((N + 3) / 4);
  if (dc) hipLaunchKernelGGL(k_swat_add_ln<Drop>, grid, dim3(256), 0, st, h, d, w, b, N, dc->at(site));
  else hipLaunchKernelGGL(k_swat_add_ln<NoDrop>, grid, dim3(256), 0, st, h, d, w, b, N, NoDrop{});
}

// layer l up to linear2 (6 launches, 7 with dropout); its norm2 follows (run_norm2) or is part of the tail (run_tail, last layer)
void run_layer(sgrl_swat* s, int l, hipStream_t st, const DropCfg* dc = nullptr) {
  const SwatGraphCfg* c = s->cur;
  const int N = c->N;
  const Ws w = carve(s);
  EnvTab et{c->d_env_off, c->d_env_L, c->d_env_rel};
  launch_gemm(st, false, w.h, E, s->WL(l, SGRL_SWAT_IN_W), s->WL(l, SGRL_SWAT_IN_B), w.qkv, 3 * E, N, 3 * E, E);
  if (dc)
    hipLaunchKernelGGL(k_swat_attn<Drop>, dim3(c->n_env), dim3(128), 0, st, w.qkv, w.o, et, c->d_rel, s->W(SGRL_SWAT_REL_W),
                       s->W(SGRL_SWAT_REL_B), l == 0 ? 1 : 0, dc->at(1 + 4 * l));
  else
    hipLaunchKernelGGL(k_swat_attn<NoDrop>, dim3(c->n_env), dim3(128), 0, st, w.qkv, w.o, et, c->d_rel, s->W(SGRL_SWAT_REL_W),
                       s->W(SGRL_SWAT_REL_B), l == 0 ? 1 : 0, NoDrop{});
  float* d1 = w.qkv;
  launch_gemm(st, false, w.o, E, s->WL(l, SGRL_SWAT_OUT_W), s->WL(l, SGRL_SWAT_OUT_B), d1, E, N, E, E);
  launch_add_ln(st, w.h, d1, s->WL(l, SGRL_SWAT_N1_W), s->WL(l, SGRL_SWAT_N1_B), N, dc, 2 + 4 * l);
  float* f = w.qkv;
  launch_gemm(st, true, w.h, E, s->WL(l, SGRL_SWAT_L1_W), s->WL(l, SGRL_SWAT_L1_B), f, FF, N, FF, E);
  if (dc) {
    const int64_t quads = (int64_t)N * (FF / 4);      // f is [N, 256] with ldc = 256: contiguous, and 16-byte aligned by carve()
    hipLaunchKernelGGL(k_swat_drop_quads, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, f, quads, dc->at(3 + 4 * l));
  }
  launch_gemm(st, false, f, FF, s->WL(l, SGRL_SWAT_L2_W), s->WL(l, SGRL_SWAT_L2_B), w.o, E, N, E, FF);
}

void run_norm2(sgrl_swat* s, int l, hipStream_t st, const DropCfg* dc = nullptr) {
  const Ws w = carve(s);
  launch_add_ln(st, w.h, w.o, s->WL(l, SGRL_SWAT_N2_W), s->WL(l, SGRL_SWAT_N2_B), s->cur->N, dc, 4 + 4 * l);
}

void run_tail(sgrl_swat* s, const Src& src, float* out, int out_ld, const TailEpi& ep, hipStream_t st, const DropCfg* dc = nullptr) {
  const SwatGraphCfg* c = s->cur;
  const int N = c->N, l = SGRL_SWAT_LAYERS - 1;
  const Ws w = carve(s);
  const int fn = SGRL_SWAT_NGLOBAL + SGRL_SWAT_LAYERS * SGRL_SWAT_NLAYER;
  const float *fw = s->tnorm ? s->p[fn] : (const float*)nullptr, *fb = s->tnorm ? s->p[fn + 1] : (const float*)nullptr;
  if (dc)
    hipLaunchKernelGGL(k_swat_tail<Drop>, dim3((N + 3) / 4), dim3(256), 0, st, w.h, w.o, s->WL(l, SGRL_SWAT_N2_W),
                       s->WL(l, SGRL_SWAT_N2_B), fw, fb, s->W(SGRL_SWAT_DEC_W), s->W(SGRL_SWAT_DEC_B), s->cond ? 1 : 0, s->F, s->O, src,
                       node_tab(c), c->d_env_L, out, out_ld, ep, N, dc->at(4 + 4 * l));
  else
    hipLaunchKernelGGL(k_swat_tail<NoDrop>, dim3((N + 3) / 4), dim3(256), 0, st, w.h, w.o, s->WL(l, SGRL_SWAT_N2_W),
                       s->WL(l, SGRL_SWAT_N2_B), fw, fb, s->W(SGRL_SWAT_DEC_W), s->W(SGRL_SWAT_DEC_B), s->cond ? 1 : 0, s->F, s->O, src,
                       node_tab(c), c->d_env_L, out, out_ld, ep, N, NoDrop{});
}

int launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return wfail(SGRL_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
  return SGRL_OK;
}

// one network, one stream: 1 + 3 x 7 launches (1 + 3 x 8 with dropout)
void run_chain(sgrl_swat* s, const Src& src, float* out, int out_ld, const TailEpi& ep, hipStream_t st, const DropCfg* dc = nullptr) {
  run_embed(s, src, st, dc);
  for (int l = 0; l < SGRL_SWAT_LAYERS; l++) {
    run_layer(s, l, st, dc);
    if (l + 1 < SGRL_SWAT_LAYERS) run_norm2(s, l, st, dc);
  }
  run_tail(s, src, out, out_ld, ep, st, dc);
}

TailEpi epi(int mode) { TailEpi e{}; e.mode = mode; return e; }

bool g_twin_streams = true;     // sgrl_swat_debug_twin_streams

int ensure_side(sgrl_swat* s) {
  if (s->side) return SGRL_OK;
  if (hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess) {
    if (s->side) (void)hipStreamDestroy(s->side);
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    s->side = nullptr; s->ev_fork = s->ev_join = nullptr;
    (void)hipGetLastError();
    return wfail(SGRL_ERR_HIP, "cannot create the twin critic's side stream (run one twin forward eagerly before capturing one)");
  }
  return SGRL_OK;
}

// Two critics over one pair of input buffers: network 1 on `st`, network 2 on the side stream of handle 1, launches issued layer
// by layer in turn so that both queues fill together.  The second network's tail always runs on its own stream; the first
// network's tail runs before the join (plain twin: nothing to wait for) or after it (wait_q2: its epilogue reads network 2's
// values).  Every kernel of a network gets the arguments of that network's own single forward, so its rows are the same bits.
int run_twin(sgrl_swat* a, sgrl_swat* b, const Src& src, float* out1, int ld1, const TailEpi& ep1, float* out2, int ld2,
             const TailEpi& ep2, bool wait_q2, hipStream_t st, const DropCfg* da = nullptr, const DropCfg* db = nullptr) {
  hipStream_t sd = st;
  if (g_twin_streams) {
    if (const int rc = ensure_side(a)) return rc;
    sd = a->side;
    (void)hipEventRecord(a->ev_fork, st);
    (void)hipStreamWaitEvent(sd, a->ev_fork, 0);
  }
  run_embed(a, src, st, da);
  run_embed(b, src, sd, db);
  for (int l = 0; l < SGRL_SWAT_LAYERS; l++) {
    run_layer(a, l, st, da);
    run_layer(b, l, sd, db);
    if (l + 1 < SGRL_SWAT_LAYERS) { run_norm2(a, l, st, da); run_norm2(b, l, sd, db); }
  }
  run_tail(b, src, out2, ld2, ep2, sd, db);
  if (sd != st) (void)hipEventRecord(a->ev_join, sd);
  if (!wait_q2) run_tail(a, src, out1, ld1, ep1, st, da);
  if (sd != st) (void)hipStreamWaitEvent(st, a->ev_join, 0);
  if (wait_q2) run_tail(a, src, out1, ld1, ep1, st, da);
  return launch_status("SWAT twin critic");
}

bool same_structure(const sgrl_swat* a, const sgrl_swat* b) {
  const SwatGraphCfg *x = a->cur, *y = b->cur;
  return x->key_i == y->key_i && x->key_f.size() == y->key_f.size() &&
         std::memcmp(x->key_f.data(), y->key_f.data(), sizeof(float) * x->key_f.size()) == 0;
}

// argument checks of a critic forward: handle `s` bound with out = 1, the limb row = [obs (feature - act_feature) | action]
int check_critic(const char* fn, const sgrl_swat* s, int obs_ld, int act_ld, int act_feature, int q_ld) {
  const std::string f(fn);
  if (!s->have_w || !s->cur) return wfail(SGRL_ERR_ARG, f + ": parameters or batch structure not set");
  if (s->O != 1) return wfail(SGRL_ERR_ARG, f + ": the handle is not bound as a critic (out = " + std::to_string(s->O) + ", need 1)");
  if (act_feature < 1 || act_feature > s->F - 1)
    return wfail(SGRL_ERR_ARG, f + ": act_feature " + std::to_string(act_feature) + " outside [1, feature - 1]");
  const int Lmax = s->cur->Lmax;
  if (obs_ld < (s->F - act_feature) * Lmax || act_ld < act_feature * Lmax || q_ld < Lmax)
    return wfail(SGRL_ERR_ARG, f + ": obs_ld < (feature - act_feature) * Lmax, act_ld < act_feature * Lmax or q_ld < Lmax "
                                   "(rows too narrow for the largest morphology)");
  return SGRL_OK;
}

// The dropout arguments of an entry whose networks take `nsites` consecutive sites from site0 (13 per network), checked after the
// plain entry's own checks (s->cur is set).  site_map (single-network entries; null = identity): site k of the network is
// site0 + site_map[k].  Fills one DropCfg per network.
int make_drop(const char* fn, const sgrl_swat* s, float p, uint64_t seed, const uint64_t* step_dev, int site0, const int32_t* site_map,
              int nets, DropCfg* out) {
  const std::string f(fn);
  if (!(p >= 0.f && p <= 1.f)) return wfail(SGRL_ERR_ARG, f + ": p outside [0, 1]");                      // refuses a NaN as well
  if (!step_dev) return wfail(SGRL_ERR_ARG, f + ": step_dev is null");
  if (site0 < 0 || site0 > sgrl_dropout::kMaxSite - (nets * kDropSites - 1))
    return wfail(SGRL_ERR_ARG, f + ": sites " + std::to_string(site0) + " .. " + std::to_string((int64_t)site0 + nets * kDropSites - 1) +
                                   " outside 0 .. 2^24 - 1");
  if (s->cur->key_i[0] != 1)
    return wfail(SGRL_ERR_ARG, f + ": the dropout entries serve a batch structure of one morphology (this one has " +
                                   std::to_string(s->cur->key_i[0]) + "): the masks are indexed as the module's tensors [B, L, ...]");
  if ((int64_t)s->cur->N * FF > (int64_t)1 << 32) return wfail(SGRL_ERR_ARG, f + ": more than 2^32 elements at a dropout site");
  for (int n = 0; n < nets; n++) {
    DropCfg& d = out[n];
    d.thr = sgrl_dropout::threshold(p);
    d.scale = sgrl_dropout::scale(p);
    d.seed = seed;
    d.step = step_dev;
    for (int k = 0; k < kDropSites; k++) {
      const int64_t site = (int64_t)site0 + n * kDropSites + (site_map ? site_map[k] : k);
      if (site < 0 || site > sgrl_dropout::kMaxSite)
        return wfail(SGRL_ERR_ARG, f + ": site_map[" + std::to_string(k) + "] leads outside 0 .. 2^24 - 1");
      d.site[k] = (int)site;
    }
  }
  return SGRL_OK;
}

struct DropArgs {      // the trailing arguments of a dropout entry
  float p;
  uint64_t seed;
  const uint64_t* step_dev;
  int site0;
  const int32_t* site_map;
};

// sgrl_swat_forward and its dropout form (da != null)
int actor_forward(const char* fn, sgrl_swat* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, const DropArgs* da,
                  void* stream) {
  const std::string f(fn);
  if (!s || !obs || !act) return wfail(SGRL_ERR_ARG, f + ": null argument");
  if (!s->have_w || !s->cur) return wfail(SGRL_ERR_ARG, f + ": parameters or batch structure not set");
  if (obs_ld < s->F * s->cur->Lmax || act_ld < s->O * s->cur->Lmax)
    return wfail(SGRL_ERR_ARG, f + ": obs_ld < feature * Lmax or act_ld < out * Lmax (rows too narrow for the largest morphology)");
  DropCfg dc;
  if (da)
    if (const int rc = make_drop(fn, s, da->p, da->seed, da->step_dev, da->site0, da->site_map, 1, &dc)) return rc;
  TailEpi ep = epi(TAIL_ACTION);
  ep.max_action = max_action;
  run_chain(s, Src{obs, obs_ld, nullptr, 0, s->F}, act, act_ld, ep, (hipStream_t)stream, da ? &dc : nullptr);
  return launch_status("SWAT forward");
}

int critic_forward(const char* fn, sgrl_swat* s, const float* obs, int obs_ld, const float* action, int act_ld, int act_feature, float* q,
                   int q_ld, const DropArgs* da, void* stream) {
  if (!s || !obs || !action || !q) return wfail(SGRL_ERR_ARG, std::string(fn) + ": null argument");
  if (const int rc = check_critic(fn, s, obs_ld, act_ld, act_feature, q_ld)) return rc;
  DropCfg dc;
  if (da)
    if (const int rc = make_drop(fn, s, da->p, da->seed, da->step_dev, da->site0, da->site_map, 1, &dc)) return rc;
  run_chain(s, Src{obs, obs_ld, action, act_ld, s->F - act_feature}, q, q_ld, epi(TAIL_Q), (hipStream_t)stream, da ? &dc : nullptr);
  return launch_status("SWAT critic forward");
}

// sgrl_swat_td_target and its dropout form: the target actor takes sites site0 .. + 12, the first critic + 13 .. + 25, the second
// + 26 .. + 38 (the order Agent.update_targets runs the modules in)
int td_target(const char* fn, sgrl_swat* actor_t, sgrl_swat* q1_t, sgrl_swat* q2_t, const float* next_obs, int obs_ld, const float* noise,
              int noise_ld, const float* reward, const float* done, float max_action, float noise_clip, float discount, float* target_q,
              int q_ld, const DropArgs* da, void* stream) {
  const std::string f(fn);
  if (!actor_t || !q1_t || !q2_t || !next_obs || !noise || !reward || !done || !target_q) return wfail(SGRL_ERR_ARG, f + ": null argument");
  if (actor_t == q1_t || actor_t == q2_t || q1_t == q2_t) return wfail(SGRL_ERR_ARG, f + ": three networks need three handles");
  if (!actor_t->have_w || !actor_t->cur) return wfail(SGRL_ERR_ARG, f + ": actor parameters or batch structure not set");
  const int aF = actor_t->F, aO = actor_t->O, Lmax = actor_t->cur->Lmax;
  const int a_ld = aO * Lmax;                         // the noisy target action stays in the actor handle's workspace
  if (const int rc = check_critic(fn, q1_t, obs_ld, a_ld, aO, q_ld)) return rc;
  if (const int rc = check_critic(fn, q2_t, obs_ld, a_ld, aO, q_ld)) return rc;
  if (q1_t->F != aF + aO || q2_t->F != aF + aO)
    return wfail(SGRL_ERR_ARG, f + ": the critics must take the actor's feature + out inputs per limb");
  if (!same_structure(actor_t, q1_t) || !same_structure(actor_t, q2_t))
    return wfail(SGRL_ERR_ARG, f + ": the handles hold different batch structures");
  if (obs_ld < aF * Lmax || noise_ld < a_ld)
    return wfail(SGRL_ERR_ARG, f + ": obs_ld < feature * Lmax or noise_ld < out * Lmax (rows too narrow for the largest morphology)");
  DropCfg dc[3];
  if (da)
    if (const int rc = make_drop(fn, actor_t, da->p, da->seed, da->step_dev, da->site0, nullptr, 3, dc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  float* a_next = carve(actor_t).out;
  float* q2 = carve(q2_t).out;
  TailEpi ea = epi(TAIL_TARGET_ACTION);
  ea.max_action = max_action; ea.noise_clip = noise_clip; ea.noise = noise; ea.noise_ld = noise_ld;
  run_chain(actor_t, Src{next_obs, obs_ld, nullptr, 0, aF}, a_next, a_ld, ea, st, da ? &dc[0] : nullptr);
  TailEpi e1 = epi(TAIL_TD_TARGET);
  e1.discount = discount; e1.q_other = q2; e1.q_other_ld = Lmax; e1.reward = reward; e1.done = done;
  return run_twin(q1_t, q2_t, Src{next_obs, obs_ld, a_next, a_ld, aF}, target_q, q_ld, e1, q2, Lmax, epi(TAIL_Q), true, st,
                  da ? &dc[1] : nullptr, da ? &dc[2] : nullptr);
}

}  // namespace

extern "C" {

int sgrl_swat_create(sgrl_swat** out) {
  if (!out) return wfail(SGRL_ERR_ARG, "out is null");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return wfail(SGRL_ERR_HIP, "no HIP device visible: the SWAT actor forward needs an MI355X (there is no CPU fallback)");
  *out = new sgrl_swat();
  return SGRL_OK;
}

void sgrl_swat_destroy(sgrl_swat* s) {
  if (!s) return;
  for (SwatGraphCfg* c : s->cfgs) { c->release(); delete c; }
  if (s->ws) (void)hipFree(s->ws);
  if (s->side) (void)hipStreamDestroy(s->side);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  delete s;
}

int sgrl_swat_bind_params(sgrl_swat* s, const void* const* ptrs, int n, int cond_decoder, int transformer_norm, int feature,
                          int out) {
  if (!s || !ptrs) return wfail(SGRL_ERR_ARG, "sgrl_swat_bind_params: null argument");
  if (n != SGRL_SWAT_NW(transformer_norm ? 1 : 0))
    return wfail(SGRL_ERR_ARG, "sgrl_swat_bind_params: expected " + std::to_string(SGRL_SWAT_NW(transformer_norm ? 1 : 0)) +
                                   " parameter addresses, got " + std::to_string(n));
  if (feature < 1 || feature > 64 || out < 1 || out > 8) return wfail(SGRL_ERR_ARG, "sgrl_swat_bind_params: need 1 <= feature <= 64, 1 <= out <= 8");
  for (int i = 0; i < n; i++)
    if (!ptrs[i] || (reinterpret_cast<uintptr_t>(ptrs[i]) & 15))
      return wfail(SGRL_ERR_ARG, "sgrl_swat_bind_params: parameter " + std::to_string(i) + " is null or not 16-byte aligned");
  for (int i = 0; i < n; i++) s->p[i] = static_cast<const float*>(ptrs[i]);
  s->cond = cond_decoder != 0;
  s->tnorm = transformer_norm != 0;
  s->F = feature;
  s->O = out;
  s->have_w = true;
  return SGRL_OK;
}

int sgrl_swat_graph(sgrl_swat* s, int n_morph, const int32_t* morph_L, const int32_t* morph_count, const int32_t* trav,
                    const float* rel) {
  if (!s || n_morph <= 0 || !morph_L || !morph_count || !trav || !rel) return wfail(SGRL_ERR_ARG, "sgrl_swat_graph: bad argument");
  size_t ntrav = 0, nrel = 0;
  for (int k = 0; k < n_morph; k++) {
    if (morph_L[k] < 1 || morph_L[k] > LMAX)
      return wfail(SGRL_ERR_ARG, "sgrl_swat_graph: limb count " + std::to_string(morph_L[k]) + " outside [1, 15] (position tables have 15 rows)");
    if (morph_count[k] < 0) return wfail(SGRL_ERR_ARG, "sgrl_swat_graph: negative morph_count");
    ntrav += 3 * (size_t)morph_L[k];
    nrel += 3 * (size_t)morph_L[k] * morph_L[k];
  }
  std::vector<int32_t> key_i;
  key_i.push_back(n_morph);
  key_i.insert(key_i.end(), morph_L, morph_L + n_morph);
  key_i.insert(key_i.end(), morph_count, morph_count + n_morph);
  key_i.insert(key_i.end(), trav, trav + ntrav);
  for (SwatGraphCfg* c : s->cfgs)
    if (c->key_i == key_i && c->key_f.size() == nrel && std::memcmp(c->key_f.data(), rel, sizeof(float) * nrel) == 0)
      return use_cfg(s, c);        // seen before: no allocation, upload or synchronisation
  std::vector<int32_t> node_env, node_limb, node_mnode, env_off, env_L, env_rel, travT;
  std::vector<int> m_node0, m_rel0;
  int TM = 0, Lmax = 0, env = 0, node = 0;
  size_t roff = 0;
  for (int k = 0; k < n_morph; k++) {
    m_node0.push_back(TM);
    m_rel0.push_back((int)roff);
    TM += morph_L[k];
    roff += 3 * (size_t)morph_L[k] * morph_L[k];
    if (morph_L[k] > Lmax) Lmax = morph_L[k];
  }
  travT.assign(3 * (size_t)TM, 0);
  for (int k = 0, tp = 0; k < n_morph; k++) {
    const int L = morph_L[k];
    for (int q = 0; q < 3; q++)
      for (int i = 0; i < L; i++) {
        const int v = trav[tp + q * L + i];
        if (v < 0 || v >= LMAX) return wfail(SGRL_ERR_ARG, "sgrl_swat_graph: traversal index out of range [0, 15)");
        travT[(size_t)q * TM + m_node0[k] + i] = v;
      }
    tp += 3 * L;
  }
  for (int k = 0; k < n_morph; k++)
    for (int c = 0; c < morph_count[k]; c++, env++) {
      env_off.push_back(node);
      env_L.push_back(morph_L[k]);
      env_rel.push_back(m_rel0[k]);
      for (int i = 0; i < morph_L[k]; i++, node++) {
        node_env.push_back(env);
        node_limb.push_back(i);
        node_mnode.push_back(m_node0[k] + i);
      }
    }
  if (node == 0) return wfail(SGRL_ERR_ARG, "sgrl_swat_graph: no environments");
  if ((int)s->cfgs.size() >= SGRL_SWAT_GRAPH_CACHE) {      // evict the least recently used structure
    size_t lru = 0;
    for (size_t i = 1; i < s->cfgs.size(); i++) if (s->cfgs[i]->last_use < s->cfgs[lru]->last_use) lru = i;
    if (s->cfgs[lru] == s->cur) s->cur = nullptr;
    s->cfgs[lru]->release();                               // hipFree waits for the device
    s->generation++;
    delete s->cfgs[lru];
    s->cfgs.erase(s->cfgs.begin() + lru);
  }
  SwatGraphCfg* c = new SwatGraphCfg();
  c->key_i = std::move(key_i);
  c->key_f.assign(rel, rel + nrel);
  c->n_env = env; c->N = node; c->TM = TM; c->Lmax = Lmax;
  const bool ok = upload(&c->d_node_env, node_env) == 0 && upload(&c->d_node_limb, node_limb) == 0 &&
                  upload(&c->d_node_mnode, node_mnode) == 0 && upload(&c->d_trav, travT) == 0 && upload(&c->d_env_off, env_off) == 0 &&
                  upload(&c->d_env_L, env_L) == 0 && upload(&c->d_env_rel, env_rel) == 0 && upload(&c->d_rel, c->key_f) == 0;
  if (!ok) { c->release(); delete c; return wfail(SGRL_ERR_HIP, "device allocation failed in sgrl_swat_graph"); }
  s->cfgs.push_back(c);
  return use_cfg(s, c);
}

int sgrl_swat_forward(sgrl_swat* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, void* stream) {
  return actor_forward("sgrl_swat_forward", s, obs, obs_ld, act, act_ld, max_action, nullptr, stream);
}

int sgrl_swat_forward_dropout(sgrl_swat* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, float p,
                              uint64_t seed, const uint64_t* step_dev, int site0, const int32_t* site_map, void* stream) {
  const DropArgs da{p, seed, step_dev, site0, site_map};
  return actor_forward("sgrl_swat_forward_dropout", s, obs, obs_ld, act, act_ld, max_action, &da, stream);
}

int sgrl_swat_forward_q(sgrl_swat* s, const float* obs, int obs_ld, const float* action, int act_ld, int act_feature, float* q,
                        int q_ld, void* stream) {
  return critic_forward("sgrl_swat_forward_q", s, obs, obs_ld, action, act_ld, act_feature, q, q_ld, nullptr, stream);
}

int sgrl_swat_forward_q_dropout(sgrl_swat* s, const float* obs, int obs_ld, const float* action, int act_ld, int act_feature, float* q,
                                int q_ld, float p, uint64_t seed, const uint64_t* step_dev, int site0, const int32_t* site_map,
                                void* stream) {
  const DropArgs da{p, seed, step_dev, site0, site_map};
  return critic_forward("sgrl_swat_forward_q_dropout", s, obs, obs_ld, action, act_ld, act_feature, q, q_ld, &da, stream);
}

int sgrl_swat_forward_twin(sgrl_swat* s1, sgrl_swat* s2, const float* obs, int obs_ld, const float* action, int act_ld,
                           int act_feature, float* q1, float* q2, int q_ld, void* stream) {
  if (!s1 || !s2 || !obs || !action || !q1 || !q2) return wfail(SGRL_ERR_ARG, "sgrl_swat_forward_twin: null argument");
  if (s1 == s2 || q1 == q2) return wfail(SGRL_ERR_ARG, "sgrl_swat_forward_twin: the two networks need two handles and two outputs");
  if (const int rc = check_critic("sgrl_swat_forward_twin", s1, obs_ld, act_ld, act_feature, q_ld)) return rc;
  if (const int rc = check_critic("sgrl_swat_forward_twin", s2, obs_ld, act_ld, act_feature, q_ld)) return rc;
  if (s1->F != s2->F) return wfail(SGRL_ERR_ARG, "sgrl_swat_forward_twin: the two critics take different feature counts");
  if (!same_structure(s1, s2)) return wfail(SGRL_ERR_ARG, "sgrl_swat_forward_twin: the handles hold different batch structures");
  const Src src{obs, obs_ld, action, act_ld, s1->F - act_feature};
  return run_twin(s1, s2, src, q1, q_ld, epi(TAIL_Q), q2, q_ld, epi(TAIL_Q), false, (hipStream_t)stream);
}

int sgrl_swat_td_target(sgrl_swat* actor_t, sgrl_swat* q1_t, sgrl_swat* q2_t, const float* next_obs, int obs_ld, const float* noise,
                        int noise_ld, const float* reward, const float* done, float max_action, float noise_clip, float discount,
                        float* target_q, int q_ld, void* stream) {
  return td_target("sgrl_swat_td_target", actor_t, q1_t, q2_t, next_obs, obs_ld, noise, noise_ld, reward, done, max_action, noise_clip,
                   discount, target_q, q_ld, nullptr, stream);
}

int sgrl_swat_td_target_dropout(sgrl_swat* actor_t, sgrl_swat* q1_t, sgrl_swat* q2_t, const float* next_obs, int obs_ld,
                                const float* noise, int noise_ld, const float* reward, const float* done, float max_action,
                                float noise_clip, float discount, float* target_q, int q_ld, float p, uint64_t seed,
                                const uint64_t* step_dev, int site0, void* stream) {
  const DropArgs da{p, seed, step_dev, site0, nullptr};
  return td_target("sgrl_swat_td_target_dropout", actor_t, q1_t, q2_t, next_obs, obs_ld, noise, noise_ld, reward, done, max_action,
                   noise_clip, discount, target_q, q_ld, &da, stream);
}

int sgrl_swat_dropout_sites(void) { return kDropSites; }
int sgrl_swat_dropout_launches(void) { return kDropLaunches; }
int sgrl_swat_td_target_dropout_launches(void) { return 3 * kDropLaunches; }
int sgrl_swat_twin_launches(void) { return 2 * kLaunches; }
int sgrl_swat_td_target_launches(void) { return 3 * kLaunches; }
int sgrl_swat_debug_twin_streams(int on) { g_twin_streams = on != 0; return SGRL_OK; }

int sgrl_swat_num_nodes(const sgrl_swat* s) { return (s && s->cur) ? s->cur->N : SGRL_ERR_ARG; }
int sgrl_swat_launches(void) { return kLaunches; }
int64_t sgrl_swat_generation(const sgrl_swat* s) { return s ? s->generation : -1; }
const char* sgrl_swat_last_error(void) { return g_swat_err.c_str(); }

}  // extern "C"
