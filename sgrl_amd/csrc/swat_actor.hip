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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sgrl.h"
#include "../../include/sgrl_swat.h"

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

using sgrl_gemm::EPI_RELU;
using sgrl_gemm::GemmArgs;
using sgrl_gemm::k_gemm2;

__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct NodeTab {
  const int32_t* node_env;    // [N]
  const int32_t* node_limb;   // [N]
  const int32_t* node_mnode;  // [N] column of the node in the traversal table
  const int32_t* trav;        // [3][TM]
  int TM;
};

// input embedding + position embedding (StructureActor.py:159-164, 16-30): 8 nodes per 128-thread block, thread = channel; the
// block's input rows are staged in LDS and every weight is loaded once per block
constexpr int kEmbedNodes = 8;
__global__ __launch_bounds__(128) void k_swat_embed(const float* __restrict__ obs, int obs_ld, int F, const float* __restrict__ Wenc,
                                                     const float* __restrict__ benc, const float* __restrict__ emb0,
                                                     const float* __restrict__ emb1, const float* __restrict__ emb2, NodeTab nt,
                                                     float* __restrict__ h, int N, float scale) {
  __shared__ float xs[kEmbedNodes][64];
  const int c = threadIdx.x, nb = blockIdx.x * kEmbedNodes;
  for (int i = c; i < kEmbedNodes * 64; i += 128) {
    const int r = i / 64, k = i % 64, n = nb + r;
    float v = 0.f;
    if (n < N && k < F) v = obs[(size_t)nt.node_env[n] * obs_ld + F * nt.node_limb[n] + k];
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
__global__ __launch_bounds__(128) void k_swat_attn(const float* __restrict__ qkv, float* __restrict__ o, EnvTab et,
                                                    const float* __restrict__ rel, const float* __restrict__ Wrel,
                                                    const float* __restrict__ brel, int use_bias) {
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
    for (int j = 0; j < L; j++) s_p[hh][i][j] *= inv;
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

// h = LayerNorm(h + d), in place; one wave per row
__global__ __launch_bounds__(256) void k_swat_add_ln(float* __restrict__ h, const float* __restrict__ d, const float* __restrict__ w,
                                                      const float* __restrict__ b, int N) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  float v0 = h[(size_t)row * E + lane] + d[(size_t)row * E + lane];
  float v1 = h[(size_t)row * E + 64 + lane] + d[(size_t)row * E + 64 + lane];
  row_ln(v0, v1, w, b, lane);
  h[(size_t)row * E + lane] = v0;
  h[(size_t)row * E + 64 + lane] = v1;
}

// last layer's norm2, the final LayerNorm (fw != null), the decoder (StructureActor.py:164-170: over h, or [h | x] with
// cond_decoder) and max_action * tanh (StructureActor.py:221-243); one wave per node.  The node of limb 0 of every environment
// also writes the zero padding act[e, out * L_e : act_ld].
__global__ __launch_bounds__(256) void k_swat_tail(const float* __restrict__ h, const float* __restrict__ d, const float* __restrict__ n2w,
                                                    const float* __restrict__ n2b, const float* __restrict__ fw, const float* __restrict__ fb,
                                                    const float* __restrict__ Wd, const float* __restrict__ bd, int cond, int F, int O,
                                                    const float* __restrict__ obs, int obs_ld, NodeTab nt, const int32_t* __restrict__ env_L,
                                                    float* __restrict__ act, int act_ld, float max_action, int N) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  float v0 = h[(size_t)row * E + lane] + d[(size_t)row * E + lane];
  float v1 = h[(size_t)row * E + 64 + lane] + d[(size_t)row * E + 64 + lane];
  row_ln(v0, v1, n2w, n2b, lane);
  if (fw) row_ln(v0, v1, fw, fb, lane);
  const int env = nt.node_env[row], limb = nt.node_limb[row];
  const int ldd = cond ? E + F : E;
  const float x = (cond && lane < F) ? obs[(size_t)env * obs_ld + F * limb + lane] : 0.f;
  float* arow = act + (size_t)env * act_ld;
  for (int j = 0; j < O; j++) {
    const float* wr = Wd + (size_t)j * ldd;
    float s = fmaf(v0, wr[lane], v1 * wr[64 + lane]);
    if (cond && lane < F) s = fmaf(x, wr[E + lane], s);
    s = wave_sum(s) + bd[j];
    if (lane == 0) arow[O * limb + j] = max_action * tanhf(s);
  }
  if (limb == 0)
    for (int k = O * env_L[env] + lane; k < act_ld; k += 64) arow[k] = 0.f;
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
  float* ws = nullptr;          // workspace: h [N, 128] | qkv [N, 384] | o [N, 128]; grows only
  int64_t ws_floats = 0;
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

int64_t ws_floats_for(int64_t N) { return (E + 3 * E + E) * N + 3 * 64; }

int use_cfg(sgrl_swat* s, SwatGraphCfg* c) {
  const int64_t need = ws_floats_for(c->N);
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

int run_forward(sgrl_swat* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, hipStream_t st) {
  const SwatGraphCfg* c = s->cur;
  const int N = c->N;
  // workspace carve-up (16-byte aligned rows for the GEMM's float4 loads): h [N, 128] | qkv [N, 384] | o [N, 128];
  // the out_proj result and the feed-forward hidden layer reuse qkv, linear2's result reuses o
  auto al = [](int64_t n) { return (n + 63) & ~int64_t(63); };
  float* h = s->ws;
  float* qkv = h + al((int64_t)E * N);
  float* o = qkv + al((int64_t)3 * E * N);
  NodeTab nt{c->d_node_env, c->d_node_limb, c->d_node_mnode, c->d_trav, c->TM};
  EnvTab et{c->d_env_off, c->d_env_L, c->d_env_rel};
  hipLaunchKernelGGL(k_swat_embed, dim3((N + kEmbedNodes - 1) / kEmbedNodes), dim3(128), 0, st, obs, obs_ld, s->F,
                     s->W(SGRL_SWAT_ENC_W), s->W(SGRL_SWAT_ENC_B), s->W(SGRL_SWAT_EMB0), s->W(SGRL_SWAT_EMB1), s->W(SGRL_SWAT_EMB2), nt,
                     h, N, sqrtf((float)E));
  const int rows4 = (N + 3) / 4;
  for (int l = 0; l < SGRL_SWAT_LAYERS; l++) {
    launch_gemm(st, false, h, E, s->WL(l, SGRL_SWAT_IN_W), s->WL(l, SGRL_SWAT_IN_B), qkv, 3 * E, N, 3 * E, E);
    hipLaunchKernelGGL(k_swat_attn, dim3(c->n_env), dim3(128), 0, st, qkv, o, et, c->d_rel, s->W(SGRL_SWAT_REL_W),
                       s->W(SGRL_SWAT_REL_B), l == 0 ? 1 : 0);
    float* d1 = qkv;
    launch_gemm(st, false, o, E, s->WL(l, SGRL_SWAT_OUT_W), s->WL(l, SGRL_SWAT_OUT_B), d1, E, N, E, E);
    hipLaunchKernelGGL(k_swat_add_ln, dim3(rows4), dim3(256), 0, st, h, d1, s->WL(l, SGRL_SWAT_N1_W), s->WL(l, SGRL_SWAT_N1_B), N);
    float* f = qkv;
    launch_gemm(st, true, h, E, s->WL(l, SGRL_SWAT_L1_W), s->WL(l, SGRL_SWAT_L1_B), f, FF, N, FF, E);
    float* d2 = o;
    launch_gemm(st, false, f, FF, s->WL(l, SGRL_SWAT_L2_W), s->WL(l, SGRL_SWAT_L2_B), d2, E, N, E, FF);
    if (l + 1 < SGRL_SWAT_LAYERS) {
      hipLaunchKernelGGL(k_swat_add_ln, dim3(rows4), dim3(256), 0, st, h, d2, s->WL(l, SGRL_SWAT_N2_W), s->WL(l, SGRL_SWAT_N2_B), N);
    } else {
      const int fn = SGRL_SWAT_NGLOBAL + SGRL_SWAT_LAYERS * SGRL_SWAT_NLAYER;
      hipLaunchKernelGGL(k_swat_tail, dim3(rows4), dim3(256), 0, st, h, d2, s->WL(l, SGRL_SWAT_N2_W), s->WL(l, SGRL_SWAT_N2_B),
                         s->tnorm ? s->p[fn] : (const float*)nullptr, s->tnorm ? s->p[fn + 1] : (const float*)nullptr,
                         s->W(SGRL_SWAT_DEC_W), s->W(SGRL_SWAT_DEC_B), s->cond ? 1 : 0, s->F, s->O, obs, obs_ld, nt, c->d_env_L,
                         act, act_ld, max_action, N);
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return wfail(SGRL_ERR_HIP, std::string("SWAT forward launch: ") + hipGetErrorString(e));
  return SGRL_OK;
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
  if (!s || !obs || !act) return wfail(SGRL_ERR_ARG, "sgrl_swat_forward: null argument");
  if (!s->have_w || !s->cur) return wfail(SGRL_ERR_ARG, "sgrl_swat_forward: parameters or batch structure not set");
  if (obs_ld < s->F * s->cur->Lmax || act_ld < s->O * s->cur->Lmax)
    return wfail(SGRL_ERR_ARG, "sgrl_swat_forward: obs_ld < feature * Lmax or act_ld < out * Lmax (rows too narrow for the largest morphology)");
  return run_forward(s, obs, obs_ld, act, act_ld, max_action, (hipStream_t)stream);
}

int sgrl_swat_num_nodes(const sgrl_swat* s) { return (s && s->cur) ? s->cur->N : SGRL_ERR_ARG; }
int sgrl_swat_launches(void) { return kLaunches; }
int64_t sgrl_swat_generation(const sgrl_swat* s) { return s ? s->generation : -1; }
const char* sgrl_swat_last_error(void) { return g_swat_err.c_str(); }

}  // extern "C"
