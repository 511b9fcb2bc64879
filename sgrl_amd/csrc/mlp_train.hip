// mlp_train.hip -- the gradient half of the monolithic MLP agent's TD3 update (C ABI: include/sgrl_mlp.h, "gradient half"): what
// autograd did for the critic loss and the actor loss, as two launches per step on top of the pack.
//
//   k_mlp_critic_fb  one workgroup (4 waves) per 32 batch rows, both Q stacks in one launch.  Per stack: the cat([obs, action]) tile
//                    into the LDS activation tile X[32][sx]; every layer forward by mlp_walk (mlp_tile.h, the walk of the
//                    no-grad forwards: whole output row block in registers, weights streamed through a double-buffered LDS
//                    panel) with a stash, so the post-ReLU rows ALSO go to the workspace (A_l [B][npad_l]); q,
//                    dq = 2 (q - target) / B, the tile's partial of sum (q - target)^2; then back:
//                    G_l = (G_{l+1} . W_{l+1}) (.) (A_l > 0) -- the backward form of the same panel product, tile_gemm -- with
//                    G_{l+1} in X as the row operand and ROWS of the packed [npad][kpad] weight as panels (reduction over npad,
//                    output columns = kpad: contiguous reads, no transposed copy); every G_l stored to the workspace.
//   k_mlp_actor_fb   actor forward with stash, a = max_action * tanh(z) (tanh(z) stashed), the critic's input tile from obs and a
//                    (action columns re-read by the lanes that stored them, as k_mlp_chain), Q1 forward with stash, dq = -1 / B, the
//                    tile's partial of sum q1, Q1 back down to its input's ACTION columns (K = npad_0, 3 L output columns read at
//                    column offset 41 L of W_0), dz = da * max_action * (1 - tanh^2), the actor back, its G_l stored.
//   k_mlp_wgrad      one launch over every layer of every stack of the step: a workgroup owns one 32 x 32 tile of one
//                    dW_l = G_l^T A_{l-1}, its four waves take the row pairs p = wave, wave + 4, ... in order and their four partial
//                    tiles are summed in LDS in wave order -- fixed order, no split-K across workgroups, no atomics.  The k-tile-0
//                    workgroups also sum the G operand they read anyway into the bias gradient; workgroup 0 reduces the loss partials.
//                    Results go to the .grad tensors unpadded, element-wise.
//
// A lane that needs a stashed value in the backward pass (the ReLU mask, tanh) is the lane that stored it: the output tile of layer l
// forward and of G_l backward have the same (chunk, wave, lane) -> column mapping.  Rows >= B of a tile carry dq = 0, so every G row
// of theirs is an exact zero and nothing of theirs is stored; the weight-gradient launch reads rows < B only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "mlp_tile.h"

using namespace sgrl_mlp_detail;

namespace {

// X holds G of the last layer (columns [0, npad[last])): G_l = (G_{l+1} . W_{l+1}) (.) (A_l > 0) for every hidden layer, top down,
// over X in place; stored to G[l] (rows < B) when `store`.
template <int MAXCH, int BK>
__device__ __forceinline__ void bwd_hidden(const Net& a, float* const* A, float* const* G, bool store, float* X, float* Ws, int sx, int row0,
                                           int B) {
  for (int l = a.n_layers - 2; l >= 0; l--) {
    const int N = a.npad[l];                   // = kpad[l + 1], the row length of W_{l+1}
    const float* Al = A[l];
    float* Gl = store ? G[l] : nullptr;
    tile_gemm<MAXCH, BK, true>(a.wp + a.w_off[l + 1], N, a.npad[l + 1], N, X, Ws, sx, [&](int n, const f32x16& acc) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int m = tile_row(e);
        const int row = row0 + m;
        float g = 0.f;
        if (row < B) {
          g = Al[(size_t)row * N + n] > 0.f ? acc[e] : 0.f;
          if (Gl) Gl[(size_t)row * N + n] = g;
        }
        X[m * sx + n] = g;
      }
    });
  }
}

// X[r][0 : width) of the rows that exist -> dst[row][0 : width)
__device__ __forceinline__ void stash_input(const float* X, int sx, int width, float* dst, int row0, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < BM; r += 4) {
    const int row = row0 + r;
    if (row >= B) break;
    for (int k = lane; k < width; k += 64) dst[(size_t)row * width + k] = X[r * sx + k];
  }
}

struct CriticFbArgs {
  const float* obs; int obs_ld;
  const float* act; int act_ld;
  const float* target;
  int n_env, obs_dim, act_dim, sx;
  Net c[2];
  float* X0;                         // [B][kpad_0]
  float* A[2][NL];                   // [stack][l]: [B][npad_l], hidden layers
  float* G[2][NL];                   // [stack][l]: [B][npad_l], every layer
  float* part;                       // [tiles][2 stacks][2 lane halves]
};

template <int MAXCH, int BK>
__global__ __launch_bounds__(256) void k_mlp_critic_fb(CriticFbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mlp_train_lds[];
  float* X = mlp_train_lds;
  float* Ws = mlp_train_lds + BM * a.sx;
  const int row0 = blockIdx.x * BM, B = a.n_env, sx = a.sx;
  const int lh = (threadIdx.x & 63) >> 5;
  for (int s = 0; s < 2; s++) {
    const Net& net = a.c[s];
    load_rows(X, sx, 0, a.obs_dim, a.obs_dim, a.obs, a.obs_ld, row0, B);
    load_rows(X, sx, a.obs_dim, a.act_dim, net.kpad[0] - a.obs_dim, a.act, a.act_ld, row0, B);
    __syncthreads();
    if (s == 0) stash_input(X, sx, net.kpad[0], a.X0, row0, B);
    const int last = net.n_layers - 1;
    float* Glast = a.G[s][last];
    const int NLp = net.npad[last];
    mlp_walk<MAXCH, BK>(net, a.A[s], X, Ws, sx, row0, B, [&](int n, const f32x16& acc, float bvv) {
      float part = 0.f;
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int m = tile_row(e);
        const int row = row0 + m;
        float g = 0.f;
        if (row < B) {
          if (n == 0) {
            const float d = acc[e] + bvv - a.target[row];
            part += d * d;
            g = 2.f * d / (float)B;
          }
          Glast[(size_t)row * NLp + n] = g;
        }
        X[m * sx + n] = g;
      }
      if (n == 0) a.part[(blockIdx.x * 2 + s) * 2 + lh] = part;
    });
    bwd_hidden<MAXCH, BK>(net, a.A[s], a.G[s], true, X, Ws, sx, row0, B);
  }
}

struct ActorFbArgs {
  const float* obs; int obs_ld;
  int n_env, in_dim, out_dim, sx;
  float max_action;
  Net actor, c1;
  float* X0;                         // actor input [B][kpad_0]
  float* A[NL];                      // actor hidden activations
  float* G[NL];                      // actor G_l
  float* T;                          // tanh(z) [B][npad_last]
  float* abuf; int abuf_ld;          // the action rows
  float* Ac[NL];                     // Q1's hidden activations (the critic handle's workspace, stack 1)
  float* part;                       // [tiles][2 lane halves]
};

template <int MAXCH, int BK>
__global__ __launch_bounds__(256) void k_mlp_actor_fb(ActorFbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mlp_train_lds[];
  float* X = mlp_train_lds;
  float* Ws = mlp_train_lds + BM * a.sx;
  const int lh = (threadIdx.x & 63) >> 5;
  const int row0 = blockIdx.x * BM, B = a.n_env, sx = a.sx;
  float* abuf = a.abuf;                        // stored and re-read by the same lanes: not restrict
  float* T = a.T;
  const int alast = a.actor.n_layers - 1;
  const int NA = a.actor.npad[alast];
  load_rows(X, sx, 0, a.in_dim, a.actor.kpad[0], a.obs, a.obs_ld, row0, B);
  __syncthreads();
  stash_input(X, sx, a.actor.kpad[0], a.X0, row0, B);
  mlp_walk<MAXCH, BK>(a.actor, a.A, X, Ws, sx, row0, B, [&](int n, const f32x16& acc, float bvv) {
    if (n < a.out_dim) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int row = row0 + tile_row(e);
        if (row < B) {
          const float th = tanhf(acc[e] + bvv);
          T[(size_t)row * NA + n] = th;
          abuf[(size_t)row * a.abuf_ld + n] = a.max_action * th;
        }
      }
    }
  });
  // Q1's input tile, the action columns re-read by the lanes that stored them
  load_obs_stored_actions<MAXCH>(X, sx, a.obs, a.obs_ld, a.in_dim, abuf, a.abuf_ld, a.out_dim, NA, a.c1.kpad[0], row0, B);
  __syncthreads();
  mlp_walk<MAXCH, BK>(a.c1, a.Ac, X, Ws, sx, row0, B, [&](int n, const f32x16& acc, float bvv) {
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int m = tile_row(e);
      const bool on = n == 0 && row0 + m < B;
      if (on) part += acc[e] + bvv;
      X[m * sx + n] = on ? -1.f / (float)B : 0.f;
    }
    if (n == 0) a.part[blockIdx.x * 2 + lh] = part;
  });
  bwd_hidden<MAXCH, BK>(a.c1, a.Ac, nullptr, false, X, Ws, sx, row0, B);
  // d loss / d action = G_0 . W_0[:, 41 L : 44 L), then through max_action * tanh
  float* Glast = a.G[alast];
  tile_gemm<MAXCH, BK, true>(a.c1.wp + a.c1.w_off[0] + a.in_dim, a.c1.kpad[0], a.c1.npad[0], a.out_dim, X, Ws, sx, [&](int n, const f32x16& acc) {
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int m = tile_row(e);
      const int row = row0 + m;
      float dz = 0.f;
      if (row < B) {
        if (n < a.out_dim) {
          const float th = T[(size_t)row * NA + n];
          dz = acc[e] * a.max_action * (1.f - th * th);
        }
        Glast[(size_t)row * NA + n] = dz;
      }
      X[m * sx + n] = dz;
    }
  });
  bwd_hidden<MAXCH, BK>(a.actor, a.A, a.G, true, X, Ws, sx, row0, B);
}

struct WgEntry {                     // one dW = G^T In  ([N][K], unpadded) and its db
  const float* G; const float* In;
  float* dW; float* db;
  int ldg, ldin, N, K, tile0, nkt;
};

struct WgArgs {
  WgEntry e[2 * NL];
  int n_entries, B;
  const float* part; int n_part;
  float scale;
  float* loss_out;
};

__global__ __launch_bounds__(256) void k_mlp_wgrad(WgArgs a) {
  __shared__ float red[4][16][64];
  __shared__ float bred[8][32];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
  int i = 0;
  while (i + 1 < a.n_entries && (int)blockIdx.x >= a.e[i + 1].tile0) i++;
  const float* __restrict__ G = a.e[i].G;
  const float* __restrict__ In = a.e[i].In;
  const int ldg = a.e[i].ldg, ldin = a.e[i].ldin, N = a.e[i].N, K = a.e[i].K, nkt = a.e[i].nkt;
  const int tile = (int)blockIdx.x - a.e[i].tile0;
  const int nt = tile / nkt, kt = tile - nt * nkt;
  const int n0 = 32 * nt, k0 = 32 * kt;
  const bool kin = k0 + li < K;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; e++) acc[e] = 0.f;
  float bsum = 0.f;
  const int npairs = (a.B + 1) / 2;
  for (int p = wave; p < npairs; p += 4) {
    const int m = 2 * p + lh;
    const bool ok = m < a.B;
    const float g = ok ? G[(size_t)m * ldg + n0 + li] : 0.f;       // G is padded to 32 columns with exact zeros
    const float x = (ok && kin) ? In[(size_t)m * ldin + k0 + li] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g, x, acc, 0, 0, 0);
    bsum += g;
  }
#pragma unroll
  for (int e = 0; e < 16; e++) red[wave][e][lane] = acc[e];
  bred[wave * 2 + lh][li] = bsum;
  __syncthreads();
  float* dW = a.e[i].dW;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int idx = t + 256 * q, e = idx >> 6, ln = idx & 63;
    const float v = ((red[0][e][ln] + red[1][e][ln]) + red[2][e][ln]) + red[3][e][ln];
    const int n = n0 + (e & 3) + 8 * (e >> 2) + 4 * (ln >> 5), k = k0 + (ln & 31);
    if (n < N && k < K) dW[(size_t)n * K + k] = v;
  }
  if (kt == 0 && t < 32 && n0 + t < N) {
    float v = 0.f;
#pragma unroll
    for (int h = 0; h < 8; h++) v += bred[h][t];
    a.e[i].db[n0 + t] = v;
  }
  if (blockIdx.x == 0 && t == 0) {
    float s = 0.f;
    for (int p = 0; p < a.n_part; p++) s += a.part[p];
    a.loss_out[0] = s * a.scale;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// pa may be null (the critic step walks the critic alone)
int make_train_plan(const Plan* pa, const Plan& pc, TilePlan* tp, const char* who) {
  int wmax = 0, nmax = 0;
  for (int k = 0; k < 2; k++) {
    const Plan* p = k ? &pc : pa;
    if (!p) continue;
    for (int l = 0; l < p->n_layers; l++) {
      wmax = p->kpad[l] > wmax ? p->kpad[l] : wmax;
      wmax = p->npad[l] > wmax ? p->npad[l] : wmax;
      nmax = p->npad[l] > nmax ? p->npad[l] : nmax;
    }
  }
  if (nmax > SGRL_MLP_TRAIN_MAX_WIDTH)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": the gradient half serves layer widths up to " + std::to_string(SGRL_MLP_TRAIN_MAX_WIDTH) +
                                   " (padded), got " + std::to_string(nmax) + ": keep the PyTorch gradient half for these networks");
  *tp = tile_plan(nmax <= CH ? 1 : 2, wmax + 4);
  if (tp->lds > LDS_LIMIT) return mfail(SGRL_ERR_LIMIT, std::string(who) + ": the activation tile does not fit in LDS");
  return SGRL_OK;
}

int wgrad_tiles(const Plan& p, int stacks) {
  int n = 0;
  for (int l = 0; l < p.n_layers; l++) n += ((p.dims[l + 1] + 31) / 32) * ((p.dims[l] + 31) / 32);
  return n * stacks;
}

// Float offsets into a handle's training workspace at B rows.
struct WsLayout {
  int64_t x0 = 0, A[2][NL] = {{0}}, G[2][NL] = {{0}}, T = 0, abuf = 0, part = 0, total = 0;
};
WsLayout ws_layout(const Plan& p, int stacks, int B) {
  WsLayout w;
  const int tiles = (B + BM - 1) / BM;
  int64_t off = 0;
  w.x0 = off; off += (int64_t)B * p.kpad[0];
  for (int s = 0; s < stacks; s++) {
    for (int l = 0; l + 1 < p.n_layers; l++) { w.A[s][l] = off; off += (int64_t)B * p.npad[l]; }
    for (int l = 0; l < p.n_layers; l++) { w.G[s][l] = off; off += (int64_t)B * p.npad[l]; }
  }
  if (stacks == 1) {
    w.T = off; off += (int64_t)B * p.npad[p.n_layers - 1];
    w.abuf = off; off += (int64_t)B * p.dims[p.n_layers];
  }
  w.part = off; off += (int64_t)tiles * 2 * stacks;
  w.total = off;
  return w;
}

// the handle's training workspace holds at least `need` floats
int ensure_tws(sgrl_mlp* s, int64_t need, bool capturing, const char* who) {
  if (need <= s->tws_floats) return SGRL_OK;
  return grow(&s->tws, &s->tws_floats, need, capturing, &s->generation, who, "training workspace");
}

typedef void (*critic_fb_fn)(CriticFbArgs);
typedef void (*actor_fb_fn)(ActorFbArgs);
#define SGRL_MLP_TRAIN_PICK(K, maxch, bk) ((bk) == 16 ? ((maxch) == 1 ? K<1, 16> : K<2, 16>) : ((maxch) == 1 ? K<1, 8> : K<2, 8>))

// the weight-gradient entries of `stacks` stacks of a handle, appended to wa
void add_wgrad_entries(WgArgs* wa, const sgrl_mlp* s, int stacks, const WsLayout& w, int* tile0) {
  const Plan& p = s->plan;
  for (int k = 0; k < stacks; k++)
    for (int l = 0; l < p.n_layers; l++) {
      WgEntry& e = wa->e[wa->n_entries++];
      e.G = s->tws + w.G[k][l];
      e.ldg = p.npad[l];
      e.In = l == 0 ? s->tws + w.x0 : s->tws + w.A[k][l - 1];
      e.ldin = l == 0 ? p.kpad[0] : p.npad[l - 1];
      e.N = p.dims[l + 1];
      e.K = p.dims[l];
      e.dW = s->gw[k][l];
      e.db = s->gb[k][l];
      e.tile0 = *tile0;
      e.nkt = (e.K + 31) / 32;
      *tile0 += ((e.N + 31) / 32) * e.nkt;
    }
}

}  // namespace

extern "C" {

int sgrl_mlp_critic_step_launches(void) { return 3; }
int sgrl_mlp_actor_step_launches(void) { return 4; }

int sgrl_mlp_train_plan(const int32_t* actor_dims, int n_a, const int32_t* critic_dims, int n_c, int batch, int32_t* info,
                        int64_t* ws_floats) {
  if (!info || !ws_floats) return mfail(SGRL_ERR_ARG, "sgrl_mlp_train_plan: null argument");
  Plan pa, pc;
  int rc = make_pair_plans(actor_dims, n_a, critic_dims, n_c, &pa, &pc, "sgrl_mlp_train_plan");
  if (rc != SGRL_OK) return rc;
  if (batch < 1 || batch > (1 << 24)) return mfail(SGRL_ERR_ARG, "sgrl_mlp_train_plan: batch outside 1 .. 2^24");
  TilePlan tp;
  rc = make_train_plan(&pa, pc, &tp, "sgrl_mlp_train_plan");
  if (rc != SGRL_OK) return rc;
  put_tile_plan(tp, info);
  info[4] = wgrad_tiles(pc, 2);
  info[5] = wgrad_tiles(pa, 1);
  info[6] = (batch + BM - 1) / BM;
  ws_floats[0] = ws_layout(pc, 2, batch).total;
  ws_floats[1] = ws_layout(pa, 1, batch).total;
  return SGRL_OK;
}

int sgrl_mlp_bind_grads(sgrl_mlp* s, const void* const* ptrs, int n_ptrs) {
  if (!s || !ptrs) return mfail(SGRL_ERR_ARG, "sgrl_mlp_bind_grads: null argument");
  if (s->kind == SGRL_MLP_KIND_NONE) return mfail(SGRL_ERR_ARG, "sgrl_mlp_bind_grads: parameters not set (sgrl_mlp_set_params / sgrl_mlp_set_critic_params)");
  const int stacks = n_stacks(s);
  const int nl = s->plan.n_layers;
  if (n_ptrs != 2 * stacks * nl)
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_bind_grads: expected " + std::to_string(2 * stacks * nl) + " gradient addresses, got " + std::to_string(n_ptrs));
  const int rc = check_addresses(ptrs, n_ptrs, "sgrl_mlp_bind_grads", "gradient");
  if (rc != SGRL_OK) return rc;
  for (int k = 0; k < stacks; k++)
    for (int l = 0; l < nl; l++) {
      s->gw[k][l] = static_cast<float*>(const_cast<void*>(ptrs[2 * (k * nl + l)]));
      s->gb[k][l] = static_cast<float*>(const_cast<void*>(ptrs[2 * (k * nl + l) + 1]));
    }
  s->grads_bound = true;
  return SGRL_OK;
}

int sgrl_mlp_critic_step_grads(sgrl_mlp* s, const float* obs, int obs_ld, const float* act, int act_ld, const float* target_q, float* loss_out,
                               void* stream) {
  const char* who = "sgrl_mlp_critic_step_grads";
  if (!s || !obs || !act || !target_q || !loss_out) return mfail(SGRL_ERR_ARG, std::string(who) + ": null argument");
  if (s->kind != SGRL_MLP_KIND_CRITIC) return mfail(SGRL_ERR_ARG, std::string(who) + ": the handle is not bound as a critic");
  if (s->n_env <= 0) return mfail(SGRL_ERR_ARG, std::string(who) + ": batch structure not set");
  if (!s->grads_bound) return mfail(SGRL_ERR_ARG, std::string(who) + ": gradients not bound (sgrl_mlp_bind_grads)");
  if (obs_ld < s->obs_w || act_ld < s->act_w)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": obs_ld or act_ld below the columns the critic reads (rows too narrow for the network)");
  const Plan& p = s->plan;
  TilePlan tp;
  int rc = make_train_plan(nullptr, p, &tp, who);
  if (rc != SGRL_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int B = s->n_env;
  const WsLayout w = ws_layout(p, 2, B);
  rc = ensure_tws(s, w.total, is_capturing(st), who);
  if (rc != SGRL_OK) return rc;
  critic_fb_fn fn = SGRL_MLP_TRAIN_PICK(k_mlp_critic_fb, tp.maxch, tp.bk);
  rc = raise_lds(reinterpret_cast<const void*>(fn), tp.lds, who);
  if (rc != SGRL_OK) return rc;
  rc = pack_now(s, st);
  if (rc != SGRL_OK) return rc;
  CriticFbArgs a;
  a.obs = obs; a.obs_ld = obs_ld; a.act = act; a.act_ld = act_ld; a.target = target_q;
  a.n_env = B; a.obs_dim = s->obs_w; a.act_dim = s->act_w; a.sx = tp.sx;
  a.X0 = s->tws + w.x0;
  a.part = s->tws + w.part;
  for (int k = 0; k < 2; k++) {
    a.c[k] = make_net(p, s->packed + k * p.total);
    for (int l = 0; l < NL; l++) {
      a.A[k][l] = l + 1 < p.n_layers ? s->tws + w.A[k][l] : nullptr;
      a.G[k][l] = l < p.n_layers ? s->tws + w.G[k][l] : nullptr;
    }
  }
  const int tiles = (B + BM - 1) / BM;
  hipLaunchKernelGGL(fn, dim3(tiles), dim3(256), tp.lds, st, a);
  rc = launched("MLP critic forward-backward");
  if (rc != SGRL_OK) return rc;
  WgArgs wa;
  wa.n_entries = 0;
  int ntiles = 0;
  add_wgrad_entries(&wa, s, 2, w, &ntiles);
  wa.B = B; wa.part = a.part; wa.n_part = tiles * 4; wa.scale = 1.f / (float)B; wa.loss_out = loss_out;
  hipLaunchKernelGGL(k_mlp_wgrad, dim3(ntiles), dim3(256), 0, st, wa);
  return launched("MLP weight gradients");
}

int sgrl_mlp_actor_step_grads(sgrl_mlp* actor, sgrl_mlp* critic, const float* obs, int obs_ld, float max_action, float* loss_out,
                              float* action_out, int action_ld, void* stream) {
  const char* who = "sgrl_mlp_actor_step_grads";
  if (!actor || !critic || !obs || !loss_out) return mfail(SGRL_ERR_ARG, std::string(who) + ": null argument");
  int rc = check_pair(actor, critic, who);
  if (rc != SGRL_OK) return rc;
  if (!actor->grads_bound) return mfail(SGRL_ERR_ARG, std::string(who) + ": gradients not bound (sgrl_mlp_bind_grads on the actor)");
  const Plan& pa = actor->plan;
  const Plan& pc = critic->plan;
  const int in_dim = pa.dims[0], out_dim = pa.dims[pa.n_layers], B = actor->n_env;
  if (obs_ld < in_dim || (action_out && action_ld < out_dim))
    return mfail(SGRL_ERR_ARG, std::string(who) + ": obs_ld or action_ld below the network's width (rows too narrow for the network)");
  TilePlan tp;
  rc = make_train_plan(&pa, pc, &tp, who);
  if (rc != SGRL_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool capturing = is_capturing(st);
  const WsLayout wa_ = ws_layout(pa, 1, B);
  const WsLayout wc = ws_layout(pc, 2, B);
  rc = ensure_tws(actor, wa_.total, capturing, who);
  if (rc != SGRL_OK) return rc;
  rc = ensure_tws(critic, wc.total, capturing, who);
  if (rc != SGRL_OK) return rc;
  actor_fb_fn fn = SGRL_MLP_TRAIN_PICK(k_mlp_actor_fb, tp.maxch, tp.bk);
  rc = raise_lds(reinterpret_cast<const void*>(fn), tp.lds, who);
  if (rc != SGRL_OK) return rc;
  rc = pack_now(actor, st);
  if (rc != SGRL_OK) return rc;
  rc = pack_now(critic, st);
  if (rc != SGRL_OK) return rc;
  ActorFbArgs a;
  a.obs = obs; a.obs_ld = obs_ld; a.n_env = B; a.in_dim = in_dim; a.out_dim = out_dim; a.sx = tp.sx; a.max_action = max_action;
  a.actor = make_net(pa, actor->packed);
  a.c1 = make_net(pc, critic->packed);
  a.X0 = actor->tws + wa_.x0;
  a.T = actor->tws + wa_.T;
  a.abuf = action_out ? action_out : actor->tws + wa_.abuf;
  a.abuf_ld = action_out ? action_ld : out_dim;
  a.part = actor->tws + wa_.part;
  for (int l = 0; l < NL; l++) {
    a.A[l] = l + 1 < pa.n_layers ? actor->tws + wa_.A[0][l] : nullptr;
    a.G[l] = l < pa.n_layers ? actor->tws + wa_.G[0][l] : nullptr;
    a.Ac[l] = l + 1 < pc.n_layers ? critic->tws + wc.A[0][l] : nullptr;
  }
  const int tiles = (B + BM - 1) / BM;
  hipLaunchKernelGGL(fn, dim3(tiles), dim3(256), tp.lds, st, a);
  rc = launched("MLP actor forward-backward");
  if (rc != SGRL_OK) return rc;
  WgArgs wg;
  wg.n_entries = 0;
  int ntiles = 0;
  add_wgrad_entries(&wg, actor, 1, wa_, &ntiles);
  wg.B = B; wg.part = a.part; wg.n_part = tiles * 2; wg.scale = -1.f / (float)B; wg.loss_out = loss_out;
  hipLaunchKernelGGL(k_mlp_wgrad, dim3(ntiles), dim3(256), 0, st, wg);
  return launched("MLP weight gradients");
}

}  // extern "C"
