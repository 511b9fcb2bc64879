// mlp_actor.hip -- the monolithic MLP agent's no-grad forwards for a whole batch of environments, ONE launch each (C ABI:
// include/sgrl_mlp.h): the actor, the twin critic, and the TD3 target chain (target actor -> clipped noise -> clamp -> twin target
// critics -> min -> Bellman target).
//
//   k_mlp_pack      live nn.Linear weights / biases -> the padded packed buffer (kpad, npad of sgrl_mlp_plan; zeros in the padding);
//                   at the top of a forward unless the caller holds the weights
//   k_mlp_forward   one workgroup (4 waves) per 32 environment rows.  The observation tile goes into the LDS activation tile
//                   X[32][sx]; mlp_walk (mlp_tile.h, the one layer walk of the family) computes every layer's whole output row
//                   block into registers -- exact-f32 32x32x2 matrix instructions, the weights streamed through a double-buffered
//                   LDS panel of 256 output columns x BK k values -- and writes relu(. + bias) back over X in place.  The last
//                   layer's epilogue writes max_action * tanh(. + bias) to the action rows and exact zeros up to the caller's
//                   leading dimension.
//   k_mlp_critic    the same walk over cat([obs, action]) rows, once per Q stack; the final N = 1 layer leaves Q in column 0 of one
//                   32-column tile, the two lanes holding it write q[row].
//   k_mlp_chain     actor walk, its epilogue adds the clipped noise, clamps and stores the target action; the workgroup then builds
//                   the critics' input tile -- observation columns from global again, action columns re-read by the very lanes
//                   that stored them (same-thread program order: no cross-workgroup traffic) -- and walks critic 1 and critic 2;
//                   Q1 waits in 16 registers of the two lanes that hold it, min and the Bellman line are done by those lanes.
//
// The tile layout and the wave -> column mapping are described in mlp_tile.h.  This unit also defines the host helpers the family
// shares (declared in mlp_internal.h): the plans, the LDS limit of a kernel, the device buffers of a handle, the pair checks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <map>
#include <string>

#include "mlp_tile.h"

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
  static_cast<TilePlan&>(*p) = tile_plan(chunks <= 1 ? 1 : (chunks == 2 ? 2 : 4), kmax + 4);
  if (p->lds > LDS_LIMIT) return mfail(SGRL_ERR_LIMIT, std::string(who) + ": the activation tile does not fit in LDS");
  return SGRL_OK;
}

int sgrl_mlp_detail::lds_bytes(int sx, int bk) { return (int)sizeof(float) * (BM * sx + 2 * CH * (bk + 4)); }

TilePlan sgrl_mlp_detail::tile_plan(int maxch, int sx) {
  TilePlan t;
  t.maxch = maxch;
  t.sx = sx;
  t.bk = lds_bytes(sx, 16) <= LDS_LIMIT ? 16 : 8;
  t.lds = lds_bytes(sx, t.bk);
  return t;
}

void sgrl_mlp_detail::put_tile_plan(const TilePlan& t, int32_t* info) { info[0] = t.maxch; info[1] = t.bk; info[2] = t.lds; info[3] = t.sx; }

int sgrl_mlp_detail::raise_lds(const void* fn, int lds, const char* who) {
  static std::map<const void*, int> raised;
  int& r = raised[fn];
  if (r >= lds) return SGRL_OK;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return mfail(SGRL_ERR_HIP, std::string(who) + ": cannot raise the kernel's dynamic LDS limit");
  r = lds;
  return SGRL_OK;
}

int sgrl_mlp_detail::grow(float** buf, int64_t* floats, int64_t need, bool capturing, int64_t* generation, const char* who, const char* what) {
  if (capturing)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": the " + what + " must grow, which a capture cannot record: run this batch size eagerly first");
  float* fresh = nullptr;
  if (hipMalloc(&fresh, sizeof(float) * (size_t)need) != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("device allocation failed (MLP ") + what + ")");
  if (*buf) {
    (void)hipDeviceSynchronize();           // work in flight may still use the old buffer
    (void)hipFree(*buf);
    (*generation)++;
  }
  *buf = fresh;
  *floats = need;
  return SGRL_OK;
}

bool sgrl_mlp_detail::is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  return cap != hipStreamCaptureStatusNone;
}

int sgrl_mlp_detail::launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
  return SGRL_OK;
}

int sgrl_mlp_detail::n_stacks(const sgrl_mlp* s) { return s->kind == SGRL_MLP_KIND_CRITIC ? 2 : 1; }

int sgrl_mlp_detail::make_pair_plans(const int32_t* actor_dims, int n_a, const int32_t* critic_dims, int n_c, Plan* pa, Plan* pc, const char* who) {
  int rc = make_plan(actor_dims, n_a, pa, (std::string(who) + " (actor)").c_str());
  if (rc != SGRL_OK) return rc;
  rc = make_plan(critic_dims, n_c, pc, (std::string(who) + " (critic)").c_str());
  if (rc != SGRL_OK) return rc;
  if (pc->dims[pc->n_layers] != 1)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": a critic's last width must be 1, got " + std::to_string(pc->dims[pc->n_layers]));
  const int both = pa->dims[0] + pa->dims[pa->n_layers];
  if (pc->dims[0] != both)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": the critic reads " + std::to_string(pc->dims[0]) + " values, not the actor's input + output width " +
                                   std::to_string(both));
  return SGRL_OK;
}

int sgrl_mlp_detail::check_pair(const sgrl_mlp* actor, const sgrl_mlp* critic, const char* who) {
  if (actor->kind != SGRL_MLP_KIND_ACTOR) return mfail(SGRL_ERR_ARG, std::string(who) + ": the first handle is not bound as an actor");
  if (critic->kind != SGRL_MLP_KIND_CRITIC) return mfail(SGRL_ERR_ARG, std::string(who) + ": the second handle is not bound as a critic");
  if (actor->n_env <= 0 || critic->n_env <= 0) return mfail(SGRL_ERR_ARG, std::string(who) + ": batch structure not set");
  if (actor->n_env != critic->n_env)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": actor and critic are configured for different batch structures (" + std::to_string(actor->n_env) +
                                   " / " + std::to_string(critic->n_env) + " environments)");
  const Plan& pa = actor->plan;
  const int in_dim = pa.dims[0], out_dim = pa.dims[pa.n_layers];
  if (critic->plan.dims[0] != in_dim + out_dim || critic->obs_w != in_dim || critic->act_w != out_dim)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": the critic reads " + std::to_string(critic->plan.dims[0]) +
                                   " values, not the actor's input + output width " + std::to_string(in_dim + out_dim));
  return SGRL_OK;
}

int sgrl_mlp_detail::check_addresses(const void* const* ptrs, int n, const char* who, const char* what) {
  for (int i = 0; i < n; i++)
    if (!ptrs[i] || (reinterpret_cast<uintptr_t>(ptrs[i]) & 3))
      return mfail(SGRL_ERR_ARG, std::string(who) + ": " + what + " " + std::to_string(i) + " is null or not 4-byte aligned");
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
  const int row0 = blockIdx.x * BM;
  // observation tile (rows beyond n_env and columns beyond the input width: zeros)
  load_rows(X, a.sx, 0, a.in_dim, a.net.kpad[0], a.obs, a.obs_ld, row0, a.n_env);
  __syncthreads();
  mlp_walk<MAXCH, BK>(a.net, nullptr, X, Ws, a.sx, row0, a.n_env, [&](int n, const f32x16& acc, float bvv) {
    if (n < a.out_dim) {
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int row = row0 + tile_row(e);
        if (row < a.n_env) a.act[(size_t)row * a.act_ld + n] = a.max_action * tanhf(acc[e] + bvv);
      }
    }
  });
  zero_tail(a.act, a.act_ld, a.out_dim, row0, a.n_env);
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
    mlp_walk<MAXCH, BK>(s ? a.c2 : a.c1, nullptr, X, Ws, a.sx, row0, a.n_env, [&](int n, const f32x16& acc, float bvv) {
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
  const int row0 = blockIdx.x * BM;
  const int sx = a.sx;
  float* abuf = a.abuf;                        // stored and re-read by the same lanes below: not restrict
  load_rows(X, sx, 0, a.in_dim, a.actor.kpad[0], a.obs, a.obs_ld, row0, a.n_env);
  __syncthreads();
  mlp_walk<MAXCH, BK>(a.actor, nullptr, X, Ws, sx, row0, a.n_env, [&](int n, const f32x16& acc, float bvv) {
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
  if (a.zero_pad) zero_tail(abuf, a.abuf_ld, a.out_dim, row0, a.n_env);
  const int n_act_pad = a.actor.npad[a.actor.n_layers - 1];
  f32x16 q1v;
#pragma unroll
  for (int e = 0; e < 16; e++) q1v[e] = 0.f;
  for (int s = 0; s < 2; s++) {
    // the critics' input tile, the action columns re-read by the lanes that stored them; the first critic's hidden activations
    // have overwritten it: built again for the second
    load_obs_stored_actions<MAXCH>(X, sx, a.obs, a.obs_ld, a.in_dim, abuf, a.abuf_ld, a.out_dim, n_act_pad, a.c1.kpad[0], row0, a.n_env);
    __syncthreads();
    if (s == 0) {
      mlp_walk<MAXCH, BK>(a.c1, nullptr, X, Ws, sx, row0, a.n_env, [&](int n, const f32x16& acc, float bvv) {
        if (n == 0) {
#pragma unroll
          for (int e = 0; e < 16; e++) q1v[e] = acc[e] + bvv;
        }
      });
    } else {
      mlp_walk<MAXCH, BK>(a.c2, nullptr, X, Ws, sx, row0, a.n_env, [&](int n, const f32x16& acc, float bvv) {
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

// What the fused chain kernel uses for the pair: the larger chunk count, the activation stride of the widest padded input of
// either network, the deepest panel that still fits.
TilePlan make_chain_plan(const Plan& pa, const Plan& pc) {
  return tile_plan(pa.maxch > pc.maxch ? pa.maxch : pc.maxch, pa.sx > pc.sx ? pa.sx : pc.sx);
}

// The pack launch at the top of a forward, unless the handle holds clean weights (a capture always packs; `always`: the gradient
// half, whose weights have just been stepped).
int pack_if_needed(sgrl_mlp* s, hipStream_t st, bool always = false) {
  const bool capturing = is_capturing(st);
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
  const int rc = launched("MLP pack");
  if (rc == SGRL_OK && !capturing) s->dirty = false;
  return rc;
}

// Shared by the two binds: plan, packed buffer of `stacks` stacks, addresses.
int bind_common(sgrl_mlp* s, const void* const* ptrs, int n_ptrs, const int32_t* dims, int n_dims, int stacks, const char* who) {
  if (!s || !ptrs) return mfail(SGRL_ERR_ARG, std::string(who) + ": null argument");
  Plan p;
  int rc = make_plan(dims, n_dims, &p, who);
  if (rc != SGRL_OK) return rc;
  if (stacks == 2 && p.dims[p.n_layers] != 1)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": a critic's last width must be 1, got " + std::to_string(p.dims[p.n_layers]));
  if (n_ptrs != 2 * stacks * p.n_layers)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": expected " + std::to_string(2 * stacks * p.n_layers) + " parameter addresses, got " + std::to_string(n_ptrs));
  rc = check_addresses(ptrs, n_ptrs, who, "parameter");
  if (rc != SGRL_OK) return rc;
  const void* fn = stacks == 1 ? reinterpret_cast<const void*>(pick_kernel(p.maxch, p.bk)) : reinterpret_cast<const void*>(pick_critic(p.maxch, p.bk));
  rc = raise_lds(fn, p.lds, who);
  if (rc != SGRL_OK) return rc;
  if (p.total * stacks != s->packed_floats) {
    rc = grow(&s->packed, &s->packed_floats, p.total * stacks, false, &s->generation, who, "packed weights");
    if (rc != SGRL_OK) return rc;
  }
  s->plan = p;
  for (int k = 0; k < stacks; k++)
    for (int l = 0; l < p.n_layers; l++) {
      s->w[k][l] = static_cast<const float*>(ptrs[2 * (k * p.n_layers + l)]);
      s->b[k][l] = static_cast<const float*>(ptrs[2 * (k * p.n_layers + l) + 1]);
    }
  s->kernel = fn;
  s->grads_bound = false;  // the gradient addresses follow the parameter bind: bind them again
  s->kind = stacks == 2 ? SGRL_MLP_KIND_CRITIC : SGRL_MLP_KIND_ACTOR;
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
  put_tile_plan(p, info);
  *total = p.total;
  return SGRL_OK;
}

int sgrl_mlp_chain_plan(const int32_t* actor_dims, int n_a, const int32_t* critic_dims, int n_c, int32_t* info) {
  if (!info) return mfail(SGRL_ERR_ARG, "sgrl_mlp_chain_plan: null argument");
  Plan pa, pc;
  const int rc = make_pair_plans(actor_dims, n_a, critic_dims, n_c, &pa, &pc, "sgrl_mlp_chain_plan");
  if (rc != SGRL_OK) return rc;
  put_tile_plan(make_chain_plan(pa, pc), info);
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
  if (s->kind == SGRL_MLP_KIND_NONE) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: parameters not set (sgrl_mlp_set_params / sgrl_mlp_set_critic_params)");
  int64_t n = 0;
  const int in_dim = s->plan.dims[0], out_dim = s->plan.dims[s->plan.n_layers];
  for (int k = 0; k < n_morph; k++) {
    if (morph_count[k] < 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: negative morph_count");
    if (s->kind == SGRL_MLP_KIND_CRITIC) {
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
  if (s->kind == SGRL_MLP_KIND_CRITIC) return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: the handle is not bound as an actor");
  if (s->kind == SGRL_MLP_KIND_NONE || s->n_env <= 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: parameters or batch structure not set");
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
  return launched("MLP forward");
}

int sgrl_mlp_critic_forward(sgrl_mlp* s, const float* obs, int obs_ld, const float* act, int act_ld, float* q1, float* q2, void* stream) {
  if (!s || !obs || !act || !q1) return mfail(SGRL_ERR_ARG, "sgrl_mlp_critic_forward: null argument");
  if (s->kind != SGRL_MLP_KIND_CRITIC) return mfail(SGRL_ERR_ARG, "sgrl_mlp_critic_forward: the handle is not bound as a critic");
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
  return launched("MLP critic forward");
}

int sgrl_mlp_td_target(sgrl_mlp* actor_t, sgrl_mlp* critic_t, const float* next_obs, int obs_ld, const float* noise, int noise_ld,
                       const float* reward, const float* done, float max_action, float noise_clip, float discount, float* target_q,
                       float* action_out, int action_ld, void* stream) {
  if (!actor_t || !critic_t || !next_obs || !noise || !reward || !done || !target_q) return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: null argument");
  const char* who = "sgrl_mlp_td_target";
  int rc = check_pair(actor_t, critic_t, who);
  if (rc != SGRL_OK) return rc;
  const Plan& pa = actor_t->plan;
  const Plan& pc = critic_t->plan;
  const int in_dim = pa.dims[0], out_dim = pa.dims[pa.n_layers], n_env = actor_t->n_env;
  if (obs_ld < in_dim || noise_ld < out_dim || (action_out && action_ld < out_dim))
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_td_target: obs_ld, noise_ld or action_ld below the network's width (rows too narrow for the network)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TilePlan c = make_chain_plan(pa, pc);
  chain_fn fn = pick_chain(c.maxch, c.bk);
  rc = raise_lds(reinterpret_cast<const void*>(fn), c.lds, who);
  if (rc != SGRL_OK) return rc;
  if (!action_out && (int64_t)n_env * out_dim > critic_t->ws_floats) {
    rc = grow(&critic_t->ws, &critic_t->ws_floats, (int64_t)n_env * out_dim, is_capturing(st), &critic_t->generation, who, "chain workspace");
    if (rc != SGRL_OK) return rc;
  }
  rc = pack_if_needed(actor_t, st);
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
  return launched("MLP target chain");
}

}  // extern "C"
