// mlp_optim.hip -- the optimizer half of the MLP agent's TD3 update (C ABI: include/sgrl_mlp.h, "optimizer half"): gradient
// clipping, Adam and, at policy iterations, the soft update of the target network, for ONE handle (an actor: 1 stack, a critic: 2
// stacks) in TWO launches.  Replaces clip_grad_norm_ + Adam.step (reference src/agent.py:161-164, 174-177) and the Polyak loop of
// the same network (common/functional.py:7-10).  The formula is k_opt_adam / k_opt_lerp of train_gemm.hip term for term; what is new
// is the shape: the handle already holds the addresses of its six to twenty tensors (parameter bind, gradient bind, and the state
// bind below), so they travel in the kernels' argument block -- no device table, no allocation, no upload -- and the total of the
// squared gradients is re-added by every workgroup of the second launch instead of by a launch of its own.
//
// The bound tensors are cut into chunks of kChunk = 1024 elements (a tensor's last chunk may be short; chunks never span tensors),
// one workgroup of 256 threads per chunk; thread t owns elements 4 t .. 4 t + 3 of its chunk -- as ONE 16-byte access where the
// tensors' addresses are 16-byte aligned and all four elements exist (chunk starts are multiples of 1024 elements), as up to four
// scalar accesses otherwise.  Both forms run the same arithmetic in the same order: the bits do not depend on the alignment.
//
//   k_mlp_opt_norm    partial[c] = sum of g^2 over chunk c;  workgroup 0 also advances every bound step counter by 1.
//                     With max_norm == 0 the squares are skipped (one workgroup, the counters only).
//   k_mlp_opt_apply   total = sum of all partials (every workgroup, itself); coef = min(1, max_norm / (sqrt(total) + 1e-6)),
//                     NaN for a NaN total; g *= coef (written back, as clip_grad_norm_ does); Adam; target = target (1 - tau) + tau p with the p just written.
//
// ORDER OF THE SUM (fixed, so a step is bit-repeatable; no atomics).  A thread adds its four squares in element order (4 additions
// from 0); a wave adds its 64 lanes by a butterfly (xor 32, 16, 8, 4, 2, 1: 6 additions); the four waves' sums are added in wave
// order ((w0 + w1) + w2) + w3 (3 additions): a partial is 13 additions deep.  In the apply launch thread t adds partials t, t + 256,
// t + 512, ... serially (ceil(chunks / 256) additions from 0), then the same butterfly and the same four-wave sum (9 additions).
// The longest chain of float additions from any g^2 to `total` is therefore 22 + ceil(chunks / 256): 24 for the [256, 256] nets,
// 28 at ~1 500 partials, and at most 22 + 41 = 63 <= 128 for the largest handle the plan admits (two stacks of five 1024-wide layers,
// 10 250 chunks).
//
// The plan, the handle and the host helpers of the family (stack count, address checks, launch check) come from mlp_internal.h.
#include "mlp_internal.h"

#include <cmath>

using namespace sgrl_mlp_detail;

namespace {

constexpr int kChunk = 1024;
constexpr int kMaxT = 4 * NL;           // tensors of a handle: weight and bias of every layer of up to two stacks

struct OptArgs {                        // by value in the argument block of both launches (~1.2 KB)
  float* p[kMaxT];
  float* g[kMaxT];
  float* m[kMaxT];
  float* v[kMaxT];
  float* tgt[kMaxT];
  float* step[kMaxT];
  long long n[kMaxT];                   // elements of tensor i
  int chunk0[kMaxT + 1];                // first chunk of tensor i; chunk0[n_tensors] = chunks of the handle
  int n_tensors, n_steps;
  float* partial;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the sum over the workgroup's 256 threads, in every thread: butterfly per wave, then the four waves in order
__device__ __forceinline__ float group_sum(float s, float* red) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ int tensor_of(const OptArgs& a, int chunk) {
  int t = 0;
  while (t + 1 < a.n_tensors && a.chunk0[t + 1] <= chunk) t++;
  return t;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ __launch_bounds__(256) void k_mlp_opt_norm(OptArgs a, int squares) {
  __shared__ float red[4];
  if (blockIdx.x == 0 && (int)threadIdx.x < a.n_steps) *a.step[threadIdx.x] += 1.0f;
  if (!squares) return;
  const int t = tensor_of(a, blockIdx.x);
  const long long first = (long long)(blockIdx.x - a.chunk0[t]) * kChunk + 4 * threadIdx.x;
  const long long left = a.n[t] - first;                      // elements of the tensor from this thread's first one on
  const float* __restrict__ g = a.g[t] + first;
  float s = 0.f;
  if (left >= 4 && aligned16(a.g[t])) {
    const float4 x = *reinterpret_cast<const float4*>(g);
    s += x.x * x.x; s += x.y * x.y; s += x.z * x.z; s += x.w * x.w;
  } else {
    for (int k = 0; k < 4; k++)
      if (k < left) s += g[k] * g[k];
  }
  s = group_sum(s, red);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
}

struct AdamConst { double b1, b2, eps; float coef, step_size, bc2_sqrt, tau, keep; };

// one element: k_opt_adam's lines, then k_opt_lerp's on the parameter just computed
template <bool CLIP, bool LERP>
__device__ __forceinline__ void opt_one(const AdamConst& c, float& p, float& g, float& m, float& v, float& tg) {
  if (CLIP) g *= c.coef;
  m = (float)(c.b1 * (double)m + (1.0 - c.b1) * (double)g);
  v = (float)(c.b2 * (double)v + (1.0 - c.b2) * (double)g * (double)g);
  const float denom = (float)((double)(sqrtf(v) / c.bc2_sqrt) + c.eps);
  p -= c.step_size * m / denom;
  if (LERP) tg = tg * c.keep + c.tau * p;
}

template <bool CLIP, bool LERP>
__global__ __launch_bounds__(256) void k_mlp_opt_apply(OptArgs a, int n_chunks, double lr, double b1, double b2, double eps, float max_norm,
                                                       float tau) {
  __shared__ float red[4];
  AdamConst c;
  c.b1 = b1; c.b2 = b2; c.eps = eps; c.tau = tau; c.keep = 1.0f - tau; c.coef = 1.0f;
  if (CLIP) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n_chunks; i += 256) s += a.partial[i];
    const float total = group_sum(s, red);
    // a select, not fminf: a NaN total gives a NaN coef, as torch.clamp(coef, max=1.0) does in clip_grad_norm_ (k_opt_adam)
    const float ratio = max_norm / (sqrtf(total) + 1e-6f);
    c.coef = ratio > 1.0f ? 1.0f : ratio;
  }
  const double t = (double)*a.step[0];                        // already advanced by k_mlp_opt_norm
  const float bc1 = (float)(1.0 - pow(b1, t));
  c.bc2_sqrt = sqrtf((float)(1.0 - pow(b2, t)));
  c.step_size = (float)(lr / (double)bc1);
  const int ti = tensor_of(a, blockIdx.x);
  const long long first = (long long)(blockIdx.x - a.chunk0[ti]) * kChunk + 4 * threadIdx.x;
  const long long left = a.n[ti] - first;
  if (left <= 0) return;
  float* __restrict__ p = a.p[ti] + first;
  float* __restrict__ g = a.g[ti] + first;
  float* __restrict__ m = a.m[ti] + first;
  float* __restrict__ v = a.v[ti] + first;
  float* __restrict__ tg = LERP ? a.tgt[ti] + first : nullptr;
  const bool vec = left >= 4 && aligned16(a.p[ti]) && aligned16(a.g[ti]) && aligned16(a.m[ti]) && aligned16(a.v[ti]) &&
                   (!LERP || aligned16(a.tgt[ti]));
  if (vec) {
    float4 P = *reinterpret_cast<float4*>(p), G = *reinterpret_cast<float4*>(g), M = *reinterpret_cast<float4*>(m),
           V = *reinterpret_cast<float4*>(v), T = make_float4(0.f, 0.f, 0.f, 0.f);
    if (LERP) T = *reinterpret_cast<float4*>(tg);
    opt_one<CLIP, LERP>(c, P.x, G.x, M.x, V.x, T.x);
    opt_one<CLIP, LERP>(c, P.y, G.y, M.y, V.y, T.y);
    opt_one<CLIP, LERP>(c, P.z, G.z, M.z, V.z, T.z);
    opt_one<CLIP, LERP>(c, P.w, G.w, M.w, V.w, T.w);
    if (CLIP) *reinterpret_cast<float4*>(g) = G;
    *reinterpret_cast<float4*>(m) = M;
    *reinterpret_cast<float4*>(v) = V;
    *reinterpret_cast<float4*>(p) = P;
    if (LERP) *reinterpret_cast<float4*>(tg) = T;
  } else {
    for (int k = 0; k < 4; k++)
      if (k < left) {
        float P = p[k], G = g[k], M = m[k], V = v[k], T = LERP ? tg[k] : 0.f;
        opt_one<CLIP, LERP>(c, P, G, M, V, T);
        if (CLIP) g[k] = G;
        m[k] = M; v[k] = V; p[k] = P;
        if (LERP) tg[k] = T;
      }
  }
}

struct Cut { int tensors = 0; long long elements = 0; int chunks = 0; long long n[kMaxT] = {0}; int chunk0[kMaxT + 1] = {0}; };

// tensors in the order of the parameter bind: per stack W0 [dims[1], dims[0]], b0 [dims[1]], W1, b1, ...
Cut make_cut(const Plan& p, int stacks) {
  Cut c;
  for (int k = 0; k < stacks; k++)
    for (int l = 0; l < p.n_layers; l++)
      for (int wb = 0; wb < 2; wb++) {
        const long long n = wb == 0 ? (long long)p.dims[l + 1] * p.dims[l] : (long long)p.dims[l + 1];
        c.n[c.tensors] = n;
        c.chunk0[c.tensors] = c.chunks;
        c.chunks += (int)((n + kChunk - 1) / kChunk);
        c.elements += n;
        c.tensors++;
      }
  c.chunk0[c.tensors] = c.chunks;
  return c;
}

}  // namespace

extern "C" {

int sgrl_mlp_optim_step_launches(void) { return 2; }

int sgrl_mlp_optim_plan(const int32_t* dims, int n_dims, int n_stacks, int64_t* info) {
  const char* who = "sgrl_mlp_optim_plan";
  if (!info) return mfail(SGRL_ERR_ARG, std::string(who) + ": null argument");
  Plan p;
  const int rc = make_plan(dims, n_dims, &p, who);
  if (rc != SGRL_OK) return rc;
  if (n_stacks != 1 && n_stacks != 2) return mfail(SGRL_ERR_ARG, std::string(who) + ": n_stacks must be 1 (an actor) or 2 (a critic), got " + std::to_string(n_stacks));
  if (n_stacks == 2 && p.dims[p.n_layers] != 1)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": a critic's last width must be 1, got " + std::to_string(p.dims[p.n_layers]));
  const Cut c = make_cut(p, n_stacks);
  info[0] = c.tensors; info[1] = c.elements; info[2] = c.chunks; info[3] = kChunk;
  return SGRL_OK;
}

int sgrl_mlp_bind_optim(sgrl_mlp* s, const void* const* exp_avg, const void* const* exp_avg_sq, int n, const void* const* steps, int n_steps,
                        const void* const* target, int n_target, float* partials, int64_t partial_floats) {
  const char* who = "sgrl_mlp_bind_optim";
  if (!s || !exp_avg || !exp_avg_sq || !steps || !partials) return mfail(SGRL_ERR_ARG, std::string(who) + ": null argument");
  if (s->kind == SGRL_MLP_KIND_NONE) return mfail(SGRL_ERR_ARG, std::string(who) + ": parameters not set (sgrl_mlp_set_params / sgrl_mlp_set_critic_params)");
  if (!s->grads_bound) return mfail(SGRL_ERR_ARG, std::string(who) + ": gradients not bound (sgrl_mlp_bind_grads)");
  const Cut c = make_cut(s->plan, n_stacks(s));
  if (n != c.tensors) return mfail(SGRL_ERR_ARG, std::string(who) + ": expected " + std::to_string(c.tensors) + " state addresses, got " + std::to_string(n));
  if (n_steps < 1 || n_steps > c.tensors)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": expected 1 .. " + std::to_string(c.tensors) + " step counters, got " + std::to_string(n_steps));
  if (n_target != 0 && n_target != n)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": expected 0 or " + std::to_string(n) + " target addresses, got " + std::to_string(n_target));
  if (n_target && !target) return mfail(SGRL_ERR_ARG, std::string(who) + ": null argument");
  if (partial_floats < c.chunks)
    return mfail(SGRL_ERR_ARG, std::string(who) + ": the partials buffer holds " + std::to_string(partial_floats) + " floats, the handle has " +
                                   std::to_string(c.chunks) + " chunks");
  if (reinterpret_cast<uintptr_t>(partials) & 3) return mfail(SGRL_ERR_ARG, std::string(who) + ": the partials buffer is not 4-byte aligned");
  int rc = check_addresses(exp_avg, n, who, "state or target address");
  if (rc == SGRL_OK) rc = check_addresses(exp_avg_sq, n, who, "state or target address");
  if (rc == SGRL_OK && n_target) rc = check_addresses(target, n, who, "state or target address");
  if (rc == SGRL_OK) rc = check_addresses(steps, n_steps, who, "step counter");
  if (rc != SGRL_OK) return rc;
  for (int i = 0; i < n; i++) {
    s->opt_m[i] = static_cast<float*>(const_cast<void*>(exp_avg[i]));
    s->opt_v[i] = static_cast<float*>(const_cast<void*>(exp_avg_sq[i]));
    s->opt_target[i] = n_target ? static_cast<float*>(const_cast<void*>(target[i])) : nullptr;
  }
  for (int i = 0; i < n_steps; i++) s->opt_step[i] = static_cast<float*>(const_cast<void*>(steps[i]));
  s->opt_n_steps = n_steps;
  s->opt_has_target = n_target != 0;
  s->opt_partial = partials;
  s->grads_bound = SGRL_MLP_BOUND_GRADS_AND_STATE;
  return SGRL_OK;
}

int sgrl_mlp_optim_bound(const sgrl_mlp* s) { return s && s->grads_bound == SGRL_MLP_BOUND_GRADS_AND_STATE ? 1 : 0; }

int sgrl_mlp_optim_step(sgrl_mlp* s, double lr, double beta1, double beta2, double eps, float max_norm, float tau, void* stream) {
  const char* who = "sgrl_mlp_optim_step";
  if (!s) return mfail(SGRL_ERR_ARG, std::string(who) + ": null handle");
  if (s->kind == SGRL_MLP_KIND_NONE) return mfail(SGRL_ERR_ARG, std::string(who) + ": parameters not set");
  if (!s->grads_bound) return mfail(SGRL_ERR_ARG, std::string(who) + ": gradients not bound (sgrl_mlp_bind_grads)");
  if (s->grads_bound != SGRL_MLP_BOUND_GRADS_AND_STATE) return mfail(SGRL_ERR_ARG, std::string(who) + ": optimizer state not bound (sgrl_mlp_bind_optim)");
  if (!std::isfinite(lr) || !std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps) || !std::isfinite(max_norm) || !std::isfinite(tau))
    return mfail(SGRL_ERR_ARG, std::string(who) + ": a hyper-parameter is not finite");
  if (max_norm < 0.f) return mfail(SGRL_ERR_ARG, std::string(who) + ": max_norm is negative");
  if (tau < 0.f || tau > 1.f) return mfail(SGRL_ERR_ARG, std::string(who) + ": tau outside [0, 1]");
  if (tau > 0.f && !s->opt_has_target) return mfail(SGRL_ERR_ARG, std::string(who) + ": tau > 0 with no target bound");
  const int nl = s->plan.n_layers;
  const Cut c = make_cut(s->plan, n_stacks(s));
  OptArgs a;
  for (int i = 0; i < kMaxT; i++) {
    const bool on = i < c.tensors;
    const int k = i / (2 * nl), l = (i % (2 * nl)) / 2;
    const bool w = (i & 1) == 0;
    a.p[i] = on ? const_cast<float*>(w ? s->w[k][l] : s->b[k][l]) : nullptr;
    a.g[i] = on ? (w ? s->gw[k][l] : s->gb[k][l]) : nullptr;
    a.m[i] = on ? s->opt_m[i] : nullptr;
    a.v[i] = on ? s->opt_v[i] : nullptr;
    a.tgt[i] = on ? s->opt_target[i] : nullptr;
    a.step[i] = i < s->opt_n_steps ? s->opt_step[i] : nullptr;
    a.n[i] = on ? c.n[i] : 0;
  }
  for (int i = 0; i <= kMaxT; i++) a.chunk0[i] = i <= c.tensors ? c.chunk0[i] : c.chunks;
  a.n_tensors = c.tensors;
  a.n_steps = s->opt_n_steps;
  a.partial = s->opt_partial;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool clip = max_norm > 0.f, lerp = tau > 0.f;
  hipLaunchKernelGGL(k_mlp_opt_norm, dim3(clip ? c.chunks : 1), dim3(256), 0, st, a, clip ? 1 : 0);
  int rc = launched("k_mlp_opt_norm");
  if (rc != SGRL_OK) return rc;
  auto fn = clip ? (lerp ? k_mlp_opt_apply<true, true> : k_mlp_opt_apply<true, false>)
                 : (lerp ? k_mlp_opt_apply<false, true> : k_mlp_opt_apply<false, false>);
  hipLaunchKernelGGL(fn, dim3(c.chunks), dim3(256), 0, st, a, c.chunks, lr, beta1, beta2, eps, max_norm, tau);
  return launched("k_mlp_opt_apply");
}

}  // extern "C"
