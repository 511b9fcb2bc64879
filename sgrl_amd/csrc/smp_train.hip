// smp_train.hip -- what lies between the linear layers of the SMP networks' differentiable passes, for gfx950 (C ABI:
// include/sgrl_train.h; Python: train_ops.smp_gather / smp_up_tail / normalize_rows; user: smp_policy `train_kernels`).
//
// Three kernel pairs, each one launch forward and one backward, float32, on the caller's stream, without atomics or scratch:
//   k_smp_gather_*   the message gather of one tree level: [ own' | 32-column segments of ONE source tensor ] (+ tanh)
//   k_smp_up_tail_*  tanh -> fc3 (64 -> 32) -> row normalisation, the tail of smp_policy._up_message
//   k_row_norm_*     F.normalize over rows of up to 256 columns (the msg_base output)
// Rows are independent.  Gather and normalisation give a row to one wavefront: every lane loads its (up to four) elements before
// anything is computed, the row's sum of squares is a butterfly over the 64 lanes (one fixed order), and every output element is
// stored exactly once by the lane that owns it -- the same input gives the same bits.  The backward of the gather writes ALL of the
// source's gradient: a (source node, 32-column group) has at most one reader, found through the inverse of the level's table, and
// a group nobody read receives zeros.  The tables are tiny (16 limbs x 8 slots) and travel BY VALUE in the kernel arguments: the
// host sees them (and refuses an entry outside its source before anything is launched) and no call copies anything to the device.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sgrl.h"
#include "../../include/sgrl_smp.h"
#include "../../include/sgrl_train.h"
#include "train_internal.h"

namespace {

using sgrl_train_detail::fail;
using sgrl_train_detail::launched;

constexpr int ML = SGRL_SMP_MAX_LIMBS;        // 16
constexpr int MC = SGRL_SMP_MAX_CHILDREN;     // 8
constexpr int MSG = 32;                       // message width: one segment
constexpr float EPS = 1e-12f;                 // F.normalize's eps
constexpr int RW = 4;                         // rows (wavefronts) per workgroup of the row kernels

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float half_sum(float v) {      // over the 32 lanes of a half wavefront
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

struct GatherTab {
  int8_t node[ML * MC];       // [j * S + s]: row block of src the segment comes from, -1 = zeros
  int8_t grp[ML * MC];        // its column offset / 32
};
struct ReaderTab {
  int16_t reader[ML * MC];    // [node * (Wsrc / 32) + group]: j * S + s of the one segment that read it, -1 = nobody
};

struct GatherArgs {
  const float* own; const float* src; float* out; float* inv;
  int W0, normalize, Wsrc, S, act, n, B;
  GatherTab tab;
};

__global__ __launch_bounds__(64 * RW) void k_smp_gather_fwd(const GatherArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * RW + (threadIdx.x >> 6);
  if (row >= (long long)a.n * a.B) return;
  const int j = (int)(row / a.B), b = (int)(row % a.B);
  const int wseg = MSG * a.S, wout = a.W0 + wseg;
  // loads first: the row's own element and up to four segment elements per lane
  float o = 0.f;
  if (lane < a.W0) o = a.own[row * a.W0 + lane];
  float sv[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int c = lane + 64 * q;
    sv[q] = 0.f;
    if (c < wseg && a.src) {
      const int e = j * a.S + (c >> 5);
      const int nd = a.tab.node[e];
      if (nd >= 0) sv[q] = a.src[((long long)nd * a.B + b) * a.Wsrc + a.tab.grp[e] * MSG + (c & 31)];
    }
  }
  if (a.normalize) {
    const float den = fmaxf(sqrtf(wave_sum(o * o)), EPS);
    o = o / den;
    if (lane == 0) a.inv[row] = 1.0f / den;
  }
  float* orow = a.out + row * wout;
  if (lane < a.W0) orow[lane] = a.act ? tanhf(o) : o;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int c = lane + 64 * q;
    if (c < wseg) orow[a.W0 + c] = a.act ? tanhf(sv[q]) : sv[q];
  }
}

struct GatherBwdArgs {
  const float* d_out; const float* out; const float* own; const float* inv;
  float* d_own; float* d_src;
  int W0, normalize, Wsrc, S, act, n, B, n_src;
  ReaderTab rd;
};

// rows 0 .. rows_own - 1: the gradient of `own`; the rows behind them: the gradient of the source, one row of it per wavefront
__global__ __launch_bounds__(64 * RW) void k_smp_gather_bwd(const GatherBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * RW + (threadIdx.x >> 6);
  const long long rows_own = a.d_own ? (long long)a.n * a.B : 0;
  const long long rows_src = a.d_src ? (long long)a.n_src * a.B : 0;
  const int wout = a.W0 + MSG * a.S;
  if (row < rows_own) {
    float g = 0.f, t = 0.f, x = 0.f, inv = 0.f;
    if (lane < a.W0) {
      g = a.d_out[row * wout + lane];
      if (a.act) t = a.out[row * wout + lane];
      if (a.normalize) x = a.own[row * a.W0 + lane];
    }
    if (a.normalize) inv = a.inv[row];
    if (a.act) g *= 1.0f - t * t;
    if (a.normalize) {
      const float y = x * inv;
      const float dot = wave_sum(g * y);
      // a row shorter than eps was divided by eps: the clamp passes no gradient to the norm (torch: dy / eps)
      g = (inv >= 1.0f / EPS) ? g * inv : (g - y * dot) * inv;
    }
    if (lane < a.W0) a.d_own[row * a.W0 + lane] = g;
  } else if (row - rows_own < rows_src) {
    const long long r = row - rows_own;
    const int ns = (int)(r / a.B), b = (int)(r % a.B);
    const int groups = a.Wsrc / MSG;
    float g[4], t[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int c = lane + 64 * q;
      g[q] = 0.f;
      t[q] = 0.f;
      if (c < a.Wsrc) {
        const int e = a.rd.reader[ns * groups + (c >> 5)];
        if (e >= 0) {
          const long long at = ((long long)(e / a.S) * a.B + b) * wout + a.W0 + MSG * (e % a.S) + (c & 31);
          g[q] = a.d_out[at];
          if (a.act) t[q] = a.out[at];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int c = lane + 64 * q;
      if (c < a.Wsrc) a.d_src[r * a.Wsrc + c] = g[q] * (1.0f - t[q] * t[q]);       // t = 0 without tanh
    }
  }
}

// ---- tail of _up_message -------------------------------------------------------------------------------------------------------
constexpr int UT = 8;            // rows per step: 8 rows x 32 outputs = one workgroup of 256 threads
constexpr int UROWS = 32;        // rows per workgroup (W3 is staged once for them)
constexpr int WP = 65;           // LDS pitch of W3's rows: lanes of one row walk 32 different rows of W3

__global__ __launch_bounds__(256) void k_smp_up_tail_fwd(const float* __restrict__ a, const float* __restrict__ w3, const float* __restrict__ b3,
                                                         float* __restrict__ t_out, float* __restrict__ u, float* __restrict__ inv, int R) {
  __shared__ float ws[32 * WP];
  __shared__ float ts[UT * 64];
  const int tid = threadIdx.x;
  float wreg[8];
#pragma unroll
  for (int i = 0; i < 8; i++) wreg[i] = w3[tid + 256 * i];
  const int o = tid & 31, rr = tid >> 5;
  const float bias = b3[o];
#pragma unroll
  for (int i = 0; i < 8; i++) { const int e = tid + 256 * i; ws[(e >> 6) * WP + (e & 63)] = wreg[i]; }
  const int row0 = blockIdx.x * UROWS;
  for (int step = 0; step < UROWS / UT; step++) {
    const int base = row0 + step * UT;
    if (base >= R) break;                               // uniform over the workgroup
    // 8 rows x 64 inputs: two per thread, loaded before the tanh
    float av[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int e = tid + 256 * i, r = base + (e >> 6);
      av[i] = r < R ? a[(long long)r * 64 + (e & 63)] : 0.f;
    }
    __syncthreads();                                    // the previous step's readers of ts are done (and ws is staged)
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int e = tid + 256 * i, r = base + (e >> 6);
      const float tv = tanhf(av[i]);
      ts[e] = tv;
      if (r < R) t_out[(long long)r * 64 + (e & 63)] = tv;
    }
    __syncthreads();
    float z = bias;
#pragma unroll 16
    for (int k = 0; k < 64; k++) z = fmaf(ws[o * WP + k], ts[rr * 64 + k], z);
    const float den = fmaxf(sqrtf(half_sum(z * z)), EPS);
    const int r = base + rr;
    if (r < R) {
      u[(long long)r * 32 + o] = z / den;
      if (o == 0) inv[r] = 1.0f / den;
    }
  }
}

__global__ __launch_bounds__(256) void k_smp_up_tail_bwd(const float* __restrict__ du, const float* __restrict__ u, const float* __restrict__ inv,
                                                         const float* __restrict__ t, const float* __restrict__ w3, float* __restrict__ dz,
                                                         float* __restrict__ da, int R) {
  __shared__ float ws[32 * 64];       // [o][k]: the second product's lanes walk k
  __shared__ float zs[UT * 32];
  const int tid = threadIdx.x;
  float wreg[8];
#pragma unroll
  for (int i = 0; i < 8; i++) wreg[i] = w3[tid + 256 * i];
#pragma unroll
  for (int i = 0; i < 8; i++) ws[tid + 256 * i] = wreg[i];
  const int o = tid & 31, rr = tid >> 5;
  const int row0 = blockIdx.x * UROWS;
  for (int step = 0; step < UROWS / UT; step++) {
    const int base = row0 + step * UT;
    if (base >= R) break;
    const int r = base + rr;
    float g = 0.f, y = 0.f, iv = 0.f, tv[2];
    if (r < R) { g = du[(long long)r * 32 + o]; y = u[(long long)r * 32 + o]; iv = inv[r]; }
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int e = tid + 256 * i, r2 = base + (e >> 6);
      tv[i] = r2 < R ? t[(long long)r2 * 64 + (e & 63)] : 0.f;
    }
    const float dot = half_sum(g * y);
    const float z = (iv >= 1.0f / EPS) ? g * iv : (g - y * dot) * iv;
    __syncthreads();                                    // the previous step's readers of zs are done (and ws is staged)
    zs[tid] = z;
    if (r < R) dz[(long long)r * 32 + o] = z;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int e = tid + 256 * i, r2 = base + (e >> 6), k = e & 63;
      float s = 0.f;
#pragma unroll 16
      for (int oo = 0; oo < 32; oo++) s = fmaf(zs[(e >> 6) * 32 + oo], ws[oo * 64 + k], s);
      if (r2 < R) da[(long long)r2 * 64 + k] = s * (1.0f - tv[i] * tv[i]);
    }
  }
}

// ---- F.normalize over rows -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * RW) void k_row_norm_fwd(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ inv, int R, int W) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * RW + (threadIdx.x >> 6);
  if (row >= R) return;
  float v[4], ss = 0.f;
#pragma unroll
  for (int q = 0; q < 4; q++) { const int c = lane + 64 * q; v[q] = c < W ? x[row * W + c] : 0.f; }
#pragma unroll
  for (int q = 0; q < 4; q++) ss = fmaf(v[q], v[q], ss);
  const float den = fmaxf(sqrtf(wave_sum(ss)), EPS);
#pragma unroll
  for (int q = 0; q < 4; q++) { const int c = lane + 64 * q; if (c < W) y[row * W + c] = v[q] / den; }
  if (lane == 0) inv[row] = 1.0f / den;
}

__global__ __launch_bounds__(64 * RW) void k_row_norm_bwd(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ inv,
                                                          float* __restrict__ dx, int R, int W) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * RW + (threadIdx.x >> 6);
  if (row >= R) return;
  float g[4], yv[4], dot = 0.f;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int c = lane + 64 * q;
    g[q] = c < W ? dy[row * W + c] : 0.f;
    yv[q] = c < W ? y[row * W + c] : 0.f;
  }
  const float iv = inv[row];
#pragma unroll
  for (int q = 0; q < 4; q++) dot = fmaf(g[q], yv[q], dot);
  dot = wave_sum(dot);
  const bool clamped = iv >= 1.0f / EPS;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int c = lane + 64 * q;
    if (c < W) dx[row * W + c] = clamped ? g[q] * iv : (g[q] - yv[q] * dot) * iv;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
unsigned row_blocks(long long rows) { return (unsigned)((rows + RW - 1) / RW); }

// shapes and tables of a gather call; fills the kernel's copy of the tables (fwd) or their inverse (bwd)
int check_gather(const char* fn, int W0, bool have_src, int n_src, int Wsrc, const int32_t* node, const int32_t* off, int S, int n, int B,
                 GatherTab* tab, ReaderTab* rd) {
  const std::string f(fn);
  if (B <= 0) return fail(SGRL_ERR_ARG, f + ": B <= 0");
  if (n < 1 || n > ML) return fail(SGRL_ERR_ARG, f + ": node count outside 1.." + std::to_string(ML));
  if (S < 1 || S > MC) return fail(SGRL_ERR_ARG, f + ": max_children (segments) outside 1.." + std::to_string(MC));
  if (W0 != 0 && W0 != 32 && W0 != 64) return fail(SGRL_ERR_ARG, f + ": own width must be 0, 32 or 64");
  if (!node || !off) return fail(SGRL_ERR_ARG, f + ": null table");
  if (have_src) {
    if (n_src < 1 || n_src > ML) return fail(SGRL_ERR_ARG, f + ": source node count outside 1.." + std::to_string(ML));
    if (Wsrc < MSG || Wsrc > MSG * MC || Wsrc % MSG) return fail(SGRL_ERR_ARG, f + ": source width must be a multiple of 32 in 32.." + std::to_string(MSG * MC));
  }
  if (rd) for (int i = 0; i < ML * MC; i++) rd->reader[i] = -1;
  for (int e = 0; e < n * S; e++) {
    const int nd = node[e], of = off[e];
    if (nd < -1) return fail(SGRL_ERR_ARG, f + ": table entry " + std::to_string(e) + " names node " + std::to_string(nd));
    if (nd >= 0 && have_src) {
      if (nd >= n_src || of < 0 || of % MSG || of + MSG > Wsrc)
        return fail(SGRL_ERR_ARG, f + ": table entry " + std::to_string(e) + " (node " + std::to_string(nd) + ", column " + std::to_string(of) +
                                      ") lies outside its source");
      if (rd) {
        int16_t& slot = rd->reader[nd * (Wsrc / MSG) + of / MSG];
        if (slot >= 0) return fail(SGRL_ERR_ARG, f + ": two table entries read node " + std::to_string(nd) + ", column " + std::to_string(of));
        slot = (int16_t)e;
      }
    }
    if (tab) {
      tab->node[e] = (int8_t)((nd >= 0 && have_src) ? nd : -1);
      tab->grp[e] = (int8_t)((nd >= 0 && have_src) ? of / MSG : 0);
    }
  }
  return SGRL_OK;
}

}  // namespace

extern "C" {

int sgrl_smp_gather_forward(const float* own, int W0, int normalize, const float* src, int n_src, int Wsrc, const int32_t* node,
                            const int32_t* off, int S, int act_tanh, float* out, float* inv, int n, int B, void* stream) {
  const char* fn = "sgrl_smp_gather_forward";
  GatherArgs a{};
  const int rc = check_gather(fn, W0, src != nullptr, n_src, Wsrc, node, off, S, n, B, &a.tab, nullptr);
  if (rc != SGRL_OK) return rc;
  if (!out || (W0 > 0 && !own) || (W0 > 0 && normalize && !inv)) return fail(SGRL_ERR_ARG, std::string(fn) + ": null pointer");
  a.own = own; a.src = src; a.out = out; a.inv = inv;
  a.W0 = W0; a.normalize = (W0 > 0 && normalize) ? 1 : 0; a.Wsrc = src ? Wsrc : MSG; a.S = S; a.act = act_tanh ? 1 : 0; a.n = n; a.B = B;
  hipLaunchKernelGGL(k_smp_gather_fwd, dim3(row_blocks((long long)n * B)), dim3(64 * RW), 0, (hipStream_t)stream, a);
  { int lrc = SGRL_OK; if (!launched("k_smp_gather_fwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_smp_gather_backward(const float* d_out, const float* out, const float* own, const float* inv, int W0, int normalize, int n_src,
                             int Wsrc, const int32_t* node, const int32_t* off, int S, int act_tanh, float* d_own, float* d_src, int n,
                             int B, void* stream) {
  const char* fn = "sgrl_smp_gather_backward";
  GatherBwdArgs a{};
  const int rc = check_gather(fn, W0, d_src != nullptr, n_src, Wsrc, node, off, S, n, B, nullptr, &a.rd);
  if (rc != SGRL_OK) return rc;
  const bool norm = W0 > 0 && normalize && d_own;
  if (!d_out || (!d_own && !d_src) || (d_own && W0 == 0) || (act_tanh && !out) || (norm && (!own || !inv)))
    return fail(SGRL_ERR_ARG, std::string(fn) + ": null pointer (or a gradient of `own` asked for without an own part)");
  a.d_out = d_out; a.out = out; a.own = own; a.inv = inv; a.d_own = d_own; a.d_src = d_src;
  a.W0 = W0; a.normalize = norm ? 1 : 0; a.Wsrc = d_src ? Wsrc : MSG; a.S = S; a.act = act_tanh ? 1 : 0; a.n = n; a.B = B;
  a.n_src = d_src ? n_src : 0;
  const long long rows = (d_own ? (long long)n * B : 0) + (d_src ? (long long)n_src * B : 0);
  hipLaunchKernelGGL(k_smp_gather_bwd, dim3(row_blocks(rows)), dim3(64 * RW), 0, (hipStream_t)stream, a);
  { int lrc = SGRL_OK; if (!launched("k_smp_gather_bwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_smp_up_tail_forward(const float* a, const float* w3, const float* b3, float* t, float* u, float* inv, int R, void* stream) {
  if (!a || !w3 || !b3 || !t || !u || !inv || R <= 0) return fail(SGRL_ERR_ARG, "sgrl_smp_up_tail_forward: bad argument (null pointer or R <= 0)");
  hipLaunchKernelGGL(k_smp_up_tail_fwd, dim3((R + UROWS - 1) / UROWS), dim3(256), 0, (hipStream_t)stream, a, w3, b3, t, u, inv, R);
  { int lrc = SGRL_OK; if (!launched("k_smp_up_tail_fwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_smp_up_tail_backward(const float* du, const float* u, const float* inv, const float* t, const float* w3, float* dz, float* da, int R,
                              void* stream) {
  if (!du || !u || !inv || !t || !w3 || !dz || !da || R <= 0)
    return fail(SGRL_ERR_ARG, "sgrl_smp_up_tail_backward: bad argument (null pointer or R <= 0)");
  hipLaunchKernelGGL(k_smp_up_tail_bwd, dim3((R + UROWS - 1) / UROWS), dim3(256), 0, (hipStream_t)stream, du, u, inv, t, w3, dz, da, R);
  { int lrc = SGRL_OK; if (!launched("k_smp_up_tail_bwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_row_normalize_forward(const float* x, float* y, float* inv, int R, int W, void* stream) {
  if (!x || !y || !inv || R <= 0) return fail(SGRL_ERR_ARG, "sgrl_row_normalize_forward: bad argument (null pointer or R <= 0)");
  if (W < 1 || W > MSG * MC) return fail(SGRL_ERR_ARG, "sgrl_row_normalize_forward: width outside 1.." + std::to_string(MSG * MC));
  hipLaunchKernelGGL(k_row_norm_fwd, dim3(row_blocks(R)), dim3(64 * RW), 0, (hipStream_t)stream, x, y, inv, R, W);
  { int lrc = SGRL_OK; if (!launched("k_row_norm_fwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

int sgrl_row_normalize_backward(const float* dy, const float* y, const float* inv, float* dx, int R, int W, void* stream) {
  if (!dy || !y || !inv || !dx || R <= 0) return fail(SGRL_ERR_ARG, "sgrl_row_normalize_backward: bad argument (null pointer or R <= 0)");
  if (W < 1 || W > MSG * MC) return fail(SGRL_ERR_ARG, "sgrl_row_normalize_backward: width outside 1.." + std::to_string(MSG * MC));
  hipLaunchKernelGGL(k_row_norm_bwd, dim3(row_blocks(R)), dim3(64 * RW), 0, (hipStream_t)stream, dy, y, inv, dx, R, W);
  { int lrc = SGRL_OK; if (!launched("k_row_norm_bwd launch failed", &lrc)) return lrc; }
  return SGRL_OK;
}

}  // extern "C"
