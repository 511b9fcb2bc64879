// mlp_actor.hip -- the monolithic MLP actor's forward for a whole batch of environments in ONE launch (C ABI: include/sgrl_mlp.h).
//
//   k_mlp_pack      live nn.Linear weights / biases -> the padded packed buffer (kpad, npad of sgrl_mlp_plan; zeros in the padding);
//                   at the top of a forward unless the caller holds the weights
//   k_mlp_forward   one workgroup (4 waves) per 32 environment rows.  The observation tile goes into the LDS activation tile
//                   X[32][sx]; every layer computes its whole output row block into registers -- exact-f32 32x32x2 matrix
//                   instructions, the weights streamed through a double-buffered LDS panel of 256 output columns x BK k values --
//                   and, once the last panel has been consumed, writes relu(. + bias) back over X in place: the hidden
//                   activations never leave the chip.  The last layer's epilogue writes max_action * tanh(. + bias) to the action
//                   rows and exact zeros up to the caller's leading dimension.
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

#include "../../include/sgrl.h"
#include "../../include/sgrl_mlp.h"

namespace {

thread_local std::string g_mlp_err;
int mfail(int code, const std::string& msg) { g_mlp_err = msg; return code; }

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NL = SGRL_MLP_MAX_LAYERS;
constexpr int BM = SGRL_MLP_TILE_ROWS;
constexpr int CH = 256;                 // output columns per chunk = rows of a weight panel
constexpr int LDS_LIMIT = 160 * 1024;

struct Plan {
  int n_layers = 0;
  int dims[NL + 1] = {0};
  int kpad[NL] = {0}, npad[NL] = {0};
  int64_t w_off[NL] = {0}, b_off[NL] = {0};
  int64_t total = 0;
  int maxch = 1, bk = 16, lds = 0, sx = 0;
};

int round_up(int x, int m) { return (x + m - 1) / m * m; }

int make_plan(const int32_t* dims, int n_dims, Plan* p, const char* who) {
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

struct PackArgs {
  const float* w[NL];
  const float* b[NL];
  int n[NL], k[NL], npad[NL], kpad[NL];
  long long w_off[NL], b_off[NL];
  int n_layers;
  long long total;
  float* dst;
};

__global__ __launch_bounds__(256) void k_mlp_pack(PackArgs a) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
    float v = 0.f;
    if (i >= a.b_off[0]) {
#pragma unroll
      for (int l = 0; l < NL; l++)
        if (l < a.n_layers && i >= a.b_off[l] && i < a.b_off[l] + a.npad[l]) {
          const int n = (int)(i - a.b_off[l]);
          if (n < a.n[l]) v = a.b[l][n];
        }
    } else {
#pragma unroll
      for (int l = 0; l < NL; l++)
        if (l < a.n_layers && i >= a.w_off[l] && i < a.w_off[l] + (long long)a.npad[l] * a.kpad[l]) {
          const long long r = i - a.w_off[l];
          const int n = (int)(r / a.kpad[l]), k = (int)(r - (long long)n * a.kpad[l]);
          if (n < a.n[l] && k < a.k[l]) v = a.w[l][(size_t)n * a.k[l] + k];
        }
    }
    a.dst[i] = v;
  }
}

struct FwdArgs {
  const float* obs; int obs_ld;
  float* act; int act_ld;
  const float* wp;                 // packed buffer
  int n_env, in_dim, out_dim, n_layers, sx;
  int kpad[NL], npad[NL];
  long long w_off[NL], b_off[NL];
  float max_action;
};

template <int MAXCH, int BK>
__global__ __launch_bounds__(256) void k_mlp_forward(FwdArgs a) {
  constexpr int SK = BK + 4;                   // panel row stride
  constexpr int QPR = BK / 4;                  // float4 per panel row
  constexpr int RPP = 256 / QPR;               // panel rows covered per staging pass
  constexpr int NP = CH / RPP;                 // staging passes per panel
  constexpr int KH = BK / 2;                   // k values per lane half
  constexpr int NQ = KH / 4;                   // float4 per lane per operand row per k block
  extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
  float* X = mlp_lds;                          // [BM][sx]
  float* Ws = mlp_lds + BM * a.sx;             // [2][CH][SK]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
  const int row0 = blockIdx.x * BM;
  const int sx = a.sx;
  {  // observation tile (rows beyond n_env and columns beyond the input width: zeros)
    const int k0 = a.kpad[0];
    for (int r = wave; r < BM; r += 4) {
      const int row = row0 + r;
      for (int k = lane; k < k0; k += 64)
        X[r * sx + k] = (row < a.n_env && k < a.in_dim) ? a.obs[(size_t)row * a.obs_ld + k] : 0.f;
    }
  }
  __syncthreads();
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
        } else if (n < a.out_dim) {
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const int row = row0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (row < a.n_env) a.act[(size_t)row * a.act_ld + n] = a.max_action * tanhf(acc[c][j][e] + bvv);
          }
        }
      }
    __syncthreads();
  }
  // slots beyond the output width, up to the caller's leading dimension: exact zeros
  for (int r = wave; r < BM; r += 4) {
    const int row = row0 + r;
    if (row >= a.n_env) break;
    for (int n = a.out_dim + lane; n < a.act_ld; n += 64) a.act[(size_t)row * a.act_ld + n] = 0.f;
  }
}

typedef void (*fwd_fn)(FwdArgs);
fwd_fn pick_kernel(int maxch, int bk) {
  if (bk == 16) return maxch == 1 ? k_mlp_forward<1, 16> : (maxch == 2 ? k_mlp_forward<2, 16> : k_mlp_forward<4, 16>);
  return maxch == 1 ? k_mlp_forward<1, 8> : (maxch == 2 ? k_mlp_forward<2, 8> : k_mlp_forward<4, 8>);
}

}  // namespace

struct sgrl_mlp {
  Plan plan;
  bool bound = false;
  const float* w[NL] = {nullptr};
  const float* b[NL] = {nullptr};
  float* packed = nullptr;
  int64_t packed_floats = 0;
  bool hold = false, dirty = true;
  int n_env = 0;
  int64_t generation = 0;
  fwd_fn kernel = nullptr;
};

extern "C" {

const char* sgrl_mlp_last_error(void) { return g_mlp_err.c_str(); }
int sgrl_mlp_forward_launches(void) { return 1; }
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

int sgrl_mlp_create(sgrl_mlp** out) {
  if (!out) return mfail(SGRL_ERR_ARG, "out is null");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return mfail(SGRL_ERR_HIP, "no HIP device visible: the MLP actor forward needs an MI355X (there is no CPU fallback)");
  *out = new sgrl_mlp();
  return SGRL_OK;
}

void sgrl_mlp_destroy(sgrl_mlp* s) {
  if (!s) return;
  if (s->packed) (void)hipFree(s->packed);
  delete s;
}

int sgrl_mlp_set_params(sgrl_mlp* s, const void* const* ptrs, int n_ptrs, const int32_t* dims, int n_dims) {
  if (!s || !ptrs) return mfail(SGRL_ERR_ARG, "sgrl_mlp_set_params: null argument");
  Plan p;
  const int rc = make_plan(dims, n_dims, &p, "sgrl_mlp_set_params");
  if (rc != SGRL_OK) return rc;
  if (n_ptrs != 2 * p.n_layers)
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_set_params: expected " + std::to_string(2 * p.n_layers) + " parameter addresses, got " + std::to_string(n_ptrs));
  for (int i = 0; i < n_ptrs; i++)
    if (!ptrs[i] || (reinterpret_cast<uintptr_t>(ptrs[i]) & 3))
      return mfail(SGRL_ERR_ARG, "sgrl_mlp_set_params: parameter " + std::to_string(i) + " is null or not 4-byte aligned");
  fwd_fn fn = pick_kernel(p.maxch, p.bk);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, p.lds) != hipSuccess)
    return mfail(SGRL_ERR_HIP, "sgrl_mlp_set_params: cannot raise the kernel's dynamic LDS limit");
  if (p.total != s->packed_floats) {
    float* buf = nullptr;
    if (hipMalloc(&buf, sizeof(float) * (size_t)p.total) != hipSuccess) return mfail(SGRL_ERR_HIP, "device allocation failed (MLP packed weights)");
    if (s->packed) {
      (void)hipDeviceSynchronize();       // a forward in flight may still read the old buffer
      (void)hipFree(s->packed);
      s->generation++;
    }
    s->packed = buf;
    s->packed_floats = p.total;
  }
  s->plan = p;
  for (int l = 0; l < p.n_layers; l++) {
    s->w[l] = static_cast<const float*>(ptrs[2 * l]);
    s->b[l] = static_cast<const float*>(ptrs[2 * l + 1]);
  }
  s->kernel = fn;
  s->bound = true;
  s->dirty = true;
  s->n_env = 0;           // the batch structure is checked against the widths: configure again
  return SGRL_OK;
}

int sgrl_mlp_hold_weights(sgrl_mlp* s, int hold) {
  if (!s) return mfail(SGRL_ERR_ARG, "sgrl_mlp_hold_weights: null handle");
  s->hold = hold != 0;
  s->dirty = true;
  return SGRL_OK;
}

int sgrl_mlp_configure(sgrl_mlp* s, int n_morph, const int32_t* morph_L, const int32_t* morph_count, int feature, int out) {
  if (!s || n_morph <= 0 || !morph_L || !morph_count || feature < 1 || out < 1) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: bad argument");
  if (!s->bound) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: parameters not set (sgrl_mlp_set_params)");
  int64_t n = 0;
  const int in_dim = s->plan.dims[0], out_dim = s->plan.dims[s->plan.n_layers];
  for (int k = 0; k < n_morph; k++) {
    if (morph_count[k] < 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: negative morph_count");
    if ((int64_t)feature * morph_L[k] != in_dim || (int64_t)out * morph_L[k] != out_dim)
      return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: morphology " + std::to_string(k) + " has " + std::to_string(morph_L[k]) +
                                     " limbs; the network was built for " + std::to_string(in_dim) + " inputs and " +
                                     std::to_string(out_dim) + " outputs (" + std::to_string(feature) + " / " + std::to_string(out) + " per limb)");
    n += morph_count[k];
  }
  if (n == 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: no environments");
  if (n > ((int64_t)1 << 24)) return mfail(SGRL_ERR_ARG, "sgrl_mlp_configure: more than 2^24 environments in one batch");
  s->n_env = (int)n;
  return SGRL_OK;
}

int sgrl_mlp_forward(sgrl_mlp* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, void* stream) {
  if (!s || !obs || !act) return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: null argument");
  if (!s->bound || s->n_env <= 0) return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: parameters or batch structure not set");
  const Plan& p = s->plan;
  const int in_dim = p.dims[0], out_dim = p.dims[p.n_layers];
  if (obs_ld < in_dim || act_ld < out_dim)
    return mfail(SGRL_ERR_ARG, "sgrl_mlp_forward: obs_ld < input width or act_ld < output width (rows too narrow for the network)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  const bool capturing = cap != hipStreamCaptureStatusNone;
  if (!s->hold || s->dirty || capturing) {
    PackArgs pa;
    for (int l = 0; l < NL; l++) {
      const bool on = l < p.n_layers;
      pa.w[l] = on ? s->w[l] : nullptr;
      pa.b[l] = on ? s->b[l] : nullptr;
      pa.n[l] = on ? p.dims[l + 1] : 0;
      pa.k[l] = on ? p.dims[l] : 0;
      pa.npad[l] = on ? p.npad[l] : 0;
      pa.kpad[l] = on ? p.kpad[l] : 0;
      pa.w_off[l] = on ? p.w_off[l] : 0;
      pa.b_off[l] = on ? p.b_off[l] : 0;
    }
    pa.n_layers = p.n_layers;
    pa.total = p.total;
    pa.dst = s->packed;
    const int blocks = (int)((p.total + 1023) / 1024);
    hipLaunchKernelGGL(k_mlp_pack, dim3(blocks), dim3(256), 0, st, pa);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("MLP pack launch: ") + hipGetErrorString(e));
    if (!capturing) s->dirty = false;
  }
  FwdArgs fa;
  fa.obs = obs; fa.obs_ld = obs_ld; fa.act = act; fa.act_ld = act_ld; fa.wp = s->packed;
  fa.n_env = s->n_env; fa.in_dim = in_dim; fa.out_dim = out_dim; fa.n_layers = p.n_layers; fa.sx = p.sx;
  for (int l = 0; l < NL; l++) {
    const bool on = l < p.n_layers;
    fa.kpad[l] = on ? p.kpad[l] : 0;
    fa.npad[l] = on ? p.npad[l] : 0;
    fa.w_off[l] = on ? p.w_off[l] : 0;
    fa.b_off[l] = on ? p.b_off[l] : 0;
  }
  fa.max_action = max_action;
  const int grid = (s->n_env + BM - 1) / BM;
  hipLaunchKernelGGL(s->kernel, dim3(grid), dim3(256), p.lds, st, fa);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mfail(SGRL_ERR_HIP, std::string("MLP forward launch: ") + hipGetErrorString(e));
  return SGRL_OK;
}

}  // extern "C"
