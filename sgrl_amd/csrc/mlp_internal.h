// mlp_internal.h -- what the three translation units of the MLP family share (mlp_actor.hip: the no-grad forwards, the pack, the
// handle; mlp_train.hip: the gradient half of a TD3 update; mlp_optim.hip: its optimizer half): the width plan, the handle, the packed stack a kernel walks, the
// tile loaders, and the few host helpers mlp_actor.hip defines for both.  Not part of the C ABI (include/sgrl_mlp.h).
#ifndef SGRL_MLP_INTERNAL_H
#define SGRL_MLP_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sgrl.h"
#include "../../include/sgrl_mlp.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace sgrl_mlp_detail {

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

struct Net {                         // one packed Linear / ReLU stack
  const float* wp;
  int n_layers;
  int kpad[NL], npad[NL];
  long long w_off[NL], b_off[NL];
};

inline Net make_net(const Plan& p, const float* wp) {
  Net n;
  n.wp = wp;
  n.n_layers = p.n_layers;
  for (int l = 0; l < NL; l++) {
    const bool on = l < p.n_layers;
    n.kpad[l] = on ? p.kpad[l] : 0;
    n.npad[l] = on ? p.npad[l] : 0;
    n.w_off[l] = on ? p.w_off[l] : 0;
    n.b_off[l] = on ? p.b_off[l] : 0;
  }
  return n;
}

// X[r][col0 + k] for k in [0, fill): src[row0 + r][k] where k < valid and the row exists, zeros elsewhere.
__device__ __forceinline__ void load_rows(float* X, int sx, int col0, int valid, int fill, const float* __restrict__ src, int ld, int row0,
                                          int n_env) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < BM; r += 4) {
    const int row = row0 + r;
    for (int k = lane; k < fill; k += 64) X[r * sx + col0 + k] = (row < n_env && k < valid) ? src[(size_t)row * ld + k] : 0.f;
  }
}

// C/D layout of a 32 x 32 tile: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int tile_row(int e) { return (e & 3) + 8 * (e >> 2) + 4 * ((threadIdx.x & 63) >> 5); }

// Defined in mlp_actor.hip.
int mfail(int code, const std::string& msg);                 // sets sgrl_mlp_last_error
int make_plan(const int32_t* dims, int n_dims, Plan* p, const char* who);
int pack_now(sgrl_mlp* s, hipStream_t st);                   // the pack launch, whatever the hold says

}  // namespace sgrl_mlp_detail

enum { SGRL_MLP_KIND_NONE = 0, SGRL_MLP_KIND_ACTOR = 1, SGRL_MLP_KIND_CRITIC = 2 };
enum { SGRL_MLP_BOUND_GRADS_AND_STATE = 2 };   // sgrl_mlp::grads_bound once sgrl_mlp_bind_optim has run

struct sgrl_mlp {
  sgrl_mlp_detail::Plan plan;
  int kind = SGRL_MLP_KIND_NONE;     // the last bind decides (sgrl_mlp_set_params / sgrl_mlp_set_critic_params)
  const float* w[2][sgrl_mlp_detail::NL] = {{nullptr}};
  const float* b[2][sgrl_mlp_detail::NL] = {{nullptr}};
  float* packed = nullptr;           // n_stacks * plan.total floats
  int64_t packed_floats = 0;
  bool hold = false, dirty = true;
  int n_env = 0;
  int obs_w = 0, act_w = 0;          // a configured critic: columns of an observation / action row it reads
  int64_t generation = 0;
  const void* kernel = nullptr;      // the k_mlp_forward (actor) / k_mlp_critic (critic) variant of the bound widths
  float* ws = nullptr;               // a critic: the chain's target actions when the caller does not ask for them
  int64_t ws_floats = 0;
  // the gradient half (mlp_train.hip): .grad addresses in the order of the parameter bind, and the stash workspace
  float* gw[2][sgrl_mlp_detail::NL] = {{nullptr}};
  float* gb[2][sgrl_mlp_detail::NL] = {{nullptr}};
  // 0 after a parameter bind, 1 (true) after sgrl_mlp_bind_grads, SGRL_MLP_BOUND_GRADS_AND_STATE after sgrl_mlp_bind_optim: the
  // optimizer bind sits on top of the gradient bind, so whatever drops or renews the gradient bind drops it too
  int grads_bound = 0;
  float* tws = nullptr;
  int64_t tws_floats = 0;
  // the optimizer half (mlp_optim.hip): Adam state, step counters and target parameters by address, in the order of the parameter
  // bind (index 2 * (stack * n_layers + layer) + (0 weight / 1 bias)); the partials buffer is the caller's
  float* opt_m[4 * sgrl_mlp_detail::NL] = {nullptr};
  float* opt_v[4 * sgrl_mlp_detail::NL] = {nullptr};
  float* opt_target[4 * sgrl_mlp_detail::NL] = {nullptr};
  float* opt_step[4 * sgrl_mlp_detail::NL] = {nullptr};
  int opt_n_steps = 0;
  bool opt_has_target = false;
  float* opt_partial = nullptr;
};

#endif  // SGRL_MLP_INTERNAL_H
