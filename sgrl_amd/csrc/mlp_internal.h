// mlp_internal.h -- the host side the three translation units of the MLP family share (mlp_actor.hip: the no-grad forwards, the pack,
// the handle; mlp_train.hip: the gradient half of a TD3 update; mlp_optim.hip: its optimizer half): the width plan, the tile variant a
// kernel is launched with, the handle, the packed stack a kernel walks, and the host helpers every entry point uses, each defined once
// in mlp_actor.hip.  The device code the row-tile kernels share is in mlp_tile.h.  Not part of the C ABI (include/sgrl_mlp.h).
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

// The variant of a row-tile kernel and its dynamic LDS: chunks of accumulators, panel depth, bytes, activation row stride.
struct TilePlan {
  int maxch = 1, bk = 16, lds = 0, sx = 0;
};

struct Plan : TilePlan {
  int n_layers = 0;
  int dims[NL + 1] = {0};
  int kpad[NL] = {0}, npad[NL] = {0};
  int64_t w_off[NL] = {0}, b_off[NL] = {0};
  int64_t total = 0;
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

// Defined in mlp_actor.hip.  `who` is the entry point's name: it opens every message.
int mfail(int code, const std::string& msg);                 // sets sgrl_mlp_last_error
int make_plan(const int32_t* dims, int n_dims, Plan* p, const char* who);
int pack_now(sgrl_mlp* s, hipStream_t st);                   // the pack launch, whatever the hold says
int lds_bytes(int sx, int bk);                               // the activation tile [BM][sx] and two panel stages [CH][bk + 4]
TilePlan tile_plan(int maxch, int sx);                       // the deepest panel (16, else 8) that fits beside the activation tile
void put_tile_plan(const TilePlan& t, int32_t* info);        // info[0 .. 3] of the three plan entry points
// The dynamic-LDS limit of a kernel is a property of the function, process-wide: the largest size asked for so far is kept per kernel
// and the attribute only ever goes up (handles of different widths share a variant).
int raise_lds(const void* fn, int lds, const char* who);
// A fresh device buffer of `need` floats in place of *buf (`what` names it in the messages): refused while capturing; the old buffer,
// if any, is freed behind a device synchronise (work in flight may still use it) and the handle's generation is bumped.  The caller
// decides when: the packed weights whenever the size differs, the workspaces only when it grows.
int grow(float** buf, int64_t* floats, int64_t need, bool capturing, int64_t* generation, const char* who, const char* what);
bool is_capturing(hipStream_t st);
int launched(const char* what);                              // hipGetLastError behind a launch -> "<what> launch: ..."
int n_stacks(const sgrl_mlp* s);                             // a critic packs its two Q stacks, an actor one
// Both plans of an actor / critic pair, a critic whose last width is 1 and whose input is the actor's input + output width.
int make_pair_plans(const int32_t* actor_dims, int n_a, const int32_t* critic_dims, int n_c, Plan* pa, Plan* pc, const char* who);
// Two configured handles of an actor / critic pair: kinds, batch structure set and equal, the critic reads the actor's input + output.
int check_pair(const sgrl_mlp* actor, const sgrl_mlp* critic, const char* who);
// n addresses, none null, all 4-byte aligned; `what` names one in the message ("<who>: <what> <i> is null or not 4-byte aligned")
int check_addresses(const void* const* ptrs, int n, const char* who, const char* what);

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
