/* sgrl_mlp.h -- C ABI of the monolithic MLP actor forward in libsgrl_hip.so.
 *
 * Replaces, for inference under torch.no_grad(), the chain
 *   Agent.select_action                    reference src/agent.py:189-198
 *   -> MlpPolicy.forward                   reference src/MLPActor.py:45-66
 *   -> DeterministicPolicyNetwork.forward  reference src/common/networks.py:218-220
 * for a whole batch of environments in ONE launch: a workgroup owns 32 environment rows and walks every layer; the hidden
 * activations live in LDS from the first layer to the last, the weights stream through LDS k-block by k-block, only the
 * observation rows are read and the action rows written.  Products are exact f32 (v_mfma_f32_32x32x2_f32).  A forward never
 * synchronises with the host and can be recorded into a hipGraph.
 *
 * Network: x -> relu(W0 x + b0) -> ... -> relu(W_{H-1} . + b_{H-1}) -> max_action * tanh(W_H . + b_H), 1 <= H <= 4 hidden layers,
 * every width (input, hidden, output) between 1 and SGRL_MLP_MAX_WIDTH.  Widths need not be multiples of anything: the library
 * pads them in its own packed copy of the weights (sgrl_mlp_plan says how).
 */
#ifndef SGRL_MLP_H
#define SGRL_MLP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgrl_mlp sgrl_mlp;

#define SGRL_MLP_MAX_HIDDEN 4
#define SGRL_MLP_MAX_LAYERS (SGRL_MLP_MAX_HIDDEN + 1)
#define SGRL_MLP_MAX_WIDTH 1024
#define SGRL_MLP_TILE_ROWS 32 /* environment rows per workgroup */

/* What the library does with the widths dims[0 .. n_dims) = input, hidden widths ..., output (n_dims = H + 2).  HOST ONLY (no
 * device needed).  Layer l maps dims[l] -> dims[l + 1]; its packed weight is [npad[l]][kpad[l]] row-major at float offset
 * w_off[l] of the packed buffer, its packed bias [npad[l]] at b_off[l], zeros in the padding:
 *   kpad[0] = dims[0] rounded up to 16,  npad[l] = dims[l + 1] rounded up to 32,  kpad[l + 1] = npad[l].
 * info[0] = column chunks of 256 a workgroup keeps accumulators for (1, 2 or 4), info[1] = k extent of a weight panel in LDS
 * (16, or 8 where 16 would not fit), info[2] = LDS bytes of a workgroup, info[3] = row stride of the activation tile in floats,
 * *total = floats of the packed buffer.  SGRL_ERR_ARG for null pointers, n_dims outside 3 .. 6, a width outside
 * 1 .. SGRL_MLP_MAX_WIDTH. */
int sgrl_mlp_plan(const int32_t* dims, int n_dims, int32_t* kpad, int32_t* npad, int64_t* w_off, int64_t* b_off, int32_t* info,
                  int64_t* total);

/* A handle with no weights and no batch structure yet.  SGRL_ERR_HIP when no device is visible (there is no CPU fallback). */
int sgrl_mlp_create(sgrl_mlp** out);
void sgrl_mlp_destroy(sgrl_mlp* s);

/* Bind the network's parameters by address: ptrs is a HOST array of n_ptrs = 2 * (n_dims - 1) DEVICE addresses
 * W0, b0, W1, b1, ... (contiguous float32 as torch stores an nn.Linear: weight [out, in] row-major, bias [out]); dims as in
 * sgrl_mlp_plan.  The handle keeps the addresses; the VALUES are copied into the padded packed buffer by one pack launch at the
 * top of a forward (see sgrl_mlp_hold_weights).  Re-bind after anything that MOVES a parameter. */
int sgrl_mlp_set_params(sgrl_mlp* s, const void* const* ptrs, int n_ptrs, const int32_t* dims, int n_dims);

/* Weight hold (the rule of sgrl_set_hold_weights).  By default every forward packs from the live parameters first.
 * sgrl_mlp_hold_weights(s, 1) is the caller's promise that the parameters stay as they are until the next call of this function:
 * the first forward after it packs, the following ones reuse the packed buffer.  Every call (1 again, or 0 = back to packing on
 * every forward) also means "the parameters may just have changed".  Forwards recorded into a hipGraph always pack. */
int sgrl_mlp_hold_weights(sgrl_mlp* s, int hold);

/* Batch structure: n_morph morphologies of morph_L[k] limbs with morph_count[k] environments each (environment blocks in this
 * order).  A monolithic network serves ONE limb count: SGRL_ERR_ARG unless feature * morph_L[k] is the bound input width and
 * out * morph_L[k] the bound output width for every k (feature / out: values per limb, 41 / 3 for the actor). */
int sgrl_mlp_configure(sgrl_mlp* s, int n_morph, const int32_t* morph_L, const int32_t* morph_count, int feature, int out);

/* act[e, 0 : out_width] = max_action * tanh(net(obs[e, 0 : in_width])), act[e, out_width : act_ld] = 0 exactly, for the
 * configured environments.  obs: DEV float [n_env, obs_ld]; act: DEV float [n_env, act_ld].  SGRL_ERR_ARG (before any launch) for
 * null pointers, obs_ld < in_width, act_ld < out_width, parameters or batch structure not set.  Asynchronous on `stream`. */
int sgrl_mlp_forward(sgrl_mlp* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, void* stream);

/* Launches of the forward proper (1) and of the pack a forward adds when it is not holding (1). */
int sgrl_mlp_forward_launches(void);
int sgrl_mlp_pack_launches(void);
int sgrl_mlp_num_envs(const sgrl_mlp* s);
/* Counter bumped whenever the handle FREES device memory a captured forward may point into (a packed buffer replaced by
 * sgrl_mlp_set_params with other widths): a hipGraph holding forwards of this handle must be captured again once it has changed. */
int64_t sgrl_mlp_generation(const sgrl_mlp* s);
const char* sgrl_mlp_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SGRL_MLP_H */
