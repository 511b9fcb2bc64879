/* sgrl_mlp.h -- C ABI of the monolithic MLP agent's no-grad forwards in libsgrl_hip.so: the actor, the twin critic and the TD3
 * target chain (further down), one launch each.
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

/* ---- twin critic and TD3 target chain ----------------------------------------------------------------------------------------
 * Replaces, under torch.no_grad(), MlpCritic.forward / Q1 (reference src/MLPCritic.py:40-52) and the target half of Agent.update
 * (reference src/agent.py:126-148).  A critic is two stacks of identical widths dims = [(feature + act_feature) L, hidden ..., 1]
 * over cat([state, action]).  A handle is an actor or a critic: the last bind decides. */

/* Bind a critic: ptrs is a HOST array of n_ptrs = 4 * (n_dims - 1) DEVICE addresses, critic1's W0, b0, W1, b1, ... then critic2's;
 * dims[n_dims - 1] must be 1.  Both stacks go into one packed buffer back to back, each in the layout sgrl_mlp_plan describes for
 * dims (stack 2 at float offset *total); ONE pack launch covers both.  sgrl_mlp_hold_weights and sgrl_mlp_generation as for an
 * actor.  On a critic handle sgrl_mlp_configure(..., feature, out) checks (feature + out) * morph_L[k] == dims[0]. */
int sgrl_mlp_set_critic_params(sgrl_mlp* s, const void* const* ptrs, int n_ptrs, const int32_t* dims, int n_dims);

/* q1[e] / q2[e] = critic{1,2}(cat(obs[e, 0 : feature L], act[e, 0 : out L])) for the configured environments; q2 == NULL: Q1 only
 * (the same bits as the twin call's q1).  obs: DEV float [n_env, obs_ld]; act: DEV float [n_env, act_ld]; q1, q2: DEV float
 * [n_env].  Columns beyond feature L / out L of a row are never read.  One launch (plus the pack when not holding).  SGRL_ERR_ARG
 * before any launch for null pointers, narrow rows, a handle not bound as a critic or not configured. */
int sgrl_mlp_critic_forward(sgrl_mlp* s, const float* obs, int obs_ld, const float* act, int act_ld, float* q1, float* q2, void* stream);

/* The whole target chain in ONE launch (plus the two packs when not holding):
 *   a           = clamp(max_action * tanh(actor_t(next_obs)) + clamp(noise, +-noise_clip), +-max_action)
 *   target_q[e] = reward[e] + (1 - done[e]) * discount * min(Q1_t, Q2_t)(next_obs[e], a[e])
 * next_obs: DEV float [n_env, obs_ld]; noise (the unclipped draw, laid out like an action row): DEV float [n_env, noise_ld];
 * reward, done, target_q: DEV float [n_env].  action_out may be NULL; otherwise DEV float [n_env, action_ld], it receives a and
 * exact zeros in columns [out width, action_ld).  With action_out NULL the actions pass through a workspace of the critic handle
 * (grown on demand, which bumps its generation; a capture cannot grow it: run the batch size eagerly first).  SGRL_ERR_ARG before
 * any launch for null pointers, narrow rows, handles of the wrong kind, different n_env, a critic whose input is not the actor's
 * input + output width. */
int sgrl_mlp_td_target(sgrl_mlp* actor_t, sgrl_mlp* critic_t, const float* next_obs, int obs_ld, const float* noise, int noise_ld,
                       const float* reward, const float* done, float max_action, float noise_clip, float discount, float* target_q,
                       float* action_out, int action_ld, void* stream);

/* HOST ONLY.  What the fused chain kernel uses for the pair: info[0] = column chunks (the larger of the two plans), info[1] = panel
 * depth, info[2] = LDS bytes, info[3] = activation row stride in floats (from the widest padded input of either network).
 * SGRL_ERR_ARG for what sgrl_mlp_plan refuses, a critic whose last width is not 1 or whose input is not the actor's input + output. */
int sgrl_mlp_chain_plan(const int32_t* actor_dims, int n_a, const int32_t* critic_dims, int n_c, int32_t* info);

/* Launches of the chain proper (1) and of a critic forward proper (1); each pack adds sgrl_mlp_pack_launches(). */
int sgrl_mlp_td_target_launches(void);
int sgrl_mlp_critic_forward_launches(void);

#ifdef __cplusplus
}
#endif
#endif /* SGRL_MLP_H */
