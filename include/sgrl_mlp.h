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

/* ---- gradient half of the TD3 update ---------------------------------------------------------------------------------------------
 * Replaces the critics' forward with autograd, the two losses and their backward passes (reference src/agent.py:150-177):
 *   critic step   loss = mse(Q1(obs, act), target) + mse(Q2(obs, act), target);  d loss / d every critic parameter   agent.py:150-160
 *   actor step    loss = -mean(Q1(obs, actor(obs)));                             d loss / d every actor parameter    agent.py:167-173
 * for MlpCritic / MlpPolicy (reference src/MLPCritic.py:40-52, src/MLPActor.py:45-66).  The clipping and the Adam steps
 * (agent.py:161-164, 174-177) stay with the caller (include/sgrl_train.h sgrl_optim_clip_adam reads the gradients written here).
 * A step is: the pack of every network it walks (the weights have just been stepped), ONE row-parallel launch (forward with the
 * hidden activations stashed in a workspace, loss partials, backward down to every layer's pre-activation gradient G_l), and ONE
 * weight-gradient launch in which a workgroup owns one 32 x 32 tile of one dW_l = G_l^T A_{l-1} and reduces over all rows itself in
 * a fixed order (no split-K, no float atomics: the gradients are bit-repeatable); the bias gradients (column sums of G_l) and the
 * reduction of the loss partials to one device float ride in that launch.  Products are exact f32 (v_mfma_f32_32x32x2_f32).  The
 * gradients are WRITTEN (not accumulated) to the bound .grad tensors, unpadded.  No call synchronises with the host; after the first
 * call at a batch size none allocates.  Served widths: every padded width up to SGRL_MLP_TRAIN_MAX_WIDTH (sgrl_mlp_train_plan). */
#define SGRL_MLP_TRAIN_MAX_WIDTH 512

/* HOST ONLY.  What the gradient half uses for an actor / critic pair at `batch` rows: info[0] = column chunks of 256 (1 or 2),
 * info[1] = panel depth, info[2] = LDS bytes of a row-parallel workgroup, info[3] = activation row stride in floats (4 + the widest
 * padded width, input or output, of either network), info[4] / info[5] = weight-gradient tiles (= workgroups of the second launch)
 * of a critic / an actor step, info[6] = row tiles (workgroups of the first launch).  ws_floats[0] / ws_floats[1] = floats of the
 * critic / actor handle's workspace at this batch: the stashed input tile [batch, kpad[0]], per stack the hidden activations
 * [batch, npad[l]] and every G_l [batch, npad[l]], the loss partials (4 / 2 per row tile) and, for the actor, tanh(z)
 * [batch, npad[last]] and the action rows [batch, out].  SGRL_ERR_ARG for what sgrl_mlp_plan refuses, a critic whose last width is
 * not 1 or whose input is not the actor's input + output, batch outside 1 .. 2^24, and widths this path does not serve (a padded
 * width above SGRL_MLP_TRAIN_MAX_WIDTH: the row-parallel kernels would need more accumulator registers than there are without
 * scratch); the message says which. */
int sgrl_mlp_train_plan(const int32_t* actor_dims, int n_a, const int32_t* critic_dims, int n_c, int batch, int32_t* info,
                        int64_t* ws_floats);

/* Bind the .grad tensors by address: ptrs is a HOST array of n_ptrs DEVICE addresses in the order (and of the shapes) of the
 * parameter bind -- dW0, db0, dW1, db1, ... (a critic: stack 1's, then stack 2's).  Contiguous float32, 4-byte aligned.  A later
 * parameter bind drops them.  SGRL_ERR_ARG for a null argument, a handle with no parameters, a wrong count, a null address. */
int sgrl_mlp_bind_grads(sgrl_mlp* s, const void* const* ptrs, int n_ptrs);

/* The critic step.  obs: DEV float [n_env, obs_ld]; act: DEV float [n_env, act_ld]; target_q: DEV float [n_env]; loss_out: DEV
 * float[1] receives sum_s mean((Q_s - target)^2).  Every bound .grad of the critic receives d loss_out / d parameter.
 * sgrl_mlp_critic_step_launches() launches (pack, row-parallel pass, weight gradients).  The workspace grows on demand (which bumps
 * sgrl_mlp_generation; a capture cannot grow it).  SGRL_ERR_ARG BEFORE ANY LAUNCH, nothing written, for null pointers, narrow rows,
 * a handle not bound as a critic or not configured, gradients not bound, widths the path does not serve. */
int sgrl_mlp_critic_step_grads(sgrl_mlp* critic, const float* obs, int obs_ld, const float* act, int act_ld, const float* target_q,
                               float* loss_out, void* stream);

/* The actor step.  a = max_action * tanh(actor(obs)); loss_out: DEV float[1] receives -mean(Q1(obs, a)); every bound .grad of the
 * ACTOR receives d loss_out / d parameter.  The critic's gradients are neither computed nor touched: its .grad tensors keep what
 * the critic step (and the caller's clipping) left there.  action_out may be NULL; otherwise DEV float [n_env, action_ld], it
 * receives a (columns beyond the output width are not written).  sgrl_mlp_actor_step_launches() launches (two packs -- the critic
 * has been stepped since its own -- the row-parallel pass, the weight gradients).  SGRL_ERR_ARG before any launch, nothing written,
 * for null pointers, narrow rows, handles of the wrong kind, actor gradients not bound, different batch structures, a critic that
 * does not read the actor's input + output, widths the path does not serve. */
int sgrl_mlp_actor_step_grads(sgrl_mlp* actor, sgrl_mlp* critic, const float* obs, int obs_ld, float max_action, float* loss_out,
                              float* action_out, int action_ld, void* stream);

int sgrl_mlp_critic_step_launches(void); /* 3 */
int sgrl_mlp_actor_step_launches(void);  /* 4 */

/* ---- optimizer half of the TD3 update --------------------------------------------------------------------------------------------
 * Replaces, for ONE handle (an actor, 1 stack, or a critic, 2 stacks) whose parameters and gradients are bound, clip_grad_norm_ +
 * Adam.step (reference src/agent.py:161-164, 174-177) and, with tau > 0, the soft update of the network's target
 * (common/functional.py:7-10), in TWO launches:
 *   coef = max_norm > 0 ? min(1, max_norm / (sqrtf(total) + 1e-6f)) : none          total = sum of g^2 over every bound gradient
 *          (a NaN total gives a NaN coef, as torch.clamp(coef, max=1.0) does in clip_grad_norm_: every g, m, v, p and target of the
 *          handle becomes NaN; an infinite total gives coef = 0; a select, not fminf, which would return 1 for a NaN)
 *   g   := g * coef               (written back to .grad when max_norm > 0, as clip_grad_norm_ does)
 *   t    = the first bound step counter, after every bound counter has been advanced by 1
 *   m   := b1 m + (1 - b1) g;   v := b2 v + (1 - b2) g g;   p := p - (lr / (1 - b1^t)) * m / (sqrtf(v) / sqrtf(1 - b2^t) + eps)
 *   tau > 0:  target := target * (1 - tau) + tau * p                                (the p just written)
 * term for term as sgrl_optim_clip_adam / sgrl_optim_lerp of include/sgrl_train.h compute it (float32 tensors; lr, beta1, beta2, eps
 * enter as doubles where they do there).  The tensors are cut into chunks of sgrl_mlp_optim_plan's chunk size, one workgroup per
 * chunk.  Launch 1: partial[c] = sum of g^2 over chunk c, and workgroup 0 advances the counters (max_norm == 0: the counters only,
 * one workgroup).  Launch 2: every workgroup re-adds all partials itself, then applies the formula to its chunk.  ORDER OF THE SUM,
 * fixed (a step is bit-repeatable; no atomics): thread t of 256 owns elements 4 t .. 4 t + 3 of its chunk and adds their squares
 * in order; a wave adds its lanes by a butterfly (6 additions); the four waves are added in order; in launch 2 thread t adds
 * partials t, t + 256, ... serially, then the same butterfly and wave sum.  The longest chain of float additions from a g^2 to the
 * total is 22 + ceil(chunks / 256), at most 63 for any handle the plan admits.  Accesses are 16 bytes wide where a tensor's
 * addresses are 16-byte aligned, scalar in a tensor's ragged tail and for unaligned tensors, with the same bits either way.
 * A step never synchronises with the host, allocates nothing, reads the step count on the device, and can be recorded into a
 * hipGraph. */

/* HOST ONLY.  info[0] = tensors of a handle of n_stacks stacks of the widths dims (2 * n_stacks * (n_dims - 1): W0, b0, W1, b1, ...
 * per stack), info[1] = their elements, info[2] = chunks (= workgroups of either launch; a tensor of n elements has
 * ceil(n / chunk size), chunks never span tensors), info[3] = the chunk size in elements.  SGRL_ERR_ARG for whatever sgrl_mlp_plan
 * refuses, n_stacks other than 1 or 2, two stacks whose last width is not 1 (sgrl_mlp_set_critic_params binds no such critic). */
int sgrl_mlp_optim_plan(const int32_t* dims, int n_dims, int n_stacks, int64_t* info);

/* Bind the optimizer state by address: exp_avg / exp_avg_sq are HOST arrays of n DEVICE addresses in the order (and of the shapes)
 * of the parameter bind, n = the plan's tensors; steps: n_steps (1 .. n) DEVICE float counters -- a step advances ALL of them by 1
 * and reads the FIRST; target: n_target = 0, or n addresses of the target network's parameters in the same order.  partials: a
 * DEVICE buffer of partial_floats >= the plan's chunks floats that stays the caller's (the library allocates nothing; a step
 * overwrites it).  Everything contiguous float32, 4-byte aligned.  Needs the parameters AND the gradients bound; a later parameter
 * bind drops this bind as it drops the gradient bind, and so does a later sgrl_mlp_bind_grads.  SGRL_ERR_ARG for a null argument, a
 * handle without parameters or gradients, a wrong count, a null or unaligned address, a partials buffer that is too small. */
int sgrl_mlp_bind_optim(sgrl_mlp* s, const void* const* exp_avg, const void* const* exp_avg_sq, int n, const void* const* steps, int n_steps,
                        const void* const* target, int n_target, float* partials, int64_t partial_floats);
/* 1 while the bind above stands, else 0. */
int sgrl_mlp_optim_bound(const sgrl_mlp* s);

/* One step (the formula above), asynchronous on `stream`.  max_norm == 0: no clipping, .grad is not written; tau == 0: the target
 * is neither read nor written.  SGRL_ERR_ARG BEFORE ANY LAUNCH, nothing written, for a null handle, parameters, gradients or state
 * not bound, tau > 0 with no target bound, tau outside [0, 1], max_norm < 0, a hyper-parameter that is not finite. */
int sgrl_mlp_optim_step(sgrl_mlp* s, double lr, double beta1, double beta2, double eps, float max_norm, float tau, void* stream);

int sgrl_mlp_optim_step_launches(void); /* 2 */

/* ---- batch prologue of the TD3 update ------------------------------------------------------------------------------------------
 * Replaces the reward scaling `reward_batch = reward_batch * self.reward_scale` (reference src/agent.py:124) and the two statistics
 * `torch.mean(reward_batch)`, `torch.var(reward_batch)` of "misc/train_reward_mean" / "misc/train_reward_var" (agent.py:160-161):
 *   reward_out[i] = reward[i] * reward_scale        one float32 product: the bits of `tensor * python_float` in torch
 *   stats[0]      = (sum of reward_out) / n
 *   stats[1]      = (sum of (reward_out[i] - stats[0])^2) / (n - 1)        two passes, unbiased, as torch.var; n = 1: NaN
 * reward: DEV float [n]; reward_out: DEV float [n], may BE reward (in place); stats: DEV float [2]; n in 1 .. 2^24.  ONE launch of
 * ONE workgroup of 256 threads.  ORDER OF THE SUMS, fixed (a call is bit-repeatable; no atomics, no scratch): thread t adds elements
 * t, t + 256, ... serially, a wave adds its lanes by a butterfly (xor 32 .. 1), the four waves are added in order -- the order of the
 * optimizer half's total.  No operation is fused: every product, sum and quotient rounds once to float32.  Asynchronous on `stream`,
 * allocates nothing, and can be recorded into a hipGraph.  SGRL_ERR_ARG BEFORE ANY LAUNCH, nothing written, for a null or unaligned
 * pointer, n out of range, a scale that is not finite. */
int sgrl_mlp_batch_stats(const float* reward, int n, float reward_scale, float* reward_out, float* stats /* [2] */, void* stream);
int sgrl_mlp_batch_stats_launches(void); /* 1 */

#ifdef __cplusplus
}
#endif
#endif /* SGRL_MLP_H */
