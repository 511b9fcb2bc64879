/* sgrl_swat.h -- C ABI of the SWAT (structure-aware transformer) actor forward, critic forward and TD3 target chain in
 * libsgrl_hip.so.
 *
 * Replaces, for inference under torch.no_grad(), the chain
 *   Agent.select_action                    reference src/agent.py:189-198
 *   -> StructurePolicy.forward             reference src/StructureActor.py:221-243
 *   -> TransformerModel.forward            reference src/StructureActor.py:159-170
 *   -> RepeatTransformerEncoder.forward    reference src/StructureActor.py:77-107
 *   -> MyTransformerEncoderLayer.forward   reference src/StructureActor.py:52-64
 *   -> MyMultiheadAttention.forward        reference src/StructureActor.py:36-45
 * for a whole batch of environments of mixed morphologies in one call (environment blocks per morphology, the nodes of one
 * environment contiguous, node-major rows).  Every per-node linear layer runs over the nodes of ALL morphologies at once
 * (exact-f32 matrix instructions, csrc/gemm_f32.h k_gemm2); attention runs per environment over its own limbs, one workgroup
 * per environment.  The number of launches per forward is fixed (22) whatever the number of morphologies; a forward never
 * synchronises with the host and can be recorded into a hipGraph.
 *
 * Shapes (sgrl_amd/swat_policy.py, the reference's default_args): embedding E = 128, 2 heads of 64, feed-forward 256, 3 layers,
 * relation features 3, position tables of 15 rows (so at most 15 limbs), `feature` inputs and `out` outputs per limb.
 */
#ifndef SGRL_SWAT_H
#define SGRL_SWAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgrl_swat sgrl_swat;

/* Parameter table of sgrl_swat_bind_params: one DEVICE address per tensor, contiguous float32 exactly as torch stores it
 * (nn.Linear weights [out, in] row-major, in_proj_weight already stacked q | k | v).  Global slots first ... */
enum {
  SGRL_SWAT_EMB0 = 0,   /* pos_encoder.embeddings.0.weight [15, 42] */
  SGRL_SWAT_EMB1,       /* pos_encoder.embeddings.1.weight [15, 42] */
  SGRL_SWAT_EMB2,       /* pos_encoder.embeddings.2.weight [15, 44] */
  SGRL_SWAT_ENC_W,      /* encoder.weight [128, feature] */
  SGRL_SWAT_ENC_B,      /* encoder.bias [128] */
  SGRL_SWAT_REL_W,      /* transformer_encoder.rel_encoder.weight [2, 3] */
  SGRL_SWAT_REL_B,      /* transformer_encoder.rel_encoder.bias [2] */
  SGRL_SWAT_DEC_W,      /* decoder.weight [out, 128] or [out, 128 + feature] (cond_decoder) */
  SGRL_SWAT_DEC_B,      /* decoder.bias [out] */
  SGRL_SWAT_NGLOBAL
};
/* ... then per layer l (slot = SGRL_SWAT_NGLOBAL + l * SGRL_SWAT_NLAYER + k), prefix transformer_encoder.layers.<l>. ... */
enum {
  SGRL_SWAT_IN_W = 0,   /* self_attn.in_proj_weight [384, 128] */
  SGRL_SWAT_IN_B,       /* self_attn.in_proj_bias [384] */
  SGRL_SWAT_OUT_W,      /* self_attn.out_proj.weight [128, 128] */
  SGRL_SWAT_OUT_B,      /* self_attn.out_proj.bias [128] */
  SGRL_SWAT_L1_W,       /* linear1.weight [256, 128] */
  SGRL_SWAT_L1_B,       /* linear1.bias [256] */
  SGRL_SWAT_L2_W,       /* linear2.weight [128, 256] */
  SGRL_SWAT_L2_B,       /* linear2.bias [128] */
  SGRL_SWAT_N1_W,       /* norm1.weight [128] */
  SGRL_SWAT_N1_B,       /* norm1.bias [128] */
  SGRL_SWAT_N2_W,       /* norm2.weight [128] */
  SGRL_SWAT_N2_B,       /* norm2.bias [128] */
  SGRL_SWAT_NLAYER
};
#define SGRL_SWAT_LAYERS 3
/* ... then, with transformer_norm only, transformer_encoder.norm.weight [128] and .bias [128] (the final LayerNorm). */
#define SGRL_SWAT_NW(transformer_norm) (SGRL_SWAT_NGLOBAL + SGRL_SWAT_LAYERS * SGRL_SWAT_NLAYER + ((transformer_norm) ? 2 : 0))
#define SGRL_SWAT_MAX_LIMBS 15

/* reference StructurePolicy.__init__ (StructureActor.py:179-219) builds the network; here: a handle with no weights and no
 * batch structure yet.  SGRL_ERR_HIP when no device is visible (there is no CPU fallback). */
int sgrl_swat_create(sgrl_swat** out);
void sgrl_swat_destroy(sgrl_swat* s);

/* Bind the network's parameters by address (reference agent.py:155-176 and common/functional.py:7-10 update the same tensors in
 * place: optimizer steps, soft updates, load_state_dict and in-place broadcasts therefore need no call).  The handle keeps only
 * the addresses and every forward reads the values behind them; re-bind after anything that MOVES a parameter (module.to(),
 * re-created tensors).  ptrs: HOST array of n = SGRL_SWAT_NW(transformer_norm) DEVICE addresses in the slot order above, each
 * 16-byte aligned.  cond_decoder: condition_decoder_on_features (StructureActor.py:146-150, 166-168); transformer_norm: the
 * final LayerNorm (StructureActor.py:131-134); feature / out: inputs / outputs per limb (41 / 3 for the actor,
 * 1 <= feature <= 64, 1 <= out <= 8). */
int sgrl_swat_bind_params(sgrl_swat* s, const void* const* ptrs, int n, int cond_decoder, int transformer_norm, int feature,
                          int out);

/* Batch structure (StructurePolicy.change_morphology for every morphology at once, reference StructureActor.py:266-273):
 *   n_morph, morph_L[n_morph] limbs (1 .. 15), morph_count[n_morph] envs per morphology (env blocks in this order),
 *   trav: HOST int32, per morphology 3*L traversal indices (pre, inlcrs, postlcrs), concatenated, each in [0, 15),
 *   rel:  HOST float, per morphology L*L*3 relation tensor (graph_dict['relation']), concatenated.
 * Structures are cached by CONTENT (up to SGRL_SWAT_GRAPH_CACHE): switching back to one seen before swaps pointers, with no
 * allocation, upload or device synchronisation.  The relation bias itself is computed inside every forward (rel_encoder is
 * trainable), never cached.  SGRL_ERR_ARG for a morphology of more than SGRL_SWAT_MAX_LIMBS limbs. */
int sgrl_swat_graph(sgrl_swat* s, int n_morph, const int32_t* morph_L, const int32_t* morph_count, const int32_t* trav,
                    const float* rel);
#define SGRL_SWAT_GRAPH_CACHE 64

/* act[e, out*l + j] = max_action * tanh(actor(obs[e, feature*l : feature*l + feature]))[l][j] for the limbs l of env e
 * (reference StructureActor.py:221-243), act[e, out*L_e : act_ld] = 0 exactly.  obs: DEV float [n_env, obs_ld]; act: DEV float
 * [n_env, act_ld].  SGRL_ERR_ARG unless obs_ld >= feature * Lmax and act_ld >= out * Lmax.  Asynchronous on `stream`. */
int sgrl_swat_forward(sgrl_swat* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, void* stream);

/* ---- critic networks and the TD3 target chain (inference under torch.no_grad(): reference src/agent.py:126-148) -------------
 * A CRITIC handle is bound with out = 1 and feature = 44 (one TransformerModel of reference src/StructureCritic.py:8-125,
 * CriticStructurePolicy.critic1 / .critic2).  The input row of limb l of environment e is
 *   [obs[e, (feature - act_feature) l : ...] | action[e, act_feature l : act_feature l + act_feature]]
 * (StructureCritic.py:96-112 concatenates them), read from the two buffers where they lie: no concatenated copy is made.
 * q[e, l] is the decoder output (no tanh), q[e, L_e : q_ld] = 0 exactly.  obs: DEV float [n_env, obs_ld]; action: DEV float
 * [n_env, act_ld]; q: DEV float [n_env, q_ld].  Same 22 launches as sgrl_swat_forward, asynchronous on `stream`, live
 * parameters, recordable into a hipGraph.  SGRL_ERR_ARG: a handle not bound as a critic (out != 1), act_feature outside
 * 1 .. feature - 1, obs_ld < (feature - act_feature) * Lmax, act_ld < act_feature * Lmax, q_ld < Lmax. */
int sgrl_swat_forward_q(sgrl_swat* s, const float* obs, int obs_ld, const float* action, int act_ld, int act_feature, float* q,
                        int q_ld, void* stream);

/* Twin critics (CriticStructurePolicy.forward): two handles holding the SAME batch structure (SGRL_ERR_ARG otherwise), one pair
 * of input buffers, q1 / q2 as sgrl_swat_forward_q of s1 / s2 -- bit for bit.  The two chains run side by side: s1's on
 * `stream`, s2's on a side stream owned by s1, forked from and joined back into `stream` by events (work queued on `stream`
 * after the call sees both results).  The side stream is created by the first twin call of a handle: make that call outside
 * any stream capture. */
int sgrl_swat_forward_twin(sgrl_swat* s1, sgrl_swat* s2, const float* obs, int obs_ld, const float* action, int act_ld,
                           int act_feature, float* q1, float* q2, int q_ld, void* stream);

/* The no-grad half of a TD3 update in one call (reference src/agent.py:126-148) over the three TARGET networks, all holding the
 * same batch structure:
 *   a'          = clamp(actor_t(next_obs) + clamp(noise, +-noise_clip), +-max_action)      in the actor's tail kernel
 *   target_q[e, l] = reward[e] + (1 - done[e]) * discount * min(Q1_t, Q2_t)(next_obs, a')[e, l]   in the first critic's tail kernel
 * with target_q[e, L_e : q_ld] = 0.  noise: DEV float [n_env, noise_ld], laid out like an action row (the caller's N(0,
 * policy_noise) draw, unclipped); reward, done: DEV float [n_env].  a' and the Q values stay in the handles' workspaces.
 * SGRL_ERR_ARG as above, and unless the critics' feature = the actor's feature + out. */
int sgrl_swat_td_target(sgrl_swat* actor_t, sgrl_swat* q1_t, sgrl_swat* q2_t, const float* next_obs, int obs_ld, const float* noise,
                        int noise_ld, const float* reward, const float* done, float max_action, float noise_clip, float discount,
                        float* target_q, int q_ld, void* stream);

/* Launches of one sgrl_swat_forward_twin (2 x 22, on two streams) and of one sgrl_swat_td_target (3 x 22). */
int sgrl_swat_twin_launches(void);
int sgrl_swat_td_target_launches(void);

/* ---- networks in TRAINING mode: counter-RNG dropout inside the forwards (reference src/agent.py:118-121 puts all four networks
 * into training mode for an update, so the three target networks of a TD3 update drop) ----------------------------------------
 * The three entries below are sgrl_swat_forward / _forward_q / _td_target with the masks of include/sgrl_train.h "counter-RNG
 * dropout" (csrc/dropout_rng.h, nothing else) applied inside the row kernels:
 *   word = replay_word(seed, *step_dev, 0x100 + site, i),  keep = word >= floor(p * 2^32),  y = keep ? x * (1 / (1 - p)) : 0
 * step_dev: DEV uint64, read by the kernels (the host never learns it: a recorded call moves with the device word).  One network
 * has sgrl_swat_dropout_sites() = 13 sites, numbered in the program order of swat_policy.TransformerModel.forward; i is the
 * row-major index in the tensor the module drops (B environments of L limbs, node n = b L + l):
 *   site 0        pos_encoder output [L, 128]            i = 128 l + c                  on pos before it is added (ONE mask for
 *                                                                                         every environment, as the module's)
 *   site 1 + 4k   softmax weights of layer k [B, 2, L, L]  i = ((2 b + h) L + i) L + j    after normalisation, before the w . v sum
 *   site 2 + 4k   dropout1: out_proj output [B, L, 128]   i = 128 n + c                  before the residual sum of norm1
 *   site 3 + 4k   dropout: relu(linear1) [B, L, 256]      i = 256 n + c                  one element-wise launch between the products
 *   site 4 + 4k   dropout2: linear2 output [B, L, 128]    i = 128 n + c                  before the residual sum of norm2
 * A single network uses sites site0 .. site0 + 12.  site_map (tests; NULL = the identity): HOST int32[13], site k of the network
 * becomes site0 + site_map[k].  25 launches per network (sgrl_swat_dropout_launches), the plain entries keep their 22.
 * A row whose weights are all dropped gives exact zeros; p = 0 gives the plain entry's bits; p = 1 drops everything and stays
 * finite.  Recordable into a hipGraph under the plain entries' rule (a handle's first calls are made outside a capture).
 * SGRL_ERR_ARG, nothing launched: everything the plain entry refuses; p outside [0, 1] or NaN; step_dev null; site0 < 0 or a
 * last site beyond 2^24 - 1; a batch structure of more than one morphology (the indices above are the modules' only then: an
 * update batch is one morphology). */
int sgrl_swat_forward_dropout(sgrl_swat* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, float p,
                              uint64_t seed, const uint64_t* step_dev, int site0, const int32_t* site_map, void* stream);
int sgrl_swat_forward_q_dropout(sgrl_swat* s, const float* obs, int obs_ld, const float* action, int act_ld, int act_feature, float* q,
                                int q_ld, float p, uint64_t seed, const uint64_t* step_dev, int site0, const int32_t* site_map,
                                void* stream);
/* The chain takes 39 sites, in the order Agent.update_targets runs the modules (critic1 before critic2 in
 * CriticStructurePolicy.forward): the target actor site0 .. + 12, the first critic site0 + 13 .. + 25, the second critic
 * site0 + 26 .. + 38.  The second critic still runs on the first handle's side stream; the noise, clamp, min and Bellman
 * epilogues are those of sgrl_swat_td_target.  75 launches (sgrl_swat_td_target_dropout_launches). */
int sgrl_swat_td_target_dropout(sgrl_swat* actor_t, sgrl_swat* q1_t, sgrl_swat* q2_t, const float* next_obs, int obs_ld,
                                const float* noise, int noise_ld, const float* reward, const float* done, float max_action,
                                float noise_clip, float discount, float* target_q, int q_ld, float p, uint64_t seed,
                                const uint64_t* step_dev, int site0, void* stream);
int sgrl_swat_dropout_sites(void);
int sgrl_swat_dropout_launches(void);
int sgrl_swat_td_target_dropout_launches(void);
/* Measurements only (process-wide): 0 = the twin's second chain follows the first on the caller's stream; 1 (default) = side stream. */
int sgrl_swat_debug_twin_streams(int on);

/* Nodes / environments of the current batch structure; launches per forward (constant). */
int sgrl_swat_num_nodes(const sgrl_swat* s);
int sgrl_swat_launches(void);
/* Counter bumped whenever the handle FREES device memory a captured forward may point into (an evicted batch structure, a
 * regrown workspace): a hipGraph holding forwards of this handle must be captured again once it has changed. */
int64_t sgrl_swat_generation(const sgrl_swat* s);
const char* sgrl_swat_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SGRL_SWAT_H */
