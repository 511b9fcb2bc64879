/* sgrl_smp.h -- C ABI of the SMP (shared modular policies) actor and critic forwards in libsgrl_hip.so.
 *
 * Replaces, for inference under torch.no_grad(), the chain
 *   Agent.select_action                    reference src/agent.py:189-198
 *   -> ActorGraphPolicy.forward            reference src/ModularActor.py:99-384 (the disable_fold path, bottom-up AND top-down)
 *   -> ActorUp / ActorDownAction.forward   reference src/ModularActor.py:12-96
 * for a whole batch of environments of mixed morphologies in one call (environment blocks per morphology, the limbs of one
 * environment contiguous in its observation / action row).  The work is scheduled by GLOBAL TREE LEVEL: level d of the batch is
 * the set of depth-d limbs of every environment of every morphology, and one set of launches serves it.  A forward of a batch
 * whose deepest tree has D levels is 6 * D launches, whatever the number of morphologies, environments or limbs; it never
 * synchronises with the host and can be recorded into a hipGraph.
 *
 * Shapes (sgrl_amd/smp_policy.py): message width 32, ActorUp 64 hidden units, MLPBase 400 / 300 hidden units, `feature` inputs
 * and `out` outputs per limb, `max_children` child slots per limb.
 */
#ifndef SGRL_SMP_H
#define SGRL_SMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgrl_smp sgrl_smp;

/* Parameter table of sgrl_smp_bind_params: one DEVICE address per tensor, contiguous float32 exactly as torch stores it
 * (nn.Linear weights [out, in] row-major).  The names are the state_dict keys of ActorGraphPolicy (the one shared module of each
 * kind is listed at index 0); mc = max_children. */
enum {
  SGRL_SMP_FC1_W = 0,   /* sNet.0.fc1.weight [64, feature] */
  SGRL_SMP_FC1_B,       /* sNet.0.fc1.bias [64] */
  SGRL_SMP_FC2_W,       /* sNet.0.fc2.weight [64, 64 + 32 * mc] */
  SGRL_SMP_FC2_B,       /* sNet.0.fc2.bias [64] */
  SGRL_SMP_FC3_W,       /* sNet.0.fc3.weight [32, 64] */
  SGRL_SMP_FC3_B,       /* sNet.0.fc3.bias [32] */
  SGRL_SMP_ACT1_W,      /* actor.0.action_base.l1.weight [400, 64] */
  SGRL_SMP_ACT1_B,      /* actor.0.action_base.l1.bias [400] */
  SGRL_SMP_ACT2_W,      /* actor.0.action_base.l2.weight [300, 400] */
  SGRL_SMP_ACT2_B,      /* actor.0.action_base.l2.bias [300] */
  SGRL_SMP_ACT3_W,      /* actor.0.action_base.l3.weight [out, 300] */
  SGRL_SMP_ACT3_B,      /* actor.0.action_base.l3.bias [out] */
  SGRL_SMP_MSG1_W,      /* actor.0.msg_base.l1.weight [400, 64] */
  SGRL_SMP_MSG1_B,      /* actor.0.msg_base.l1.bias [400] */
  SGRL_SMP_MSG2_W,      /* actor.0.msg_base.l2.weight [300, 400] */
  SGRL_SMP_MSG2_B,      /* actor.0.msg_base.l2.bias [300] */
  SGRL_SMP_MSG3_W,      /* actor.0.msg_base.l3.weight [32 * mc, 300] */
  SGRL_SMP_MSG3_B,      /* actor.0.msg_base.l3.bias [32 * mc] */
  SGRL_SMP_NW
};
#define SGRL_SMP_MAX_LIMBS 16
#define SGRL_SMP_MAX_LEVELS 16
#define SGRL_SMP_MAX_CHILDREN 8

/* reference ActorGraphPolicy.__init__ (ModularActor.py:102-115) builds the network; here: a handle with no weights and no batch
 * structure yet.  SGRL_ERR_HIP when no device is visible (there is no CPU fallback). */
int sgrl_smp_create(sgrl_smp** out);
void sgrl_smp_destroy(sgrl_smp* s);

/* Bind the network's parameters by address (reference agent.py:155-176 and common/functional.py:7-10 update the same tensors in
 * place: optimizer steps, soft updates, load_state_dict and in-place broadcasts therefore need no call).  The handle keeps only
 * the addresses and every forward reads the values behind them; re-bind after anything that MOVES a parameter (module.to(),
 * re-created tensors).  ptrs: HOST array of n = SGRL_SMP_NW DEVICE addresses in the slot order above, each 16-byte aligned.
 * max_children: child slots per limb (ModularActor.py:12-47, 1 .. 8); feature / out: inputs / outputs per limb (41 / 3 for the
 * actor, 1 <= feature <= 64, 1 <= out <= 8). */
int sgrl_smp_bind_params(sgrl_smp* s, const void* const* ptrs, int n, int max_children, int feature, int out);

/* Batch structure (ActorGraphPolicy.change_morphology for every morphology at once, reference ModularActor.py:283-326):
 *   n_morph, morph_L[n_morph] limbs (1 .. 16), morph_count[n_morph] envs per morphology (env blocks in this order),
 *   max_children: the width of the children rows below (must equal the bound parameters' at the time of a forward),
 *   tree: HOST int32, per morphology L rows of 3 + max_children entries, concatenated:
 *         level | parent (-1 at a root) | slot in the parent's outgoing message | children (limb indices, -1 = empty slot)
 *         exactly as sgrl_amd/smp_policy._Tree lays the morphology out (sgrl_amd/smp_hip.level_schedule): the library derives
 *         nothing about the tree itself, it only checks the rows for consistency and expands them over the environments.
 * Structures are cached by CONTENT (up to SGRL_SMP_GRAPH_CACHE): switching back to one seen before swaps pointers, with no
 * allocation, upload or device synchronisation.  SGRL_ERR_ARG for more than 16 limbs or 16 levels, and for rows that do not
 * describe a forest (a child that is not one level below its parent, a limb missing from its parent's children, ...). */
int sgrl_smp_graph(sgrl_smp* s, int n_morph, const int32_t* morph_L, const int32_t* morph_count, int max_children,
                   const int32_t* tree);
#define SGRL_SMP_GRAPH_CACHE 64

/* act[e, out*l + j] = max_action * tanh(action_base(...))[l][j] for the limbs l of env e (reference ModularActor.py:240-326,
 * agent.py:189-198), act[e, out*L_e : act_ld] = 0 exactly.  obs: DEV float [n_env, obs_ld]; act: DEV float [n_env, act_ld].
 * SGRL_ERR_ARG unless obs_ld >= feature * Lmax and act_ld >= out * Lmax.  Asynchronous on `stream`. */
int sgrl_smp_forward(sgrl_smp* s, const float* obs, int obs_ld, float* act, int act_ld, float max_action, void* stream);

/* Nodes / tree levels of the current batch structure; launches of one forward of it (6 * levels). */
int sgrl_smp_num_nodes(const sgrl_smp* s);
int sgrl_smp_num_levels(const sgrl_smp* s);
int sgrl_smp_launches(const sgrl_smp* s);
/* Counter bumped whenever the handle FREES device memory a captured forward may point into (an evicted batch structure, a
 * regrown workspace): a hipGraph holding forwards of this handle must be captured again once it has changed. */
int64_t sgrl_smp_generation(const sgrl_smp* s);
const char* sgrl_smp_last_error(void);

/* ---- critic (reference src/ModularCritic.py, CriticGraphPolicy with bottom-up AND top-down messages) ---------------------------
 * The same handle type serves a CriticGraphPolicy once sgrl_smp_bind_critic_params has bound it: the level schedule, the
 * bottom-up pass and msg_base are the actor's (CriticUp.fc1 reads [obs | action] per limb from the two buffers where they lie);
 * the twin Q heads read the RAW (normalised, not tanh'd) [up 32 | action 3 | parent message slot 32] of every node and the
 * per-limb values are summed over the limbs of an environment in limb order.  A handle is an actor OR a critic: the last bind
 * decides, and the other kind's entry points return SGRL_ERR_ARG.
 *
 * Parameter table of sgrl_smp_bind_critic_params, the state_dict keys of CriticGraphPolicy (index 0 of the per-limb listing): */
enum {
  SGRL_SMPQ_FC1_W = 0,  /* sNet.0.fc1.weight [64, feature] */
  SGRL_SMPQ_FC1_B,      /* sNet.0.fc1.bias [64] */
  SGRL_SMPQ_FC2_W,      /* sNet.0.fc2.weight [64, 64 + 32 * mc] */
  SGRL_SMPQ_FC2_B,      /* sNet.0.fc2.bias [64] */
  SGRL_SMPQ_FC3_W,      /* sNet.0.fc3.weight [32, 64] */
  SGRL_SMPQ_FC3_B,      /* sNet.0.fc3.bias [32] */
  SGRL_SMPQ_Q1L1_W,     /* critic.0.baseQ1.l1.weight [400, 64 + act_feature] */
  SGRL_SMPQ_Q1L1_B,     /* critic.0.baseQ1.l1.bias [400] */
  SGRL_SMPQ_Q1L2_W,     /* critic.0.baseQ1.l2.weight [300, 400] */
  SGRL_SMPQ_Q1L2_B,     /* critic.0.baseQ1.l2.bias [300] */
  SGRL_SMPQ_Q1L3_W,     /* critic.0.baseQ1.l3.weight [1, 300] */
  SGRL_SMPQ_Q1L3_B,     /* critic.0.baseQ1.l3.bias [1] */
  SGRL_SMPQ_Q2L1_W,     /* critic.0.baseQ2.l1.weight [400, 64 + act_feature] */
  SGRL_SMPQ_Q2L1_B,     /* critic.0.baseQ2.l1.bias [400] */
  SGRL_SMPQ_Q2L2_W,     /* critic.0.baseQ2.l2.weight [300, 400] */
  SGRL_SMPQ_Q2L2_B,     /* critic.0.baseQ2.l2.bias [300] */
  SGRL_SMPQ_Q2L3_W,     /* critic.0.baseQ2.l3.weight [1, 300] */
  SGRL_SMPQ_Q2L3_B,     /* critic.0.baseQ2.l3.bias [1] */
  SGRL_SMPQ_MSG1_W,     /* critic.0.msg_base.l1.weight [400, 64] */
  SGRL_SMPQ_MSG1_B,     /* critic.0.msg_base.l1.bias [400] */
  SGRL_SMPQ_MSG2_W,     /* critic.0.msg_base.l2.weight [300, 400] */
  SGRL_SMPQ_MSG2_B,     /* critic.0.msg_base.l2.bias [300] */
  SGRL_SMPQ_MSG3_W,     /* critic.0.msg_base.l3.weight [32 * mc, 300] */
  SGRL_SMPQ_MSG3_B,     /* critic.0.msg_base.l3.bias [32 * mc] */
  SGRL_SMPQ_NW
};

/* As sgrl_smp_bind_params, for a critic: ptrs is a HOST array of n = SGRL_SMPQ_NW DEVICE addresses in the slot order above.
 * feature: inputs of CriticUp.fc1 per limb = observation + action (44), act_feature: the action's share of them (3);
 * 2 <= feature <= 64, 1 <= act_feature <= 8, act_feature < feature.  The 16-byte alignment is asked of the ADDRESSES only: the
 * 64 + act_feature = 67 wide rows of baseQ*.l1.weight are read element by element and never past their end. */
int sgrl_smp_bind_critic_params(sgrl_smp* s, const void* const* ptrs, int n, int max_children, int feature, int act_feature);

/* q1[e] / q2[e] = sum over the limbs l = 0 .. L_e - 1 (in this order) of baseQ1 / baseQ2 of limb l of env e (CriticGraphPolicy.forward,
 * reference ModularCritic.py:286-290); q2 == NULL: Q1 only (CriticGraphPolicy.Q1), q1 then equals the twin call's bit for bit.
 * obs: DEV float [n_env, obs_ld] (feature - act_feature per limb), action: DEV float [n_env, act_ld] (act_feature per limb),
 * q1 / q2: DEV float [n_env].  SGRL_ERR_ARG on a handle not bound as a critic, unless obs_ld >= (feature - act_feature) * Lmax
 * and act_ld >= act_feature * Lmax, and when the batch structure's max_children is not the bound parameters'.  Asynchronous on
 * `stream`, no host synchronisation, can be recorded into a hipGraph. */
int sgrl_smp_forward_q(sgrl_smp* s, const float* obs, int obs_ld, const float* action, int act_ld, float* q1, float* q2, void* stream);

/* The no-grad half of a TD3 update (reference src/agent.py:126-148) in one call on `stream`:
 *   a         = clamp(max_action * tanh(actor_t(next_obs)) + clamp(noise, +-noise_clip), +-max_action)   kept in critic_t's workspace
 *   target_q  = reward + (1 - done) * discount * min(Q1_t, Q2_t)(next_obs, a)                             DEV float [n_env]
 * actor_t: a handle bound by sgrl_smp_bind_params, critic_t: one bound by sgrl_smp_bind_critic_params; noise: DEV float
 * [n_env, noise_ld] laid out like an action row (the unclipped draw), reward / done: DEV float [n_env].  SGRL_ERR_ARG unless
 * both handles hold the SAME batch structure (same morphologies, counts and max_children), the critic's feature equals the
 * actor's feature + out and its act_feature the actor's out, obs_ld >= feature * Lmax and noise_ld >= out * Lmax. */
int sgrl_smp_td_target(sgrl_smp* actor_t, sgrl_smp* critic_t, const float* next_obs, int obs_ld, const float* noise, int noise_ld,
                       const float* reward, const float* done, float max_action, float noise_clip, float discount,
                       float* target_q, void* stream);

/* Launches of one sgrl_smp_forward_q of the handle's current batch structure: 6 * D + 2 + twin (D = tree levels of the deepest
 * morphology, twin = 1 for both heads, 0 for Q1 only): 1 embedding + 2 D bottom-up + 4 (D - 1) top-down + 1 staging of the two
 * l1 weights + 1 stacked l1 product + (1 + twin) l2 products + 1 l3 row kernel + 1 limb sum.  Of one sgrl_smp_td_target:
 * 6 * D (target actor) + 6 * D + 3 (twin critic) = 12 * D + 3.  Neither depends on morphologies, environments or limbs. */
int sgrl_smp_forward_q_launches(const sgrl_smp* s, int twin);
int sgrl_smp_td_target_launches(const sgrl_smp* s);

#ifdef __cplusplus
}
#endif
#endif /* SGRL_SMP_H */
