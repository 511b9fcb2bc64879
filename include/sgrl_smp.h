/* sgrl_smp.h -- C ABI of the SMP (shared modular policies) actor forward in libsgrl_hip.so.
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

#ifdef __cplusplus
}
#endif
#endif /* SGRL_SMP_H */
