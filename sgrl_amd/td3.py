"""TD3 agent behind the reference's `Agent` surface (reference src/agent.py:20-215).

Same constructor argument (`args` namespace), attributes (`actor`, `actor_target`, `critic`, `critic_target`, the two
Adam optimizers), methods (`update`, `try_update_target_network`, `select_action`, `change_morphology`, `models2eval`,
`models2train`) and `state_dict()` keys as the reference, so a `save.pth` written by either side loads on the other
(sgrl_amd/snapshot.py).  The update is ordinary PyTorch-ROCm autograd through the differentiable path of
`SEPolicy` / `SECritic` (set_policy.py); everything evaluated under `torch.no_grad()` on the GPU -- the target action
and the twin target Q values (agent.py:126-148), `select_action` (agent.py:189-198) -- runs on the HIP kernels
(csrc/set_actor.hip), which read the parameters' live storage on every call and therefore follow the in-place Polyak
updates (`target_param.data.copy_`, common/functional.py:7-10).

Pinned by tests/golden/td3_update.npz, produced by executing the reference's own `Agent.update`
(tools/capture_golden_update.py)."""
import os
import types

import contextlib
import gc

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import train_ops
from .set_policy import SECritic, SEPolicy, default_args


def soft_update_network(source_network, target_network, tau):
    """target <- tau * source + (1 - tau) * target for every parameter (reference common/functional.py:7-10), written through
    `.data` like the reference does.  On the GPU the ~300 tensors of a network pair are updated by two multi-tensor launches
    instead of four small kernels per tensor (the per-tensor loop was 40 % of all launches of a TD3 update); per element the
    same two products and one sum (the second product inside the addition)."""
    with torch.no_grad():
        targets = [p.data for p in target_network.parameters()]
        sources = [p.data for p in source_network.parameters()]
        if _TABLE_OPT and targets and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and s.is_contiguous() and
                                          s.dtype == torch.float32 and s.device == t.device and s.numel() == t.numel()
                                          for t, s in zip(targets, sources)):
            import ctypes
            from . import train_ops
            dev = targets[0].device
            ent = _table("lerp", [(t.data_ptr(), s.data_ptr(), 0, 0, 0, t.numel()) for t, s in zip(targets, sources)], dev)
            if ent is not None:
                train_ops._call("sgrl_optim_lerp", ctypes.c_void_p(ent["dev_tab"].data_ptr()), ctypes.c_void_p(ent["dev_chunks"].data_ptr()),
                                ent["n_chunks"], float(tau), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
                _touched(list(target_network.parameters()))
                return
        if targets and targets[0].is_cuda:
            torch._foreach_mul_(targets, 1 - tau)
            torch._foreach_add_(targets, sources, alpha=tau)
        else:
            for t, l in zip(targets, sources):
                t.copy_(tau * l + (1 - tau) * t)


# False: the foreach chain (bit-compatible with torch.optim.Adam's multi-tensor path) instead of the fused kernel
_FUSED_ADAM = hasattr(torch, "_fused_adam_")
# Gradient clipping + Adam, and the soft target update, over a device TABLE of tensor addresses (csrc/train_gemm.hip k_opt_*,
# include/sgrl_train.h sgrl_optim_*): three launches and one instead of torch's ~50 multi-tensor launches of ~18 us per update.
_TABLE_OPT = True
_tables = {}          # key (kind, address tuple) -> dict(dev table, dev chunks, pinned copies, scratch): see _table()
_capture_owner = None  # whoever is capturing a hipGraph right now (GraphedUpdates: (id, morphology key, flag)); see release_tables()


def _touched(params):
    """A kernel of this library wrote these tensors through raw pointers: bump their version counters, as an in-place PyTorch
    operation would have, so that whoever fingerprints parameters (rollout.Rollout's held weight pack, autograd's saved-tensor
    checks) sees the write.  Host-side only: 12 us for 300 tensors."""
    torch.autograd.graph.increment_version(params)


def _optim_lib():
    """The library with the sgrl_optim_* entry points bound (train_ops._ABI binds every prototype of include/sgrl_train.h)."""
    from . import train_ops
    return train_ops._L()


_spare_pinned = {}    # (dtype, shape) -> pinned host tensors allocated OUTSIDE captures (hipHostMalloc is not permitted inside one)


def _stock_pinned(n=4):
    """Before a capture: every table size seen so far has at least n spare pinned buffers."""
    if torch.cuda.is_current_stream_capturing():
        return
    for (dt, shape), pool in _spare_pinned.items():
        while len(pool) < n:
            pool.append(torch.empty(shape, dtype=dt).pin_memory())


def _pinned_copy(t):
    """A pinned copy of the small CPU tensor t; during a capture from the stock (None when it is empty: the caller falls back)."""
    pool = _spare_pinned.setdefault((t.dtype, tuple(t.shape)), [])
    if torch.cuda.is_current_stream_capturing():
        if not pool:
            return None
        buf = pool.pop()
    else:
        buf = torch.empty(t.shape, dtype=t.dtype).pin_memory()
        _stock_pinned(4)
    buf.copy_(t)
    return buf


def _table(kind, rows, device):
    """Device copy of a tensor table (rows of six int64: five addresses and the element count) and its chunk list, cached by
    content.  The upload is a copy from PINNED host memory on the current stream: inside a hipGraph capture it becomes a memcpy
    node of the graph, so entries made during a capture are kept (with their host buffers) for as long as the process lives."""
    key = (kind, device.index, tuple(rows))
    ent = _tables.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ent is not None:
        if capturing:
            ent["captured"] = True                 # a graph now points at this entry's device buffers: kept while an owner lives
            ent["owners"].add(_capture_owner)
        elif not ent["eager_valid"]:               # made during a capture (its upload exists only as a node of that graph)
            ent["dev_tab"].copy_(ent["host_tab"], non_blocking=True)
            ent["dev_chunks"].copy_(ent["host_chunks"], non_blocking=True)
            ent["eager_valid"] = True
        return ent
    chunk = int(train_ops._L().sgrl_optim_chunk())
    chunks = [(i, o) for i, r in enumerate(rows) for o in range(0, r[5], chunk)]
    host_tab = _pinned_copy(torch.tensor(rows, dtype=torch.int64))
    host_chunks = _pinned_copy(torch.tensor(chunks, dtype=torch.int32))
    if host_tab is None or host_chunks is None:
        return None                                  # capturing with no pinned buffer in stock: the caller takes torch's path
    ent = {"host_tab": host_tab, "host_chunks": host_chunks, "n": len(rows), "n_chunks": len(chunks), "captured": capturing,
           "dev_tab": torch.empty_like(host_tab, device=device), "dev_chunks": torch.empty_like(host_chunks, device=device),
           "scratch": torch.zeros(1 + len(chunks), dtype=torch.float32, device=device), "eager_valid": not capturing,
           "owners": {_capture_owner} if capturing else set()}
    ent["dev_tab"].copy_(host_tab, non_blocking=True)
    ent["dev_chunks"].copy_(host_chunks, non_blocking=True)
    if not capturing and len(_tables) > 64:          # eager callers whose gradient addresses keep changing: bounded cache
        for k in [k for k, v in _tables.items() if not v["captured"]][:32]:
            del _tables[k]
    _tables[key] = ent
    return ent


def release_tables(owner):
    """The graph(s) captured under `owner` are gone (GraphedUpdates dropped them to capture again): table entries that only they
    pointed at become ordinary cache entries again -- evictable -- instead of living as long as the process."""
    for ent in _tables.values():
        if owner in ent["owners"]:
            ent["owners"].discard(owner)
            if not ent["owners"]:
                ent["captured"] = False


def clip_and_step(opt, max_norm):
    """torch.nn.utils.clip_grad_norm_(params, max_norm) (max_norm > 0) followed by opt.step() for a capturable torch.optim.Adam
    (reference agent.py:161-164, 174-177) on the optimizer's OWN state tensors -- as three launches over a table of the tensors'
    addresses where everything is float32 on one GPU, through clip_grad_norm_ + adam_step otherwise."""
    params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    ok = _TABLE_OPT and len(opt.param_groups) == 1 and params and all(
        p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous() and p.grad.dtype == torch.float32
        and p.grad.device == p.device for p in params)
    group = opt.param_groups[0]
    ok = ok and group.get("capturable", False) and group.get("weight_decay", 0) == 0 and not group.get("amsgrad", False) and \
        not group.get("maximize", False)
    if not ok:
        if max_norm and max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], max_norm)
        return adam_step(opt)
    host = opt.__dict__.setdefault("_sgrl_step_class", {})
    rows = []
    for p in params:
        st = opt.state[p]
        if len(st) == 0:            # torch.optim.Adam's lazy state initialisation (capturable: the counter lives on the device)
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            host[id(p)] = 0
        elif id(p) not in host:
            host[id(p)] = int(st["step"].item())
        host[id(p)] += 1
        rows.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(), p.numel()))
    dev = params[0].device
    ent = _table("adam", rows, dev)
    if ent is None:
        for p in params:
            host[id(p)] -= 1                        # adam_step counts the step itself
        if max_norm and max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], max_norm)
        return adam_step(opt)
    import ctypes
    from . import train_ops
    beta1, beta2 = group["betas"]
    lr = group["lr"]
    train_ops._call("sgrl_optim_clip_adam", ctypes.c_void_p(ent["dev_tab"].data_ptr()), ent["n"], ctypes.c_void_p(ent["dev_chunks"].data_ptr()),
                    ent["n_chunks"], float(lr), float(beta1), float(beta2), float(group["eps"]),
                    float(max_norm) if (max_norm and max_norm > 0) else 0.0, ctypes.c_void_p(ent["scratch"].data_ptr()),
                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _touched(params)


def adam_step(opt):
    """`opt.step()` for a torch.optim.Adam whose groups are `capturable` (step counters on the device: GraphedUpdates), on the
    optimizer's OWN state tensors (state_dict unchanged).  torch's capturable multi-tensor path divides every parameter's
    tensors by per-parameter 0-dim bias-correction tensors, which its foreach kernels cannot batch: ~3 small launches per
    parameter, ~900 per TD3 update, a third of the update's launches.  Parameters that have always been stepped together share
    one step count, so here the two bias corrections are computed ONCE per such class (from its first counter; the classes
    are kept on the host: a parameter that skipped a step -- no gradient -- forms its own) and applied as single scalar
    tensors: a dozen multi-tensor launches per optimizer.  Same formula, term for term, as torch.optim.Adam (no weight decay,
    no amsgrad, not maximising -- the reference's optimizers, agent.py:96-115)."""
    for group in opt.param_groups:
        if not group.get("capturable", False) or group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or \
                group.get("maximize", False):
            return opt.step()
    host = opt.__dict__.setdefault("_sgrl_step_class", {})       # id(param) -> number of steps taken, as far as the host knows
    for group in opt.param_groups:
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            continue
        beta1, beta2 = group["betas"]
        classes = {}
        for p in params:
            st = opt.state[p]
            if len(st) == 0:        # torch.optim.Adam's lazy state initialisation (capturable: the counter lives on the device)
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                host[id(p)] = 0
            elif id(p) not in host:  # state loaded from a checkpoint: read the counter once (never during a capture)
                host[id(p)] = int(st["step"].item())
            classes.setdefault(host[id(p)], []).append(p)
            host[id(p)] += 1
        with torch.no_grad():
            for members in classes.values():
                grads = [p.grad for p in members]
                steps = [opt.state[p]["step"] for p in members]
                exp_avgs = [opt.state[p]["exp_avg"] for p in members]
                exp_avg_sqs = [opt.state[p]["exp_avg_sq"] for p in members]
                torch._foreach_add_(steps, 1)
                if _FUSED_ADAM and members[0].is_cuda:
                    # the whole update of the class in one multi-tensor kernel (torch's own `fused=True` Adam kernel: per-
                    # parameter step counters are read on the device, so nothing here divides by 0-dim tensors): three launches
                    # instead of a dozen per class.  Same formula; its float32 operation order differs from the foreach chain
                    # below in the last bit (tests/test_td3_update.py holds both to the reference's Agent.update).
                    torch._fused_adam_([p.data for p in members], grads, exp_avgs, exp_avg_sqs, [], steps, amsgrad=False,
                                       lr=group["lr"], beta1=beta1, beta2=beta2, weight_decay=0.0, eps=group["eps"],
                                       maximize=False, grad_scale=None, found_inf=None)
                    continue
                torch._foreach_lerp_(exp_avgs, grads, 1 - beta1)
                torch._foreach_mul_(exp_avg_sqs, beta2)
                torch._foreach_addcmul_(exp_avg_sqs, grads, grads, 1 - beta2)
                step = steps[0]
                neg_step_size = (group["lr"] / (1 - beta1 ** step)).neg()
                bias_correction2_sqrt = (1 - beta2 ** step).sqrt()
                denom = torch._foreach_sqrt(exp_avg_sqs)
                torch._foreach_div_(denom, bias_correction2_sqrt)
                torch._foreach_add_(denom, group["eps"])
                torch._foreach_div_(denom, neg_step_size)
                torch._foreach_addcdiv_([p.data for p in members], exp_avgs, denom)


_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay")


def optimizer_state(opt):
    """What checkpoint.save_checkpoint keeps of a torch.optim.Adam with ONE group: the group's hyper-parameters and, per parameter
    in the group's order (= `parameters()` order), None where it has no state yet or its `step` as a VALUE (a float, wherever the
    counter lives) with CPU copies of the moment tensors.  Plain values and tensors only (torch.load(weights_only=True))."""
    if len(opt.param_groups) != 1:
        raise ValueError("optimizer_state serves optimizers with one parameter group (got %d)" % len(opt.param_groups))
    g = opt.param_groups[0]
    if isinstance(g["lr"], torch.Tensor):
        raise ValueError("optimizer_state does not serve a tensor learning rate")
    group = {"lr": float(g["lr"]), "betas": [float(b) for b in g["betas"]], "eps": float(g["eps"]),
             "weight_decay": float(g.get("weight_decay", 0))}
    states = []
    for p in g["params"]:
        st = opt.state.get(p)
        if not st:
            states.append(None)
            continue
        states.append({k: (float(v) if k == "step" else v.detach().cpu().clone()) for k, v in st.items()})
    return {"group": group, "state": states}


def restore_optimizer(opt, saved):
    """`optimizer_state(...)`'s record back into `opt`, IN PLACE: no tensor that exists before the call changes its data_ptr(), so
    the address tables of clip_and_step, the binds of mlp_hip.HipMlpOptim and captured hipGraphs stay valid.
      state on both sides   copy_ / fill_ into the optimizer's own tensors (device and dtype stay as the optimizer has them; a step
                            count is a value, whether it lives in a 0-dim CPU tensor or on the device)
      only in `saved`       created in the form the group asks for: a capturable (or fused) group gets a device step tensor, as
                            clip_and_step creates it, a plain group the 0-dim CPU tensor torch.optim.Adam creates
      only in `opt`         deleted: the saved run had not stepped this parameter yet
    Then every host mirror of a step count is dropped (`_sgrl_step_class`; a mirror left behind would give Adam a wrong bias
    correction without any error): a plain group keeps none, a group with device counters gets a new one holding the restored
    counts.  A live mlp_hip.HipMlpOptim keeps mirrors of its own: call its resync() afterwards (Agent.load_resume_state does).
    Returns True when state was DELETED: the tensors a captured GraphedUpdates graph steps are then gone
    (GraphedUpdates.forget_graphs)."""
    if len(opt.param_groups) != 1:
        raise ValueError("restore_optimizer serves optimizers with one parameter group (got %d)" % len(opt.param_groups))
    g = opt.param_groups[0]
    params = g["params"]
    if len(saved["state"]) != len(params):
        raise ValueError("restore_optimizer: the record holds %d parameters, the optimizer %d" % (len(saved["state"]), len(params)))
    for p, s in zip(params, saved["state"]):
        for k, v in (s or {}).items():
            if k != "step" and tuple(v.shape) != tuple(p.shape):
                raise ValueError("restore_optimizer: %s of shape %s for a parameter of shape %s" % (k, tuple(v.shape), tuple(p.shape)))
    for k in _GROUP_KEYS:
        if k in saved["group"]:
            g[k] = tuple(saved["group"][k]) if k == "betas" else saved["group"][k]
    on_device = bool(g.get("capturable", False) or g.get("fused", False))
    deleted = False
    with torch.no_grad():
        for p, s in zip(params, saved["state"]):
            if s is None:
                if opt.state.get(p):
                    del opt.state[p]
                    deleted = True
                continue
            st = opt.state[p]
            for k, v in s.items():
                if k == "step":
                    if not torch.is_tensor(st.get(k)):
                        st[k] = torch.zeros((), dtype=torch.float32, device=p.device) if on_device else torch.tensor(0.0, dtype=torch.float32)
                    st[k].fill_(float(v))
                else:
                    if not torch.is_tensor(st.get(k)):
                        st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st[k].copy_(v)
    opt.__dict__.pop("_sgrl_step_class", None)
    if on_device:
        # device counters: the mirror is made again from the counts just written, here, where nothing is being captured -- left
        # absent, the next clip_and_step would read every counter back with .item(), which a stream capture does not permit
        opt.__dict__["_sgrl_step_class"] = {id(p): int(s["step"]) for p, s in zip(params, saved["state"]) if s is not None}
    return deleted


def default_train_args(**over):
    """The reference's TD3 / SET hyper-parameters (reference arguments.py:55-160, configs/default.py:9-12).

    Two batch sizes, as in the reference: `agent_batch_size` = 256 is what an update SAMPLES (configs/default.py:61 "trainer":
    {"agent_batch_size": 256}, passed as **args['trainer'] at main.py:164-171, read at trainer.py:289-291
    `self.env_buffer[name].sample(self.agent_batch_size)`); `batch_size` = 100 (arguments.py:66-68 --batch_size) only reaches the
    policies' constructor argument, which none of them uses (agent.py:42)."""
    a = default_args()
    a.agent_batch_size = 256
    a.actor_type = a.critic_type = "set"
    a.limb_obs_size, a.limb_action_size = 41, 3
    a.msg_dim, a.batch_size, a.max_action, a.max_children = 32, 100, 1.0, 3
    a.disable_fold, a.td, a.bu = True, False, False
    a.lr, a.discount, a.policy_noise, a.noise_clip, a.policy_freq = 1e-4, 0.99, 0.2, 0.5, 2
    a.expl_noise, a.grad_clipping_value, a.max_episode_steps = 0.126, 0.1, 1000
    # policy_network / q_network (configs/default.py:13-28) and mlp_num_limbs are read by the 'mlp' types only (mlp_policy.py)
    a.agent = types.SimpleNamespace(target_smoothing_tau=0.005, reward_scale=1.0, policy_network={"hidden_dims": [256, 256]},
                                    q_network={"hidden_dims": [256, 256]})
    a.mlp_num_limbs = None
    for k, v in over.items():
        setattr(a, k, v)
    return a


# Whether an mlp + mlp agent on the GPU takes the HIP gradient half (mlp_hip.HipMlpGrads) when the caller does not say: decided by
# tools/mlp_update_bench.py (profiles/mlp_update_bench.json)
MLP_HIP_GRADS_DEFAULT = True
# Whether such an agent also takes the HIP optimizer half (mlp_hip.HipMlpOptim: clip, Adam and the soft update of a network in two
# launches) when the caller does not say: opt-in (tools/mlp_optim_bench.py, profiles/mlp_optim_bench.json)
MLP_HIP_OPTIM_DEFAULT = False
# Whether a swat + swat agent on the GPU runs the differentiable passes of its update (both critics' forward and backward, the actor
# loss through critic.Q1(actor(obs))) on the training kernels of train_ops (swat_policy `train_kernels`) when the caller does not say:
# opt-in until a SWAT learning curve has been re-run with it (tools/swat_update_bench.py)
SWAT_TRAIN_KERNELS_DEFAULT = False
# The same for an smp + smp agent in its published mode (td and bu; smp_policy `train_kernels`): opt-in, no SMP learning curve has
# been run with it (tools/smp_update_bench.py)
SMP_TRAIN_KERNELS_DEFAULT = False
# Whether a set, swat or smp agent on the GPU computes its two losses and their gradients with the loss kernels (train_ops.twin_mse /
# neg_mean: one launch each way instead of about a dozen; float64 sums, so the last bit of a loss may differ from PyTorch's) when the
# caller does not say: opt-in, no learning curve has been run with it
LOSS_KERNELS_DEFAULT = False
# Whether a set + set agent on the GPU runs the no-grad target chain of its update as ONE library call over the target modules' HIP
# handles (set_hip.HipSetTargets, include/sgrl_set.h sgrl_set_td_target: the three forwards' launches and nothing else) when the
# caller does not say: opt-in (no update-time table yet).  Takes effect where the target critics' no-grad forward is two
# passes of the rollout kernels (set_policy.TWIN_TARGETS = False); with the default twin pass the chain yields (Agent._hip_targets)
SET_HIP_TARGETS_DEFAULT = False
# Whether a swat + swat agent with dropout_rate > 0 runs the target chain of an update -- whose three networks are then in training
# mode, as the reference's are -- on the HIP chain's dropout entries (swat_hip.HipSwatTargets.target_q(dropout=...),
# include/sgrl_swat.h sgrl_swat_td_target_dropout: 75 launches) instead of the modules under torch.no_grad() with the torch
# restatement of the counter RNG, when the caller does not say: opt-in (profiles/swat_dropout_chain.json).  The masks are
# the same function of (seed, step, site, index) either way; the values differ by float32 rounding
SWAT_HIP_DROPOUT_DEFAULT = False


def _switch(args, name, given):
    """The value of the Agent switch `name`: the constructor's keyword, else args.<name>, else the constant <NAME>_DEFAULT above as
    it stands NOW (read from the module on every call)."""
    if given is None:
        given = getattr(args, name, None)
    return globals()[name.upper() + "_DEFAULT"] if given is None else given


# agent kind -> (module of this package, class) of its HIP target chain; imported by Agent._hip_targets when a chain is first wanted
_TARGET_CHAINS = {"set": ("set_hip", "HipSetTargets"), "swat": ("swat_hip", "HipSwatTargets"), "smp": ("smp_hip", "HipSmpTargets"),
                  "mlp": ("mlp_hip", "HipMlpTargets")}


class Agent(nn.Module):
    def __init__(self, args, device=None, use_hip=True, mlp_hip_grads=None, mlp_hip_optim=None, swat_train_kernels=None,
                 smp_train_kernels=None, loss_kernels=None, set_hip_targets=None, swat_hip_dropout=None):
        super().__init__()
        self.args = args
        atype, ctype = getattr(args, "actor_type", "set"), getattr(args, "critic_type", "set")
        if atype not in ("set", "swat", "smp", "mlp") or ctype not in ("set", "swat", "smp", "mlp"):
            raise NotImplementedError("actor / critic types 'set', 'swat', 'smp' and 'mlp' are built (the actors with a batched HIP forward for "
                                      "collection, smp in its td and bu mode; the target chain of a swat, an smp (td and bu) or an mlp update on HIP, "
                                      "that of a set update as one call over the HIP forwards where `set_hip_targets` says so, "
                                      "the differentiable passes of those updates on the training kernels where `swat_train_kernels` / "
                                      "`smp_train_kernels` / `mlp_hip_grads` say so, in PyTorch otherwise); got actor_type %r, critic_type %r"
                                      % (atype, ctype))
        if (atype == "mlp") != (ctype == "mlp"):
            raise NotImplementedError("an 'mlp' actor goes with an 'mlp' critic only (got actor_type %r, critic_type %r): the monolithic "
                                      "networks read rows of the last training morphology's own length (reference main.py:118-120), the graph "
                                      "types rows padded to the widest morphology" % (atype, ctype))
        self.networks = {}
        from .smp_policy import ActorGraphPolicy, CriticGraphPolicy
        from .swat_policy import CriticStructurePolicy, StructurePolicy
        from .mlp_policy import MlpCritic, MlpPolicy

        def actor():
            if atype == "mlp":
                return MlpPolicy(args.limb_obs_size, args.limb_action_size, args.msg_dim, args.batch_size, args.max_action,
                                 args.max_children, args.disable_fold, args.td, args.bu, args, device=device)
            if atype == "swat":
                return StructurePolicy(args.limb_obs_size, args.limb_action_size, args.msg_dim, args.batch_size, args.max_action,
                                       args.max_children, args.disable_fold, args.td, args.bu, args, device=device)
            if atype == "smp":
                return ActorGraphPolicy(args.limb_obs_size, args.limb_action_size, args.msg_dim, args.batch_size, args.max_action,
                                        args.max_children, args.disable_fold, args.td, args.bu, args, device=device)
            return SEPolicy(args.limb_obs_size, args.limb_action_size, args.msg_dim, args.batch_size, args.max_action,
                            args.max_children, args.disable_fold, args.td, args.bu, args, device=device, use_hip=use_hip)

        def critic():
            if ctype == "mlp":
                return MlpCritic(args.limb_obs_size, args.limb_action_size, args.msg_dim, args.batch_size, args.max_children,
                                 args.disable_fold, args.td, args.bu, args, device=device)
            if ctype == "swat":
                return CriticStructurePolicy(args.limb_obs_size, args.limb_action_size, args.msg_dim, args.batch_size,
                                             args.max_children, args.disable_fold, args.td, args.bu, args, device=device)
            if ctype == "smp":
                return CriticGraphPolicy(args.limb_obs_size, args.limb_action_size, args.msg_dim, args.batch_size,
                                         args.max_children, args.disable_fold, args.td, args.bu, args, device=device)
            return SECritic(args.limb_obs_size, args.limb_action_size, args.msg_dim, args.batch_size, args.max_children,
                            args.disable_fold, args.td, args.bu, args, device=device, use_hip=use_hip)
        self.actor, self.actor_target = actor(), actor()
        self.critic, self.critic_target = critic(), critic()
        soft_update_network(self.actor, self.actor_target, 1.0)
        soft_update_network(self.critic, self.critic_target, 1.0)
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=args.lr)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr=args.lr)
        self.models2eval()
        self.tot_update_count = 0
        self.target_smoothing_tau = args.agent.target_smoothing_tau
        self.reward_scale = args.agent.reward_scale
        # Which HIP paths this agent takes.  Every switch (the *_DEFAULT constants above say what each one does) is the keyword, else
        # args.<name>, else its constant (_switch), and follows use_hip; agent kinds it is not for ignore it.
        # The no-grad target chain of an update runs on HIP for a swat + swat, an smp + smp (td and bu; the td-only mode stays PyTorch)
        # and an mlp + mlp agent, and for a set + set agent that asks for it: ONE chain object (_TARGET_CHAINS), made by the first update
        # on a float32 CUDA batch (_hip_targets); anything else keeps the PyTorch chain of update_targets
        hip = bool(use_hip)
        self.use_swat_hip = hip and atype == "swat" and ctype == "swat"
        self.use_smp_hip = hip and atype == "smp" and ctype == "smp" and bool(args.td) and bool(args.bu)
        self.use_mlp_hip = hip and atype == "mlp" and ctype == "mlp"
        self.use_set_hip = hip and atype == "set" and ctype == "set" and bool(_switch(args, "set_hip_targets", set_hip_targets))
        self._targets = None
        # SWAT_ / SMP_TRAIN_KERNELS_DEFAULT: the ONLINE actor and critic differentiate on the training kernels; the smp switch is applied after the swat one, which leaves
        # every switch of a non-swat agent off
        self.set_swat_train_kernels(self.use_swat_hip and bool(_switch(args, "swat_train_kernels", swat_train_kernels)))
        self.set_smp_train_kernels(_switch(args, "smp_train_kernels", smp_train_kernels))
        # MLP_HIP_GRADS_ / MLP_HIP_OPTIM_DEFAULT: the two halves of an mlp + mlp update after the target chain: float32 batches on the GPU;
        # the optimizer half only together with the gradient half
        self.use_mlp_hip_grads = self.use_mlp_hip and bool(_switch(args, "mlp_hip_grads", mlp_hip_grads))
        self._mlp_grads = None
        self.use_mlp_hip_optim = self.use_mlp_hip_grads and bool(_switch(args, "mlp_hip_optim", mlp_hip_optim))
        self._mlp_optim = None
        # LOSS_KERNELS_DEFAULT: an mlp agent ignores it (its gradient half has losses of its own).  An Agent switch, not one of GraphedUpdates: an eager and a
        # graphed agent with the same switches run the same arithmetic
        self.use_loss_kernels = hip and atype != "mlp" and bool(_switch(args, "loss_kernels", loss_kernels))
        # dropout_rate: read by the swat networks only (the reference forces the SET networks to 0, SEActor.py:185; smp and mlp have
        # none).  With a rate > 0 every update() runs inside a train_ops.dropout_rng context: seed = args.seed (0 when absent), step =
        # a one-element int64 tensor on the batch's device, created by the first update and incremented once at the top of each one,
        # on the update's stream.  A plain attribute: no parameter, no buffer, not in state_dict() -- a reference-format snapshot does
        # not hold it, a checkpoint (checkpoint.py, resume_state / load_resume_state) carries its value
        self.dropout_rate = float(getattr(args, "dropout_rate", 0.0) or 0.0) if "swat" in (atype, ctype) else 0.0
        self.dropout_seed = int(getattr(args, "seed", 0) or 0)
        self._dropout_step = None
        # SWAT_HIP_DROPOUT_DEFAULT; off: a chain with the targets in training mode runs the modules (_target_kind returns None)
        self.swat_hip_dropout = self.use_swat_hip and bool(_switch(args, "swat_hip_dropout", swat_hip_dropout))

    def set_swat_train_kernels(self, on):
        """Turn the training kernels of the online swat networks on or off (no other agent type has the switch)."""
        self.use_swat_train_kernels = bool(on) and getattr(self.args, "actor_type", "set") == "swat" and \
            getattr(self.args, "critic_type", "set") == "swat"
        for net in (self.actor, self.critic):
            if hasattr(type(net), "train_kernels"):
                net.train_kernels = self.use_swat_train_kernels

    def set_smp_train_kernels(self, on):
        """Turn the training kernels of the online smp networks on or off: only an smp + smp agent with the HIP target chain (td and
        bu, use_hip) has them; the targets stay off."""
        from .smp_policy import _GraphModule
        self.use_smp_train_kernels = bool(on) and bool(self.use_smp_hip)
        for net in (self.actor, self.critic):
            if isinstance(net, _GraphModule):
                net.train_kernels = self.use_smp_train_kernels

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_targets"] = d["_mlp_grads"] = d["_mlp_optim"] = None     # per-process device handles: never pickled / deep-copied with the agent
        return d

    def _hip_grads(self, data_batch):
        """mlp_hip.HipMlpGrads when this update's gradient half runs on HIP, else None.  Widths the kernels do not serve
        (sgrl_mlp_train_plan refuses them, with a message kept in `mlp_hip_grads_refusal`) keep the PyTorch gradient half."""
        obs = data_batch["obs"]
        if not (self.use_mlp_hip_grads and obs.is_cuda and obs.dtype == torch.float32 and self.device.type == "cuda"):
            return None
        g = self._mlp_grads
        if g is None or g.actor.policy is not self.actor or g.critic.module is not self.critic:
            from . import _lib, mlp_hip             # raises SgrlError when the extension is missing (no fallback)
            _lib.lib()
            try:
                mlp_hip.train_plan(mlp_hip.net_dims(self.actor.actor), mlp_hip.net_dims(self.critic.critic1), obs.shape[0])
            except _lib.SgrlError as e:
                self.use_mlp_hip_grads, self.mlp_hip_grads_refusal = False, str(e)
                return None
            g = self._mlp_grads = mlp_hip.HipMlpGrads(self.actor, self.critic)
        return g

    def _hip_optim(self, grads):
        """mlp_hip.HipMlpOptim over `grads` when this update's optimizer half runs on HIP, else None: off unless asked for
        (`mlp_hip_optim`), and optimizers it does not serve (weight decay, amsgrad, maximize, more than one group; the reason is kept
        in `mlp_hip_optim_refusal`) or a tau outside [0, 1] keep clip_and_step and soft_update_network."""
        if not self.use_mlp_hip_optim:
            return None
        from .mlp_hip import HipMlpOptim
        o = self._mlp_optim
        if o is None or o.grads is not grads or o.actor_optimizer is not self.actor_optimizer or o.critic_optimizer is not self.critic_optimizer \
                or o.actor_target is not self.actor_target or o.critic_target is not self.critic_target:
            o = self._mlp_optim = None
        why = HipMlpOptim.refusal(self.actor_optimizer, grads.actor._params() if o is None else None) or \
            HipMlpOptim.refusal(self.critic_optimizer, grads.critic._params() if o is None else None)
        if why is None and not 0.0 <= float(self.target_smoothing_tau) <= 1.0:
            why = "target_smoothing_tau outside [0, 1]"
        self.mlp_hip_optim_refusal = why
        if why is not None:
            return None
        if o is None:
            o = self._mlp_optim = HipMlpOptim(grads, self.actor_optimizer, self.critic_optimizer, self.actor_target, self.critic_target)
        return o

    def _target_kind(self, next_obs):
        """Which HIP target chain serves this update's batch -- a key of _TARGET_CHAINS -- or None: the modules run."""
        if not ((self.use_swat_hip or self.use_smp_hip or self.use_mlp_hip or self.use_set_hip) and next_obs.is_cuda and
                next_obs.dtype == torch.float32 and self.device.type == "cuda"):
            return None
        if self.use_set_hip:
            from . import set_policy
            if set_policy.TWIN_TARGETS and set_policy.TWIN_CRITICS and train_ops.ENABLED:
                # The switch promises the switch-off agent's results bit for bit.  Here that agent's `critic_target(...)` is ONE twin
                # pass of the training kernels (SECritic.forward), another kernel family than the chain's two forwards: their values
                # differ by rounding (measured 3.0e-8 in a target), so the chain yields and update_targets stays the code it was.  It
                # runs where SECritic.forward itself takes two passes of the rollout kernels (set_policy.TWIN_TARGETS = False,
                # TWIN_CRITICS = False, SGRL_TRAIN_GEMM=0).
                return None
            return "set"
        if self.use_swat_hip and self.dropout_rate > 0 and (self.actor_target.training or self.critic_target.training):
            # the plain HIP chain has no dropout: targets in training mode run the modules, as the reference's do -- unless the switch
            # hands them to the chain's dropout entries, which serve the three networks in ONE mode (_targets_drop)
            if not (self.swat_hip_dropout and self.actor_target.training and self.critic_target.training):
                return None
        if self.use_smp_hip:
            return "smp"
        if self.use_mlp_hip:
            if float(self.actor_target.max_action) != float(self.args.max_action):
                raise ValueError("the HIP target chain of an mlp agent scales and clamps with one max_action: the target policy's (%r) differs "
                                 "from args.max_action (%r); build the agent with use_hip=False" % (self.actor_target.max_action, self.args.max_action))
            return "mlp"
        return "swat"

    def _hip_targets(self, next_obs):
        """The chain object of `_target_kind(next_obs)` (swat_hip.HipSwatTargets / smp_hip.HipSmpTargets / mlp_hip.HipMlpTargets /
        set_hip.HipSetTargets) when this update's target chain runs on HIP, else None.  The object is kept in `_targets` and made
        again when it is of another kind or a target module has been replaced."""
        kind = self._target_kind(next_obs)
        if kind is None:
            return None
        module, cls = _TARGET_CHAINS[kind]
        t = self._targets
        if t is None or type(t).__name__ != cls or t.actor.policy is not self.actor_target or t.critic.module is not self.critic_target:
            import importlib
            # raises SgrlError when the extension is missing (no fallback)
            t = self._targets = getattr(importlib.import_module("." + module, __package__), cls)(self.actor_target, self.critic_target)
        return t

    def _targets_drop(self):
        """True when the HIP chain `_hip_targets` has just returned must DROP: a swat agent with a rate > 0 whose target networks
        are (both) in training mode -- `_hip_targets` returns a chain for that only with `swat_hip_dropout`."""
        return bool(self.use_swat_hip and self.dropout_rate > 0 and self.actor_target.training and self.critic_target.training)

    @property
    def device(self):
        return next(self.actor.parameters()).device

    def update(self, data_batch, it, noise=None, lazy_stats=False, skip_unused_critic_grads=False):
        """One TD3 step on a batch of ONE morphology (reference agent.py:117-183).  `noise` replaces the N(0, policy_noise)
        draw of agent.py:128 (tests: so that a run can be compared with the reference number for number; graph capture: a
        static buffer refilled before every replay).  lazy_stats: keep the two reward statistics as device tensors instead
        of `.item()` floats (no host sync -- required inside a hipGraph capture).

        With `mlp_hip_grads` (mlp + mlp agents, float32 batches on the GPU) everything after the target chain is
        mlp_hip.HipMlpGrads.critic_step -> clip_and_step -> (policy iterations) actor_step -> clip_and_step -> soft updates: no
        autograd graph, no zero_grad (the kernels overwrite `.grad`).  Stale gradients: after an actor step `critic.*.grad` holds
        the CLIPPED critic-loss gradients, not the reference's unused accumulation from the actor pass -- the documented state of
        skip_unused_critic_grads=True, whatever that argument says.  With `mlp_hip_optim` as well, each clip_and_step and the soft
        update of the same network are one mlp_hip.HipMlpOptim step (two launches); the target critic is then written before the
        actor pass, which reads the online critic only."""
        if self.dropout_rate > 0:
            with self._dropout_rng(data_batch["obs"].device):
                return self._update(data_batch, it, noise, lazy_stats, skip_unused_critic_grads)
        return self._update(data_batch, it, noise, lazy_stats, skip_unused_critic_grads)

    def _dropout_rng(self, device):
        """The train_ops.dropout_rng context of one update: the step counter moves first (one launch on the current stream), every
        dropout call of the update's three parts then numbers itself from site 0.  The counter's value is part of a checkpoint
        (resume_state; load_resume_state writes it back into this tensor), not of a reference-format snapshot."""
        step = self._dropout_step
        if step is None or step.device != device:
            step = self._dropout_step = torch.zeros(1, dtype=torch.int64, device=device)
        step.add_(1)
        return train_ops.dropout_rng(self.dropout_seed, step)

    def _update(self, data_batch, it, noise, lazy_stats, skip_unused_critic_grads):
        grads = self._hip_grads(data_batch)
        if grads is not None:
            return self._update_hip_grads(grads, data_batch, it, noise, lazy_stats)
        reward_batch, target_Q = self.update_targets(data_batch, noise)
        current_Q1, current_Q2 = self.update_critic_forward(data_batch)
        return self.update_finish(data_batch, it, reward_batch, target_Q, current_Q1, current_Q2, lazy_stats, skip_unused_critic_grads)

    def _update_hip_grads(self, grads, data_batch, it, noise, lazy_stats):
        args = self.args
        reward_batch, target_Q = self.update_targets(data_batch, noise)
        obs_batch = data_batch["obs"].contiguous()
        policy_it = it % args.policy_freq == 0       # delayed policy update
        optim = self._hip_optim(grads)
        critic_loss = grads.critic_step(obs_batch, data_batch["action"].contiguous(), target_Q).clone()
        if optim is not None:
            # the soft update of the target critic rides in the critic's apply pass: the actor pass below reads the online critic
            # only, so the parameters end as in the reference's order (agent.py:161-183: both steps, then both soft updates)
            optim.critic_step(args.grad_clipping_value, self.target_smoothing_tau if policy_it else 0.0)
        else:
            clip_and_step(self.critic_optimizer, args.grad_clipping_value)
        rmean, rvar = torch.mean(reward_batch), torch.var(reward_batch)
        loss_dict = {"loss/critic_loss": critic_loss, "misc/train_reward_mean": rmean if lazy_stats else rmean.item(),
                     "misc/train_reward_var": rvar if lazy_stats else rvar.item()}
        if policy_it:
            actor_loss = grads.actor_step(obs_batch).clone()
            if optim is not None:
                optim.actor_step(args.grad_clipping_value, self.target_smoothing_tau)
            else:
                clip_and_step(self.actor_optimizer, args.grad_clipping_value)
                self.try_update_target_network()
            loss_dict.update({"loss/actor_loss": actor_loss})
        return loss_dict

    # The three parts of an update.  The first two -- the no-grad target chain (actor_target -> critic_target) and the critics'
    # forward with autograd -- need nothing from each other: GraphedUpdates records them as separate graphs and replays them
    # side by side on two streams (both are chains of small latency-bound launches that leave most of the chip idle).
    def update_targets(self, data_batch, noise=None):
        args = self.args
        action_batch, next_obs_batch = data_batch["action"], data_batch["next_obs"]
        reward_batch, done_batch = data_batch["reward"] * self.reward_scale, data_batch["done"]
        with torch.no_grad():
            if noise is None:
                noise = torch.zeros_like(action_batch).normal_(0, args.policy_noise)
            hip, drop = self._hip_targets(next_obs_batch), {}
            if hip is not None and self._targets_drop():
                # the three target networks in training mode on the chain's dropout entries: the masks of this update's context,
                # and the 39 site numbers the modules would take here (actor_target, critic1, critic2: 13 each, in that order), so
                # that the online passes behind number from 39 as they do behind the modules.  Outside a context the modules would
                # draw from torch's generator, which no kernel restates: they run
                rng = train_ops._rng
                if rng is None or rng.step.device != next_obs_batch.device:
                    hip = None
                else:
                    from .swat_hip import SITES_PER_NET
                    drop = {"dropout": (self.dropout_rate, rng.seed, rng.step, rng.reserve(3 * SITES_PER_NET))}
            if hip is not None:      # one library call: target actor, noise clip and clamp, twin target critics, min, Bellman target
                target_Q = hip.target_q(next_obs_batch.contiguous(), noise.contiguous(), reward_batch, done_batch,
                                        self.actor_target.graph, args.noise_clip, args.discount, **drop)
                return reward_batch, target_Q
            noise = noise.clamp(-args.noise_clip, args.noise_clip)
            next_action = (self.actor_target(next_obs_batch) + noise).clamp(-args.max_action, args.max_action)
            target_Q1, target_Q2 = self.critic_target(next_obs_batch, next_action)    # per-limb values [B, L]
            target_Q = torch.min(target_Q1, target_Q2)
            target_Q = reward_batch + ((1.0 - done_batch) * args.discount * target_Q)  # reward [B, 1] broadcast over limbs
        return reward_batch, target_Q

    def update_critic_forward(self, data_batch):
        return self.critic(data_batch["obs"], data_batch["action"])

    def update_finish(self, data_batch, it, reward_batch, target_Q, current_Q1, current_Q2, lazy_stats=False,
                      skip_unused_critic_grads=False):
        args = self.args
        obs_batch = data_batch["obs"]
        if self.use_loss_kernels:
            critic_loss = train_ops.twin_mse(current_Q1, current_Q2, target_Q)
        else:
            critic_loss = F.mse_loss(current_Q1, target_Q) + F.mse_loss(current_Q2, target_Q)
        self.critic_optimizer.zero_grad()
        # (graphed path) the weight gradients are not on the backward pass's critical path: collected, issued together at the end
        with train_ops.deferred_wgrads(enabled=skip_unused_critic_grads):
            critic_loss.backward()
        clip_and_step(self.critic_optimizer, args.grad_clipping_value)
        rmean, rvar = torch.mean(reward_batch), torch.var(reward_batch)
        # the losses are returned DETACHED: a loss that keeps its autograd graph alive also keeps the parameters' AccumulateGrad
        # nodes -- and the stream they were created on -- alive into the next update; a hipGraph captured on another stream then
        # records a cross-stream hand-over per parameter (a 2 500-node update graph cost 39 ms to launch instead of 19)
        loss_dict = {"loss/critic_loss": critic_loss.detach(), "misc/train_reward_mean": rmean if lazy_stats else rmean.item(),
                     "misc/train_reward_var": rvar if lazy_stats else rvar.item()}
        if it % args.policy_freq == 0:       # delayed policy update
            # The actor loss back-propagates THROUGH the critic, but the critic's own parameter gradients from this pass are
            # never used (reference agent.py:167-176: only actor_optimizer steps; critic_optimizer.zero_grad() discards them
            # at the top of the next update).  skip_unused_critic_grads: do not compute them -- a third of the pass's
            # weight-gradient products; parameters, losses and actions are unchanged, only the stale `critic.*.grad` left behind
            # differs from the reference's (default off: the reference's exact state; GraphedUpdates turns it on).
            critic_params = [p for p in self.critic.parameters() if p.requires_grad] if skip_unused_critic_grads else []
            for p in critic_params:
                p.requires_grad_(False)
            try:
                actor_q = self.critic.Q1(obs_batch, self.actor(obs_batch))
                actor_loss = train_ops.neg_mean(actor_q) if self.use_loss_kernels else -actor_q.mean()
                self.actor_optimizer.zero_grad()
                with train_ops.deferred_wgrads(enabled=skip_unused_critic_grads):
                    actor_loss.backward()
            finally:
                for p in critic_params:
                    p.requires_grad_(True)
            clip_and_step(self.actor_optimizer, args.grad_clipping_value)
            self.try_update_target_network()
            loss_dict.update({"loss/actor_loss": actor_loss.detach()})
        return loss_dict

    def try_update_target_network(self):
        soft_update_network(self.critic, self.critic_target, self.target_smoothing_tau)
        soft_update_network(self.actor, self.actor_target, self.target_smoothing_tau)

    @torch.no_grad()
    def select_action(self, obs, deterministic=False):
        if len(obs.shape) == 1:
            obs = obs[None, ]
        if not isinstance(obs, torch.Tensor):
            obs = torch.as_tensor(obs, dtype=torch.float32).to(self.device)
        return self.actor(obs).cpu().numpy()

    def change_morphology(self, graph):
        self.actor.change_morphology(graph)
        self.actor_target.change_morphology(graph)
        self.critic.change_morphology(graph)
        self.critic_target.change_morphology(graph)

    def models2eval(self):
        for m in (self.actor, self.actor_target, self.critic, self.critic_target):
            m.eval()

    def models2train(self):
        for m in (self.actor, self.actor_target, self.critic, self.critic_target):
            m.train()

    # ---- what a checkpoint keeps of the agent besides state_dict() (checkpoint.py) -----------------------------------
    def resume_state(self):
        """Plain values and tensors only: `tot_update_count`, the VALUE of the dropout step (None while no update has created the
        tensor; reading it synchronises) and both optimizers (optimizer_state)."""
        step = self._dropout_step
        return {"tot_update_count": int(self.tot_update_count), "dropout_step": None if step is None else int(step.item()),
                "actor_optimizer": optimizer_state(self.actor_optimizer), "critic_optimizer": optimizer_state(self.critic_optimizer)}

    def load_resume_state(self, d):
        """`resume_state()` back, in place.  The dropout step is written INTO the existing tensor -- captured graphs hold its address
        and record its increment -- or, where no update has made one yet, into a new one on the agent's device; a record without a
        step zeroes an existing tensor (the first update's increment then makes it 1, as in a fresh agent).  The optimizers go
        through restore_optimizer; a live mlp_hip.HipMlpOptim is then brought back in line with the restored counts (resync).
        Returns True when optimizer state was deleted (see restore_optimizer)."""
        self.tot_update_count = int(d["tot_update_count"])
        step = d["dropout_step"]
        if self._dropout_step is not None:
            self._dropout_step.fill_(0 if step is None else int(step))
        elif step is not None:
            self._dropout_step = torch.full((1,), int(step), dtype=torch.int64, device=self.device)
        deleted = restore_optimizer(self.actor_optimizer, d["actor_optimizer"])
        deleted = restore_optimizer(self.critic_optimizer, d["critic_optimizer"]) or deleted
        if self._mlp_optim is not None:
            self._mlp_optim.resync()
        return deleted


def _concurrent_stream(cur, tries=8):
    """A stream that REALLY runs beside `cur`: HIP multiplexes its streams onto a handful of hardware queues and two streams on
    one queue execute strictly one after the other (csrc/stream_pick.h has the story); there is no query for the mapping, so it
    is measured with two spin kernels -- one spin time when the queues differ, two when they are the same.  Rejected candidates
    stay alive until the search ends so that the runtime does not hand the same queue out again."""
    cycles = 400000
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(other):
        best = 1e9
        for _ in range(2):
            if other is not None:
                other.wait_stream(cur)
            ev[0].record(cur)
            torch.cuda._sleep(cycles)
            if other is not None:
                with torch.cuda.stream(other):
                    torch.cuda._sleep(cycles)
                cur.wait_stream(other)
            ev[1].record(cur)
            ev[1].synchronize()
            best = min(best, ev[0].elapsed_time(ev[1]))
        return best
    single = timed(None)
    rejected = []
    for _ in range(tries):
        cand = torch.cuda.Stream()
        if timed(cand) < 1.6 * single:
            return cand
        rejected.append(cand)
    return rejected[0]


@contextlib.contextmanager
def _no_finalizers_during_capture():
    """Collect dead Python cycles NOW and keep the cyclic collector off until the capture has ended.  A collector pass in the
    middle of a capture may finalize an object of an earlier phase that owns device resources (a `HipSetActor`, a vec-env, a
    `DeviceTrainer`: their destructors call hipFree / hipStreamDestroy), and any such call invalidates a global-mode capture
    (`hipErrorStreamCaptureInvalidated` at the next launch).  torch.cuda.graph collected unconditionally in older releases; this one
    only does with torch.compiler.config.force_cudagraph_gc -- found as a test failure that came and went with the number of
    objects pytest had allocated before the capture."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def target_handles(targets):
    """The library handles behind a swat_hip.HipSwatTargets or a set_hip.HipSetTargets (target actor, critic.q1, critic.q2) or an
    smp_hip.HipSmpTargets (target actor, target critic); none for None."""
    if targets is None:
        return []
    c = targets.critic
    return [targets.actor] + ([c.q1, c.q2] if hasattr(c, "q1") else [c])


def handles_stamp(handles):
    """What a hipGraph has baked of these handles, as a comparable tuple of plain values (duck-typed, like mlp_update_stamp): per
    handle its `generation()` -- bumped whenever the library frees device memory a recorded forward may point into: an evicted batch
    structure, a regrown workspace (include/sgrl_swat.h sgrl_swat_generation, include/sgrl_smp.h sgrl_smp_generation) -- and `_bound`,
    the parameter addresses it holds: a rebinding frees nothing, but a graph carries the old addresses in its kernels' arguments."""
    return tuple((int(h.generation()), None if h._bound is None else tuple(h._bound)) for h in handles)


class _GraphedSurface(object):
    """What GraphedUpdates and GraphedMlpUpdates promise the trainer -- `warm`, `warm_from`, `update`, `update_from` over `agent`, `B`,
    `slots` and `warmed` -- and the host work both do around a replay.  A subclass supplies the slot (`_slot(key, graph, L)` and
    `_widths(L)`, the row widths of its obs and action tensors, which creates nothing), `_warm(key, graph, L, load, iters, first_it)`
    and `_replay(sl, key, graph, it)`: everything of an update after the slot's static tensors have been filled."""

    def _load(self, sl, data_batch):
        for k, t in sl["batch"].items():
            t.copy_(data_batch[k].reshape(t.shape))
        sl["noise"].normal_(0, self.agent.args.policy_noise)

    def _load_from(self, sl, buffer, seed, draw):
        buffer.sample_into(sl["batch"], self.B, seed, draw, noise=sl["noise"], noise_std=self.agent.args.policy_noise)

    def _morphology(self, graph):
        if graph is not None:
            self.agent.change_morphology(graph)

    def warm(self, key, graph, L, data_batch, iters=3, first_it=0):
        """Eager updates on the slot.  They are REAL updates: the caller passes the first `iters` iterations of its schedule
        (`data_batch` may be a callable returning a fresh batch per iteration, `first_it` the index of the first one) instead of
        adding updates of its own.  Returns the loss dicts."""
        return self._warm(key, graph, L, lambda sl, n: self._load(sl, data_batch() if callable(data_batch) else data_batch), iters, first_it)

    def warm_from(self, key, graph, L, buffer, seed, draw, iters=3, first_it=0):
        """`warm` with the slot filled by `buffer.sample_into` (replay.DeviceReplayBuffer): iteration n of the `iters` uses draw
        number `draw + n`.  The buffer must hold at least a full batch."""
        if buffer.max_sample_size < self.B:
            raise RuntimeError("warm_from needs at least %d rows in the buffer" % self.B)
        return self._warm(key, graph, L, lambda sl, n: self._load_from(sl, buffer, seed, draw + n), iters, first_it)

    def update(self, key, graph, L, data_batch, it):
        """Same contract as Agent.update(data_batch, it) (a replay: with lazy_stats=True) for the morphology `graph` (dict)
        identified by `key`."""
        if data_batch["obs"].shape[0] != self.B:
            self._morphology(graph)                     # short batch (buffer not yet filled): eager
            return self.agent.update(data_batch, it)
        sl = self._slot(key, graph, L)
        self._load(sl, data_batch)
        return self._replay(sl, key, graph, it)

    def update_from(self, key, graph, L, buffer, it, seed, draw):
        """`update` with the batch drawn by the library: the slot's static batch and noise tensors are filled by ONE
        `buffer.sample_into(..., seed, draw, noise=...)` (replay.DeviceReplayBuffer, include/sgrl_replay.h) -- launched outside the
        captured graph, before the replay (seed and draw are by-value arguments: not part of the graph) -- instead of sample() + five
        copies + normal_().  What the graphs record is unchanged."""
        if buffer.max_sample_size < self.B:             # short batch (buffer not yet filled): eager, on the k rows there are
            self._morphology(graph)
            k, dev, (n_obs, n_act) = buffer.max_sample_size, self.agent.device, self._widths(L)
            e = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
            batch = {"obs": e(k, n_obs), "action": e(k, n_act), "next_obs": e(k, n_obs), "reward": e(k, 1), "done": e(k, 1)}
            noise = torch.zeros((k, n_act), dtype=torch.float32, device=dev)
            buffer.sample_into(batch, k, seed, draw, noise=noise, noise_std=self.agent.args.policy_noise)
            return self.agent.update(batch, it, noise=noise)
        sl = self._slot(key, graph, L)
        self._load_from(sl, buffer, seed, draw)
        return self._replay(sl, key, graph, it)

    def _announce(self, flag):
        """A replay runs no host code: the writes of its optimizer / soft-update kernels are announced here."""
        a = self.agent
        touched = list(a.critic.parameters())
        if flag == 0:
            for mod in (a.actor, a.actor_target, a.critic_target):
                touched.extend(mod.parameters())
        _touched(touched)


class GraphedUpdates(_GraphedSurface):
    """`Agent.update` captured into hipGraphs (MI355X: the update is ~3 400 small launches -- PyTorch autograd through three
    SET networks at batch 100 plus the HIP target kernels -- and launch-bound when issued eagerly: 50 ms; a replay is
    GPU-bound: 32 ms).  One graph per (morphology, with / without the delayed actor step); the batch is copied into static
    tensors and the target-policy noise redrawn into a static tensor before each replay, so the replayed arithmetic is
    the eager update's.  Everything reachable from `Agent.update` is capturable: the SET kernels are launched on the
    capturing stream (their side-stream fork / join becomes part of the graph), parameters are read live, Adam runs with
    `capturable=True`, the reward statistics stay on the device.

    Capture rules honoured here: every (morphology, batch size) is run eagerly first (so the SET handles have cached the
    batch structure and grown their workspace to its final size before any pointer is baked into a graph).

    hip_kernels=False: a SWAT or SMP agent is switched to plain PyTorch throughout (HIP target chain and training kernels off) and
    its graphs record that.  hip_kernels=True: the agent's switches are left exactly as it was built -- a swat + swat or an smp + smp
    (td and bu) agent then records its HIP target chain (swat_hip.HipSwatTargets / smp_hip.HipSmpTargets: every chain of the
    former forks onto the handle's side stream, which the warm-up creates) and, with `swat_train_kernels` / `smp_train_kernels`,
    its differentiable passes on the training kernels.  The stamp of a graph then also covers that target object's handles
    (`handles_stamp`), and a capture is refused (RuntimeError) when the target object is not the one the slot's warm-up ran with.
    The three-graph form (`split`) is not built for it.  A SET agent built with `set_hip_targets` records its one-call chain
    (set_hip.HipSetTargets) with either value of hip_kernels -- its HIP forwards are recorded in both -- under the same two rules: the
    chain's first call, which reserves workspace, is made by the warm-up's eager updates.  `captures[(key, flag)]` counts the captures of each graph; `stale(key, flag)`
    says, launching nothing, whether a captured graph would be dropped by the next update of that kind.

    Dropout (`agent.dropout_rate` > 0): accepted with hip_kernels=True on an agent whose target chain runs the HIP dropout entries
    (`use_swat_hip` and `swat_hip_dropout`), refused otherwise.  The step counter's increment is recorded, the site numbers are baked
    in, the stamp also carries the four networks' `training` flags and the step tensor's address (see __init__)."""

    dropout = False       # True: the agent's updates drop (dropout_rate > 0) and are captured with the HIP chain's dropout entries

    def __init__(self, agent, batch_size, hip_kernels=False):
        self.agent, self.B = agent, int(batch_size)
        self.hip_kernels = bool(hip_kernels)
        self.captures = {}       # (key, flag) -> number of times that graph has been captured
        if getattr(agent.args, "actor_type", "set") == "mlp":
            raise NotImplementedError("GraphedUpdates is not built for 'mlp' agents: run their updates eagerly (DeviceTrainer(graph_updates=False))")
        self.dropout = getattr(agent, "dropout_rate", 0.0) > 0
        if self.dropout and not (self.hip_kernels and getattr(agent, "use_swat_hip", False) and getattr(agent, "swat_hip_dropout", False)):
            # the site numbers of an update are host state and its passes differ between training and eval mode: nobody has made the
            # capture of a dropout update sound where the targets run the modules, so it is refused rather than replayed with stale
            # masks.  With the HIP chain's dropout entries (hip_kernels and the agent's swat_hip_dropout) it is sound:
            #   - the step is a device word: `Agent._dropout_rng`'s increment is RECORDED, every replay moves the masks, and every
            #     kernel reads the word itself; the warm-up's eager updates create the tensor before any capture, and
            #     `_check_capture` refuses a capture on another tensor than the slot was warmed with;
            #   - the site numbers are baked in and right in every replay: the program order of an update is fixed per
            #     (morphology, flag);
            #   - the passes an update runs depend on the four networks' `training` flags: they and the step tensor's address are
            #     part of a graph's stamp (`_stamp`), a mismatch captures again
            raise NotImplementedError("GraphedUpdates does not replay updates with dropout (dropout_rate %g): run them eagerly "
                                      "(DeviceTrainer(graph_updates=False)) or set dropout_rate to 0" % agent.dropout_rate)
        dev = agent.device
        if dev.type != "cuda":
            raise RuntimeError("GraphedUpdates needs the agent on the GPU")
        if not train_ops.ENABLED:
            # round 6: a config-5 run of this combination went NaN in its third round (profiles/r6_takeoff/bisect
            # r6_takeoff_vendor_graphed_*); the vendor path is an A/B arm for EAGER updates, nobody has made its capture sound
            raise RuntimeError("GraphedUpdates replays this library's own training kernels: with SGRL_TRAIN_GEMM=0 (vendor kernels) run the "
                               "updates eagerly (DeviceTrainer(graph_updates=False))")
        if not self.hip_kernels:
            # without hip_kernels the workspace stamps below follow the SET handles only: a SWAT or SMP agent's graphs record the
            # PyTorch target chain
            agent.use_swat_hip = False
            agent.set_swat_train_kernels(False)      # graphed SWAT agents stay plain PyTorch throughout, as before
            agent.use_smp_hip = False
            agent.set_smp_train_kernels(False)       # and graphed SMP agents: the switch goes off together with the HIP target chain
        for opt in (agent.actor_optimizer, agent.critic_optimizer):
            if opt.state:
                raise RuntimeError("switch to graphed updates before the first optimizer step (Adam's step counters must be device tensors)")
            for g in opt.param_groups:
                g["capturable"] = True
        self.slots = {}            # key -> dict(static tensors, graphs)
        self.warmed = set()
        # True (tools/diag/split_update_graphs_probe.py): target chain and critic forward as graphs of their own, replayed on two
        # streams -- measured 1-2 % faster per update (LAB_LOG round 3), not the default
        self.split = False
        self._cap_stream = self._side = None

    def _slot(self, key, graph, L):
        sl = self.slots.get(key)
        if sl is None:
            dev, B, (n_obs, n_act) = self.agent.device, self.B, self._widths(L)
            z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
            sl = {"graph": graph, "batch": {"obs": z(B, n_obs), "action": z(B, n_act), "next_obs": z(B, n_obs), "reward": z(B, 1),
                                            "done": z(B, 1)}, "noise": z(B, n_act), "graphs": {}, "out": {}, "stamp": {}}
            self.slots[key] = sl
        return sl

    def _widths(self, L):
        return 41 * L, 3 * L

    def _hip_handles(self):
        """The HIP handles whose forwards the update graphs record: the target actor and the two target critics."""
        out = []
        for mod in (self.agent.actor_target, self.agent.critic_target):
            h = getattr(mod, "_hip", None)
            out.extend([h] if hasattr(h, "h") else [getattr(h, "q1", None), getattr(h, "q2", None)])
        return [hh for hh in out if hh is not None]

    def _workspace_stamp(self):
        """What the captured HIP target kernels point into, per handle: the workspace's size and the handle's GENERATION
        (include/sgrl_set.h sgrl_set_generation: bumped whenever the handle frees device memory a recorded forward may
        reference -- a batch structure evicted from its cache, the flat weight buffers of a rebinding, a regrown workspace --
        or is told to change the form of its tile products)."""
        return tuple((int(hh.L.sgrl_set_workspace_bytes(hh.h)), int(hh.L.sgrl_set_generation(hh.h))) for hh in self._hip_handles())

    def _targets(self, sl):
        """The object whose target chain an update on this slot records -- what `Agent._hip_targets` returns NOW (it re-creates the
        object when a target module has been replaced) -- or None: without hip_kernels, and for agents whose chain is PyTorch.  A SET
        agent's chain object (`set_hip_targets`) counts with either value of hip_kernels: its forwards are recorded in both."""
        if not self.hip_kernels and not getattr(self.agent, "use_set_hip", False):
            return None
        return self.agent._hip_targets(sl["batch"]["next_obs"])

    def _stamp(self, sl):
        """The stamp of a graph on this slot: the SET handles' (`_workspace_stamp`) and, with hip_kernels, the SWAT / SMP target
        handles' (`handles_stamp`: three for SWAT, two for SMP)."""
        base = (self._workspace_stamp(), handles_stamp(target_handles(self._targets(sl))))
        if not self.dropout:
            return base
        a = self.agent
        step = a._dropout_step
        return base + (tuple(bool(m.training) for m in (a.actor, a.actor_target, a.critic, a.critic_target)),
                       None if step is None else int(step.data_ptr()))

    def stale(self, key, flag):
        """True when a graph has been captured for (key, flag) and its stamp is no longer the current one: the next update of that
        kind drops it and captures again.  Launches nothing."""
        sl = self.slots.get(key)
        if sl is None or flag not in sl["graphs"]:
            return False
        return sl["stamp"].get(flag) != self._stamp(sl)

    def forget_graphs(self):
        """Drop every captured graph and every warm-up: Adam state tensors the graphs step have been freed (restore_optimizer
        deleted them -- a checkpoint from before the first update loaded into an agent that has stepped; the stamp does not
        carry their addresses).  The next round warms every morphology again, eagerly, before anything is captured."""
        for key, sl in self.slots.items():
            for flag in list(sl["graphs"]):
                del sl["graphs"][flag]
                release_tables((id(self), key, flag))
            sl["stamp"].clear()
        self.warmed.clear()

    def _check_capture(self, sl, key):
        """What must hold on the host before torch.cuda.graph(...) is entered for a graph on this slot."""
        if self.hip_kernels and self.split:
            raise RuntimeError("GraphedUpdates(hip_kernels=True) records ONE graph per update: the three-graph form is not built for the "
                               "SWAT / SMP kernels; leave `split` False")
        if key not in self.warmed:
            raise RuntimeError("warm(%r, ...) every morphology before the first graphed update" % (key,))
        if self._targets(sl) is not sl.get("targets"):
            # a fresh target object: its handles have run nothing yet, so the capture would hold their first call -- which binds the
            # parameters, builds the batch structure, allocates the workspace and creates the twin chain's side stream
            # (include/sgrl_swat.h sgrl_swat_forward_twin: "make that call outside any stream capture")
            raise RuntimeError("the agent's HIP target chain is not the one morphology %r was warmed with (a target network has been "
                               "replaced, or the chain was switched on or off): warm(%r, ...) again before the next graphed update"
                               % (key, key))
        if self.dropout and (self.agent._dropout_step is None or self.agent._dropout_step is not sl.get("dropout_step")):
            # the graph records the increment of, and every kernel's reads from, the step tensor the warm-up's updates created
            raise RuntimeError("the agent's dropout step tensor is not the one morphology %r was warmed with: warm(%r, ...) again before "
                               "the next graphed update" % (key, key))

    def _warm(self, key, graph, L, load, iters, first_it):
        """The eager updates of `warm` / `warm_from`, on a side stream (PyTorch's capture protocol)."""
        sl = self._slot(key, graph, L)
        self.agent.change_morphology(graph)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        outs = []
        with torch.cuda.stream(s):
            for n, it in enumerate(range(first_it, first_it + iters)):
                load(sl, n)
                outs.append(self.agent.update(sl["batch"], it, noise=sl["noise"], lazy_stats=True, skip_unused_critic_grads=True))
        torch.cuda.current_stream().wait_stream(s)
        self.warmed.add(key)
        if outs:
            sl["targets"] = self._targets(sl)   # (hip_kernels) whose first calls have now happened outside any capture
            sl["dropout_step"] = self.agent._dropout_step      # (dropout) created by the first eager update
        return outs

    def _replay(self, sl, key, graph, it):
        """Everything of a graphed update after the slot's static tensors have been filled."""
        if key not in self.warmed:
            raise RuntimeError("warm(%r, ...) every morphology before the first graphed update" % (key,))
        flag = 0 if it % self.agent.args.policy_freq == 0 else 1
        # A graph bakes the addresses of the SET handles' workspaces.  They only ever grow, and every morphology is run eagerly
        # before any capture -- but a graph captured before a LATER regrowth would fault on replay (a GPU memory fault, not an
        # exception): the workspaces' sizes are compared with those at capture time and such a graph is captured again.
        # With hip_kernels the same holds for the SWAT / SMP target handles: the stamp also carries their generations and bound addresses.
        stamp = self._stamp(sl)
        owner = (id(self), key, flag)
        if flag in sl["graphs"] and sl["stamp"].get(flag) != stamp:
            del sl["graphs"][flag]
            release_tables(owner)
        if flag not in sl["graphs"]:
            self._check_capture(sl, key)
            self.captures[(key, flag)] = self.captures.get((key, flag), 0) + 1
        global _capture_owner
        if flag not in sl["graphs"] and self.split:
            # Three graphs, all recorded on ONE capture stream (autograd's nodes then belong to one stream: no cross-stream
            # hand-overs inside the backward) but each with its own memory pool: the target chain and the critics' forward are
            # REPLAYED side by side, so neither may reuse a block the other has freed.
            self.agent.change_morphology(graph)
            if self._cap_stream is None:
                self._cap_stream, self._side = torch.cuda.Stream(), _concurrent_stream(torch.cuda.current_stream())
            gs = [torch.cuda.CUDAGraph() for _ in range(3)]
            _stock_pinned(4)
            _capture_owner = owner
            with _no_finalizers_during_capture():
                with torch.cuda.graph(gs[0], stream=self._cap_stream):
                    rb, tq = self.agent.update_targets(sl["batch"], sl["noise"])
                with torch.cuda.graph(gs[1], stream=self._cap_stream):
                    q1, q2 = self.agent.update_critic_forward(sl["batch"])
                with torch.cuda.graph(gs[2], stream=self._cap_stream):
                    sl["out"][flag] = self.agent.update_finish(sl["batch"], flag, rb, tq, q1, q2, lazy_stats=True,
                                                               skip_unused_critic_grads=True)
            _capture_owner = None
            sl["graphs"][flag] = gs
            sl["stamp"][flag] = self._stamp(sl)
        if flag not in sl["graphs"]:
            self.agent.change_morphology(graph)
            g = torch.cuda.CUDAGraph()
            dump = os.environ.get("SGRL_GRAPH_DUMP")      # diagnostics: <dir> receives one .dot file per captured graph
            if dump:
                g.enable_debug_mode()
            _stock_pinned(4)
            _capture_owner = owner
            try:
                with _no_finalizers_during_capture(), torch.cuda.graph(g):
                    sl["out"][flag] = self.agent.update(sl["batch"], flag, noise=sl["noise"], lazy_stats=True,
                                                        skip_unused_critic_grads=True)
            finally:
                _capture_owner = None
            if dump:
                g.debug_dump(os.path.join(dump, "update_%s_flag%d.dot" % (key, flag)))
            sl["graphs"][flag] = g           # capturing records the work without running it
            sl["stamp"][flag] = self._stamp(sl)
        g = sl["graphs"][flag]
        if isinstance(g, list):
            cur = torch.cuda.current_stream()
            self._side.wait_stream(cur)          # the batch / noise just loaded on the caller's stream
            g[0].replay()
            with torch.cuda.stream(self._side):
                g[1].replay()
            cur.wait_stream(self._side)
            g[2].replay()
        else:
            g.replay()
        self._announce(flag)
        # the capture's output tensors are overwritten by the next replay: hand out copies
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sl["out"][flag].items()}


def mlp_update_stamp(handles, nets, optimizers, sides, scalars):
    """Everything a hipGraph of an MLP agent's update has baked -- device addresses and by-value scalars -- as one comparable tuple
    of PLAIN values (duck-typed: tests/test_mlp_graph_plan.py feeds it stubs).
      handles     the four mlp_hip handles a replay's kernels were recorded from (target actor, target critic, the gradient half's actor
                  and critic): `generation()` (bumped whenever the library frees device memory a recorded launch may point into)
                  and `_bound`, the parameter addresses the library holds
      nets        per network (target actor, target critic, online actor, online critic) its parameters: where their storage and
                  their `.grad` are NOW (a moved tensor is bound again by the next eager call, not by a replay)
      optimizers  per optimizer (actor, critic) `(opt, params)`: the addresses of exp_avg, exp_avg_sq and the step tensor of every
                  parameter, and lr, betas, eps of the group
      sides       per optimizer the mlp_hip._OptimSide: its partials and its own device counter (plain groups)
      scalars     grad_clipping_value, tau, noise_clip, discount, max_action, reward_scale"""
    ptr = lambda t: None if t is None else int(t.data_ptr())
    hs = tuple((int(h.generation()), None if h._bound is None else tuple(h._bound)) for h in handles)
    ps = tuple(tuple((ptr(p), ptr(getattr(p, "grad", None))) for p in params) for params in nets)
    os_ = []
    for opt, params in optimizers:
        g = opt.param_groups[0]
        st = [opt.state.get(p, {}) for p in params]
        os_.append((tuple((ptr(s.get("exp_avg")), ptr(s.get("exp_avg_sq")), ptr(s.get("step"))) for s in st),
                    float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"])))
    sd = tuple((ptr(s.partials), ptr(s.counter)) for s in sides)
    return (hs, ps, tuple(os_), sd, tuple(None if v is None else float(v) for v in scalars))


class _EveryKey(object):
    """`GraphedMlpUpdates.warmed`: the one slot serves every morphology, so every key is warmed once it is."""

    def __init__(self, owner):
        self._owner = owner

    def __contains__(self, key):
        return self._owner._warmed

    def __bool__(self):
        return self._owner._warmed


class GraphedMlpUpdates(_GraphedSurface):
    """The TD3 update of an mlp + mlp agent replayed from hipGraphs: the trainer-facing surface of `GraphedUpdates` (`warm`,
    `warm_from`, `update`, `update_from`, `warmed`, `slots`; fewer rows than B: an eager `agent.update`) over an update that is
    entirely this library's launches -- mlp_hip.batch_stats -> HipMlpTargets.target_q -> HipMlpGrads.critic_step ->
    HipMlpOptim.critic_step and, on policy iterations, HipMlpGrads.actor_step -> HipMlpOptim.actor_step: the calls of
    `Agent._update_hip_grads` in its order with its arguments, so the parameters come out bit-identical to `Agent.update`.  The
    graph is a plain chain of kernel nodes on ONE stream (`launches(flag)`: 9, or 15 with the policy step): no autograd, no side
    stream, no allocation, hence no memory pool of its own, and no runtime setting is read or set.

    ONE slot for every morphology (a monolithic network has one limb count): static obs / action / next_obs / reward / done / noise,
    the scaled reward, the target [B, 1] and the 4-float record {critic_loss, actor_loss, reward_mean, reward_var}; two graphs, with
    (flag 0) and without (flag 1) the policy step.  `key`, `graph` and `L` are accepted for interface compatibility.

    A graph bakes addresses and by-value scalars: `_stamp()` (mlp_update_stamp) lists them.  `eager_ok[flag]` is the stamp right
    after the last EAGER run of that kind on the slot; a graph is captured only when it equals the current stamp (the eager run has
    then bound and grown everything the capture will point at), and a captured graph whose stamp differs from the current one is
    dropped.  In either case that update runs eagerly on the slot and the capture happens on a later call: no `warm` is needed, the
    first update of each kind is the eager one.  `stale(flag)` says, launching nothing, whether the next update of that kind would
    NOT be a replay.  Values are read live: an in-place write into a parameter is seen by the next replay; a changed learning rate
    is a by-value argument and makes the graphs stale."""

    def __init__(self, agent, batch_size):
        self.agent, self.B = agent, int(batch_size)
        atype, ctype = getattr(agent.args, "actor_type", "set"), getattr(agent.args, "critic_type", "set")
        if atype != "mlp" or ctype != "mlp":
            raise NotImplementedError("GraphedMlpUpdates serves 'mlp' + 'mlp' agents only (got actor_type %r, critic_type %r): the other "
                                      "types replay through GraphedUpdates" % (atype, ctype))
        if agent.device.type != "cuda":
            raise RuntimeError("GraphedMlpUpdates needs the agent on the GPU")
        if not agent.use_mlp_hip:
            raise RuntimeError("GraphedMlpUpdates replays the HIP update of an mlp agent: this one was built with use_hip=False")
        from . import _lib, mlp_hip
        self._mlp_hip = mlp_hip
        try:
            mlp_hip.train_plan(mlp_hip.net_dims(agent.actor.actor), mlp_hip.net_dims(agent.critic.critic1), self.B)
        except _lib.SgrlError as e:
            agent.mlp_hip_grads_refusal = str(e)
            raise NotImplementedError("GraphedMlpUpdates: the gradient half does not serve these widths: %s" % e)
        for opt, net in ((agent.actor_optimizer, agent.actor.actor), (agent.critic_optimizer, None)):
            params = [p for n in ([net] if net is not None else [agent.critic.critic1, agent.critic.critic2])
                      for l in mlp_hip.linears(n) for p in (l.weight, l.bias)]
            why = mlp_hip.HipMlpOptim.refusal(opt, params)
            if why:
                raise NotImplementedError("GraphedMlpUpdates: the optimizer half does not serve this optimizer: %s" % why)
        if not 0.0 <= float(agent.target_smoothing_tau) <= 1.0:
            raise NotImplementedError("GraphedMlpUpdates: target_smoothing_tau outside [0, 1]")
        agent.use_mlp_hip_grads = agent.use_mlp_hip_optim = True      # the groups stay as they are, plain or capturable
        self.slots = {}              # one entry, key None: the shared slot
        self._warmed = False
        self.warmed = _EveryKey(self)
        self.eager_ok = {0: None, 1: None}
        self.replays = 0             # updates served by a graph replay so far

    # ---- the slot -------------------------------------------------------------------------------------
    def _slot(self, key=None, graph=None, L=None):
        sl = self.slots.get(None)
        if sl is None:
            dev, B, (n_in, n_out) = self.agent.device, self.B, self._widths(L)
            z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
            sl = {"batch": {"obs": z(B, n_in), "action": z(B, n_out), "next_obs": z(B, n_in), "reward": z(B, 1), "done": z(B, 1)},
                  "noise": z(B, n_out), "reward": z(B, 1), "target": z(B, 1), "rec": z(4), "graphs": {}, "stamp": {}}
            self.slots[None] = sl
        return sl

    def _widths(self, L):
        dims = self._mlp_hip.net_dims(self.agent.actor.actor)
        return dims[0], dims[-1]

    def _handles(self, sl):
        """(HipMlpTargets, HipMlpGrads, HipMlpOptim) of the agent -- its own, so that an eager `agent.update` and this object see the
        same binds and generations; made on first use as `Agent.update` makes them."""
        a = self.agent
        t, g = a._hip_targets(sl["batch"]["next_obs"]), a._hip_grads(sl["batch"])
        o = a._hip_optim(g) if g is not None else None
        if t is None or g is None or o is None:
            raise RuntimeError("GraphedMlpUpdates: the agent no longer takes the HIP update (%s)"
                               % (getattr(a, "mlp_hip_optim_refusal", None) or getattr(a, "mlp_hip_grads_refusal", None) or "use_mlp_hip* turned off"))
        return t, g, o

    def launches(self, flag):
        """Kernel launches (= graph nodes) of an update with (flag 0) or without (flag 1) the policy step, from the ABI's counts: the
        prologue, the chain with its two packs, the critic's gradient and optimizer steps; then the actor's."""
        m = self._mlp_hip
        L = m._lib.lib()
        m._bind(L)
        n = L.sgrl_mlp_batch_stats_launches() + 2 * L.sgrl_mlp_pack_launches() + L.sgrl_mlp_td_target_launches() + \
            L.sgrl_mlp_critic_step_launches() + L.sgrl_mlp_optim_step_launches()
        if flag == 0:
            n += L.sgrl_mlp_actor_step_launches() + L.sgrl_mlp_optim_step_launches()
        return int(n)

    # ---- one update on the slot, eagerly or under capture ---------------------------------------------------
    def _run(self, sl, hs, policy_it):
        a, args = self.agent, self.agent.args
        targets, grads, optim = hs
        batch, rec = sl["batch"], sl["rec"]
        tau = a.target_smoothing_tau
        self._mlp_hip.batch_stats(batch["reward"], a.reward_scale, sl["reward"], rec[2:4])
        targets.target_q(batch["next_obs"], sl["noise"], sl["reward"], batch["done"], a.actor_target.graph, args.noise_clip, args.discount,
                         out=sl["target"])
        grads.critic_step(batch["obs"], batch["action"], sl["target"], loss_out=rec[0])
        optim.critic_step(args.grad_clipping_value, tau if policy_it else 0.0)
        if policy_it:
            grads.actor_step(batch["obs"], loss_out=rec[1])
            optim.actor_step(args.grad_clipping_value, tau)

    def _stamp(self, hs):
        a, args = self.agent, self.agent.args
        targets, grads, optim = hs
        handles = (targets.actor, targets.critic, grads.actor, grads.critic)
        return mlp_update_stamp(handles, [h._params() for h in handles],
                                ((a.actor_optimizer, grads.actor._params()), (a.critic_optimizer, grads.critic._params())),
                                (optim._actor, optim._critic),
                                (args.grad_clipping_value, a.target_smoothing_tau, args.noise_clip, args.discount, a.actor_target.max_action,
                                 a.reward_scale))

    def stale(self, flag):
        """True when the next update of this kind (0: with the policy step, 1: without) would NOT be a replay: no graph yet, or one
        whose baked addresses or scalars are no longer the current ones.  Launches nothing."""
        sl = self.slots.get(None)
        if sl is None or flag not in sl["graphs"]:
            return True
        hs = self._handles(sl)
        return sl["stamp"][flag] != self._stamp(hs) or not hs[2].counts_current(critic=True, actor=flag == 0)

    def _result(self, sl, policy_it):
        out = sl["rec"].clone()      # ONE copy: the record is overwritten by the next update
        d = {"loss/critic_loss": out[0], "misc/train_reward_mean": out[2], "misc/train_reward_var": out[3]}
        if policy_it:
            d["loss/actor_loss"] = out[1]
        return d

    def _eager(self, sl, hs, flag):
        self._run(sl, hs, flag == 0)
        self.eager_ok[flag] = self._stamp(hs)
        self._warmed = True
        return self._result(sl, flag == 0)

    def _replay(self, sl, key, graph, it):
        """Everything of an update after the slot's static tensors have been filled."""
        a = self.agent
        self._morphology(graph)
        flag = 0 if it % a.args.policy_freq == 0 else 1
        hs = self._handles(sl)
        optim = hs[2]
        stamp = self._stamp(hs)
        current = optim.counts_current(critic=True, actor=flag == 0)
        if flag in sl["graphs"] and (sl["stamp"][flag] != stamp or not current):
            del sl["graphs"][flag]               # it points at what has moved, or carries a scalar that has changed
        if flag not in sl["graphs"]:
            if self.eager_ok[flag] != stamp or not current:
                return self._eager(sl, hs, flag)     # binds and grows whatever moved; the capture happens on a later call
            g = torch.cuda.CUDAGraph()
            counts = optim.host_counts()
            try:
                with _no_finalizers_during_capture(), torch.cuda.graph(g):
                    self._run(sl, hs, flag == 0)
            except self._mlp_hip._lib.SgrlError:
                g = None                             # e.g. "must grow": nothing was recorded that will ever run
            finally:
                optim.set_host_counts(counts)        # the recorded steps have not run: their host-side counts are taken back
            if g is None or self._stamp(hs) != stamp:
                return self._eager(sl, hs, flag)
            sl["graphs"][flag], sl["stamp"][flag] = g, stamp
        sl["graphs"][flag].replay()
        self.replays += 1
        # a replay runs no host code: the steps' host-side counts and the writes of their kernels are announced here
        optim.replayed(critic=True, actor=flag == 0)
        self._announce(flag)
        return self._result(sl, flag == 0)

    def _warm(self, key, graph, L, load, iters, first_it):
        """The `iters` updates of `warm` / `warm_from`, run eagerly on the slot (optional here: the first update of each kind is eager
        anyway)."""
        sl = self._slot()
        self._morphology(graph)
        outs = []
        for n, it in enumerate(range(first_it, first_it + iters)):
            load(sl, n)
            outs.append(self._eager(sl, self._handles(sl), 0 if it % self.agent.args.policy_freq == 0 else 1))
        return outs
