"""Batched HIP forwards of the SMP actor and critic (csrc/smp_actor.hip, C ABI in include/sgrl_smp.h).

`HipSmpActor` binds the parameters of an `ActorGraphPolicy` in its published mode (`td and bu`; smp_policy.py,
reference-compatible state_dict) to a handle BY ADDRESS: nothing is packed, the library reads the live tensors on every
forward, so optimizer steps, soft updates, `load_state_dict` and in-place broadcasts need no notification; only a parameter
whose storage MOVES (`.to()`, re-created tensors) needs a re-bind, which `sync_weights` does by itself.  It has the surface
`Rollout` uses on `HipSetActor` / `HipSwatActor` (`configure`, `forward_batch`, `hold_weights`, `sync_weights`, `n_env`,
`max_limbs`).  The tree schedule (levels, children rows, message slots) comes from `smp_policy._Tree` alone: `level_schedule`
lays it out as the rows the library takes.  No CPU fallback: without the MI355X every entry point raises `_lib.SgrlError`.

`HipSmpCritic` is the same over a `CriticGraphPolicy` (twin Q values summed over the limbs, [B, 1] each, or Q1 only);
`HipSmpTargets` runs the no-grad half of a TD3 update -- target actor, clipped noise, twin target critic, min and Bellman target
(reference src/agent.py:126-148) -- as one library call (`td3.Agent.update_targets`).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .set_hip import graph_key
from .smp_policy import _Tree

MSG, HU, H1, H2 = 32, 64, 400, 300
MAX_LIMBS, MAX_LEVELS, MAX_CHILDREN = 16, 16, 8


def _config(policy):
    """(feature, out, max_children) of a smp_policy.ActorGraphPolicy; refuses what the HIP forward is not built for."""
    if not (getattr(policy, "td", False) and getattr(policy, "bu", False)):
        raise _lib.SgrlError("the HIP SMP forward serves the published mode only (td and bu: bottom-up AND top-down messages)")
    up, down = policy.sNet[0], policy.actor[0]
    mc = int(policy.max_children)
    dims = (int(policy.msg_dim), int(up.fc1.out_features), int(down.action_base.l1.out_features),
            int(down.action_base.l2.out_features))
    if dims != (MSG, HU, H1, H2):
        raise _lib.SgrlError("the HIP SMP forward is built for message width 32 and hidden sizes 64 / 400 / 300")
    if not 1 <= mc <= MAX_CHILDREN:
        raise _lib.SgrlError("the HIP SMP forward takes 1 <= max_children <= %d, not %d" % (MAX_CHILDREN, mc))
    return int(up.fc1.in_features), int(down.action_base.l3.out_features), mc


def plan_params(policy):
    """[(name, shape)] of `policy` (a smp_policy.ActorGraphPolicy with td and bu) in the slot order of sgrl_smp_bind_params
    (include/sgrl_smp.h).  The names are those of the one shared ActorUp / ActorDownAction (index 0 of the per-limb listing).
    Host only: works on a module on any device."""
    feature, out, mc = _config(policy)
    plan = [("sNet.0.fc1", (HU, feature)), ("sNet.0.fc2", (HU, HU + MSG * mc)), ("sNet.0.fc3", (MSG, HU))]
    for base, last in (("actor.0.action_base", out), ("actor.0.msg_base", MSG * mc)):
        plan += [(base + ".l1", (H1, HU)), (base + ".l2", (H2, H1)), (base + ".l3", (last, H2))]
    return [q for n, s in plan for q in ((n + ".weight", s), (n + ".bias", s[:1]))]


def _critic_config(module):
    """(feature, act_feature, max_children) of a smp_policy.CriticGraphPolicy; refuses what the HIP forward is not built for."""
    if not (getattr(module, "td", False) and getattr(module, "bu", False)):
        raise _lib.SgrlError("the HIP SMP critic serves the published mode only (td and bu: bottom-up AND top-down messages)")
    up, down = module.sNet[0], module.critic[0]
    mc = int(module.max_children)
    dims = (int(module.msg_dim), int(up.fc1.out_features), int(down.baseQ1.l1.out_features), int(down.baseQ1.l2.out_features))
    if dims != (MSG, HU, H1, H2):
        raise _lib.SgrlError("the HIP SMP critic is built for message width 32 and hidden sizes 64 / 400 / 300")
    if not 1 <= mc <= MAX_CHILDREN:
        raise _lib.SgrlError("the HIP SMP critic takes 1 <= max_children <= %d, not %d" % (MAX_CHILDREN, mc))
    feature, act_feature = int(up.fc1.in_features), int(module.action_dim)
    if not (1 <= act_feature <= 8 and act_feature < feature <= 64 and feature == int(module.state_dim) + act_feature):
        raise _lib.SgrlError("the HIP SMP critic takes state_dim + action_dim <= 64 inputs per limb, 1 <= action_dim <= 8")
    return feature, act_feature, mc


def plan_critic_params(module):
    """[(name, shape)] of `module` (a smp_policy.CriticGraphPolicy with td and bu) in the slot order of
    sgrl_smp_bind_critic_params (include/sgrl_smp.h).  The names are those of the one shared CriticUp / CriticDownAction (index 0
    of the per-limb listing).  Host only: works on a module on any device."""
    feature, act_feature, mc = _critic_config(module)
    plan = [("sNet.0.fc1", (HU, feature)), ("sNet.0.fc2", (HU, HU + MSG * mc)), ("sNet.0.fc3", (MSG, HU))]
    for q in ("critic.0.baseQ1", "critic.0.baseQ2"):      # the heads read [up 32 | action | parent message slot 32]
        plan += [(q + ".l1", (H1, HU + act_feature)), (q + ".l2", (H2, H1)), (q + ".l3", (1, H2))]
    plan += [("critic.0.msg_base.l1", (H1, HU)), ("critic.0.msg_base.l2", (H2, H1)), ("critic.0.msg_base.l3", (MSG * mc, H2))]
    return [q for n, s in plan for q in ((n + ".weight", s), (n + ".bias", s[:1]))]


def level_schedule(parents_list, max_children):
    """What `configure` hands to sgrl_smp_graph for the morphologies `parents_list` (one parents vector each), taken from
    smp_policy._Tree and nothing else.  Returns a dict:
      L [n_morph] limbs; offset [n_morph] first row of a morphology in `tree`;
      tree [sum L, 3 + max_children] int32, one row per limb: level | parent (-1 at a root) | slot it reads of its parent's
           outgoing message (mirrored at the root of a flipped structure) | children (limb indices, -1 = empty slot);
      levels: tree levels of the deepest morphology = level steps of a forward of the batch; max_children.
    Host only.  `_lib.SgrlError` when a limb has more children than max_children."""
    mc = int(max_children)
    if not 1 <= mc <= MAX_CHILDREN:
        raise _lib.SgrlError("the HIP SMP forward takes 1 <= max_children <= %d, not %d" % (MAX_CHILDREN, mc))
    rows, Ls, offs, levels = [], [], [], 0
    for parents in parents_list:
        parents = [int(p) for p in parents]
        for i in range(len(parents)):
            n = parents.count(i)
            if n > mc:
                raise _lib.SgrlError("limb %d of the morphology with parents %s has %d children, the policy's max_children is %d"
                                     % (i, parents, n, mc))
        tr = _Tree(parents, mc)
        level = [0] * tr.L
        for d, members in enumerate(tr.levels):
            for i in members:
                level[i] = d
        offs.append(sum(Ls))
        Ls.append(tr.L)
        levels = max(levels, len(tr.levels))
        for i in range(tr.L):
            rows.append([level[i], tr.parents[i] if tr.parents[i] >= 0 else -1, tr.slot[i]] + list(tr.children[i]))
    return {"L": np.asarray(Ls, dtype=np.int32), "offset": np.asarray(offs, dtype=np.int32),
            "tree": np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 3 + mc)), "levels": int(levels),
            "max_children": mc}


def _bind(L):
    if getattr(L, "_smp_bound", False):
        return
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.sgrl_smp_create.argtypes = [ctypes.POINTER(vp)]
    L.sgrl_smp_create.restype = ci
    L.sgrl_smp_destroy.argtypes = [vp]
    L.sgrl_smp_destroy.restype = None
    L.sgrl_smp_bind_params.argtypes = [vp, vp, ci, ci, ci, ci]
    L.sgrl_smp_bind_params.restype = ci
    L.sgrl_smp_graph.argtypes = [vp, ci, vp, vp, ci, vp]
    L.sgrl_smp_graph.restype = ci
    L.sgrl_smp_forward.argtypes = [vp, vp, ci, vp, ci, ctypes.c_float, vp]
    L.sgrl_smp_forward.restype = ci
    cf = ctypes.c_float
    L.sgrl_smp_bind_critic_params.argtypes = [vp, vp, ci, ci, ci, ci]
    L.sgrl_smp_bind_critic_params.restype = ci
    L.sgrl_smp_forward_q.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp]
    L.sgrl_smp_forward_q.restype = ci
    L.sgrl_smp_td_target.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, cf, cf, cf, vp, vp]
    L.sgrl_smp_td_target.restype = ci
    L.sgrl_smp_forward_q_launches.argtypes = [vp, ci]
    L.sgrl_smp_forward_q_launches.restype = ci
    L.sgrl_smp_td_target_launches.argtypes = [vp]
    L.sgrl_smp_td_target_launches.restype = ci
    for name in ("sgrl_smp_num_nodes", "sgrl_smp_num_levels", "sgrl_smp_launches"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = ci
    L.sgrl_smp_generation.argtypes = [vp]
    L.sgrl_smp_generation.restype = ctypes.c_int64
    L.sgrl_smp_last_error.argtypes = []
    L.sgrl_smp_last_error.restype = ctypes.c_char_p
    L._smp_bound = True


def _check(L, rc, what):
    if rc != 0:
        raise _lib.SgrlError("%s failed (%d): %s" % (what, rc, L.sgrl_smp_last_error().decode()))


class HipSmpActor(object):
    """HIP forward of an `ActorGraphPolicy` built with td and bu."""

    def _describe(self, policy):
        self.feature, self.out_dim, self.max_children = _config(policy)
        self.plan = plan_params(policy)

    def _bind_call(self, arr, n):
        _check(self.L, self.L.sgrl_smp_bind_params(self.h, arr, n, self.max_children, self.feature, self.out_dim), "sgrl_smp_bind_params")

    def __init__(self, policy, device=None):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("%s needs an MI355X (no CPU fallback)" % type(self).__name__)
        self.L = _lib.lib()
        _bind(self.L)
        self.policy = policy
        self._describe(policy)
        self.device = torch.device(device) if device is not None else next(policy.parameters()).device
        if self.device.type != "cuda":
            raise _lib.SgrlError("the %s must live on the GPU for the HIP path" % type(policy).__name__)
        h = ctypes.c_void_p()
        _check(self.L, self.L.sgrl_smp_create(ctypes.byref(h)), "sgrl_smp_create")
        self.h = h
        self._bound = None
        self._cfg_key = None
        self._cfg_info = {}
        self.n_env = 0
        self.max_limbs = 0
        self.num_nodes = 0
        self.num_levels = 0

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.sgrl_smp_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- weights ------------------------------------------------------------------------------------
    def _params(self):
        named = dict(self.policy.named_parameters())       # the shared modules are listed once, at index 0
        return [named[n] for n, _ in self.plan]

    def sync_weights(self, force=False):
        """Bind the handle to the parameters' storage (include/sgrl_smp.h sgrl_smp_bind_params).  The VALUES are read by every
        forward; this binds again only when a parameter's address moved (module.to(), re-created tensors) or with force."""
        params = self._params()
        ptrs = tuple(p.data_ptr() for p in params)
        if not force and ptrs == self._bound:
            return
        for (name, shape), p in zip(self.plan, params):
            if not (p.is_cuda and p.device == self.device and p.dtype == torch.float32 and p.is_contiguous()
                    and tuple(p.shape) == tuple(shape) and p.data_ptr() % 16 == 0):
                raise _lib.SgrlError("SMP parameter %s must be a contiguous, 16-byte aligned float32 %s tensor on %s (got %s %s on %s)"
                                     % (name, tuple(shape), self.device, p.dtype, tuple(p.shape), p.device))
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        self._bind_call(ctypes.cast(arr, ctypes.c_void_p), len(ptrs))
        self._bound = ptrs

    def hold_weights(self, hold=True):
        """No-op apart from binding: nothing is packed, every forward reads the live parameters (HipSetActor.hold_weights
        promises stability so that a packed copy can be reused; there is no copy here)."""
        self.sync_weights()

    # ---- batch structure ------------------------------------------------------------------------------
    def configure(self, graphs, counts):
        """graphs: per-morphology dicts with 'parents'; counts: envs each.  Structures seen before are switched to without
        device work (the library caches them by content).  `_lib.SgrlError` when a limb has more children than the policy's
        max_children, or a morphology more than 16 limbs or tree levels."""
        key = (tuple(graph_key(g) for g in graphs), tuple(int(c) for c in counts))
        if key == self._cfg_key:
            return
        args = self._cfg_info.get(key)
        if args is None:
            sch = level_schedule([g["parents"] for g in graphs], self.max_children)
            args = (sch["L"], np.asarray(counts, dtype=np.int32), sch["tree"])
            if len(self._cfg_info) >= 64:
                self._cfg_info.clear()
            self._cfg_info[key] = args
        Ls, cnt, tree = args
        vp = lambda a: ctypes.c_void_p(a.ctypes.data)
        _check(self.L, self.L.sgrl_smp_graph(self.h, len(Ls), vp(Ls), vp(cnt), self.max_children, vp(tree)), "sgrl_smp_graph")
        self._cfg_key = key
        self.n_env = int(cnt.sum())
        self.max_limbs = int(Ls.max())
        self.num_nodes = self.L.sgrl_smp_num_nodes(self.h)
        self.num_levels = self.L.sgrl_smp_num_levels(self.h)

    def launches(self):
        """Kernel launches of one forward of the current batch structure: 6 x its tree levels."""
        return int(self.L.sgrl_smp_launches(self.h))

    def generation(self):
        return int(self.L.sgrl_smp_generation(self.h))

    @staticmethod
    def _ld(t):
        return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])

    def forward_batch(self, obs, out=None, act_ld=None):
        """obs: float32 CUDA [n_env, obs_ld] -> actions float32 [n_env, act_ld] (ActorGraphPolicy.forward for every environment;
        slots beyond out * L_e of a row are exact zeros)."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.stride(1) == 1
        assert obs.shape[0] == self.n_env
        assert obs.shape[1] >= self.feature * self.max_limbs, "observation rows narrower than feature * max_limbs"
        self.sync_weights()
        act_ld = act_ld or self.out_dim * self.max_limbs
        assert act_ld >= self.out_dim * self.max_limbs, "action rows narrower than out * max_limbs"
        if out is None:
            out = torch.empty((self.n_env, act_ld), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.shape == (self.n_env, act_ld)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_smp_forward(self.h, ctypes.c_void_p(obs.data_ptr()), self._ld(obs),
                                               ctypes.c_void_p(out.data_ptr()), int(act_ld),
                                               ctypes.c_float(float(self.policy.max_action)), stream), "sgrl_smp_forward")
        return out

    def forward_single(self, state, graph):
        """ActorGraphPolicy.forward(state [B, feature * L]) for one morphology."""
        self.configure([graph], [state.shape[0]])
        return self.forward_batch(state.contiguous().float(), act_ld=self.out_dim * len(graph["parents"]))


class HipSmpCritic(HipSmpActor):
    """HIP forward of a `CriticGraphPolicy` built with td and bu (inference only: the TD3 target values, reference
    agent.py:136-148).  One handle serves both heads: they share the trunk, the twin forward is one chain on the caller's stream.
    Weights, batch structure, `generation` and re-binding as on `HipSmpActor`."""

    def _describe(self, module):
        self.feature, self.act_feature, self.max_children = _critic_config(module)
        self.out_dim = 1
        self.plan = plan_critic_params(module)

    def _bind_call(self, arr, n):
        _check(self.L, self.L.sgrl_smp_bind_critic_params(self.h, arr, n, self.max_children, self.feature, self.act_feature),
               "sgrl_smp_bind_critic_params")

    def __init__(self, module, device=None):
        super().__init__(module, device=device)
        self.module = module
        self.sync_weights()           # the library sizes a critic's workspace by the handle's kind: bound before any structure

    def launches(self, twin=True):
        """Kernel launches of one forward_q of the current batch structure: 6 x its tree levels + 2 + twin."""
        return int(self.L.sgrl_smp_forward_q_launches(self.h, int(bool(twin))))

    def check_rows(self, t, per_limb, what):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == self.n_env, what
        assert t.shape[1] >= per_limb * self.max_limbs, "%s rows narrower than %d * max_limbs" % (what, per_limb)

    def forward_batch(self, *a, **k):
        raise _lib.SgrlError("a critic's handle has no action forward: use forward_q")

    def forward_q(self, obs, action, twin=True):
        """obs [n_env, obs_ld], action [n_env, act_ld] (float32 CUDA, the limbs of an environment contiguous in its row) ->
        (q1, q2) float32 [n_env, 1] each (CriticGraphPolicy.forward for every environment), or q1 alone with twin=False
        (CriticGraphPolicy.Q1; bit-identical to the twin call's q1)."""
        self.check_rows(obs, self.feature - self.act_feature, "observation")
        self.check_rows(action, self.act_feature, "action")
        self.sync_weights()
        out = torch.empty((2 if twin else 1, self.n_env, 1), dtype=torch.float32, device=self.device)
        vp = ctypes.c_void_p
        stream = vp(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_smp_forward_q(self.h, vp(obs.data_ptr()), self._ld(obs), vp(action.data_ptr()), self._ld(action),
                                                 vp(out[0].data_ptr()), vp(out[1].data_ptr()) if twin else vp(None), stream),
               "sgrl_smp_forward_q")
        return (out[0], out[1]) if twin else out[0]

    def forward_single(self, state, action, graph, twin=True):
        """CriticGraphPolicy.forward(state [B, 41 L], action [B, 3 L]) for one morphology."""
        self.configure([graph], [state.shape[0]])
        return self.forward_q(state.contiguous().float(), action.contiguous().float(), twin=twin)


class HipSmpTargets(object):
    """The no-grad half of a TD3 update of an SMP agent (reference src/agent.py:126-148) on the HIP path: the handles of the
    target actor (`ActorGraphPolicy`) and the twin target critic (`CriticGraphPolicy`), and `target_q` over sgrl_smp_td_target.
    The noisy target action and the per-limb Q values never leave the library's workspace."""

    def __init__(self, actor_target, critic_target):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("HipSmpTargets needs an MI355X (no CPU fallback)")
        self.actor = actor_target.hip_handle()        # cached on the modules (dropped when they are pickled / deep-copied)
        self.critic = critic_target.hip_handle()
        self.L, self.device = self.actor.L, self.actor.device
        if self.critic.feature != self.actor.feature + self.actor.out_dim or self.critic.act_feature != self.actor.out_dim:
            raise _lib.SgrlError("the target critic must take the target actor's feature + out inputs per limb")
        if self.critic.max_children != self.actor.max_children:
            raise _lib.SgrlError("target actor and target critic must have the same max_children")

    def configure(self, graphs, counts):
        self.actor.configure(graphs, counts)
        self.critic.configure(graphs, counts)

    def launches(self):
        """Kernel launches of one target chain of the current batch structure: 12 x its tree levels + 3."""
        return int(self.L.sgrl_smp_td_target_launches(self.critic.h))

    def target_q(self, next_obs, noise, reward, done, graph, noise_clip, discount, counts=None, out=None):
        """reward + (1 - done) * discount * min(Q1_t, Q2_t)(next_obs, clamp(actor_t(next_obs) + clamp(noise, +-noise_clip),
        +-max_action)) -> float32 [B, 1].  next_obs [B, >= 41 Lmax], noise [B, >= 3 Lmax] (the unclipped draw, laid out like an
        action row), reward / done [B] or [B, 1].  graph: the morphology's graph dict, or a list of them with `counts`
        environments each (row blocks in that order)."""
        graphs = graph if isinstance(graph, (list, tuple)) else [graph]
        self.configure(graphs, counts if counts is not None else [next_obs.shape[0]])
        a, c = self.actor, self.critic
        c.check_rows(next_obs, a.feature, "observation")
        c.check_rows(noise, a.out_dim, "noise")
        reward, done = reward.reshape(-1).contiguous(), done.reshape(-1).contiguous()
        for t in (reward, done):
            assert t.is_cuda and t.dtype == torch.float32 and t.shape[0] == a.n_env
        a.sync_weights()
        c.sync_weights()
        if out is None:
            out = torch.empty((a.n_env, 1), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.shape == (a.n_env, 1) and out.dtype == torch.float32
        vp, cf = ctypes.c_void_p, ctypes.c_float
        stream = vp(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_smp_td_target(a.h, c.h, vp(next_obs.data_ptr()), a._ld(next_obs), vp(noise.data_ptr()),
                                                 a._ld(noise), vp(reward.data_ptr()), vp(done.data_ptr()),
                                                 cf(float(a.policy.max_action)), cf(float(noise_clip)), cf(float(discount)),
                                                 vp(out.data_ptr()), stream), "sgrl_smp_td_target")
        return out
