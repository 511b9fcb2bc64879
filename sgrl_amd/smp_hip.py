"""Batched HIP forward of the SMP actor (csrc/smp_actor.hip, C ABI in include/sgrl_smp.h).

`HipSmpActor` binds the parameters of an `ActorGraphPolicy` in its published mode (`td and bu`; smp_policy.py,
reference-compatible state_dict) to a handle BY ADDRESS: nothing is packed, the library reads the live tensors on every
forward, so optimizer steps, soft updates, `load_state_dict` and in-place broadcasts need no notification; only a parameter
whose storage MOVES (`.to()`, re-created tensors) needs a re-bind, which `sync_weights` does by itself.  It has the surface
`Rollout` uses on `HipSetActor` / `HipSwatActor` (`configure`, `forward_batch`, `hold_weights`, `sync_weights`, `n_env`,
`max_limbs`).  The tree schedule (levels, children rows, message slots) comes from `smp_policy._Tree` alone: `level_schedule`
lays it out as the rows the library takes.  No CPU fallback: without the MI355X every entry point raises `_lib.SgrlError`.
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

    def __init__(self, policy, device=None):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("HipSmpActor needs an MI355X (no CPU fallback)")
        self.L = _lib.lib()
        _bind(self.L)
        self.policy = policy
        self.feature, self.out_dim, self.max_children = _config(policy)
        self.device = torch.device(device) if device is not None else next(policy.parameters()).device
        if self.device.type != "cuda":
            raise _lib.SgrlError("the ActorGraphPolicy must live on the GPU for the HIP path")
        self.plan = plan_params(policy)
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
        _check(self.L, self.L.sgrl_smp_bind_params(self.h, ctypes.cast(arr, ctypes.c_void_p), len(ptrs), self.max_children,
                                                   self.feature, self.out_dim), "sgrl_smp_bind_params")
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
