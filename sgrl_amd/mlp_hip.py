"""Batched HIP forwards of the monolithic MLP agent (csrc/mlp_actor.hip, C ABI in include/sgrl_mlp.h): the actor, the twin critic
and the TD3 target chain, one launch each; and of the gradient half of its TD3 update (csrc/mlp_train.hip, `HipMlpGrads`) and its
optimizer half (csrc/mlp_optim.hip, `HipMlpOptim`: clip, Adam and the soft target update of a network in two launches).

`HipMlpActor` binds the `nn.Linear` parameters of an `MlpPolicy` (mlp_policy.py, reference-compatible state_dict) to a handle BY
ADDRESS.  The library pads the widths in a packed copy of its own (`plan`), built by one pack launch at the top of a forward;
`hold_weights(True)` is the caller's promise that the parameters stay put until the next `hold_weights` / `weights_changed`, so a
collection round packs once.  The forward of all environments is ONE launch.  It has the surface `Rollout` uses on the other
actors (`configure`, `forward_batch`, `hold_weights`, `sync_weights`, `n_env`, `max_limbs`).  No CPU fallback: without the MI355X
every device entry point raises `_lib.SgrlError`; `plan` and `chain_plan` alone are host-side.

`HipMlpCritic` binds the two Q stacks of an `MlpCritic` the same way (one packed buffer, one pack launch); `HipMlpTargets` runs the
no-grad half of a TD3 update (target actor -> clipped noise -> clamp -> twin target critics -> min -> Bellman target) as ONE launch
of the fused chain kernel over the two handles.  `batch_stats` is the update's prologue (csrc/mlp_batch.hip: the scaled reward and its
two statistics, one launch); with it td3.GraphedMlpUpdates records a whole update as a chain of this file's launches."""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_HIDDEN, MAX_WIDTH, TILE_ROWS = 4, 1024, 32


def _bind(L):
    if getattr(L, "_mlp_bound", False):
        return
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.sgrl_mlp_plan.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.sgrl_mlp_plan.restype = ci
    L.sgrl_mlp_create.argtypes = [ctypes.POINTER(vp)]
    L.sgrl_mlp_create.restype = ci
    L.sgrl_mlp_destroy.argtypes = [vp]
    L.sgrl_mlp_destroy.restype = None
    L.sgrl_mlp_set_params.argtypes = [vp, vp, ci, vp, ci]
    L.sgrl_mlp_set_params.restype = ci
    L.sgrl_mlp_hold_weights.argtypes = [vp, ci]
    L.sgrl_mlp_hold_weights.restype = ci
    L.sgrl_mlp_configure.argtypes = [vp, ci, vp, vp, ci, ci]
    L.sgrl_mlp_configure.restype = ci
    L.sgrl_mlp_forward.argtypes = [vp, vp, ci, vp, ci, ctypes.c_float, vp]
    L.sgrl_mlp_forward.restype = ci
    L.sgrl_mlp_set_critic_params.argtypes = [vp, vp, ci, vp, ci]
    L.sgrl_mlp_set_critic_params.restype = ci
    L.sgrl_mlp_critic_forward.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp]
    L.sgrl_mlp_critic_forward.restype = ci
    cf = ctypes.c_float
    L.sgrl_mlp_td_target.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, cf, cf, cf, vp, vp, ci, vp]
    L.sgrl_mlp_td_target.restype = ci
    L.sgrl_mlp_chain_plan.argtypes = [vp, ci, vp, ci, vp]
    L.sgrl_mlp_chain_plan.restype = ci
    L.sgrl_mlp_train_plan.argtypes = [vp, ci, vp, ci, ci, vp, vp]
    L.sgrl_mlp_train_plan.restype = ci
    L.sgrl_mlp_bind_grads.argtypes = [vp, vp, ci]
    L.sgrl_mlp_bind_grads.restype = ci
    L.sgrl_mlp_critic_step_grads.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp]
    L.sgrl_mlp_critic_step_grads.restype = ci
    L.sgrl_mlp_actor_step_grads.argtypes = [vp, vp, vp, ci, cf, vp, vp, ci, vp]
    L.sgrl_mlp_actor_step_grads.restype = ci
    cd = ctypes.c_double
    L.sgrl_mlp_optim_plan.argtypes = [vp, ci, ci, vp]
    L.sgrl_mlp_optim_plan.restype = ci
    L.sgrl_mlp_bind_optim.argtypes = [vp, vp, vp, ci, vp, ci, vp, ci, vp, ctypes.c_int64]
    L.sgrl_mlp_bind_optim.restype = ci
    L.sgrl_mlp_optim_bound.argtypes = [vp]
    L.sgrl_mlp_optim_bound.restype = ci
    L.sgrl_mlp_optim_step.argtypes = [vp, cd, cd, cd, cd, cf, cf, vp]
    L.sgrl_mlp_optim_step.restype = ci
    L.sgrl_mlp_batch_stats.argtypes = [vp, ci, cf, vp, vp, vp]
    L.sgrl_mlp_batch_stats.restype = ci
    for name in ("sgrl_mlp_forward_launches", "sgrl_mlp_pack_launches", "sgrl_mlp_td_target_launches", "sgrl_mlp_critic_forward_launches",
                 "sgrl_mlp_critic_step_launches", "sgrl_mlp_actor_step_launches", "sgrl_mlp_optim_step_launches", "sgrl_mlp_batch_stats_launches"):
        getattr(L, name).argtypes = []
        getattr(L, name).restype = ci
    L.sgrl_mlp_num_envs.argtypes = [vp]
    L.sgrl_mlp_num_envs.restype = ci
    L.sgrl_mlp_generation.argtypes = [vp]
    L.sgrl_mlp_generation.restype = ctypes.c_int64
    L.sgrl_mlp_last_error.argtypes = []
    L.sgrl_mlp_last_error.restype = ctypes.c_char_p
    L._mlp_bound = True


def _check(L, rc, what):
    if rc != 0:
        raise _lib.SgrlError("%s failed (%d): %s" % (what, rc, L.sgrl_mlp_last_error().decode()))


def linears(net):
    """The nn.Linear layers of an MLP stack (`networks` Sequential of mlp_policy.MLPNetwork) in order."""
    return [m for m in net.networks if isinstance(m, torch.nn.Linear)]


def net_dims(net):
    """[input, hidden widths ..., output] of an MLP stack."""
    ls = linears(net)
    for a, b in zip(ls[:-1], ls[1:]):
        assert a.out_features == b.in_features
    return [int(ls[0].in_features)] + [int(l.out_features) for l in ls]


def plan(dims, n_env=None):
    """What the library does with the widths `dims` = [input, hidden ..., output] (include/sgrl_mlp.h sgrl_mlp_plan; host only, no
    device needed): dict of kpad / npad per layer, float offsets w_off / b_off into the packed buffer, its size `total`, the
    kernel variant (`chunks` of 256 columns, panel depth `bk`), `lds_bytes`, the activation tile's row stride `sx`, `tile_rows`
    and, with n_env, the number of workgroups `tiles`."""
    L = _lib.lib()
    _bind(L)
    d = np.asarray(dims, dtype=np.int32)
    nl = max(len(d) - 1, 1)
    kpad, npad = np.zeros(nl, dtype=np.int32), np.zeros(nl, dtype=np.int32)
    w_off, b_off = np.zeros(nl, dtype=np.int64), np.zeros(nl, dtype=np.int64)
    info, total = np.zeros(4, dtype=np.int32), np.zeros(1, dtype=np.int64)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    _check(L, L.sgrl_mlp_plan(vp(d), len(d), vp(kpad), vp(npad), vp(w_off), vp(b_off), vp(info), vp(total)), "sgrl_mlp_plan")
    out = {"kpad": kpad.tolist(), "npad": npad.tolist(), "w_off": w_off.tolist(), "b_off": b_off.tolist(), "total": int(total[0]),
           "chunks": int(info[0]), "bk": int(info[1]), "lds_bytes": int(info[2]), "sx": int(info[3]), "tile_rows": TILE_ROWS}
    if n_env is not None:
        out["tiles"] = (int(n_env) + TILE_ROWS - 1) // TILE_ROWS
    return out


def chain_plan(actor_dims, critic_dims):
    """What the fused target-chain kernel uses for an actor / critic pair (include/sgrl_mlp.h sgrl_mlp_chain_plan; host only): dict
    of `chunks` (the larger of the two plans), panel depth `bk`, `lds_bytes`, the activation tile's row stride `sx` (from the widest
    padded input of either network) and `tile_rows`.  Raises for a critic whose last width is not 1 or whose input is not the
    actor's input + output width."""
    L = _lib.lib()
    _bind(L)
    a, c = np.asarray(actor_dims, dtype=np.int32), np.asarray(critic_dims, dtype=np.int32)
    info = np.zeros(4, dtype=np.int32)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    _check(L, L.sgrl_mlp_chain_plan(vp(a), len(a), vp(c), len(c), vp(info)), "sgrl_mlp_chain_plan")
    return {"chunks": int(info[0]), "bk": int(info[1]), "lds_bytes": int(info[2]), "sx": int(info[3]), "tile_rows": TILE_ROWS}


def train_plan(actor_dims, critic_dims, batch):
    """What the gradient half of an update uses for an actor / critic pair at `batch` rows (include/sgrl_mlp.h sgrl_mlp_train_plan;
    host only): dict of `chunks`, panel depth `bk`, `lds_bytes`, activation row stride `sx`, the weight-gradient workgroups of a
    critic / an actor step (`critic_wgrad_tiles`, `actor_wgrad_tiles`), `row_tiles`, and the floats of the two handles' workspaces
    (`critic_ws_floats`, `actor_ws_floats`).  Raises for what chain_plan refuses and for widths the path does not serve (a padded
    layer width above 512)."""
    L = _lib.lib()
    _bind(L)
    a, c = np.asarray(actor_dims, dtype=np.int32), np.asarray(critic_dims, dtype=np.int32)
    info, ws = np.zeros(7, dtype=np.int32), np.zeros(2, dtype=np.int64)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    _check(L, L.sgrl_mlp_train_plan(vp(a), len(a), vp(c), len(c), int(batch), vp(info), vp(ws)), "sgrl_mlp_train_plan")
    return {"chunks": int(info[0]), "bk": int(info[1]), "lds_bytes": int(info[2]), "sx": int(info[3]), "critic_wgrad_tiles": int(info[4]),
            "actor_wgrad_tiles": int(info[5]), "row_tiles": int(info[6]), "critic_ws_floats": int(ws[0]), "actor_ws_floats": int(ws[1]),
            "tile_rows": TILE_ROWS}


def optim_plan(dims, n_stacks):
    """How the optimizer half cuts a handle of `n_stacks` stacks (1: an actor, 2: a critic) of the widths `dims` (include/sgrl_mlp.h
    sgrl_mlp_optim_plan; host only): dict of `tensors`, `elements`, `chunks` (= workgroups of either launch) and `chunk` (elements
    of a chunk).  Raises for what `plan` refuses, other stack counts, and two stacks whose last width is not 1."""
    L = _lib.lib()
    _bind(L)
    d = np.asarray(dims, dtype=np.int32)
    info = np.zeros(4, dtype=np.int64)
    _check(L, L.sgrl_mlp_optim_plan(ctypes.c_void_p(d.ctypes.data), len(d), int(n_stacks), ctypes.c_void_p(info.ctypes.data)), "sgrl_mlp_optim_plan")
    return {"tensors": int(info[0]), "elements": int(info[1]), "chunks": int(info[2]), "chunk": int(info[3])}


class _HipMlpHandle(object):
    """What the actor's and the critic's handles share: the library handle, the parameters bound by address (`nets`: the MLP
    stacks in the order the bind takes them, all of the widths `dims`), the weight hold and the batch structure.  `per_limb`:
    the two per-limb sizes sgrl_mlp_configure checks the limb counts with."""

    def __init__(self, module, nets, dims, per_limb, num_limbs, device=None):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("%s needs an MI355X (no CPU fallback)" % type(self).__name__)
        self.L = _lib.lib()
        _bind(self.L)
        self.nets, self.dims, self._per_limb, self.num_limbs = list(nets), list(dims), tuple(per_limb), int(num_limbs)
        self.device = torch.device(device) if device is not None else next(self.nets[0].parameters()).device
        if self.device.type != "cuda":
            raise _lib.SgrlError("the %s must live on the GPU for the HIP path" % type(module).__name__)
        h = ctypes.c_void_p()
        _check(self.L, self.L.sgrl_mlp_create(ctypes.byref(h)), "sgrl_mlp_create")
        self.h = h
        self._bound = None
        self._cfg_key = None
        self._hold = False
        self.n_env = 0
        self.max_limbs = 0

    def _bind_call(self, arr, n, dims):
        raise NotImplementedError

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.sgrl_mlp_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- weights ------------------------------------------------------------------------------------
    def _params(self):
        return [p for net in self.nets for l in linears(net) for p in (l.weight, l.bias)]

    def sync_weights(self, force=False):
        """Bind the handle to the parameters' storage (include/sgrl_mlp.h sgrl_mlp_set_params).  The VALUES are packed at the top
        of a forward (see hold_weights); this binds again only when a parameter's address moved or with force."""
        params = self._params()
        ptrs = tuple(p.data_ptr() for p in params)
        if not force and ptrs == self._bound:
            return
        for p in params:
            if not (p.is_cuda and p.device == self.device and p.dtype == torch.float32 and p.is_contiguous()):
                raise _lib.SgrlError("MLP parameters must be contiguous float32 tensors on %s (got %s %s on %s)"
                                     % (self.device, p.dtype, tuple(p.shape), p.device))
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        dims = np.asarray(self.dims, dtype=np.int32)
        self._bind_call(ctypes.cast(arr, ctypes.c_void_p), len(ptrs), dims)
        self._bound = ptrs
        cfg, self._cfg_key = self._cfg_key, None      # a new binding drops the batch structure: set it again
        if cfg is not None:
            self._configure(*cfg)

    def hold_weights(self, hold=True):
        """Promise that the bound parameters do not change until the next call (include/sgrl_mlp.h sgrl_mlp_hold_weights): the next
        forward packs once, the following ones reuse the packed buffer.  Every call also says "the parameters may have changed"."""
        self.sync_weights()
        _check(self.L, self.L.sgrl_mlp_hold_weights(self.h, 1 if hold else 0), "sgrl_mlp_hold_weights")
        self._hold = bool(hold)

    def weights_changed(self):
        """The parameters were just updated: a holding handle packs again on its next forward (and keeps holding)."""
        self.hold_weights(self._hold)

    # ---- batch structure ------------------------------------------------------------------------------
    def configure(self, graphs, counts):
        """graphs: per-morphology dicts with 'parents'; counts: environments each.  Every morphology must have the limb count the
        network was built for (ValueError otherwise: a monolithic network cannot read another row width)."""
        Ls = tuple(len(g["parents"]) for g in graphs)
        for k, L in enumerate(Ls):
            if L != self.num_limbs:
                raise ValueError("morphology %d has %d limbs; this MLP policy was built for %d" % (k, L, self.num_limbs))
        self.sync_weights()
        self._configure(Ls, tuple(int(c) for c in counts))

    def _configure(self, Ls, counts):
        if (Ls, counts) == self._cfg_key:
            return
        la, ca = np.asarray(Ls, dtype=np.int32), np.asarray(counts, dtype=np.int32)
        _check(self.L, self.L.sgrl_mlp_configure(self.h, len(la), ctypes.c_void_p(la.ctypes.data), ctypes.c_void_p(ca.ctypes.data),
                                                 self._per_limb[0], self._per_limb[1]), "sgrl_mlp_configure")
        self._cfg_key = (Ls, counts)
        self.n_env = int(ca.sum())
        self.max_limbs = int(la.max())

    def pack_launches(self):
        return int(self.L.sgrl_mlp_pack_launches())

    def generation(self):
        return int(self.L.sgrl_mlp_generation(self.h))

    def plan(self):
        return plan(self.dims, self.n_env or None)

    @staticmethod
    def _ld(t):
        return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])

    def check_rows(self, t, width, what):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == self.n_env, what
        assert t.shape[1] >= width, "%s rows narrower than the network's %d columns" % (what, width)


class HipMlpActor(_HipMlpHandle):
    """HIP forward of the actor network of an `MlpPolicy` (or, with `net=`, any mlp_policy.MLPNetwork followed by tanh)."""

    def __init__(self, policy, device=None, net=None):
        self.policy = policy
        self.net = net if net is not None else policy.actor
        dims = net_dims(self.net)
        self.feature, self.out_dim = int(policy.state_dim), int(policy.action_dim)
        num_limbs = dims[0] // self.feature
        if dims[0] != self.feature * num_limbs or dims[-1] != self.out_dim * num_limbs:
            raise _lib.SgrlError("the MLP maps %d -> %d values: not %d / %d per limb of one limb count"
                                 % (dims[0], dims[-1], self.feature, self.out_dim))
        super().__init__(policy, [self.net], dims, (self.feature, self.out_dim), num_limbs, device=device)

    def _bind_call(self, arr, n, dims):
        _check(self.L, self.L.sgrl_mlp_set_params(self.h, arr, n, ctypes.c_void_p(dims.ctypes.data), len(dims)), "sgrl_mlp_set_params")

    def launches(self):
        """Kernel launches of the forward proper (constant: 1; a forward that packs adds `pack_launches()`)."""
        return int(self.L.sgrl_mlp_forward_launches())

    def forward_batch(self, obs, out=None, act_ld=None):
        """obs: float32 CUDA [n_env, obs_ld] -> actions float32 [n_env, act_ld] (MlpPolicy.forward for every environment; slots
        beyond out * L of a row are exact zeros)."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.stride(1) == 1
        assert obs.shape[0] == self.n_env
        assert obs.shape[1] >= self.dims[0], "observation rows narrower than the network's input"
        self.sync_weights()
        act_ld = act_ld or self.dims[-1]
        assert act_ld >= self.dims[-1], "action rows narrower than the network's output"
        if out is None:
            out = torch.empty((self.n_env, act_ld), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.shape == (self.n_env, act_ld)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_mlp_forward(self.h, ctypes.c_void_p(obs.data_ptr()), self._ld(obs),
                                               ctypes.c_void_p(out.data_ptr()), int(act_ld),
                                               ctypes.c_float(float(self.policy.max_action)), stream), "sgrl_mlp_forward")
        return out

    def forward_single(self, state, graph):
        """MlpPolicy.forward(state [B, feature * L])."""
        self.configure([graph], [state.shape[0]])
        return self.forward_batch(state.contiguous().float())


class HipMlpCritic(_HipMlpHandle):
    """HIP forward of an `MlpCritic` (inference only: the TD3 target values).  One handle serves both Q stacks: they share one
    packed buffer and one pack launch, the twin forward is one launch.  Weights, batch structure, `hold_weights`, `generation` and
    re-binding as on `HipMlpActor`."""

    def __init__(self, module, device=None):
        self.module = module
        dims = net_dims(module.critic1)
        if net_dims(module.critic2) != dims or dims[-1] != 1:
            raise _lib.SgrlError("an MlpCritic's two stacks must have the same widths and one output (got %s / %s)"
                                 % (dims, net_dims(module.critic2)))
        self.feature, self.act_feature = int(module.state_dim), int(module.action_dim)
        per_limb = self.feature + self.act_feature
        num_limbs = dims[0] // per_limb
        if dims[0] != per_limb * num_limbs:
            raise _lib.SgrlError("the critic reads %d values: not %d + %d per limb of one limb count" % (dims[0], self.feature, self.act_feature))
        super().__init__(module, [module.critic1, module.critic2], dims, (self.feature, self.act_feature), num_limbs, device=device)

    def _bind_call(self, arr, n, dims):
        _check(self.L, self.L.sgrl_mlp_set_critic_params(self.h, arr, n, ctypes.c_void_p(dims.ctypes.data), len(dims)),
               "sgrl_mlp_set_critic_params")

    def launches(self):
        """Kernel launches of one forward_q, twin or not (constant: 1; a forward that packs adds `pack_launches()`)."""
        return int(self.L.sgrl_mlp_critic_forward_launches())

    def forward_q(self, obs, action, twin=True):
        """obs [n_env, >= 41 L], action [n_env, >= 3 L] (float32 CUDA) -> (q1, q2) float32 [n_env, 1] each (MlpCritic.forward for
        every environment), or q1 alone with twin=False (MlpCritic.Q1; bit-identical to the twin call's q1)."""
        self.check_rows(obs, self.feature * self.num_limbs, "observation")
        self.check_rows(action, self.act_feature * self.num_limbs, "action")
        self.sync_weights()
        out = torch.empty((2 if twin else 1, self.n_env, 1), dtype=torch.float32, device=self.device)
        vp = ctypes.c_void_p
        stream = vp(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_mlp_critic_forward(self.h, vp(obs.data_ptr()), self._ld(obs), vp(action.data_ptr()), self._ld(action),
                                                      vp(out[0].data_ptr()), vp(out[1].data_ptr()) if twin else vp(None), stream),
               "sgrl_mlp_critic_forward")
        return (out[0], out[1]) if twin else out[0]

    def forward_single(self, state, action, graph, twin=True):
        """MlpCritic.forward(state [B, 41 L], action [B, 3 L])."""
        self.configure([graph], [state.shape[0]])
        return self.forward_q(state.contiguous().float(), action.contiguous().float(), twin=twin)


def _action_out_arg(action_out, n_env, width):
    """(address, leading dimension) of an optional `action_out` [n_env, >= width]; a null address and 0 for None."""
    if action_out is None:
        return ctypes.c_void_p(None), 0
    assert action_out.is_cuda and action_out.dtype == torch.float32 and action_out.is_contiguous() and action_out.dim() == 2
    assert action_out.shape[0] == n_env and action_out.shape[1] >= width, "action_out rows narrower than the actor's output"
    return ctypes.c_void_p(action_out.data_ptr()), int(action_out.shape[1])


class HipMlpTargets(object):
    """The no-grad half of a TD3 update of an MLP agent (reference src/agent.py:126-148) on the HIP path: the handles of the target
    actor (`MlpPolicy`) and the twin target critic (`MlpCritic`), and `target_q` over sgrl_mlp_td_target -- ONE launch (plus one pack
    per handle: the handles do not hold, so every chain reads the live target parameters)."""

    def __init__(self, actor_target, critic_target):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("HipMlpTargets needs an MI355X (no CPU fallback)")
        self.actor = actor_target.hip_handle()        # cached on the modules (dropped when they are pickled / deep-copied)
        self.critic = critic_target.hip_handle()
        self.L, self.device = self.actor.L, self.actor.device
        a, c = self.actor, self.critic
        if c.dims[0] != a.dims[0] + a.dims[-1] or c.feature != a.feature or c.act_feature != a.out_dim:
            raise _lib.SgrlError("the target critic must read the target actor's input + output (%d + %d values), not %d"
                                 % (a.dims[0], a.dims[-1], c.dims[0]))

    def configure(self, graphs, counts):
        self.actor.configure(graphs, counts)
        self.critic.configure(graphs, counts)

    def launches(self):
        """Kernel launches of the chain proper (constant: 1; each handle that packs adds `pack_launches()`)."""
        return int(self.L.sgrl_mlp_td_target_launches())

    def plan(self):
        return chain_plan(self.actor.dims, self.critic.dims)

    def target_q(self, next_obs, noise, reward, done, graph, noise_clip, discount, counts=None, out=None, action_out=None):
        """reward + (1 - done) * discount * min(Q1_t, Q2_t)(next_obs, clamp(actor_t(next_obs) + clamp(noise, +-noise_clip),
        +-max_action)) -> float32 [B, 1].  next_obs [B, >= 41 L], noise [B, >= 3 L] (the unclipped draw, laid out like an action
        row), reward / done [B] or [B, 1].  graph: the morphology's graph dict (a list of them with `counts`; None: the limb count
        the networks were built for).  action_out: float32 [B, >= 3 L] contiguous, receives the noisy clamped target action (exact
        zeros beyond 3 L).  Both the tanh head and the final clamp use the target policy's `max_action` (td3.Agent refuses the HIP
        chain when args.max_action differs from it)."""
        a, c = self.actor, self.critic
        if graph is None:
            graph = {"parents": [0] * a.num_limbs}
        graphs = graph if isinstance(graph, (list, tuple)) else [graph]
        self.configure(graphs, counts if counts is not None else [next_obs.shape[0]])
        c.check_rows(next_obs, a.dims[0], "observation")
        c.check_rows(noise, a.dims[-1], "noise")
        reward, done = reward.reshape(-1).contiguous(), done.reshape(-1).contiguous()
        for t in (reward, done):
            assert t.is_cuda and t.dtype == torch.float32 and t.shape[0] == a.n_env
        a.sync_weights()
        c.sync_weights()
        if out is None:
            out = torch.empty((a.n_env, 1), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.shape == (a.n_env, 1) and out.dtype == torch.float32
        vp, cf = ctypes.c_void_p, ctypes.c_float
        act_ptr, act_ld = _action_out_arg(action_out, a.n_env, a.dims[-1])
        stream = vp(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_mlp_td_target(a.h, c.h, vp(next_obs.data_ptr()), a._ld(next_obs), vp(noise.data_ptr()), a._ld(noise),
                                                 vp(reward.data_ptr()), vp(done.data_ptr()), cf(float(a.policy.max_action)),
                                                 cf(float(noise_clip)), cf(float(discount)), vp(out.data_ptr()), act_ptr, act_ld, stream),
               "sgrl_mlp_td_target")
        return out


class HipMlpGrads(object):
    """The gradient half of a TD3 update of an MLP agent (reference src/agent.py:150-177 without the clipping and the optimizer
    steps) on the HIP path: handles of its OWN on the online `MlpPolicy` and `MlpCritic` (never the modules' cached inference
    handles: those may be holding weights for a collection round), persistent contiguous float32 `.grad` tensors for every parameter,
    bound by address.  `critic_step` and `actor_step` WRITE the gradients (no zero_grad needed, nothing accumulates) and return the
    loss as a 0-d device tensor; neither synchronises with the host.  Every step packs the live parameters first.

    Stale gradients: `actor_step` computes the actor's gradients only.  Afterwards `critic.*.grad` still holds what `critic_step` and
    the caller's clipping left there, not the reference's unused accumulation from the actor pass -- the documented state of
    `Agent.update(skip_unused_critic_grads=True)`."""

    def __init__(self, actor, critic):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("HipMlpGrads needs an MI355X (no CPU fallback)")
        self.actor, self.critic = HipMlpActor(actor), HipMlpCritic(critic)
        self.L, self.device = self.actor.L, self.actor.device
        a, c = self.actor, self.critic
        self.plan(1)                                 # raises for pairs and widths the path does not serve
        self._gbound = {id(a): None, id(c): None}
        self._loss = torch.zeros(2, dtype=torch.float32, device=self.device)

    def plan(self, batch=None):
        return train_plan(self.actor.dims, self.critic.dims, batch or self.actor.n_env or 1)

    def critic_launches(self):
        """Kernel launches of one critic_step (constant: pack, row-parallel pass, weight gradients)."""
        return int(self.L.sgrl_mlp_critic_step_launches())

    def actor_launches(self):
        """Kernel launches of one actor_step (constant: two packs, row-parallel pass, weight gradients)."""
        return int(self.L.sgrl_mlp_actor_step_launches())

    def _bind_grads(self, h):
        """Parameters bound, every `.grad` a contiguous float32 tensor on the device (created where it is None or unusable), their
        addresses bound; again whenever a parameter or a `.grad` has moved."""
        h.sync_weights()
        params = h._params()
        for p in params:
            g = p.grad
            if g is None or g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.shape != p.shape:
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
        ptrs = tuple(p.grad.data_ptr() for p in params)
        if (ptrs, h._bound) != self._gbound[id(h)]:      # a parameter bind drops the gradient addresses (h._bound: what it bound)
            arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
            _check(self.L, self.L.sgrl_mlp_bind_grads(h.h, ctypes.cast(arr, ctypes.c_void_p), len(ptrs)), "sgrl_mlp_bind_grads")
            self._gbound[id(h)] = (ptrs, h._bound)
        return params

    def _configure(self, n):
        g = [{"parents": [0] * self.actor.num_limbs}]
        self.actor.configure(g, [n])
        self.critic.configure(g, [n])

    def _loss_arg(self, k, loss_out):
        """Where step k (0 critic, 1 actor) writes its loss: this object's own element, or the caller's 0-d / 1-element tensor."""
        if loss_out is None:
            return self._loss[k]
        assert loss_out.is_cuda and loss_out.dtype == torch.float32 and loss_out.numel() == 1 and loss_out.device == self.device, "loss_out"
        return loss_out

    def critic_step(self, obs, action, target_q, loss_out=None):
        """mse(Q1(obs, action), target_q) + mse(Q2(obs, action), target_q) -> 0-d device tensor; its gradient in every critic
        parameter's `.grad`.  obs [B, >= 41 L], action [B, >= 3 L], target_q [B] or [B, 1]: float32 CUDA.  loss_out: a caller-owned
        0-d or 1-element float32 device tensor that receives (and is returned as) the loss instead of this object's own."""
        c = self.critic
        self._configure(obs.shape[0])
        params = self._bind_grads(c)
        c.check_rows(obs, c.feature * c.num_limbs, "observation")
        c.check_rows(action, c.act_feature * c.num_limbs, "action")
        target_q = target_q.reshape(-1).contiguous()
        assert target_q.is_cuda and target_q.dtype == torch.float32 and target_q.shape[0] == c.n_env
        vp = ctypes.c_void_p
        loss = self._loss_arg(0, loss_out)
        stream = vp(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_mlp_critic_step_grads(c.h, vp(obs.data_ptr()), c._ld(obs), vp(action.data_ptr()), c._ld(action),
                                                         vp(target_q.data_ptr()), vp(loss.data_ptr()), stream), "sgrl_mlp_critic_step_grads")
        torch.autograd.graph.increment_version([p.grad for p in params])
        return loss

    def actor_step(self, obs, action_out=None, loss_out=None):
        """-mean(Q1(obs, actor(obs))) -> 0-d device tensor; its gradient in every ACTOR parameter's `.grad` (the critic's are left as
        they are, see the class).  action_out: float32 [B, >= 3 L] contiguous, receives actor(obs).  loss_out: as on critic_step."""
        a, c = self.actor, self.critic
        self._configure(obs.shape[0])
        params = self._bind_grads(a)
        c.sync_weights()
        a.check_rows(obs, a.dims[0], "observation")
        vp = ctypes.c_void_p
        act_ptr, act_ld = _action_out_arg(action_out, a.n_env, a.dims[-1])
        loss = self._loss_arg(1, loss_out)
        stream = vp(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_mlp_actor_step_grads(a.h, c.h, vp(obs.data_ptr()), a._ld(obs), ctypes.c_float(float(a.policy.max_action)),
                                                        vp(loss.data_ptr()), act_ptr, act_ld, stream), "sgrl_mlp_actor_step_grads")
        torch.autograd.graph.increment_version([p.grad for p in params])
        return loss

    def replayed(self, critic=True, actor=False):
        """A critic_step (and, with actor, an actor_step) ran inside a hipGraph replay, which runs no host code: bump the versions of
        the `.grad` tensors those kernels wrote, as the eager steps do after their launches."""
        wrote = [p.grad for on, h in ((critic, self.critic), (actor, self.actor)) if on for p in h._params() if p.grad is not None]
        torch.autograd.graph.increment_version(wrote)


class _OptimSide(object):
    """One network of a HipMlpOptim: the handle, its optimizer and target, and what is bound."""

    def __init__(self, handle, opt, target_nets):
        self.h, self.opt, self.target_nets = handle, opt, target_nets
        self.key = None
        self.partials = None
        self.counter = None          # plain groups: the device step counter this object owns
        self.host_step = None        # plain groups: the count `counter` holds
        self.clipped = False         # whether the last step clipped (wrote .grad)


class HipMlpOptim(object):
    """The optimizer half of a TD3 update of an MLP agent (reference src/agent.py:161-164, 174-177 and the soft updates of
    common/functional.py:7-10) on the HIP path: gradient clipping, the Adam step and, with tau > 0, the Polyak update of the target
    network, for one network in TWO launches (include/sgrl_mlp.h "optimizer half", csrc/mlp_optim.hip).  Built over the two handles
    of a `HipMlpGrads`, whose `.grad` tensors it reads; `critic_step(max_norm, tau)` / `actor_step(max_norm, tau)` replace
    `td3.clip_and_step(opt, max_norm)` followed (tau > 0) by `td3.soft_update_network(net, target, tau)`.

    The Adam state is the optimizers' own `opt.state[p]` (`exp_avg`, `exp_avg_sq`, `step`; created lazily exactly as torch.optim.Adam
    / `td3.clip_and_step` create it), so `state_dict()` is unchanged and either path continues the other's count.  Groups whose
    counters live on the device (`capturable`): those counters are bound, and the host-side count `td3.adam_step` keeps is advanced
    with them.  Plain groups (CPU counters): this object owns ONE device counter per network, filled from the state when it binds
    (and again only if somebody else has stepped the optimizer since), and advances the state's CPU counters on the host.  All
    parameters of a network must share one step count.  Neither step synchronises with the host or allocates once bound; a bind
    happens again when a parameter, gradient, state or target tensor has moved."""

    def __init__(self, grads, actor_optimizer, critic_optimizer, actor_target=None, critic_target=None):
        self.grads, self.L, self.device = grads, grads.L, grads.device
        self.actor_optimizer, self.critic_optimizer = actor_optimizer, critic_optimizer
        self.actor_target, self.critic_target = actor_target, critic_target
        for opt, h in ((actor_optimizer, grads.actor), (critic_optimizer, grads.critic)):
            why = self.refusal(opt, h._params())
            if why:
                raise _lib.SgrlError("HipMlpOptim: " + why)
        self._actor = _OptimSide(grads.actor, actor_optimizer, [actor_target.actor] if actor_target is not None else None)
        self._critic = _OptimSide(grads.critic, critic_optimizer,
                                  [critic_target.critic1, critic_target.critic2] if critic_target is not None else None)

    @staticmethod
    def refusal(opt, params=None):
        """Why this path does not serve the optimizer (None: it does): torch.optim.Adam with ONE group, no weight decay, no amsgrad,
        not maximising -- the reference's optimizers (agent.py:96-115) -- over exactly `params`."""
        if not isinstance(opt, torch.optim.Adam) or len(opt.param_groups) != 1:
            return "one torch.optim.Adam with one parameter group is served"
        g = opt.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False) or g.get("differentiable", False):
            return "weight decay, amsgrad, maximize and differentiable groups are not served"
        if isinstance(g["lr"], torch.Tensor):
            return "a tensor learning rate is not served"
        if params is not None and sorted(id(p) for p in g["params"]) != sorted(id(p) for p in params):
            return "the optimizer's group must hold exactly the network's parameters"
        return None

    def launches(self):
        """Kernel launches of one critic_step or actor_step (constant: 2)."""
        return int(self.L.sgrl_mlp_optim_step_launches())

    def plan(self):
        return {"actor": optim_plan(self.grads.actor.dims, 1), "critic": optim_plan(self.grads.critic.dims, 2)}

    def critic_step(self, max_norm, tau=0.0):
        """Clip the critic's gradients to max_norm (None / 0: no clipping), step its Adam, and with tau > 0 move the target critic."""
        self._step(self._critic, max_norm, tau)

    def actor_step(self, max_norm, tau=0.0):
        self._step(self._actor, max_norm, tau)

    def replayed(self, critic=True, actor=False, tau=None):
        """The host half of `_step` for steps that ran inside a hipGraph replay (which runs no host code): for every side named, advance
        the host-side counts -- the `_sgrl_step_class` mirrors of capturable groups; the CPU `st["step"]` tensors and this object's
        `host_step` of plain groups -- by one, and bump the version of everything the step wrote: the parameters, `.grad` when the
        step clipped (as the side's last eager or recorded step did), both moment tensors, the device counters, and the targets when it
        carried tau > 0.  tau=None: the update's rule -- the critic step carries tau > 0 exactly on policy iterations (actor=True), the
        actor step always.  Covers the gradient half too (HipMlpGrads.replayed)."""
        self.grads.replayed(critic=critic, actor=actor)
        for side in self._sides(critic, actor):
            params = side.h._params()
            states = [side.opt.state[p] for p in params]
            on_device = states[0]["step"].is_cuda
            if on_device:
                host = side.opt.__dict__.setdefault("_sgrl_step_class", {})
                for p in params:
                    host[id(p)] += 1
            else:
                for st in states:
                    st["step"] += 1
                side.host_step += 1
            wrote = list(params) + [st["exp_avg"] for st in states] + [st["exp_avg_sq"] for st in states]
            if side.clipped:
                wrote += [p.grad for p in params]
            wrote += [st["step"] for st in states] if on_device else [side.counter]
            with_tau = bool(actor) if tau is None else float(tau) > 0
            if with_tau and side.target_nets is not None:
                wrote += [p for net in side.target_nets for l in linears(net) for p in (l.weight, l.bias)]
            torch.autograd.graph.increment_version(wrote)

    def _sides(self, critic, actor):
        return [side for on, side in ((critic, self._critic), (actor, self._actor)) if on]

    def counts_current(self, critic=True, actor=False):
        """Whether a step of the sides named would need NO host-to-device traffic for its step count -- what a recorded step relies
        on: every parameter has state; capturable groups: the host mirror knows every parameter; plain groups: this object's device
        counter holds the state's CPU count (nobody else has stepped the optimizer since).  Host only."""
        for side in self._sides(critic, actor):
            params = side.h._params()
            states = [side.opt.state.get(p) for p in params]
            if any(not st for st in states):
                return False
            if states[0]["step"].is_cuda:
                host = side.opt.__dict__.get("_sgrl_step_class", {})
                if any(id(p) not in host for p in params):
                    return False
            elif side.counter is None or any(float(st["step"]) != side.host_step for st in states):
                return False
        return True

    def host_counts(self):
        """The host-side step counts of both sides, for set_host_counts: a capture runs the host half of its steps, not their kernels."""
        out = []
        for side in (self._critic, self._actor):
            states = [side.opt.state.get(p) for p in side.h._params()]
            host = side.opt.__dict__.get("_sgrl_step_class")
            out.append((side.host_step, None if host is None else dict(host),
                        [float(st["step"]) if st and not st["step"].is_cuda else None for st in states]))
        return out

    def set_host_counts(self, counts):
        for side, (host_step, host, cpu) in zip((self._critic, self._actor), counts):
            side.host_step = host_step
            if host is not None:
                side.opt.__dict__["_sgrl_step_class"] = host
            for p, c in zip(side.h._params(), cpu):
                if c is not None:
                    side.opt.state[p]["step"].fill_(c)

    def resync(self):
        """Somebody wrote the optimizers' step counts by value (td3.restore_optimizer: a checkpoint load): bring this object's
        mirrors back in line, so that counts_current() holds again and a captured step keeps running on the restored count.
        Plain groups: the device counter this object owns is filled with the state's CPU count, IN PLACE (recorded steps hold its
        address), and `host_step` follows.  Capturable groups: the host mirror `_sgrl_step_class` is read again from the device
        counters (one synchronisation per parameter, here and never in a step).  A side whose state is gone or whose parameters
        disagree forgets its count: its next step fills the counter, as after a bind."""
        for side in (self._critic, self._actor):
            params = side.h._params()
            states = [side.opt.state.get(p) for p in params]
            if any(not st for st in states):
                side.host_step = None
                continue
            if states[0]["step"].is_cuda:
                host = side.opt.__dict__.setdefault("_sgrl_step_class", {})
                for p, st in zip(params, states):
                    host[id(p)] = int(st["step"].item())
                continue
            counts = [float(st["step"]) for st in states]
            if side.counter is None or any(c != counts[0] for c in counts):
                side.host_step = None
                continue
            side.counter.fill_(counts[0])
            side.host_step = counts[0]

    def _state(self, side, params):
        """opt.state[p] of every parameter, created where empty; -> (states, True when the counters live on the device)."""
        opt = side.opt
        on_device = bool(opt.param_groups[0].get("capturable", False) or opt.param_groups[0].get("fused", False))
        states = []
        for p in params:
            st = opt.state[p]
            if len(st) == 0:                  # torch.optim.Adam's lazy state initialisation
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if on_device else torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            states.append(st)
        return states, states[0]["step"].is_cuda

    def _step(self, side, max_norm, tau):
        h, opt = side.h, side.opt
        why = self.refusal(opt)
        if why:
            raise _lib.SgrlError("HipMlpOptim: " + why)
        tau = float(tau)
        params = self.grads._bind_grads(h)                 # parameters and .grad bound (again where one has moved)
        states, on_device = self._state(side, params)
        targets = [p for net in side.target_nets for l in linears(net) for p in (l.weight, l.bias)] if side.target_nets is not None else []
        if tau > 0 and not targets:
            raise _lib.SgrlError("HipMlpOptim: tau > 0 needs the target network")
        if on_device:
            host = opt.__dict__.setdefault("_sgrl_step_class", {})      # the count td3.adam_step keeps: advanced with the counters
            for p, st in zip(params, states):
                if id(p) not in host:
                    host[id(p)] = int(st["step"].item())                # once per parameter, never in a steady step
            counts = [host[id(p)] for p in params]
        else:
            counts = [float(st["step"]) for st in states]               # CPU tensors
        if any(c != counts[0] for c in counts):
            raise _lib.SgrlError("HipMlpOptim: the parameters of a network must share one step count (got %s)" % sorted(set(counts)))
        key = (h._bound, tuple(p.grad.data_ptr() for p in params), tuple(st["exp_avg"].data_ptr() for st in states),
               tuple(st["exp_avg_sq"].data_ptr() for st in states), tuple(st["step"].data_ptr() for st in states) if on_device else None,
               tuple(t.data_ptr() for t in targets))
        if key != side.key or not self.L.sgrl_mlp_optim_bound(h.h):
            self._bind_side(side, params, states, targets, on_device)
            side.key = key
            side.host_step = None
        if not on_device:
            if side.host_step != counts[0]:                             # at the bind, or somebody else stepped the optimizer since
                side.counter.fill_(counts[0])
            side.host_step = counts[0] + 1
        group = opt.param_groups[0]
        beta1, beta2 = group["betas"]
        clip = float(max_norm) if (max_norm and max_norm > 0) else 0.0
        side.clipped = clip > 0
        cdbl, cf = ctypes.c_double, ctypes.c_float
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _check(self.L, self.L.sgrl_mlp_optim_step(h.h, cdbl(float(group["lr"])), cdbl(float(beta1)), cdbl(float(beta2)), cdbl(float(group["eps"])),
                                                  cf(clip), cf(tau), stream), "sgrl_mlp_optim_step")
        if on_device:
            for p in params:
                host[id(p)] += 1
        else:
            for st in states:
                st["step"] += 1
        wrote = list(params) + [st["exp_avg"] for st in states] + [st["exp_avg_sq"] for st in states]
        if clip > 0:
            wrote += [p.grad for p in params]
        if on_device:
            wrote += [st["step"] for st in states]
        if tau > 0:
            wrote += targets
        torch.autograd.graph.increment_version(wrote)

    def _bind_side(self, side, params, states, targets, on_device):
        h = side.h
        for t in [st[k] for st in states for k in ("exp_avg", "exp_avg_sq")] + list(targets):
            if not (t.is_cuda and t.device == self.device and t.dtype == torch.float32 and t.is_contiguous()):
                raise _lib.SgrlError("HipMlpOptim: Adam state and target parameters must be contiguous float32 tensors on %s (got %s %s on %s)"
                                     % (self.device, t.dtype, tuple(t.shape), t.device))
        for p, t in zip(params, targets):
            if t.shape != p.shape:
                raise _lib.SgrlError("HipMlpOptim: the target network's parameters must have the network's shapes")
        n = len(params)
        chunks = optim_plan(h.dims, len(h.nets))["chunks"]
        if side.partials is None or side.partials.numel() < chunks:
            side.partials = torch.zeros(chunks, dtype=torch.float32, device=self.device)
        if on_device:
            for st in states:
                if not (st["step"].is_cuda and st["step"].dtype == torch.float32):
                    raise _lib.SgrlError("HipMlpOptim: device step counters must be float32")
            steps = [st["step"].data_ptr() for st in states]
        else:
            if side.counter is None:
                side.counter = torch.zeros(1, dtype=torch.float32, device=self.device)
            steps = [side.counter.data_ptr()]
        vp = ctypes.c_void_p
        arr = lambda ptrs: ctypes.cast((vp * len(ptrs))(*ptrs), vp) if ptrs else vp(None)
        m, v = arr([st["exp_avg"].data_ptr() for st in states]), arr([st["exp_avg_sq"].data_ptr() for st in states])
        _check(self.L, self.L.sgrl_mlp_bind_optim(h.h, m, v, n, arr(steps), len(steps), arr([t.data_ptr() for t in targets]), len(targets),
                                                  vp(side.partials.data_ptr()), int(side.partials.numel())), "sgrl_mlp_bind_optim")


def batch_stats_launches():
    L = _lib.lib()
    _bind(L)
    return int(L.sgrl_mlp_batch_stats_launches())


def batch_stats(reward, scale, out, stats):
    """The batch prologue of an update (include/sgrl_mlp.h sgrl_mlp_batch_stats; ONE launch): out <- reward * scale (out may be reward
    itself), stats[0] <- mean(out), stats[1] <- the unbiased variance of out (NaN for one row).  reward, out: float32 CUDA with the
    same number of elements, contiguous; stats: float32 CUDA, 2 elements.  Asynchronous, allocates nothing.  Returns out."""
    L = _lib.lib()
    _bind(L)
    for t, what in ((reward, "reward"), (out, "out"), (stats, "stats")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == reward.device):
            raise _lib.SgrlError("batch_stats: %s must be a contiguous float32 tensor on the reward's GPU" % what)
    if out.numel() != reward.numel() or stats.numel() != 2:
        raise _lib.SgrlError("batch_stats: out must have the reward's %d elements and stats 2 (got %d and %d)"
                             % (reward.numel(), out.numel(), stats.numel()))
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(reward.device).cuda_stream)
    _check(L, L.sgrl_mlp_batch_stats(vp(reward.data_ptr()), int(reward.numel()), ctypes.c_float(float(scale)), vp(out.data_ptr()),
                                     vp(stats.data_ptr()), stream), "sgrl_mlp_batch_stats")
    torch.autograd.graph.increment_version([out, stats])
    return out
