"""Batched HIP forwards of the SWAT actor and critics (csrc/swat_actor.hip, C ABI in include/sgrl_swat.h).

`HipSwatActor` binds the parameters of a `StructurePolicy` (swat_policy.py, reference-compatible state_dict) to a handle BY
ADDRESS: nothing is packed, the library reads the live tensors on every forward, so optimizer steps, soft updates,
`load_state_dict` and in-place broadcasts need no notification; only a parameter whose storage MOVES (`.to()`, re-created
tensors) needs a re-bind, which `sync_weights` does by itself.  It has the surface `Rollout` uses on `HipSetActor`
(`configure`, `forward_batch`, `hold_weights`, `sync_weights`, `n_env`, `max_limbs`).  No CPU fallback: without the MI355X
every entry point raises `_lib.SgrlError`.

`HipSwatCritic` is the same over the two networks of a `CriticStructurePolicy` (per-limb Q values, single or twin, the surface
of set_hip.HipSetCritic); `HipSwatTargets` runs the no-grad half of a TD3 update -- target actor, clipped noise, twin target
critics, min and Bellman target (reference src/agent.py:126-148) -- as one library call (`td3.Agent.update_targets`).

Dropout: the forwards take an optional `dropout=(p, seed, step_tensor, site0)` and then run the library's dropout entries
(sgrl_swat_forward_dropout / _forward_q_dropout / _td_target_dropout) -- the forward of a module in TRAINING mode under a
train_ops.dropout_rng context with that (seed, step), the network's 13 sites numbered from site0 in the order of
`dropout_site_plan()`.  Batches of one morphology only.  Without the argument nothing changes: a module in training mode with
dropout > 0 is refused, collection and evaluation run dropout-free in eval mode.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .set_hip import graph_key

LAYERS = 3
_LAYER_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                 "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias",
                 "norm2.weight", "norm2.bias")


def _config(net):
    """(feature, out, cond_decoder, transformer_norm, E, hidden) of a swat_policy.TransformerModel."""
    feature = int(net.encoder.in_features)
    out = int(net.decoder.out_features)
    E = int(net.encoder.out_features)
    hid = int(net.transformer_encoder.layers[0].linear1.out_features)
    return feature, out, bool(net.condition_decoder), net.transformer_encoder.norm is not None, E, hid


def plan_params(net):
    """[(name, shape)] of `net` (a swat_policy.TransformerModel, e.g. StructurePolicy.actor) in the slot order of
    sgrl_swat_bind_params (include/sgrl_swat.h): globals, then 12 per layer, then the final norm with transformer_norm.
    Host only: works on a module on any device."""
    feature, out, cond, tnorm, E, hid = _config(net)
    if (E, hid, len(net.transformer_encoder.layers), net.transformer_encoder.nhead) != (128, 256, LAYERS, 2):
        raise _lib.SgrlError("the HIP SWAT forward is built for E = 128, 2 heads, feed-forward 256, 3 layers")
    emb = [int(e.weight.shape[1]) for e in net.pos_encoder.embeddings]
    plan = [("pos_encoder.embeddings.%d.weight" % i, (15, w)) for i, w in enumerate(emb)]
    plan += [("encoder.weight", (E, feature)), ("encoder.bias", (E,)),
             ("transformer_encoder.rel_encoder.weight", (2, 3)), ("transformer_encoder.rel_encoder.bias", (2,)),
             ("decoder.weight", (out, E + feature if cond else E)), ("decoder.bias", (out,))]
    shapes = {"self_attn.in_proj_weight": (3 * E, E), "self_attn.in_proj_bias": (3 * E,),
              "self_attn.out_proj.weight": (E, E), "self_attn.out_proj.bias": (E,), "linear1.weight": (hid, E),
              "linear1.bias": (hid,), "linear2.weight": (E, hid), "linear2.bias": (E,)}
    for l in range(LAYERS):
        plan += [("transformer_encoder.layers.%d.%s" % (l, n), shapes.get(n, (E,))) for n in _LAYER_PARAMS]
    if tnorm:
        plan += [("transformer_encoder.norm.weight", (E,)), ("transformer_encoder.norm.bias", (E,))]
    return plan


# The dropout sites of ONE network in the program order of swat_policy.TransformerModel.forward: (kind, layer, shape of the tensor the
# module drops as a function of (B, L)); the element index of a mask is the row-major index in that tensor.  The one host-side
# statement of the order: site k of a network is site0 + k (include/sgrl_swat.h has the kernels' side of the table)
SITES_PER_NET = 1 + 4 * LAYERS


def dropout_site_plan():
    """[(kind, layer, shape(B, L))] * 13: 'pos' (pos_encoder's output, layer None), then per layer 'attn' (softmax weights),
    'dropout1' (out_proj's output), 'dropout' (ReLU(linear1)) and 'dropout2' (linear2's output)."""
    plan = [("pos", None, lambda B, L: (L, 128))]
    for l in range(LAYERS):
        plan += [("attn", l, lambda B, L: (B, 2, L, L)), ("dropout1", l, lambda B, L: (B, L, 128)),
                 ("dropout", l, lambda B, L: (B, L, 256)), ("dropout2", l, lambda B, L: (B, L, 128))]
    return plan


def _bind(L):
    if getattr(L, "_swat_bound", False):
        return
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.sgrl_swat_create.argtypes = [ctypes.POINTER(vp)]
    L.sgrl_swat_create.restype = ci
    L.sgrl_swat_destroy.argtypes = [vp]
    L.sgrl_swat_destroy.restype = None
    L.sgrl_swat_bind_params.argtypes = [vp, vp, ci, ci, ci, ci, ci]
    L.sgrl_swat_bind_params.restype = ci
    L.sgrl_swat_graph.argtypes = [vp, ci, vp, vp, vp, vp]
    L.sgrl_swat_graph.restype = ci
    L.sgrl_swat_forward.argtypes = [vp, vp, ci, vp, ci, ctypes.c_float, vp]
    L.sgrl_swat_forward.restype = ci
    cf = ctypes.c_float
    L.sgrl_swat_forward_q.argtypes = [vp, vp, ci, vp, ci, ci, vp, ci, vp]
    L.sgrl_swat_forward_q.restype = ci
    L.sgrl_swat_forward_twin.argtypes = [vp, vp, vp, ci, vp, ci, ci, vp, vp, ci, vp]
    L.sgrl_swat_forward_twin.restype = ci
    L.sgrl_swat_td_target.argtypes = [vp, vp, vp, vp, ci, vp, ci, vp, vp, cf, cf, cf, vp, ci, vp]
    L.sgrl_swat_td_target.restype = ci
    u64 = ctypes.c_uint64
    L.sgrl_swat_forward_dropout.argtypes = [vp, vp, ci, vp, ci, cf, cf, u64, vp, ci, vp, vp]
    L.sgrl_swat_forward_dropout.restype = ci
    L.sgrl_swat_forward_q_dropout.argtypes = [vp, vp, ci, vp, ci, ci, vp, ci, cf, u64, vp, ci, vp, vp]
    L.sgrl_swat_forward_q_dropout.restype = ci
    L.sgrl_swat_td_target_dropout.argtypes = [vp, vp, vp, vp, ci, vp, ci, vp, vp, cf, cf, cf, vp, ci, cf, u64, vp, ci, vp]
    L.sgrl_swat_td_target_dropout.restype = ci
    for name in ("sgrl_swat_dropout_sites", "sgrl_swat_dropout_launches", "sgrl_swat_td_target_dropout_launches"):
        getattr(L, name).argtypes = []
        getattr(L, name).restype = ci
    L.sgrl_swat_twin_launches.argtypes = []
    L.sgrl_swat_twin_launches.restype = ci
    L.sgrl_swat_td_target_launches.argtypes = []
    L.sgrl_swat_td_target_launches.restype = ci
    L.sgrl_swat_debug_twin_streams.argtypes = [ci]
    L.sgrl_swat_debug_twin_streams.restype = ci
    L.sgrl_swat_num_nodes.argtypes = [vp]
    L.sgrl_swat_num_nodes.restype = ci
    L.sgrl_swat_launches.argtypes = []
    L.sgrl_swat_launches.restype = ci
    L.sgrl_swat_generation.argtypes = [vp]
    L.sgrl_swat_generation.restype = ctypes.c_int64
    L.sgrl_swat_last_error.argtypes = []
    L.sgrl_swat_last_error.restype = ctypes.c_char_p
    L._swat_bound = True


def _check(L, rc, what):
    if rc != 0:
        raise _lib.SgrlError("%s failed (%d): %s" % (what, rc, L.sgrl_swat_last_error().decode()))


class HipSwatActor(object):
    """HIP forward of the actor network of a `StructurePolicy` (or, with `net=`, any swat_policy.TransformerModel)."""

    def __init__(self, policy, device=None, net=None):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("%s needs an MI355X (no CPU fallback)" % type(self).__name__)
        self.L = _lib.lib()
        _bind(self.L)
        self.policy = policy
        self.net = net if net is not None else policy.actor
        self.device = torch.device(device) if device is not None else next(self.net.parameters()).device
        if self.device.type != "cuda":
            raise _lib.SgrlError("the StructurePolicy must live on the GPU for the HIP path")
        self.feature, self.out_dim, self.cond, self.tnorm = _config(self.net)[:4]
        self.plan = plan_params(self.net)
        h = ctypes.c_void_p()
        _check(self.L, self.L.sgrl_swat_create(ctypes.byref(h)), "sgrl_swat_create")
        self.h = h
        self._bound = None
        self._cfg_key = None
        self._cfg_info = {}
        self.n_env = 0
        self.max_limbs = 0
        self.num_nodes = 0
        self.act_feature = 0          # per-limb action inputs of a critic network (set by HipSwatCritic)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.sgrl_swat_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- weights ------------------------------------------------------------------------------------
    def _params(self):
        named = dict(self.net.named_parameters())
        return [named[n] for n, _ in self.plan]

    def sync_weights(self, force=False, dropout=False):
        """Bind the handle to the parameters' storage (include/sgrl_swat.h sgrl_swat_bind_params).  The VALUES are read by every
        forward; this binds again only when a parameter's address moved (module.to(), re-created tensors) or with force.
        dropout=True: the caller runs a dropout entry, which is the forward of a module in training mode."""
        if not dropout and self.net.training and getattr(self.net, "dropout", 0.0) > 0.0:
            # every forward of this handle comes through here: the kernels behind it have no dropout, and training mode asks for it
            raise _lib.SgrlError("the HIP forward of a SWAT network has no dropout: the module is in training mode with dropout %g "
                                 "(call eval() for collection / evaluation; an update's passes run the modules)" % self.net.dropout)
        params = self._params()
        ptrs = tuple(p.data_ptr() for p in params)
        if not force and ptrs == self._bound:
            return
        for (name, shape), p in zip(self.plan, params):
            if not (p.is_cuda and p.device == self.device and p.dtype == torch.float32 and p.is_contiguous()
                    and tuple(p.shape) == tuple(shape) and p.data_ptr() % 16 == 0):
                raise _lib.SgrlError("SWAT parameter %s must be a contiguous, 16-byte aligned float32 %s tensor on %s (got %s %s on %s)"
                                     % (name, tuple(shape), self.device, p.dtype, tuple(p.shape), p.device))
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        _check(self.L, self.L.sgrl_swat_bind_params(self.h, ctypes.cast(arr, ctypes.c_void_p), len(ptrs), int(self.cond),
                                                    int(self.tnorm), self.feature, self.out_dim), "sgrl_swat_bind_params")
        self._bound = ptrs

    def hold_weights(self, hold=True):
        """No-op apart from binding: nothing is packed, every forward reads the live parameters (HipSetActor.hold_weights
        promises stability so that a packed copy can be reused; there is no copy here)."""
        self.sync_weights()

    # ---- batch structure ------------------------------------------------------------------------------
    def configure(self, graphs, counts):
        """graphs: per-morphology dicts with 'parents', 'traversals' (3 index vectors) and 'relation' [L, L, 3]; counts: envs
        each.  Structures seen before are switched to without device work (the library caches them by content)."""
        key = (tuple(graph_key(g) for g in graphs), tuple(int(c) for c in counts))
        if key == self._cfg_key:
            return
        args = self._cfg_info.get(key)
        if args is None:
            Ls, trav, rel = [], [], []
            for g in graphs:
                t = [np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.int32) for v in g["traversals"]]
                Ls.append(len(t[0]))
                trav.append(np.concatenate(t))
                r = g["relation"]
                rel.append(np.asarray(r.detach().cpu() if torch.is_tensor(r) else r, dtype=np.float32).reshape(-1))
            args = (np.asarray(Ls, dtype=np.int32), np.asarray(counts, dtype=np.int32),
                    np.ascontiguousarray(np.concatenate(trav), dtype=np.int32),
                    np.ascontiguousarray(np.concatenate(rel), dtype=np.float32))
            if len(self._cfg_info) >= 64:
                self._cfg_info.clear()
            self._cfg_info[key] = args
        Ls, cnt, trav, rel = args
        vp = lambda a: ctypes.c_void_p(a.ctypes.data)
        _check(self.L, self.L.sgrl_swat_graph(self.h, len(Ls), vp(Ls), vp(cnt), vp(trav), vp(rel)), "sgrl_swat_graph")
        self._cfg_key = key
        self.n_env = int(cnt.sum())
        self.max_limbs = int(Ls.max())
        self.num_nodes = self.L.sgrl_swat_num_nodes(self.h)

    def launches(self):
        """Kernel launches per forward (constant)."""
        return int(self.L.sgrl_swat_launches())

    def generation(self):
        return int(self.L.sgrl_swat_generation(self.h))

    @staticmethod
    def _ld(t):
        return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])

    def dropout_args(self, dropout, site_map=None, with_map=False):
        """`dropout=(p, seed, step_tensor, site0)` -> the trailing ctypes arguments (p, seed, step_dev, site0[, site_map]) of a
        dropout entry.  step_tensor: a one-element int64 tensor on the handle's device, which the kernels read."""
        p, seed, step, site0 = dropout
        if not (torch.is_tensor(step) and step.dtype == torch.int64 and step.numel() == 1 and step.is_contiguous()
                and step.device == self.device):
            raise _lib.SgrlError("dropout=(p, seed, step_tensor, site0): step_tensor must be a one-element int64 tensor on %s" % (self.device,))
        args = [ctypes.c_float(float(p)), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), ctypes.c_void_p(step.data_ptr()), int(site0)]
        if with_map:                     # the single-network entries: a HOST int32[13], read during the call, or NULL
            sm = None if site_map is None else np.ascontiguousarray(site_map, dtype=np.int32)
            assert sm is None or sm.shape == (SITES_PER_NET,)
            args.append(ctypes.c_void_p(None if sm is None else sm.ctypes.data))
            self._site_map = sm          # alive over the call
        return args

    def dropout_launches(self):
        """Kernel launches of one dropout forward (constant)."""
        return int(self.L.sgrl_swat_dropout_launches())

    def forward_batch(self, obs, out=None, act_ld=None, dropout=None, site_map=None):
        """obs: float32 CUDA [n_env, obs_ld] -> actions float32 [n_env, act_ld] (StructurePolicy.forward for every environment;
        slots beyond out * L_e of a row are exact zeros).  dropout=(p, seed, step_tensor, site0): the forward of the module in
        training mode, sites site0 .. site0 + 12 (one morphology; site_map: tests, include/sgrl_swat.h)."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.stride(1) == 1
        assert obs.shape[0] == self.n_env
        assert obs.shape[1] >= self.feature * self.max_limbs, "observation rows narrower than feature * max_limbs"
        self.sync_weights(dropout=dropout is not None)
        act_ld = act_ld or self.out_dim * self.max_limbs
        assert act_ld >= self.out_dim * self.max_limbs, "action rows narrower than out * max_limbs"
        if out is None:
            out = torch.empty((self.n_env, act_ld), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.shape == (self.n_env, act_ld)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if dropout is not None:
            extra = self.dropout_args(dropout, site_map, with_map=True)
            _check(self.L, self.L.sgrl_swat_forward_dropout(self.h, ctypes.c_void_p(obs.data_ptr()), self._ld(obs),
                                                            ctypes.c_void_p(out.data_ptr()), int(act_ld),
                                                            ctypes.c_float(float(self.policy.max_action)), *extra, stream),
                   "sgrl_swat_forward_dropout")
            return out
        _check(self.L, self.L.sgrl_swat_forward(self.h, ctypes.c_void_p(obs.data_ptr()), self._ld(obs),
                                                ctypes.c_void_p(out.data_ptr()), int(act_ld),
                                                ctypes.c_float(float(self.policy.max_action)), stream), "sgrl_swat_forward")
        return out

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def check_rows(self, t, per_limb, what):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == self.n_env, what
        assert t.shape[1] >= per_limb * self.max_limbs, "%s rows narrower than %d * max_limbs" % (what, per_limb)

    def forward_q(self, obs, action, out=None, q_ld=None, dropout=None, site_map=None):
        """Critic network (a handle over CriticStructurePolicy.critic1 / .critic2): obs [n_env, obs_ld], action [n_env, act_ld]
        (out_dim-of-the-actor slots per limb) -> per-limb Q [n_env, q_ld], exact zeros beyond L_e.  dropout: as forward_batch."""
        act_feature = self.act_feature                # 0 on an actor's handle: the library refuses it
        self.check_rows(obs, self.feature - act_feature, "observation")
        self.check_rows(action, act_feature, "action")
        self.sync_weights(dropout=dropout is not None)
        q_ld = q_ld or self.max_limbs
        assert q_ld >= self.max_limbs
        if out is None:
            out = torch.empty((self.n_env, q_ld), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.shape == (self.n_env, q_ld)
        if dropout is not None:
            extra = self.dropout_args(dropout, site_map, with_map=True)
            _check(self.L, self.L.sgrl_swat_forward_q_dropout(self.h, ctypes.c_void_p(obs.data_ptr()), self._ld(obs),
                                                              ctypes.c_void_p(action.data_ptr()), self._ld(action), act_feature,
                                                              ctypes.c_void_p(out.data_ptr()), int(q_ld), *extra, self._stream()),
                   "sgrl_swat_forward_q_dropout")
            return out
        _check(self.L, self.L.sgrl_swat_forward_q(self.h, ctypes.c_void_p(obs.data_ptr()), self._ld(obs),
                                                  ctypes.c_void_p(action.data_ptr()), self._ld(action), act_feature,
                                                  ctypes.c_void_p(out.data_ptr()), int(q_ld), self._stream()), "sgrl_swat_forward_q")
        return out

    def forward_single(self, state, graph):
        """StructurePolicy.forward(state [B, feature * L]) for one morphology."""
        self.configure([graph], [state.shape[0]])
        return self.forward_batch(state.contiguous().float(), act_ld=self.out_dim * len(graph["parents"]))


class HipSwatCritic(object):
    """Twin critics of a `CriticStructurePolicy` on the HIP path (inference only: the TD3 target values, reference
    agent.py:136-148): two handles, one per TransformerModel, sharing the batch structure.  Both networks in one call run as
    sgrl_swat_forward_twin (two chains side by side on two streams); each network's values are those of its own single forward,
    bit for bit."""

    def __init__(self, critic_module, device=None):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("HipSwatCritic needs an MI355X (no CPU fallback)")
        self.module = critic_module
        self.q1 = HipSwatActor(critic_module, device=device, net=critic_module.critic1)
        self.q2 = HipSwatActor(critic_module, device=device, net=critic_module.critic2)
        self.L, self.device = self.q1.L, self.q1.device
        self.act_feature = self.q1.act_feature = self.q2.act_feature = int(critic_module.action_dim)
        self.n_env = self.max_limbs = 0
        if (self.q1.out_dim, self.q2.out_dim) != (1, 1) or self.q1.feature != int(critic_module.state_dim) + self.act_feature:
            raise _lib.SgrlError("HipSwatCritic needs critics with one output and state_dim + action_dim inputs per limb")

    def configure(self, graphs, counts):
        self.q1.configure(graphs, counts)
        self.q2.configure(graphs, counts)
        self.n_env, self.max_limbs = self.q1.n_env, self.q1.max_limbs

    def launches(self):
        """Kernel launches of one twin forward (constant)."""
        return int(self.L.sgrl_swat_twin_launches())

    def forward_batch(self, obs, action, q_ld=None, which=(1, 2), dropout=None):
        """obs [n_env, obs_ld], action [n_env, act_ld] (float32 CUDA) -> tuple of per-limb Q [n_env, q_ld], one per network in
        `which`; slots beyond L_e of a row are exact zeros.  dropout=(p, seed, step_tensor, site0): the networks in training mode,
        one dropout forward each, the networks of `which` taking 13 sites each from site0 in their order (CriticStructurePolicy.
        forward: critic1 site0 .. + 12, critic2 site0 + 13 .. + 25; Q1 alone: site0 .. + 12)."""
        if dropout is not None:
            p, seed, step, site0 = dropout
            nets = [h for k, h in ((1, self.q1), (2, self.q2)) if k in which]
            return tuple(h.forward_q(obs, action, q_ld=q_ld, dropout=(p, seed, step, site0 + SITES_PER_NET * n)) for n, h in enumerate(nets))
        if not (1 in which and 2 in which):
            return tuple(h.forward_q(obs, action, q_ld=q_ld) for k, h in ((1, self.q1), (2, self.q2)) if k in which)
        q1 = self.q1
        q1.check_rows(obs, q1.feature - self.act_feature, "observation")
        q1.check_rows(action, self.act_feature, "action")
        q1.sync_weights()
        self.q2.sync_weights()
        q_ld = q_ld or self.max_limbs
        assert q_ld >= self.max_limbs
        out = torch.empty((2, self.n_env, q_ld), dtype=torch.float32, device=self.device)
        vp = ctypes.c_void_p
        _check(self.L, self.L.sgrl_swat_forward_twin(q1.h, self.q2.h, vp(obs.data_ptr()), q1._ld(obs), vp(action.data_ptr()),
                                                     q1._ld(action), self.act_feature, vp(out[0].data_ptr()), vp(out[1].data_ptr()),
                                                     int(q_ld), q1._stream()), "sgrl_swat_forward_twin")
        return out[0], out[1]

    def forward_single(self, state, action, graph, which=(1, 2)):
        """CriticStructurePolicy.forward(state [B, 41 L], action [B, 3 L]) for one morphology -> per-limb Q [B, L] each."""
        B, L = state.shape[0], len(graph["parents"])
        self.configure([graph], [B])
        return self.forward_batch(state.contiguous().float(), action.contiguous().float(), q_ld=L, which=which)


class HipSwatTargets(object):
    """The no-grad half of a TD3 update of a SWAT agent (reference src/agent.py:126-148) on the HIP path: the handles of the
    target actor (`StructurePolicy`) and the twin target critics (`CriticStructurePolicy`), and `target_q` over
    sgrl_swat_td_target.  The noisy target action and the Q values never leave the library's workspaces."""

    def __init__(self, actor_target, critic_target):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("HipSwatTargets needs an MI355X (no CPU fallback)")
        self.actor = actor_target.hip_handle()        # cached on the modules (dropped when they are pickled / deep-copied)
        self.critic = critic_target.hip_handle()
        self.L, self.device = self.actor.L, self.actor.device
        if self.critic.q1.feature != self.actor.feature + self.actor.out_dim:
            raise _lib.SgrlError("the target critics must take the target actor's feature + out inputs per limb")

    def configure(self, graphs, counts):
        self.actor.configure(graphs, counts)
        self.critic.configure(graphs, counts)

    def launches(self):
        """Kernel launches of one target chain (constant)."""
        return int(self.L.sgrl_swat_td_target_launches())

    def dropout_launches(self):
        """Kernel launches of one target chain with dropout (constant)."""
        return int(self.L.sgrl_swat_td_target_dropout_launches())

    def target_q(self, next_obs, noise, reward, done, graph, noise_clip, discount, counts=None, out=None, q_ld=None, dropout=None):
        """reward + (1 - done) * discount * min(Q1_t, Q2_t)(next_obs, clamp(actor_t(next_obs) + clamp(noise, +-noise_clip),
        +-max_action)) per limb -> float32 [B, q_ld].  next_obs [B, >= 41 Lmax], noise [B, >= 3 Lmax] (the unclipped draw, laid
        out like an action row), reward / done [B] or [B, 1].  graph: the morphology's graph dict, or a list of them with
        `counts` environments each (row blocks in that order).  dropout=(p, seed, step_tensor, site0): the three target networks in
        training mode (one morphology): the target actor takes sites site0 .. + 12, critic1 + 13 .. + 25, critic2 + 26 .. + 38, the
        order `Agent.update_targets` runs the modules in."""
        graphs = graph if isinstance(graph, (list, tuple)) else [graph]
        self.configure(graphs, counts if counts is not None else [next_obs.shape[0]])
        a = self.actor
        a.check_rows(next_obs, a.feature, "observation")
        a.check_rows(noise, a.out_dim, "noise")
        reward, done = reward.reshape(-1), done.reshape(-1)
        for t in (reward, done):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == a.n_env
        for h in (a, self.critic.q1, self.critic.q2):
            h.sync_weights(dropout=dropout is not None)
        q_ld = q_ld or a.max_limbs
        assert q_ld >= a.max_limbs
        if out is None:
            out = torch.empty((a.n_env, q_ld), dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.shape == (a.n_env, q_ld)
        vp, cf = ctypes.c_void_p, ctypes.c_float
        if dropout is not None:
            _check(self.L, self.L.sgrl_swat_td_target_dropout(a.h, self.critic.q1.h, self.critic.q2.h, vp(next_obs.data_ptr()), a._ld(next_obs),
                                                              vp(noise.data_ptr()), a._ld(noise), vp(reward.data_ptr()), vp(done.data_ptr()),
                                                              cf(float(a.policy.max_action)), cf(float(noise_clip)), cf(float(discount)),
                                                              vp(out.data_ptr()), int(q_ld), *a.dropout_args(dropout), a._stream()),
                   "sgrl_swat_td_target_dropout")
            return out
        _check(self.L, self.L.sgrl_swat_td_target(a.h, self.critic.q1.h, self.critic.q2.h, vp(next_obs.data_ptr()), a._ld(next_obs),
                                                  vp(noise.data_ptr()), a._ld(noise), vp(reward.data_ptr()), vp(done.data_ptr()),
                                                  cf(float(a.policy.max_action)), cf(float(noise_clip)), cf(float(discount)),
                                                  vp(out.data_ptr()), int(q_ld), a._stream()), "sgrl_swat_td_target")
        return out
