"""Batched HIP forward of the monolithic MLP actor (csrc/mlp_actor.hip, C ABI in include/sgrl_mlp.h).

`HipMlpActor` binds the `nn.Linear` parameters of an `MlpPolicy` (mlp_policy.py, reference-compatible state_dict) to a handle BY
ADDRESS.  The library pads the widths in a packed copy of its own (`plan`), built by one pack launch at the top of a forward;
`hold_weights(True)` is the caller's promise that the parameters stay put until the next `hold_weights` / `weights_changed`, so a
collection round packs once.  The forward of all environments is ONE launch.  It has the surface `Rollout` uses on the other
actors (`configure`, `forward_batch`, `hold_weights`, `sync_weights`, `n_env`, `max_limbs`).  No CPU fallback: without the MI355X
every device entry point raises `_lib.SgrlError`; `plan` alone is host-side."""
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
    for name in ("sgrl_mlp_forward_launches", "sgrl_mlp_pack_launches"):
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


class HipMlpActor(object):
    """HIP forward of the actor network of an `MlpPolicy` (or, with `net=`, any mlp_policy.MLPNetwork followed by tanh)."""

    def __init__(self, policy, device=None, net=None):
        if not torch.cuda.is_available():
            raise _lib.SgrlError("%s needs an MI355X (no CPU fallback)" % type(self).__name__)
        self.L = _lib.lib()
        _bind(self.L)
        self.policy = policy
        self.net = net if net is not None else policy.actor
        self.device = torch.device(device) if device is not None else next(self.net.parameters()).device
        if self.device.type != "cuda":
            raise _lib.SgrlError("the MlpPolicy must live on the GPU for the HIP path")
        self.dims = net_dims(self.net)
        self.feature, self.out_dim = int(policy.state_dim), int(policy.action_dim)
        self.num_limbs = self.dims[0] // self.feature
        if self.dims[0] != self.feature * self.num_limbs or self.dims[-1] != self.out_dim * self.num_limbs:
            raise _lib.SgrlError("the MLP maps %d -> %d values: not %d / %d per limb of one limb count"
                                 % (self.dims[0], self.dims[-1], self.feature, self.out_dim))
        h = ctypes.c_void_p()
        _check(self.L, self.L.sgrl_mlp_create(ctypes.byref(h)), "sgrl_mlp_create")
        self.h = h
        self._bound = None
        self._cfg_key = None
        self._hold = False
        self.n_env = 0
        self.max_limbs = 0

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.sgrl_mlp_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- weights ------------------------------------------------------------------------------------
    def _params(self):
        return [p for l in linears(self.net) for p in (l.weight, l.bias)]

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
        _check(self.L, self.L.sgrl_mlp_set_params(self.h, ctypes.cast(arr, ctypes.c_void_p), len(ptrs),
                                                  ctypes.c_void_p(dims.ctypes.data), len(dims)), "sgrl_mlp_set_params")
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
                                                 self.feature, self.out_dim), "sgrl_mlp_configure")
        self._cfg_key = (Ls, counts)
        self.n_env = int(ca.sum())
        self.max_limbs = int(la.max())

    def launches(self):
        """Kernel launches of the forward proper (constant: 1; a forward that packs adds `pack_launches()`)."""
        return int(self.L.sgrl_mlp_forward_launches())

    def pack_launches(self):
        return int(self.L.sgrl_mlp_pack_launches())

    def generation(self):
        return int(self.L.sgrl_mlp_generation(self.h))

    def plan(self):
        return plan(self.dims, self.n_env or None)

    @staticmethod
    def _ld(t):
        return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])

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
