"""SMP (shared modular policies: message passing along the limb tree) actor / critic behind the reference's module
surfaces.

`ActorGraphPolicy` / `CriticGraphPolicy` keep the constructor signatures, `forward`, `Q1`, `change_morphology` and the
`state_dict()` keys of reference src/ModularActor.py:99-384 / src/ModularCritic.py:143-520 (`sNet.<i>.*`,
`actor.<i>.*` / `critic.<i>.*`: ONE shared module listed once per limb, exactly as the reference's
`nn.ModuleList([module] * num_limbs)` shows it).  Only the reference's `disable_fold` code path exists here (torchfold's
dynamic batching is replaced by what it was a workaround for: the limbs of one tree DEPTH are evaluated as one batched
call of the shared module -- bottom-up from the deepest level, top-down from the root).  Message passing modes: `bu and td`
(both ways, the published SMP) and `td` only -- the two the reference's `disable_fold` path can run (without top-down
messages its forward raises at ModularActor.py:244, `torch.stack` of a list of None).
Plain differentiable PyTorch by default: this is what the TD3 updates run through.  With `train_kernels` on (default False;
td3.Agent(smp_train_kernels=True)) the differentiable passes of the published mode keep whole [limbs of a level, B, .] tensors per tree
level and run on the training kernels of train_ops (linear, smp_gather, smp_up_tail, normalize_rows: `_level_plan`, `_up_levels`,
`_down_levels` below) wherever those kernels run; everywhere else the switch changes no bit.
Collection in the device loop runs the actor in its published mode (`bu and td`) through the batched HIP forward instead
(smp_hip.HipSmpActor, csrc/smp_actor.hip; `_Tree` below stays the one source of its schedule).  The no-grad target chain of an update (td3.Agent.update_targets: target actor and twin
target critic, both `bu and td`) runs on the same kernels through `hip_handle()` (smp_hip.HipSmpTargets): the handle a module
caches is per-process device state and is dropped whenever the module is pickled or deep-copied.  The `td`-only ablation has no
HIP path.  Outputs are pinned to fixtures produced by executing the reference's own modules (tests/golden/smp_forward.npz,
tools/capture_golden_smp.py).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import train_ops
from .swat_policy import _TrainKernelsSwitch


class MLPBase(nn.Module):
    """reference utils.MLPBase (utils.py:222-233): 400 / 300 hidden units, ReLU."""

    def __init__(self, num_inputs, num_outputs):
        super().__init__()
        self.l1 = nn.Linear(num_inputs, 400)
        self.l2 = nn.Linear(400, 300)
        self.l3 = nn.Linear(300, num_outputs)

    def forward(self, x):
        return self.l3(F.relu(self.l2(F.relu(self.l1(x)))))


def _up_message(mod, x, m):
    """fc1 -> normalise -> [., m] -> tanh -> fc2 -> tanh -> fc3 -> normalise (ModularActor.py:35-47)."""
    h = F.normalize(mod.fc1(x), dim=-1)
    h = torch.tanh(torch.cat([h, m], dim=-1))
    h = torch.tanh(mod.fc2(h))
    return F.normalize(mod.fc3(h), dim=-1)


# ---- actor node modules (parameter names of ModularActor.py:12-96) ------------------------------------------------------
class ActorUp(nn.Module):
    def __init__(self, state_dim, msg_dim, max_children):
        super().__init__()
        self.fc1 = nn.Linear(state_dim, 64)
        self.fc2 = nn.Linear(64 + msg_dim * max_children, 64)
        self.fc3 = nn.Linear(64, msg_dim)

    def forward(self, x, m):
        return _up_message(self, x, m)


class ActorDownAction(nn.Module):
    def __init__(self, self_input_dim, action_dim, msg_dim, max_action, max_children):
        super().__init__()
        self.max_action = max_action
        self.action_base = MLPBase(self_input_dim + msg_dim, action_dim)
        self.msg_base = MLPBase(self_input_dim + msg_dim, msg_dim * max_children)

    def forward(self, x, m):
        xm = torch.tanh(torch.cat([x, m], dim=-1))
        return self.max_action * torch.tanh(self.action_base(xm)), F.normalize(self.msg_base(xm), dim=-1)


# ---- critic node modules (ModularCritic.py:11-140) ----------------------------------------------------------------------
class CriticUp(nn.Module):
    def __init__(self, state_dim, action_dim, msg_dim, max_children):
        super().__init__()
        self.fc1 = nn.Linear(state_dim + action_dim, 64)
        self.fc2 = nn.Linear(64 + msg_dim * max_children, 64)
        self.fc3 = nn.Linear(64, msg_dim)

    def forward(self, x, u, m):
        return _up_message(self, torch.cat([x, u], dim=-1), m)


class CriticDownAction(nn.Module):
    def __init__(self, self_input_dim, action_dim, msg_dim, max_children):
        super().__init__()
        self.baseQ1 = MLPBase(self_input_dim + action_dim + msg_dim, 1)
        self.baseQ2 = MLPBase(self_input_dim + action_dim + msg_dim, 1)
        self.msg_base = MLPBase(self_input_dim + msg_dim, msg_dim * max_children)

    def forward(self, x, u, m, twin=True):
        xum = torch.cat([x, u, m], dim=-1)
        msg_down = F.normalize(self.msg_base(torch.tanh(torch.cat([x, m], dim=-1))), dim=-1)
        return self.baseQ1(xum), (self.baseQ2(xum) if twin else None), msg_down


# ---- the tree schedule ----------------------------------------------------------------------------------------------------
class _Tree(object):
    """Evaluation order of one morphology: limbs grouped by depth, the children slots of every limb, and the slot a limb
    occupies in its parent's outgoing message (ModularActor.py:283-326)."""

    def __init__(self, parents, max_children):
        parents = [int(p) for p in parents]
        L = len(parents)
        self.L = L
        depth = [0] * L
        for i in range(1, L):
            depth[i] = depth[parents[i]] + 1 if parents[i] >= 0 else 0
        self.levels = [[i for i in range(L) if depth[i] == d] for d in range(max(depth) + 1)]
        self.children = []
        for i in range(L):
            ch = [j for j, p in enumerate(parents) if p == i]
            assert len(ch) <= max_children, "limb %d has %d children, max_children is %d" % (i, len(ch), max_children)
            self.children.append(ch + [-1] * (max_children - len(ch)))
        self.slot = []
        for i in range(L):
            k = parents[:i].count(parents[i])
            if parents[0] == -2 and i == 1:      # flipped structure: message order mirrored at the root
                k = (max_children - 1) - k
            self.slot.append(k)
        self.parents = parents


class _LevelPlan(object):
    """What the level-tensor path (`train_kernels`) reads off a _Tree, built once per morphology (_GraphModule._level_plan):
    `perm` (the limbs in level order) and `inv` (where limb i stands in it), `sizes` (limbs per level), and per level the two gather tables of
    train_ops.smp_gather over positions WITHIN the neighbouring level -- every child of a level-d limb lies in level d + 1, every parent
    in level d - 1, so both directions gather from ONE tensor per level:
      up[d]    [n_d, max_children]: the children's up messages (source: level d + 1, 32 wide), -1 where _Tree.children has -1;
      down[d]  [n_d, 1]: the parent's outgoing message (source: level d - 1), columns slot * msg_dim .. of it, -1 at a root."""

    def __init__(self, tree, msg_dim, max_children):
        self.sizes = [len(lv) for lv in tree.levels]
        self.perm = [i for lv in tree.levels for i in lv]
        pos = {}
        for lv in tree.levels:
            for k, i in enumerate(lv):
                pos[i] = k
        self.inv = [0] * tree.L
        for k, i in enumerate(self.perm):
            self.inv[i] = k
        self.up, self.down = [], []
        for lv in tree.levels:
            self.up.append(train_ops.SmpTable([[pos[c] if c >= 0 else -1 for c in tree.children[i]] for i in lv],
                                              [[0] * max_children for _ in lv]))
            self.down.append(train_ops.SmpTable([[pos[tree.parents[i]] if tree.parents[i] >= 0 else -1] for i in lv],
                                                [[tree.slot[i] * msg_dim if tree.parents[i] >= 0 else 0] for i in lv]))
        # what the kernels hold (include/sgrl_train.h); a morphology outside it keeps the PyTorch path
        self.fits = msg_dim == train_ops.SMP_MSG and 1 <= max_children <= train_ops.SMP_MAX_CHILDREN and \
            max(self.sizes) <= train_ops.SMP_MAX_LIMBS and all(t.one_reader for t in self.up + self.down) and \
            all(t.max_off + msg_dim <= msg_dim * max_children for t in self.down)
        self._index = {}

    def index(self, device):
        """(perm, inv) as index tensors on `device`, made once."""
        key = str(device)
        if key not in self._index:
            self._index[key] = (torch.tensor(self.perm, dtype=torch.long, device=device), torch.tensor(self.inv, dtype=torch.long, device=device))
        return self._index[key]


def _mlp_base(base, x, slot=None):
    """MLPBase.forward on train_ops.linear: each ReLU output feeds one layer, so its mask is applied once, in the epilogue of that
    layer's input gradient (train_ops.linear premasked / x_relu)."""
    h = train_ops.linear(x, base.l1.weight, base.l1.bias, relu=True, premasked=True, slot=slot)
    h = train_ops.linear(h, base.l2.weight, base.l2.bias, relu=True, premasked=True, x_relu=True)
    return train_ops.linear(h, base.l3.weight, base.l3.bias, x_relu=True)


class _GraphModule(_TrainKernelsSwitch, nn.Module):
    def _init_common(self, state_dim, action_dim, msg_dim, batch_size, max_children, disable_fold, td, bu):
        if not disable_fold:
            raise NotImplementedError("the torchfold path of the reference is not rebuilt: construct with disable_fold=True "
                                      "(limbs of one tree depth are batched instead)")
        self.num_limbs = 1
        self.msg_dim, self.batch_size, self.max_children, self.disable_fold = msg_dim, batch_size, max_children, disable_fold
        self.state_dim, self.action_dim = state_dim, action_dim
        if not td:
            raise NotImplementedError("SMP without top-down messages: the reference's disable_fold path cannot run it "
                                      "(ModularActor.py:244 stacks a list of None); modes built: td, td + bu")
        self.td, self.bu = td, bu
        self.parents = [-1]
        self._tree = _Tree(self.parents, max_children)
        self._smp_hip = None
        self._plan = None

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_smp_hip"] = None      # per-process device handle: never pickled / deep-copied with the module
        d["_plan"] = None         # derived from the trees (holds per-device index tensors): rebuilt on first use
        return d

    def _level_plan(self):
        """The _LevelPlan of the current morphology; kept per parents list, so that a trainer cycling through its morphologies builds
        each plan (and uploads its two index tensors) once."""
        plans = self.__dict__.get("_plan")
        if plans is None or len(plans) > 64:
            plans = self._plan = {}
        key = tuple(self.parents)
        if key not in plans:
            plans[key] = _LevelPlan(self._tree, self.msg_dim, self.max_children)
        return plans[key]

    def _kernel_pass(self, *inputs):
        """True when this pass takes the level-tensor path: the switch is on, the mode is the published one, the training kernels run
        for these inputs (GPU, float32, autograd recording) and hold this morphology."""
        if not (self.train_kernels and self.bu and self.td):
            return False
        return train_ops._on_device_with_grad(*inputs, *self.parameters()) and self._level_plan().fits

    def _up_levels(self, h1, plan):
        """Bottom-up over whole levels: h1 [L, B, 64] = fc1 of every limb, in level order -> the up messages per level [n_d, B, 32]."""
        mod = self.sNet[0]
        parts = h1.split(plan.sizes)
        ups = [None] * len(parts)
        for d in reversed(range(len(parts))):
            g = train_ops.smp_gather(parts[d], ups[d + 1] if d + 1 < len(parts) else None, plan.up[d], normalize=True, act_tanh=True)
            ups[d] = train_ops.smp_up_tail(train_ops.linear(g, mod.fc2.weight, mod.fc2.bias), mod.fc3.weight, mod.fc3.bias)
        return ups

    def _down_levels(self, ups, plan, heads, heads_read_xm):
        """Top-down over whole levels.  heads(d, xm, slot, down) is called per level with the previous level's outgoing messages
        `down` [n_(d-1), B, 32 max_children] (None at the root level) and, if heads_read_xm, xm = tanh([up | parent message slot])
        [n_d, B, 64], the input of msg_base: an alias for ONE train_ops.linear consumer, with its fan-out slot.  The last level's
        outgoing messages are never read and not computed (nor is xm there when only msg_base reads it)."""
        down = None
        D = len(ups)
        for d in range(D):
            last = d == D - 1
            xm = slot = None
            if heads_read_xm or not last:
                xm = train_ops.smp_gather(ups[d], down, plan.down[d], normalize=False, act_tanh=True)
            if heads_read_xm and not last:          # two consumers, both linear layers: their input gradients meet in one buffer
                slot, (xm, xm_msg) = train_ops.fan_out(xm, 2)
            else:
                xm_msg = xm
            heads(d, xm, slot, down)
            if not last:
                down = train_ops.normalize_rows(_mlp_base(self._msg_base(), xm_msg, slot))

    def hip_handle(self):
        """The module's smp_hip.HipSmpActor / HipSmpCritic, created on first use (raises _lib.SgrlError without an MI355X, and
        for the td-only mode: no fallback)."""
        if getattr(self, "_smp_hip", None) is None:
            from . import smp_hip
            self._smp_hip = getattr(smp_hip, self._hip_class)(self)
        return self._smp_hip

    def _relist(self, names):
        for n in names:
            if hasattr(self, n):
                setattr(self, n, nn.ModuleList([getattr(self, n)[0]] * self.num_limbs))

    def change_morphology(self, graph):
        self.graph = graph
        self.parents = [int(p) for p in graph["parents"]]
        self.num_limbs = len(self.parents)
        self._tree = _Tree(self.parents, self.max_children)
        self._relist(self._lists)

    def _split(self, t, dim):
        assert t.shape[1] == dim * self.num_limbs, \
            "state.shape[1] expects {} but got {} with num_limbs being {} and state_dim being {}".format(
                dim * self.num_limbs, t.shape[1], self.num_limbs, dim)
        return t.reshape(t.shape[0], self.num_limbs, dim).transpose(0, 1)       # [L, B, dim]

    def _bottom_up(self, fn):
        """fn(nodes, msg_in [n, B, msg_dim * max_children]) -> msg_up [n, B, msg_dim]; deepest level first."""
        tr = self._tree
        up = [None] * tr.L
        for level in reversed(tr.levels):
            B = self._B
            zero = torch.zeros((B, self.msg_dim), device=self._dev, dtype=self._dt)
            m = torch.stack([torch.cat([up[c] if c >= 0 else zero for c in tr.children[i]], dim=-1) for i in level])
            out = fn(level, m)
            for k, i in enumerate(level):
                up[i] = out[k]
        return up

    def _top_down(self, fn):
        """fn(nodes, msg_in [n, B, msg_dim]) -> msg_down [n, B, msg_dim * max_children]; root level first."""
        tr = self._tree
        down = [None] * tr.L
        for level in tr.levels:
            zero = torch.zeros((self._B, self.msg_dim * self.max_children), device=self._dev, dtype=self._dt)
            ms = []
            for i in level:
                pm = down[tr.parents[i]] if tr.parents[i] >= 0 else zero
                ms.append(pm[:, tr.slot[i] * self.msg_dim:(tr.slot[i] + 1) * self.msg_dim])
            out = fn(level, torch.stack(ms))
            for k, i in enumerate(level):
                down[i] = out[k]
        return down


class ActorGraphPolicy(_GraphModule):
    """Drop-in for reference ModularActor.ActorGraphPolicy (constructor of ModularActor.py:102-115)."""
    _lists = ("sNet", "actor")
    _hip_class = "HipSmpActor"

    def __init__(self, state_dim, action_dim, msg_dim, batch_size, max_action, max_children, disable_fold, td, bu,
                 args=None, device=None):
        super().__init__()
        self._init_common(state_dim, action_dim, msg_dim, batch_size, max_children, disable_fold, td, bu)
        self.max_action = max_action
        if bu:
            self.sNet = nn.ModuleList([ActorUp(state_dim, msg_dim, max_children)])
        self.actor = nn.ModuleList([ActorDownAction(msg_dim if bu else state_dim, action_dim, msg_dim, max_action, max_children)])
        if device is not None:
            self.to(device)

    def clear_buffer(self):
        self.action = None

    def _msg_base(self):
        return self.actor[0].msg_base

    def _forward_levels(self, state):
        """forward() on whole level tensors (train_kernels): fc1 once over all limbs, per level one gather, fc2 and the tail going up,
        one gather and the two MLPBase chains going down; the actions return to limb order through the plan's one permutation."""
        plan = self._level_plan()
        perm, inv = plan.index(state.device)
        x = self._split(state, self.state_dim).index_select(0, perm)                     # [L, B, state_dim], level order
        up = self.sNet[0]
        ups = self._up_levels(train_ops.linear(x, up.fc1.weight, up.fc1.bias), plan)
        acts = []
        self._down_levels(ups, plan, lambda d, xm, slot, down: acts.append(_mlp_base(self.actor[0].action_base, xm, slot)), True)
        a = self.max_action * torch.tanh(torch.cat(acts).index_select(0, inv))       # [L, B, A], limb order
        return a.transpose(0, 1).reshape(state.shape[0], -1)

    def forward(self, state, mode="train"):
        if self._kernel_pass(state):
            self.action = self._forward_levels(state)
            return self.action
        x = self._split(state, self.state_dim)
        self._B, self._dev, self._dt = state.shape[0], state.device, state.dtype
        act = [None] * self.num_limbs
        if self.bu:
            up = self._bottom_up(lambda level, m: self.sNet[0](x[level], m))

        def down_fn(level, m):
            # both ways: a limb's own input is the message it sent up (ModularActor.py:294-297)
            a, msg = self.actor[0](torch.stack([up[i] for i in level]) if self.bu else x[level], m)
            for k, i in enumerate(level):
                act[i] = a[k]
            return msg
        self._top_down(down_fn)
        self.action = torch.stack(act, dim=1).reshape(state.shape[0], -1)       # [B, L, A] -> [B, L * A]
        return self.action


class CriticGraphPolicy(_GraphModule):
    """Drop-in for reference ModularCritic.CriticGraphPolicy: twin Q values, per-limb outputs summed over the limbs -> [B, 1]
    each (ModularCritic.py:286-290)."""
    _lists = ("sNet", "critic")
    _hip_class = "HipSmpCritic"

    def __init__(self, state_dim, action_dim, msg_dim, batch_size, max_children, disable_fold, td, bu, args=None,
                 device=None):
        super().__init__()
        self._init_common(state_dim, action_dim, msg_dim, batch_size, max_children, disable_fold, td, bu)
        if bu:
            self.sNet = nn.ModuleList([CriticUp(state_dim, action_dim, msg_dim, max_children)])
        self.critic = nn.ModuleList([CriticDownAction(msg_dim if bu else state_dim, action_dim, msg_dim, max_children)])
        if device is not None:
            self.to(device)

    def clear_buffer(self):
        self.x1 = self.x2 = None

    def _msg_base(self):
        return self.critic[0].msg_base

    def _run_levels(self, state, action, twin):
        """_run() on whole level tensors (train_kernels).  The Q heads read the RAW [up | action | parent message slot]: the parent's slot
        comes from the same gather without an own part or tanh; the per-limb values are summed in level order."""
        plan = self._level_plan()
        perm, _ = plan.index(state.device)
        x = self._split(state, self.state_dim).index_select(0, perm)
        u = self._split(action, self.action_dim).index_select(0, perm)
        up, crit = self.sNet[0], self.critic[0]
        ups = self._up_levels(train_ops.linear(torch.cat([x, u], dim=-1), up.fc1.weight, up.fc1.bias), plan)
        us = u.split(plan.sizes)
        q1, q2 = [], []

        def heads(d, xm, slot, down):
            m = train_ops.smp_gather(None, down, plan.down[d], batch=state.shape[0]) if down is not None else \
                torch.zeros((plan.sizes[d], state.shape[0], self.msg_dim), device=state.device, dtype=state.dtype)
            xum = torch.cat([ups[d], us[d], m], dim=-1)
            q1.append(_mlp_base(crit.baseQ1, xum))
            if twin:
                q2.append(_mlp_base(crit.baseQ2, xum))
        self._down_levels(ups, plan, heads, False)
        B = state.shape[0]
        self.x1 = torch.cat(q1).sum(dim=0).reshape(B, -1)
        self.x2 = torch.cat(q2).sum(dim=0).reshape(B, -1) if twin else None
        return self.x1, self.x2

    def _run(self, state, action, twin):
        if self._kernel_pass(state, action):
            return self._run_levels(state, action, twin)
        x, u = self._split(state, self.state_dim), self._split(action, self.action_dim)
        self._B, self._dev, self._dt = state.shape[0], state.device, state.dtype
        L = self.num_limbs
        q1, q2 = [None] * L, [None] * L
        if self.bu:
            up = self._bottom_up(lambda level, m: self.sNet[0](x[level], u[level], m))

        def down_fn(level, m):
            xs = torch.stack([up[i] for i in level]) if self.bu else x[level]
            a, b, msg = self.critic[0](xs, u[level], m, twin=twin)
            for k, i in enumerate(level):
                q1[i] = a[k]
                q2[i] = b[k] if twin else None
            return msg
        self._top_down(down_fn)
        self.x1 = torch.stack(q1, dim=-1).sum(dim=-1).reshape(state.shape[0], -1)
        self.x2 = torch.stack(q2, dim=-1).sum(dim=-1).reshape(state.shape[0], -1) if twin else None
        return self.x1, self.x2

    def forward(self, state, action):
        return self._run(state, action, True)

    def Q1(self, state, action):
        return self._run(state, action, False)[0]
