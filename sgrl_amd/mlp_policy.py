"""Monolithic MLP actor / critic behind the reference's module surfaces: the single-morphology baseline.

`MlpPolicy` / `MlpCritic` keep the constructor signatures, `forward`, `Q1`, `change_morphology` and the `state_dict()` keys,
shapes and buffers of reference src/MLPActor.py:11-97 and src/MLPCritic.py:9-58 (networks of src/common/networks.py:92-124,
184-220), so a reference checkpoint loads unchanged.  One network reads the whole observation row of ONE limb count L:
  actor   Linear(41 L, h0) ReLU ... Linear(h_last, 3 L), then max_action * tanh   (`actor.networks.{0,2,4}.{weight,bias}`,
          buffers `actor.action_scale` / `actor.action_bias` of the action space's shape, 3 L - 3)
  critic  two of Linear(44 L, h0) ReLU ... Linear(h_last, 1) over cat([state, action])   (`critic{1,2}.networks.{0,2,4}...`)
L comes from `args.mlp_num_limbs` when set, otherwise from `args.graphs[args.envs_train_names[-1]]` (the reference's rule,
MLPActor.py:42); the hidden widths from `args.agent['policy_network']['hidden_dims']` / `args.agent['q_network']['hidden_dims']`
when present, otherwise the reference's [256, 256] (configs/default.py:13-28).  Pinned to fixtures produced by executing the
reference's own modules (tests/golden/mlp_forward.npz, tools/capture_golden_mlp.py).  The batched rollout runs the actor's
no-grad forward as one HIP launch (mlp_hip.HipMlpActor, csrc/mlp_actor.hip), a TD3 update its no-grad target chain as one launch over
the target modules' handles (mlp_hip.HipMlpTargets); `forward` itself stays plain PyTorch for autograd."""
import torch
import torch.nn as nn

DEFAULT_HIDDEN = (256, 256)


def _agent_entry(args, key):
    """args.agent[key] whether args.agent is a dict (the reference's config) or a namespace (td3.default_train_args); None if absent."""
    agent = getattr(args, "agent", None)
    if agent is None:
        return None
    if isinstance(agent, dict):
        return agent.get(key)
    try:
        return agent[key]
    except (TypeError, KeyError, IndexError):
        return getattr(agent, key, None)


def hidden_dims(args, key):
    """Hidden widths of `key` ('policy_network' / 'q_network'): a list of 1 or more positive ints."""
    ent = _agent_entry(args, key)
    dims = None
    if ent is not None:
        dims = ent.get("hidden_dims") if isinstance(ent, dict) else getattr(ent, "hidden_dims", None)
    if dims is None:
        dims = DEFAULT_HIDDEN
    if isinstance(dims, int):
        dims = [dims]
    dims = [int(d) for d in dims]
    if not dims or min(dims) < 1:
        raise ValueError("%s hidden_dims must be one or more positive widths, got %r" % (key, dims))
    return dims


def mlp_num_limbs(args):
    """The limb count an MLP agent is built for: args.mlp_num_limbs, else len(args.graphs[args.envs_train_names[-1]])."""
    L = getattr(args, "mlp_num_limbs", None)
    if L is None:
        graphs, names = getattr(args, "graphs", None), getattr(args, "envs_train_names", None)
        if graphs is None or not names:
            raise ValueError("an MLP agent needs its limb count: set args.mlp_num_limbs, or args.graphs and args.envs_train_names "
                             "(the network is sized for the LAST training morphology, reference MLPActor.py:42)")
        L = len(graphs[names[-1]])
    L = int(L)
    if L < 1:
        raise ValueError("mlp_num_limbs must be positive, got %d" % L)
    return L


def _action_space(args, L, action_dim):
    """(low, high) float32 vectors of the last training morphology's action space: args.action_space[name] when the caller has one
    (reference main.py), otherwise the shipped environments' [-1, 1] box of 3 L - 3 motors."""
    spaces, names = getattr(args, "action_space", None), getattr(args, "envs_train_names", None)
    if spaces is not None and names and names[-1] in spaces:
        sp = spaces[names[-1]]
        return torch.as_tensor(sp.low, dtype=torch.float32), torch.as_tensor(sp.high, dtype=torch.float32)
    n = action_dim * L - 3
    return -torch.ones(n), torch.ones(n)


class MLPNetwork(nn.Module):
    """reference common/networks.py:92-124: Linear / ReLU pairs and a final Linear (+ Identity), as `networks`."""

    def __init__(self, input_dim, out_dim, hidden):
        super().__init__()
        dims = [int(input_dim)] + [int(h) for h in hidden]
        layers = []
        for i in range(len(dims) - 1):
            layers += [nn.Linear(dims[i], dims[i + 1]), nn.ReLU()]
        layers += [nn.Linear(dims[-1], int(out_dim)), nn.Identity()]
        self.networks = nn.Sequential(*layers)

    def forward(self, x):
        return self.networks(x)

    def linears(self):
        return [m for m in self.networks if isinstance(m, nn.Linear)]


class DeterministicPolicyNetwork(MLPNetwork):
    """reference common/networks.py:184-220: the same stack with action_space.shape[0] + 3 outputs (networks.py:162) and the
    action space's scale / bias as buffers (part of the state_dict; `forward` does not use them)."""

    def __init__(self, input_dim, low, high, hidden):
        super().__init__(input_dim, int(low.numel()) + 3, hidden)
        self.register_buffer("action_scale", (high - low) / 2.0)
        self.register_buffer("action_bias", (high + low) / 2.0)


class MlpPolicy(nn.Module):
    """Drop-in for reference MLPActor.MlpPolicy (constructor of MLPActor.py:14-26)."""

    def __init__(self, state_dim, action_dim, msg_dim, batch_size, max_action, max_children, disable_fold, td, bu, args=None,
                 device=None):
        super().__init__()
        self.max_action = max_action
        self.msg_dim, self.batch_size = msg_dim, batch_size
        self.state_dim, self.action_dim = state_dim, action_dim
        self.mlp_num_limbs = mlp_num_limbs(args)
        low, high = _action_space(args, self.mlp_num_limbs, action_dim)
        self.actor = DeterministicPolicyNetwork(state_dim * self.mlp_num_limbs, low, high, hidden_dims(args, "policy_network"))
        if device is not None:
            self.to(device)
        self.graph = None
        self.num_limbs = self.mlp_num_limbs
        self._mlp_hip = None

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_mlp_hip"] = None      # per-process device handle: never pickled / deep-copied with the module
        return d

    def hip_handle(self):
        """The module's mlp_hip.HipMlpActor, created on first use (raises _lib.SgrlError without an MI355X: no fallback)."""
        if getattr(self, "_mlp_hip", None) is None:
            from .mlp_hip import HipMlpActor
            self._mlp_hip = HipMlpActor(self)
        return self._mlp_hip

    def forward(self, state, mode="train"):
        self.action = self.max_action * torch.tanh(self.actor(state))
        return self.action

    def change_morphology(self, graph):
        self.graph = graph
        self.parents = graph["parents"]
        self.num_limbs = len(self.parents)


class MlpCritic(nn.Module):
    """Drop-in for reference MLPCritic.MlpCritic (twin Q values [B, 1] over cat([state, action]))."""

    def __init__(self, state_dim, action_dim, msg_dim, batch_size, max_children, disable_fold, td, bu, args=None, device=None):
        super().__init__()
        self.msg_dim, self.batch_size, self.max_children, self.disable_fold = msg_dim, batch_size, max_children, disable_fold
        self.state_dim, self.action_dim = state_dim, action_dim
        self.mlp_num_limbs = mlp_num_limbs(args)
        hidden = hidden_dims(args, "q_network")
        self.critic1 = MLPNetwork((state_dim + action_dim) * self.mlp_num_limbs, 1, hidden)
        self.critic2 = MLPNetwork((state_dim + action_dim) * self.mlp_num_limbs, 1, hidden)
        if device is not None:
            self.to(device)
        self.graph = None
        self.num_limbs = self.mlp_num_limbs
        self._mlp_hip = None

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_mlp_hip"] = None      # per-process device handle: never pickled / deep-copied with the module
        return d

    def hip_handle(self):
        """The module's mlp_hip.HipMlpCritic, created on first use (raises _lib.SgrlError without an MI355X: no fallback)."""
        if getattr(self, "_mlp_hip", None) is None:
            from .mlp_hip import HipMlpCritic
            self._mlp_hip = HipMlpCritic(self)
        return self._mlp_hip

    def forward(self, state, action):
        inpt = torch.cat([state, action], dim=-1)
        return self.critic1(inpt), self.critic2(inpt)

    def Q1(self, state, action):
        return self.critic1(torch.cat([state, action], dim=-1))

    def change_morphology(self, graph):
        self.graph = graph
        self.parents = graph["parents"]
        self.num_limbs = len(self.parents)
