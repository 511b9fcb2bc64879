"""SWAT (structure-aware transformer) actor / critic behind the reference's module surfaces.

`StructurePolicy` / `CriticStructurePolicy` keep the constructor signatures, `forward`, `Q1`, `change_morphology` and the
`state_dict()` keys of reference src/StructureActor.py:176-273 / src/StructureCritic.py:8-125: a plain transformer over the
limbs (embedding size 128, 2 heads, 3 layers) with the three traversal-index position embeddings added once and the
relation bias (PPR, symmetric Laplacian, distance -> one additive bias per head) on the first layer only.  Plain
differentiable PyTorch; outputs are pinned to fixtures produced by executing the reference's own modules
(tests/golden/swat_forward.npz, tools/capture_golden_swat.py).  The batched rollout runs the actor's no-grad forward on the HIP
kernels of swat_hip.HipSwatActor (csrc/swat_actor.hip), which read this module's parameters in place; `forward` itself is what
the TD3 update back-props through: PyTorch operations by default, the training kernels of train_ops with `train_kernels` on
(_TrainKernelsSwitch; td3.Agent(swat_train_kernels=True)).  The no-grad target chain of an update (td3.Agent.update_targets) runs on the
same kernels through `hip_handle()`: the handle a module caches is per-process device state and is dropped whenever the
module is pickled or deep-copied.

Dropout (`args.dropout_rate`, which the reference hands to these networks only): in training mode the reference's five kinds of
site -- position embedding, attention weights, dropout1, dropout, dropout2 -- go through train_ops.dropout / swat_attention on both
paths; inside a train_ops.dropout_rng context (td3.Agent.update opens one) the masks are the counter RNG's (include/sgrl_train.h),
otherwise torch's.  The HIP forwards behind `hip_handle()` have no dropout: they refuse a module that is in training mode with
dropout > 0 (swat_hip.HipSwatActor.sync_weights), so collection and evaluation run in eval mode.
"""
import copy
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import train_ops
from .set_policy import ConcatPositionalEmbedding


class _TrainKernelsSwitch(object):
    """`train_kernels` (default False): the differentiable passes of the module on the library's own training kernels
    (train_ops: linear, swat_attention, add_layer_norm) instead of PyTorch's operations.  Setting it on a module sets it on every
    module below it.  A plain attribute: no parameter, not in state_dict(), kept by pickle / deepcopy.  Every train_ops entry falls
    back to the operations of the switch-off forward wherever its kernels do not run (CPU, float64, torch.no_grad()), so there
    the switch changes no bit."""

    @property
    def train_kernels(self):
        return self.__dict__.get("_train_kernels", False)

    @train_kernels.setter
    def train_kernels(self, on):
        for m in self.modules():
            if isinstance(m, _TrainKernelsSwitch):
                m.__dict__["_train_kernels"] = bool(on)


class _SelfAttention(_TrainKernelsSwitch, nn.Module):
    """Parameters of torch.nn.MultiheadAttention (in_proj_weight / in_proj_bias / out_proj), forward of the reference's
    attentions.multi_head_attention_forward: q scaled by head_dim^-0.5, additive float mask [B * H, L, L]."""

    dropout = 0.0          # (class default: a module pickled before the attribute existed)

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, float(dropout)
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)

    def forward(self, x, bias=None, slot=None):
        """x [B, L, E]; bias [H, L, L] or None.  slot (train_kernels): x is an alias handed out by train_ops.fan_out."""
        B, L, E = x.shape
        H = self.num_heads
        hd = E // H
        if self.train_kernels:
            qkv = train_ops.linear(x, self.in_proj_weight, self.in_proj_bias, slot=slot)
            o = train_ops.swat_attention(qkv, bias, float(hd) ** -0.5, H, dropout_p=self.dropout, training=self.training)
            return train_ops.linear(o, self.out_proj.weight, self.out_proj.bias)
        q, k, v = F.linear(x, self.in_proj_weight, self.in_proj_bias).chunk(3, dim=-1)
        q = (q * float(hd) ** -0.5).view(B, L, H, hd)
        k, v = k.view(B, L, H, hd), v.view(B, L, H, hd)
        s = torch.einsum("bihd,bjhd->bhij", q, k)
        if bias is not None:
            s = s + bias.unsqueeze(0)
        w = train_ops.dropout(F.softmax(s, dim=-1), self.dropout, self.training)       # reference attentions.py:163
        o = torch.einsum("bhij,bjhd->bihd", w, v).reshape(B, L, E)
        return self.out_proj(o)


class _EncoderLayer(_TrainKernelsSwitch, nn.Module):
    """reference MyTransformerEncoderLayer (StructureActor.py:48-66): post-norm, ReLU feed-forward; in training mode with
    `dropout` > 0 the reference's four dropouts: the attention weights (inside self_attn), dropout1 behind out_proj, `dropout`
    between the ReLU and linear2, dropout2 behind linear2 (train_ops.dropout: the identity otherwise, nothing launched)."""

    dropout = 0.0

    def __init__(self, d_model, nhead, dim_feedforward, dropout=0.0):
        super().__init__()
        self.dropout = float(dropout)
        self.self_attn = _SelfAttention(d_model, nhead, dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)

    def forward(self, x, bias=None):
        drop = lambda t: train_ops.dropout(t, self.dropout, self.training)
        if self.train_kernels:
            # x feeds in_proj and the residual, the first norm's output linear1 and the residual: handed out as aliases
            # (train_ops.fan_out), so that the two products add their input gradients onto the residual's instead of leaving an
            # element-wise addition each to autograd.  The hidden activation feeds linear2 only: the masked pair of train_ops.linear
            sa, (xa, xb) = train_ops.fan_out(x, 2)
            x = train_ops.add_layer_norm(xb, drop(self.self_attn(xa, bias, slot=sa)), self.norm1)
            sf, (xa, xb) = train_ops.fan_out(x, 2)
            h = train_ops.linear(xa, self.linear1.weight, self.linear1.bias, relu=True, premasked=True, slot=sf)
            # A dropout between the masked pair keeps it exact.  linear2's input is hd = dropout(h) = h * keep * s with s = 1 / (1 - p)
            # >= 1, so hd > 0 exactly where (h > 0) & keep (no product with s underflows to zero).  x_relu masks linear2's input
            # gradient by hd > 0: g = d_hd * [(h > 0) & keep].  The dropout's backward multiplies by keep * s, which changes nothing
            # where keep is already applied: d_h = d_hd * s * [(h > 0) & keep] -- the ReLU's mask AND the dropout's, which is what
            # linear1 (premasked: it applies no mask of its own) needs at its pre-activation.  p = 1: hd = 0, both sides are zero.
            h = drop(h)
            return train_ops.add_layer_norm(xb, drop(train_ops.linear(h, self.linear2.weight, self.linear2.bias, x_relu=True)), self.norm2)
        x = self.norm1(x + drop(self.self_attn(x, bias)))
        return self.norm2(x + drop(self.linear2(drop(F.relu(self.linear1(x))))))


class _Encoder(_TrainKernelsSwitch, nn.Module):
    """reference RepeatTransformerEncoder (StructureActor.py:68-107)."""

    def __init__(self, layer, num_layers, nhead, norm=None, d_rel=3):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(num_layers)])
        self.norm = norm
        self.nhead = nhead
        self.rel_encoder = nn.Linear(d_rel, nhead)

    def forward(self, x, pos, rel):
        x = x + pos.unsqueeze(0)
        bias = self.rel_encoder(rel).permute(2, 0, 1)          # [H, i, j]
        for i, layer in enumerate(self.layers):
            x = layer(x, bias if i == 0 else None)
        if self.norm is not None and self.train_kernels:
            return train_ops.add_layer_norm(x, None, self.norm)
        return self.norm(x) if self.norm is not None else x


class TransformerModel(_TrainKernelsSwitch, nn.Module):
    """reference StructureActor.TransformerModel (StructureActor.py:110-168)."""

    dropout = 0.0

    def __init__(self, feature_size, output_size, ninp, nhead, nhid, nlayers, dropout=0.0, condition_decoder=False,
                 transformer_norm=False, num_positions=0, rel_size=1):
        super().__init__()
        self.model_type = "Structure"
        # dropout (args.dropout_rate; a plain attribute, no parameter): applied in training mode to the position embedding's output
        # (reference StructureActor.py:29) and inside every encoder layer (_EncoderLayer)
        self.dropout = float(dropout)
        self.pos_encoder = ConcatPositionalEmbedding(ninp, num_positions=num_positions)
        self.transformer_encoder = _Encoder(_EncoderLayer(ninp, nhead, nhid, self.dropout), nlayers, nhead,
                                            norm=nn.LayerNorm(ninp) if transformer_norm else None, d_rel=rel_size)
        self.encoder = nn.Linear(feature_size, ninp)
        self.ninp = ninp
        self.condition_decoder = bool(condition_decoder)
        self.decoder = nn.Linear(ninp + feature_size if condition_decoder else ninp, output_size)
        with torch.no_grad():
            self.encoder.weight.uniform_(-0.1, 0.1)
            self.decoder.bias.zero_()
            self.decoder.weight.uniform_(-0.1, 0.1)

    def forward(self, x, graph):
        """x [B, L, feature] (node-major) -> [B, L, output_size]."""
        kernels = self.train_kernels
        h = (train_ops.linear(x, self.encoder.weight, self.encoder.bias) if kernels else self.encoder(x)) * math.sqrt(self.ninp)
        pos = train_ops.dropout(self.pos_encoder(graph["traversals"]), self.dropout, self.training)
        h = self.transformer_encoder(h, pos, graph["relation"])
        if self.condition_decoder:
            h = torch.cat([h, x], dim=2)
        return train_ops.linear(h, self.decoder.weight, self.decoder.bias) if kernels else self.decoder(h)


def _model(feature, out, args):
    return TransformerModel(feature, out, args.attention_embedding_size, args.attention_heads, args.attention_hidden_size,
                            args.attention_layers, args.dropout_rate, condition_decoder=args.condition_decoder_on_features,
                            transformer_norm=args.transformer_norm, num_positions=len(args.traversal_types),
                            rel_size=args.rel_size)


class StructurePolicy(_TrainKernelsSwitch, nn.Module):
    """Drop-in for reference StructureActor.StructurePolicy (constructor of StructureActor.py:179-191)."""

    def __init__(self, state_dim, action_dim, msg_dim, batch_size, max_action, max_children, disable_fold, td, bu,
                 args=None, device=None):
        super().__init__()
        self.num_limbs = 1
        self.max_action = max_action
        self.msg_dim, self.batch_size, self.max_children, self.disable_fold = msg_dim, batch_size, max_children, disable_fold
        self.state_dim, self.action_dim = state_dim, action_dim
        self.actor = _model(state_dim, action_dim, args)
        if device is not None:
            self.actor.to(device)
        self.graph = None
        self._swat_hip = None

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_swat_hip"] = None     # per-process device handle: never pickled / deep-copied with the module
        return d

    def hip_handle(self):
        """The module's swat_hip.HipSwatActor, created on first use (raises _lib.SgrlError without an MI355X: no fallback)."""
        if getattr(self, "_swat_hip", None) is None:
            from .swat_hip import HipSwatActor
            self._swat_hip = HipSwatActor(self)
        return self._swat_hip

    def clear_buffer(self):
        self.action = None
        self.input_state = None

    def forward(self, state, mode="train"):
        self.clear_buffer()
        B = state.shape[0]
        x = state.reshape(B, self.num_limbs, -1)
        self.action = (self.max_action * torch.tanh(self.actor(x, self.graph))).reshape(B, -1)
        return self.action

    def change_morphology(self, graph):
        self.graph = graph
        self.parents = graph["parents"]
        self.num_limbs = len(self.parents)


class CriticStructurePolicy(_TrainKernelsSwitch, nn.Module):
    """Drop-in for reference StructureCritic.CriticStructurePolicy (per-limb twin Q values [B, L])."""

    def __init__(self, state_dim, action_dim, msg_dim, batch_size, max_children, disable_fold, td, bu, args=None,
                 device=None):
        super().__init__()
        self.num_limbs = 1
        self.msg_dim, self.batch_size, self.max_children, self.disable_fold = msg_dim, batch_size, max_children, disable_fold
        self.state_dim, self.action_dim = state_dim, action_dim
        self.critic1 = _model(state_dim + action_dim, 1, args)
        self.critic2 = _model(state_dim + action_dim, 1, args)
        if device is not None:
            self.to(device)
        self.graph = None
        self._swat_hip = None

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_swat_hip"] = None     # per-process device handles: never pickled / deep-copied with the module
        return d

    def hip_handle(self):
        """The module's swat_hip.HipSwatCritic, created on first use (raises _lib.SgrlError without an MI355X: no fallback)."""
        if getattr(self, "_swat_hip", None) is None:
            from .swat_hip import HipSwatCritic
            self._swat_hip = HipSwatCritic(self)
        return self._swat_hip

    def _input(self, state, action):
        B = state.shape[0]
        assert state.shape[1] == self.state_dim * self.num_limbs, \
            "state.shape[1] expects {} but got {}".format(self.state_dim * self.num_limbs, state.shape[1])
        return torch.cat([state.reshape(B, self.num_limbs, -1), action.reshape(B, self.num_limbs, -1)], dim=2)

    def forward(self, state, action):
        x = self._input(state, action)
        B = x.shape[0]
        return self.critic1(x, self.graph).reshape(B, -1), self.critic2(x, self.graph).reshape(B, -1)

    def Q1(self, state, action):
        x = self._input(state, action)
        return self.critic1(x, self.graph).reshape(x.shape[0], -1)

    def clear_buffer(self):
        pass

    def change_morphology(self, graph):
        self.graph = graph
        self.parents = graph["parents"]
        self.num_limbs = len(self.parents)
