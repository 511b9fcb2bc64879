"""Shared by tests/test_set_full_rank.py and tests/test_set_full_rank_gpu.py: the float64 CPU modules as the reference of the SET
forwards (action / Q and the hooked stages), the parity bounds, and the column-swap census that qualifies a weight set.

Stages: forward hooks on `layers[i].self_attn` (the attention's vector and scalar outputs), `layers[i]` (the layer's g and ng)
and `transformer_encoder` (g and the final norm's ng) -- 14 tensors, node-major [B * L, ...] as the device keeps them."""
import numpy as np
import torch

from sgrl_amd import graph as G, mjcf
from sgrl_amd.set_policy import make_critic, make_policy

TRAV = ["pre", "inlcrs", "postlcrs"]
TOL_ACTION = 2e-5           # absolute, on tanh-squashed actions (tests/test_set_gpu.py)
TOL_STAGE = 2e-5            # x (1 + max |ref|) (tests/test_set_gpu.py test_layer_probes_on_the_gpu)
TOL_Q = 2e-5                # x max |q_ref|


def graph_dict(name, device="cpu", f64=False):
    gd = G.getGraphDict(mjcf.load_asset(name).parents, TRAV, [], device=torch.device(device))
    if f64:
        gd = dict(gd)
        gd["relation"] = gd["relation"].double()
    return gd


def num_limbs(name):
    return mjcf.load_asset(name).num_limbs


def critic_actions(L, B, seed):
    return np.random.RandomState(seed).uniform(-1, 1, size=(B, 3 * L))


class Hooks(object):
    """Collects the 14 stage tensors of one TransformerModel forward as float64 NumPy, node-major."""

    def __init__(self, net):
        self.out = {}
        enc = net.transformer_encoder
        self.handles = [enc.register_forward_hook(self._keep("encoder"))]
        for i, layer in enumerate(enc.layers):
            self.handles.append(layer.register_forward_hook(self._keep("layer%d" % i)))
            self.handles.append(layer.self_attn.register_forward_hook(self._keep("layer%d/attn" % i)))

    def _keep(self, name):
        def hook(module, args, output):
            for k in (0, 1):
                t = output[k].detach()
                self.out["%s/out%d" % (name, k)] = t.reshape(t.shape[0] * t.shape[1], -1).double().numpy().copy()
        return hook

    def remove(self):
        for h in self.handles:
            h.remove()


def actor_forward(pol, name, obs, f64=True):
    """(action [B, 3 L], stages) of a CPU SEPolicy in its own dtype on morphology `name`."""
    pol.change_morphology(graph_dict(name, f64=f64))
    hk = Hooks(pol.actor)
    try:
        with torch.no_grad():
            a = pol(torch.from_numpy(obs).to(next(pol.parameters()).dtype))
    finally:
        hk.remove()
    return a.double().numpy(), hk.out


def critic_forward(crit, name, obs, action, f64=True):
    """((q1, q2) [B, L] each, (stages of critic1, of critic2)) of a CPU SECritic in its own dtype."""
    crit.change_morphology(graph_dict(name, f64=f64))
    hk = [Hooks(crit.critic1), Hooks(crit.critic2)]
    dt = next(crit.parameters()).dtype
    try:
        with torch.no_grad():
            q1, q2 = crit(torch.from_numpy(obs).to(dt), torch.from_numpy(action).to(dt))
    finally:
        for h in hk:
            h.remove()
    return (q1.double().numpy(), q2.double().numpy()), (hk[0].out, hk[1].out)


def stage_bounds(stages):
    return {k: TOL_STAGE * (1.0 + np.abs(v).max()) for k, v in stages.items()}


def cpu_modules(kind, apply, dtype):
    """A CPU module (kind 'actor' / 'critic') with `apply(module)` weights in `dtype` (values generated in float64, then cast)."""
    m = (make_policy if kind == "actor" else make_critic)(device="cpu", use_hip=False)
    m = m.to(dtype).eval()
    return apply(m)


# ---- the census ---------------------------------------------------------------------------------------------------------------
def swap_sites(net):
    """[(parameter name, tensor, c0, c1)]: for every 2-D parameter with at least 16 input columns the exchanges 3 <-> 11 and
    5 <-> 5 + 8 (K // 16) -- what a wrong pack permutation, K-slice order, perm32, Gram fold or fragment layout does."""
    sites = []
    for name, p in net.named_parameters():
        if p.dim() == 2 and p.shape[1] >= 16:
            K = p.shape[1]
            sites.append((name, p, 3, 11))
            sites.append((name, p, 5, 5 + 8 * (K // 16)))
    return sites


def _swap(p, c0, c1):
    with torch.no_grad():
        a = p[:, c0].clone()
        p[:, c0] = p[:, c1]
        p[:, c1] = a


def census(net, run, bounds):
    """run() -> {quantity: float64 array} with key 'out' the network's output; bounds: {quantity: device-test bound}.  Every swap of
    swap_sites(net) is applied, run and undone.  Returns [(label, live, out shift / bound, largest shift / bound over all)]."""
    base = run()
    rows = []
    for name, p, c0, c1 in swap_sites(net):
        _swap(p, c0, c1)
        try:
            got = run()
        finally:
            _swap(p, c0, c1)
        ratio = {k: np.abs(got[k] - base[k]).max() / bounds[k] for k in base}
        rows.append(("%s[:, %d<->%d]" % (name, c0, c1), ratio["out"] > 0.0, ratio["out"], max(ratio.values())))
    return rows


def census_summary(rows):
    live = [r for r in rows if r[1]]
    return dict(swaps=len(rows), live=len(live), hidden_in_output=sum(r[2] < 1.0 for r in live),
                hidden_everywhere=sum(r[3] < 1.0 for r in live), weakest=min(r[3] for r in live),
                weakest_name=min(live, key=lambda r: r[3])[0])
