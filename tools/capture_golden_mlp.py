#!/usr/bin/env python3
"""Golden vectors for the monolithic MLP baseline: EXECUTES the reference's MlpPolicy / MlpCritic (reference src/MLPActor.py:11-97,
src/MLPCritic.py:9-58, src/common/networks.py:92-220) and its `Agent.update` with actor_type = critic_type = 'mlp' (src/agent.py:
117-183) on seed-generated weights (tests/mlp_restate.py `apply_seeded_`: the fixtures store the seed, not the weights) and
synthetic rows.  The action space is the import harness's stand-in for gym.spaces.Box (tools/refstub.py) with the shipped
environments' [-1, 1] range over 3 L - 3 motors.  Build container only; numbers and name lists only.  Writes into tests/golden/:
  mlp_state_dict_keys.json   keys and shapes of both modules for hopper_3 and walker_7
  mlp_forward.npz            per morphology: 6 observation / action rows, the reference's actions and Q1 / Q2
  td3_update_mlp.npz         two updates on walker_7 at 6 rows (it = 0: critic, actor and targets move; it = 1: critic only), in the
                             layout of td3_update.npz (losses, per-tensor sums of clipped gradients and of every parameter of the
                             four networks) plus, per tensor, the RAW gradient's L2 norm and eight sampled elements where the
                             reference clips, and the L2 norm of every parameter's step -- float32 as the reference runs and the
                             same script in float64 (the yardstick of tests/test_td3_update_init.py)."""
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import refstub
refstub.install()
_shim = types.ModuleType("numpy.lib.arraysetops")      # agent.py:1 imports `isin` from it and never uses it
_shim.isin = np.isin
sys.modules["numpy.lib.arraysetops"] = _shim
warnings.filterwarnings("ignore", "Redundant parameters for MLP network")

import gym  # noqa: E402  (the stub)
import utils as ref_utils  # noqa: E402
from agent import Agent  # noqa: E402
from MLPActor import MlpPolicy  # noqa: E402
from MLPCritic import MlpCritic  # noqa: E402
from configs.default import default_args as REF_DEFAULTS  # noqa: E402
from capture_golden import _args_ns  # noqa: E402
from capture_golden_update import HYPER  # noqa: E402
from capture_golden_update_init import grad_record  # noqa: E402
from mlp_restate import apply_seeded_  # noqa: E402
from oracle.formula import scripted_batch, synth_obs  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
SEED = 17
ROWS = 6
NAMES = ["3d_hopper_3_shin", "3d_walker_7_full"]


class AttrDict(dict):
    """args.agent of the reference is read both ways (agent.py:113 `.target_smoothing_tau`, MLPActor.py:42 `['policy_network']`)."""
    __getattr__ = dict.__getitem__


def make_args(name):
    xm = refstub.all_xmls()
    a = _args_ns()
    a.actor_type = a.critic_type = "mlp"
    a.limb_obs_size, a.limb_action_size, a.msg_dim, a.batch_size = 41, 3, 32, 100
    a.max_action, a.max_children, a.disable_fold, a.td, a.bu = HYPER["max_action"], 3, True, False, False
    for k in ("lr", "policy_noise", "noise_clip", "discount", "policy_freq", "grad_clipping_value"):
        setattr(a, k, HYPER[k])
    a.agent = AttrDict(target_smoothing_tau=HYPER["target_smoothing_tau"], reward_scale=HYPER["reward_scale"],
                       policy_network=dict(REF_DEFAULTS["agent"]["policy_network"]), q_network=dict(REF_DEFAULTS["agent"]["q_network"]))
    a.envs_train_names = [name]
    a.graphs = {name: ref_utils.getGraphStructure(xm[name])}
    L = len(a.graphs[name])
    a.action_space = {name: gym.spaces.Box(-np.ones(3 * L - 3, dtype=np.float32), np.ones(3 * L - 3, dtype=np.float32))}
    return a, L


def forward_fixtures():
    keys, res = {}, {"seed": np.array(SEED), "names": np.array(NAMES)}
    for name in NAMES:
        a, L = make_args(name)
        pol = MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, a).eval()
        crit = MlpCritic(41, 3, 32, 100, 3, True, False, False, a).eval()
        keys[name] = {"actor": {k: list(v.shape) for k, v in pol.state_dict().items()},
                      "critic": {k: list(v.shape) for k, v in crit.state_dict().items()}}
        apply_seeded_(pol, SEED)
        apply_seeded_(crit, SEED)
        gd = ref_utils.getGraphDict(a.graphs[name], ["pre", "inlcrs", "postlcrs"], [], device=torch.device("cpu"))
        pol.change_morphology(gd)
        crit.change_morphology(gd)
        obs = synth_obs(L, ROWS, 31 + L).astype(np.float32)
        act = np.random.RandomState(100 + L).uniform(-1, 1, size=(ROWS, 3 * L)).astype(np.float32)
        with torch.no_grad():
            out = pol(torch.from_numpy(obs))
            q1, q2 = crit(torch.from_numpy(obs), torch.from_numpy(act))
            assert torch.equal(q1, crit.Q1(torch.from_numpy(obs), torch.from_numpy(act)))
        res[name + "/obs"], res[name + "/act_in"], res[name + "/action"] = obs, act, out.numpy()
        res[name + "/q1"], res[name + "/q2"] = q1.numpy(), q2.numpy()
        res[name + "/action_scale"] = pol.state_dict()["actor.action_scale"].numpy()
        res[name + "/action_bias"] = pol.state_dict()["actor.action_bias"].numpy()
        print(name, "|action| mean %.3f, q1 mean %.3f" % (np.abs(out.numpy()).mean(), q1.mean()))
    with open(os.path.join(GOLD, "mlp_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
    np.savez_compressed(os.path.join(GOLD, "mlp_forward.npz"), **res)


def tensor_sums(module, grads=False):
    return np.array([0.0 if (p.grad if grads else p) is None else float((p.grad if grads else p).detach().double().sum())
                     for _, p in module.named_parameters()])


def run_update(dtype):
    torch.set_default_dtype(dtype)
    name = "3d_walker_7_full"
    a, L = make_args(name)
    torch.manual_seed(0)
    agent = Agent(a)
    apply_seeded_(agent.actor, SEED)
    apply_seeded_(agent.critic, SEED)
    with torch.no_grad():       # targets = 0.97 x online so that the Polyak step is visible (as tools/capture_golden_update.py)
        for tgt, src in ((agent.actor_target, agent.actor), (agent.critic_target, agent.critic)):
            for tp, sp in zip(tgt.parameters(), src.parameters()):
                tp.copy_(0.97 * sp)
    agent.change_morphology(ref_utils.getGraphDict(a.graphs[name], ["pre", "inlcrs", "postlcrs"], [], device=torch.device("cpu")))
    agent.models2train()
    res, grabbed = {}, {}
    real_clip, real_normal = torch.nn.utils.clip_grad_norm_, torch.Tensor.normal_

    def clip_spy(params, max_norm, *args, **kw):
        params = list(params)
        which = "critic" if params[0] is next(agent.critic.parameters()) else "actor"
        grabbed[which] = grad_record(getattr(agent, which))
        return real_clip(params, max_norm, *args, **kw)

    def normal32(self, mean=0, std=1, *, generator=None):      # the float64 run consumes the float32 run's noise
        if self.dtype == torch.float64:
            tmp = torch.empty(self.shape, dtype=torch.float32)
            real_normal(tmp, mean, std)
            return self.copy_(tmp)
        return real_normal(self, mean, std)

    torch.nn.utils.clip_grad_norm_, torch.Tensor.normal_ = clip_spy, normal32
    try:
        for it, seed in enumerate((11, 23)):
            b = scripted_batch(L, ROWS, seed)
            torch.manual_seed(1000 + it)
            noise = torch.zeros(ROWS, 3 * L, dtype=torch.float32).normal_(0, HYPER["policy_noise"]).numpy().copy()
            before = {nm: [p.detach().double().clone() for p in getattr(agent, nm).parameters()] for nm in ("actor", "critic")}
            grabbed.clear()
            torch.manual_seed(1000 + it)
            loss = agent.update({k: torch.from_numpy(v).to(dtype) for k, v in b.items()}, it)
            tag = "it%d/" % it
            res[tag + "name"], res[tag + "batch_seed"], res[tag + "noise"] = np.array(name), np.array(seed), noise
            for k, v in b.items():
                res[tag + k] = v
            res[tag + "critic_loss"] = np.array(float(loss["loss/critic_loss"]))
            res[tag + "actor_loss"] = np.array(float(loss["loss/actor_loss"]) if "loss/actor_loss" in loss else np.nan)
            res[tag + "train_reward_mean"] = np.array(loss["misc/train_reward_mean"])
            res[tag + "critic_grad_sums"] = tensor_sums(agent.critic, grads=True)
            res[tag + "actor_grad_sums"] = tensor_sums(agent.actor, grads=True)
            for nm in ("actor", "critic", "actor_target", "critic_target"):
                res[tag + nm + "_param_sums"] = tensor_sums(getattr(agent, nm))
            for nm in ("critic", "actor"):
                if nm in grabbed:
                    res[tag + nm + "_grad_norms"], res[tag + nm + "_grad_samples"] = grabbed[nm]
                res[tag + nm + "_step_norms"] = np.array([float((p.detach().double() - q).norm())
                                                          for p, q in zip(getattr(agent, nm).parameters(), before[nm])])
            print(dtype, it, "critic_loss %.6f" % res[tag + "critic_loss"], "actor_loss", res[tag + "actor_loss"])
    finally:
        torch.nn.utils.clip_grad_norm_, torch.Tensor.normal_ = real_clip, real_normal
        torch.set_default_dtype(torch.float32)
    names = {"actor_param_names": np.array([n for n, _ in agent.actor.named_parameters()]),
             "critic_param_names": np.array([n for n, _ in agent.critic.named_parameters()]),
             "actor_numel": np.array([p.numel() for p in agent.actor.parameters()]),
             "critic_numel": np.array([p.numel() for p in agent.critic.parameters()])}
    return res, names


def update_fixture():
    r32, names = run_update(torch.float32)
    r64, _ = run_update(torch.float64)
    hyper = dict(HYPER, batch=ROWS)
    out = dict(names)
    out["seed"] = np.array(SEED)
    out["hyper_keys"] = np.array(sorted(hyper))
    out["hyper_vals"] = np.array([float(hyper[k]) for k in sorted(hyper)])
    out.update(r32)
    for k, v in r64.items():
        if v.dtype.kind == "f" and k.split("/")[-1] not in ("noise", "obs", "next_obs", "action", "reward", "done"):
            out[k + "_f64"] = v
    np.savez_compressed(os.path.join(GOLD, "td3_update_mlp.npz"), **out)


if __name__ == "__main__":
    forward_fixtures()
    update_fixture()
    for f in ("mlp_state_dict_keys.json", "mlp_forward.npz", "td3_update_mlp.npz"):
        print(f, os.path.getsize(os.path.join(GOLD, f)), "bytes")
