"""Monolithic MLP baseline (sgrl_amd/mlp_policy.py, td3.Agent with actor_type = critic_type = 'mlp') against fixtures produced by
executing the reference's MlpPolicy / MlpCritic and its Agent.update (tools/capture_golden_mlp.py): state_dict keys and shapes
identical, forward within f32 rounding, one critic-and-policy update and one critic-only update at the per-tensor tolerance of
tests/test_td3_update_init.py; plus the refusals: a limb count the network was not built for, mixes with the graph types, graphed
updates."""
import json
import os

import numpy as np
import pytest
import torch

from mlp_restate import apply_seeded_
from sgrl_amd import graph as G, mjcf
from sgrl_amd import td3
from sgrl_amd.mlp_policy import MlpCritic, MlpPolicy
from sgrl_amd.td3 import Agent, default_train_args

TRAV = ["pre", "inlcrs", "postlcrs"]
NS = 8


@pytest.fixture(scope="module")
def gold(golden_dir):
    with open(os.path.join(golden_dir, "mlp_state_dict_keys.json")) as f:
        keys = json.load(f)
    return keys, np.load(os.path.join(golden_dir, "mlp_forward.npz"))


def _graph(name):
    return G.getGraphDict(mjcf.load_asset(name).parents, TRAV, [], device=torch.device("cpu"))


@pytest.mark.parametrize("name", ["3d_hopper_3_shin", "3d_walker_7_full"])
def test_mlp_actor_and_critic_match_the_reference(gold, name):
    keys, z = gold
    L = mjcf.load_asset(name).num_limbs
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L)
    pol = MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, args).eval()
    crit = MlpCritic(41, 3, 32, 100, 3, True, False, False, args).eval()
    assert {k: list(v.shape) for k, v in pol.state_dict().items()} == keys[name]["actor"]
    assert {k: list(v.shape) for k, v in crit.state_dict().items()} == keys[name]["critic"]
    np.testing.assert_array_equal(pol.state_dict()["actor.action_scale"].numpy(), z[name + "/action_scale"])
    np.testing.assert_array_equal(pol.state_dict()["actor.action_bias"].numpy(), z[name + "/action_bias"])
    apply_seeded_(pol, int(z["seed"]))
    apply_seeded_(crit, int(z["seed"]))
    gd = _graph(name)
    pol.change_morphology(gd)
    crit.change_morphology(gd)
    assert pol.graph is gd and pol.num_limbs == L and crit.num_limbs == L
    obs, act = torch.from_numpy(z[name + "/obs"]), torch.from_numpy(z[name + "/act_in"])
    with torch.no_grad():
        a = pol(obs)
        q1, q2 = crit(obs, act)
        q1b = crit.Q1(obs, act)
    assert a.shape == (6, 3 * L) and q1.shape == (6, 1) and q2.shape == (6, 1)
    np.testing.assert_allclose(a.numpy(), z[name + "/action"], atol=2e-6)
    scale = max(1.0, np.abs(z[name + "/q1"]).max())
    np.testing.assert_allclose(q1.numpy(), z[name + "/q1"], atol=1e-5 * scale)
    np.testing.assert_allclose(q2.numpy(), z[name + "/q2"], atol=1e-5 * scale)
    assert torch.equal(q1, q1b)


def test_limb_count_and_hidden_widths_come_from_the_arguments():
    gd = {"3d_hopper_3_shin": [-1, 0, 1], "3d_walker_7_full": [-1, 0, 1, 2, 0, 4, 5]}
    args = default_train_args(actor_type="mlp", critic_type="mlp", graphs=gd, envs_train_names=["3d_hopper_3_shin", "3d_walker_7_full"])
    pol = MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, args)
    assert pol.mlp_num_limbs == 7 and pol.actor.networks[0].in_features == 287 and pol.actor.networks[4].out_features == 21
    args.mlp_num_limbs = 3                                   # the explicit count wins
    args.agent.policy_network = {"hidden_dims": [40, 72, 16]}
    args.agent.q_network = {"hidden_dims": 24}
    pol = MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, args)
    crit = MlpCritic(41, 3, 32, 100, 3, True, False, False, args)
    assert [tuple(m.weight.shape) for m in pol.actor.networks if isinstance(m, torch.nn.Linear)] == [(40, 123), (72, 40), (16, 72), (9, 16)]
    assert [tuple(m.weight.shape) for m in crit.critic2.networks if isinstance(m, torch.nn.Linear)] == [(24, 132), (1, 24)]
    assert tuple(pol.actor.action_scale.shape) == (6,)
    with pytest.raises(ValueError, match="limb count"):
        MlpPolicy(41, 3, 32, 100, 1.0, 3, True, False, False, default_train_args())
    # the defaults of the other types did not move
    d = default_train_args()
    assert (d.actor_type, d.critic_type, d.agent.target_smoothing_tau, d.agent.reward_scale, d.agent_batch_size) == ("set", "set", 0.005, 1.0, 256)


def test_refused_mixes_and_graphed_updates():
    for a, c in (("mlp", "set"), ("swat", "mlp"), ("mlp", "smp")):
        with pytest.raises(NotImplementedError, match="'mlp' actor goes with an 'mlp' critic"):
            Agent(default_train_args(actor_type=a, critic_type=c, mlp_num_limbs=3), device="cpu")
    with pytest.raises(NotImplementedError):
        Agent(default_train_args(actor_type="gnn", critic_type="gnn"), device="cpu")
    agent = Agent(default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3), device="cpu")
    assert isinstance(agent.actor, MlpPolicy) and isinstance(agent.critic_target, MlpCritic)
    assert not agent.use_swat_hip and not agent.use_smp_hip
    for p, q in zip(agent.actor.parameters(), agent.actor_target.parameters()):
        assert torch.equal(p, q)
    with pytest.raises(NotImplementedError, match="GraphedUpdates is not built for 'mlp'"):
        td3.GraphedUpdates(agent, 256)
    from sgrl_amd.rollout import hip_actor_class
    from sgrl_amd.mlp_hip import HipMlpActor
    assert hip_actor_class(agent.actor) is HipMlpActor


def test_limb_count_mismatch_names_the_environment():
    from sgrl_amd.rollout import Rollout, check_mlp_limbs
    agent = Agent(default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=3), device="cpu")
    check_mlp_limbs(agent.actor, ["3d_hopper_3_shin", "3d_walker_3_left_knee_right_knee"])      # two morphologies of three limbs
    with pytest.raises(ValueError, match="3d_walker_7_full.*7 limbs.*built for 3"):
        check_mlp_limbs(agent.actor, ["3d_hopper_3_shin", "3d_walker_7_full"])
    # the rollout (training, evaluation and demo environments all go through it) refuses at construction, before any device work
    with pytest.raises(ValueError, match="3d_hopper_4_lower_shin"):
        Rollout(["3d_hopper_3_shin", "3d_hopper_4_lower_shin"], 2, policy=agent.actor, device="cpu")
    check_mlp_limbs(None, ["3d_walker_7_full"])                # any other policy passes
    set_agent = Agent(default_train_args(), device="cpu", use_hip=False)
    check_mlp_limbs(set_agent.actor, ["3d_hopper_3_shin", "3d_walker_7_full"])


# ---- Agent.update against the reference's ---------------------------------------------------------------------------------------
def _sample_idx(numel):
    return np.unique(np.linspace(0, numel - 1, NS).astype(np.int64)) if numel >= NS else np.arange(numel)


def _grad_record(module):
    norms, samples = [], []
    for _, p in module.named_parameters():
        g = p.grad.detach().double().reshape(-1).cpu()
        norms.append(float(g.norm()))
        s = g[torch.from_numpy(_sample_idx(g.numel()))].numpy()
        samples.append(np.pad(s, (0, NS - s.size), constant_values=np.nan))
    return np.array(norms), np.stack(samples)


def test_update_matches_the_reference_on_cpu(golden_dir):
    z = np.load(os.path.join(golden_dir, "td3_update_mlp.npz"))
    hyper = dict(zip([str(k) for k in z["hyper_keys"]], z["hyper_vals"]))
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=7, lr=hyper["lr"], policy_noise=hyper["policy_noise"],
                              noise_clip=hyper["noise_clip"], discount=hyper["discount"], policy_freq=int(hyper["policy_freq"]),
                              grad_clipping_value=hyper["grad_clipping_value"], max_action=hyper["max_action"])
    args.agent.target_smoothing_tau, args.agent.reward_scale = hyper["target_smoothing_tau"], hyper["reward_scale"]
    agent = Agent(args, device="cpu")
    assert [n for n, _ in agent.actor.named_parameters()] == [str(s) for s in z["actor_param_names"]]
    assert [n for n, _ in agent.critic.named_parameters()] == [str(s) for s in z["critic_param_names"]]
    apply_seeded_(agent.actor, int(z["seed"]))
    apply_seeded_(agent.critic, int(z["seed"]))
    with torch.no_grad():
        for tgt, src in ((agent.actor_target, agent.actor), (agent.critic_target, agent.critic)):
            for tp, sp in zip(tgt.parameters(), src.parameters()):
                tp.copy_(0.97 * sp)
    agent.change_morphology(_graph("3d_walker_7_full"))
    agent.models2train()
    grabbed = {}
    real = td3.clip_and_step

    def spy(opt, max_norm):
        which = "critic" if opt is agent.critic_optimizer else "actor"
        grabbed[which] = _grad_record(getattr(agent, which))
        return real(opt, max_norm)

    td3.clip_and_step = spy
    try:
        for it in range(2):
            tag = "it%d/" % it
            batch = {k: torch.from_numpy(z[tag + k]) for k in ("obs", "action", "next_obs", "reward", "done")}
            before = {nm: [p.detach().double().clone() for p in getattr(agent, nm).parameters()] for nm in ("actor", "critic")}
            grabbed.clear()
            loss = agent.update(batch, it, noise=torch.from_numpy(z[tag + "noise"]))
            # losses: the relative tolerance of tests/test_td3_update_init.py check()
            ref_cl = float(z[tag + "critic_loss"])
            assert abs(float(loss["loss/critic_loss"]) - ref_cl) < 1e-4 * abs(ref_cl), it
            ref_al = float(z[tag + "actor_loss"])
            assert np.isnan(ref_al) == ("loss/actor_loss" not in loss)
            if not np.isnan(ref_al):
                assert abs(float(loss["loss/actor_loss"]) - ref_al) < 1e-4 * abs(ref_al) + 2e-6
            assert abs(loss["misc/train_reward_mean"] - float(z[tag + "train_reward_mean"])) < 1e-6
            for nm in ("critic", "actor"):
                k = tag + nm + "_grad_norms"
                if k not in z.files:
                    assert nm not in grabbed, "policy_freq: actor stepped at the wrong iteration"
                else:
                    # raw gradients where the reference clips, per tensor: 1e-3 of the tensor's own float64 norm plus ten times what
                    # the reference's own float32 run leaves unresolved (test_td3_update_init.py check())
                    n32, n64 = z[k], z[k + "_f64"]
                    s32, s64 = z[tag + nm + "_grad_samples"], z[tag + nm + "_grad_samples_f64"]
                    got_n, got_s = grabbed[nm]
                    tol_n = 1e-3 * n64 + 10.0 * np.abs(n32 - n64)
                    tol_s = 1e-3 * n64 + 10.0 * np.nanmax(np.abs(s32 - s64), axis=1)
                    names = z[nm + "_param_names"]
                    assert (np.abs(got_n - n64) <= tol_n).all(), (it, nm, [str(names[i]) for i in np.nonzero(np.abs(got_n - n64) > tol_n)[0]])
                    assert (np.nanmax(np.abs(got_s - s64), axis=1) <= tol_s).all(), (it, nm)
                # the steps: clip + Adam
                st = np.array([float((p.detach().double() - q).norm()) for p, q in zip(getattr(agent, nm).parameters(), before[nm])])
                st64 = z[tag + nm + "_step_norms_f64"]
                ulp_floor = np.sqrt(z[nm + "_numel"]) * np.array([float(q.abs().max()) for q in before[nm]]) * 1.2e-7
                assert (np.abs(st - st64) <= 2e-3 * st64 + ulp_floor).all(), (it, nm)
                if k not in z.files:
                    assert st.max() == 0.0
            # every parameter of the four networks after the update (per-tensor sums, the layout of td3_update.npz): the updated
            # online networks and the Polyak-averaged targets
            for nm in ("actor", "critic", "actor_target", "critic_target"):
                got = np.array([float(p.detach().double().sum()) for p in getattr(agent, nm).parameters()])
                ref = z[tag + nm + "_param_sums"]
                numel = np.array([p.numel() for p in getattr(agent, nm).parameters()])
                assert (np.abs(got - ref) <= 2e-3 * hyper["lr"] * numel + 1e-6 * np.abs(ref) + 1e-7).all(), (it, nm)
    finally:
        td3.clip_and_step = real
