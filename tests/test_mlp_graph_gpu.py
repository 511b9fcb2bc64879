"""The graphed TD3 update of the MLP agent on the MI355X: the batch prologue kernel (csrc/mlp_batch.hip, mlp_hip.batch_stats) and
td3.GraphedMlpUpdates / DeviceTrainer(graph_updates=True, actor_type mlp).

1  the kernel against its NumPy restatement (tests/mlp_batch_restate.py: the same bits) and against float64 within the worst-case
   summation bounds of tests/test_mlp_graph_plan.py; the scaled reward equal to torch's product; in place == out of place; two calls
   give the same bits; the argument errors are raised
2  graphed against eager, bit for bit: 2 eager + 6 replayed updates against Agent.update on a deep copy fed the same batches and noise
3  live values: an in-place write into a target weight is seen by the next replay, a changed learning rate makes the graphs stale
   -- and a library error raised under capture ends the capture, the update runs eagerly, the host-side counts are taken back
4  moved storage and a regrown workspace make the graphs stale; two eager updates, then replays again, all bit-identical
5  update_from against update fed the rows and the noise tests/test_replay_sample.py's restatement predicts
6  a graphed and an eager DeviceTrainer draw the same batches in the same order and end with the same parameters

Measured on the MI355X (the printed lines of a run): the kernel gives the restatement's bits at every B and seed; worst error / bar
against float64, mean / variance: B = 2 0.24 / 0.088, 31 0.065 / 0.021, 33 0.047 / 0.019, 66 0.035 / 0.017, 256 5.0e-3 / 3.1e-3, 1024
1.5e-3 / 7.4e-4, 4096 4.8e-4 / 2.2e-4.  Two deliberately wrong builds fail these tests and tests/test_mlp_graph_plan.py (82 in all):
`replayed()` left out fails 6 (test 2's three cases, both tests of 3, and 4: the host-side step counts stay behind), lr left out of
the stamp fails 3 (test 3 at its `stale` assertion, before any replay, and the two lr cases of the stub stamp test).

Replaying a graph whose baked address has been freed is a GPU memory fault, not an exception: tests 3 and 4 assert `stale(flag)`
BEFORE they call `update`, so a wrong stamp fails the assertion and never reaches a replay."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from mlp_batch_restate import bars, batch_stats_f64, batch_stats_restated
from mlp_restate import apply_seeded_
from tests.test_replay_sample import draw_noise, draw_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TRAV = ["pre", "inlcrs", "postlcrs"]
MORPHS = {3: "3d_hopper_3_shin", 7: "3d_walker_7_full"}
BS = [1, 2, 31, 33, 66, 256, 1024, 4096]
SCALE = 0.3
NETS = ("actor", "critic", "actor_target", "critic_target")


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("B", BS)
def test_kernel_against_restatement_and_float64(B):
    from sgrl_amd import mlp_hip
    worst = [0.0, 0.0]
    for seed in range(20):
        r = np.random.RandomState(1000 * B + seed).normal(1.0, 0.5, B).astype(np.float32)
        rt = torch.from_numpy(r).to(DEV).reshape(B, 1)
        out, stats = torch.full((B, 1), 7.0, device=DEV), torch.full((2,), 7.0, device=DEV)
        assert mlp_hip.batch_stats(rt, SCALE, out, stats) is out
        assert torch.equal(out, rt * SCALE)                               # the statement it replaces, bit for bit
        want_out, want_mean, want_var = batch_stats_restated(r, SCALE)
        got = stats.cpu().numpy()
        mean64, var64 = batch_stats_f64(r, SCALE)
        mean_bar, var_bar = bars(r, SCALE)
        print("B %d seed %d: mean %.9g (f64 %.9g, bar %.3g)  var %.9g (f64 %.9g, bar %.3g)" % (B, seed, got[0], mean64, mean_bar, got[1], var64, var_bar))
        assert np.array_equal(_bits(out.cpu().numpy().reshape(-1)), _bits(want_out))
        assert np.array_equal(_bits(got), _bits([want_mean, want_var])), (B, seed, got, want_mean, want_var)
        assert abs(float(got[0]) - mean64) <= mean_bar
        worst[0] = max(worst[0], abs(float(got[0]) - mean64) / mean_bar)
        if B == 1:
            assert np.isnan(got[1]) and bool(torch.isnan(torch.var(rt * SCALE)))
        else:
            assert abs(float(got[1]) - var64) <= var_bar
            worst[1] = max(worst[1], abs(float(got[1]) - var64) / var_bar)
        # in place, and the same call again: the same bits
        inplace, stats2 = rt.clone(), torch.zeros(2, device=DEV)
        mlp_hip.batch_stats(inplace, SCALE, inplace, stats2)
        stats3 = torch.zeros(2, device=DEV)
        mlp_hip.batch_stats(rt, SCALE, out, stats3)
        assert torch.equal(inplace, out)
        for s in (stats2, stats3):
            assert np.array_equal(_bits(s.cpu().numpy()), _bits(got))
    print("B %d: worst error / bar: mean %.3g, variance %.3g" % (B, worst[0], worst[1]))


def test_kernel_argument_errors_launch_nothing():
    from sgrl_amd import _lib, mlp_hip
    L = _lib.lib()
    mlp_hip._bind(L)
    r, out, stats = torch.full((8,), 7.0, device=DEV), torch.full((8,), 7.0, device=DEV), torch.full((2,), 7.0, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    null, cf = ctypes.c_void_p(None), ctypes.c_float
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args, what in (((null, 8, cf(0.3), vp(out), vp(stats)), b"null"), ((vp(r), 8, cf(0.3), null, vp(stats)), b"null"),
                       ((vp(r), 8, cf(0.3), vp(out), null), b"null"), ((vp(r), 0, cf(0.3), vp(out), vp(stats)), b"n outside"),
                       ((vp(r), (1 << 24) + 1, cf(0.3), vp(out), vp(stats)), b"n outside"),
                       ((vp(r), 8, cf(float("nan")), vp(out), vp(stats)), b"not finite"), ((vp(r), 8, cf(float("-inf")), vp(out), vp(stats)), b"not finite")):
        assert L.sgrl_mlp_batch_stats(*args, st) == -1 and what in L.sgrl_mlp_last_error(), (what, L.sgrl_mlp_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((stats == 7).all())
    for bad in (dict(out=torch.zeros(7, device=DEV)), dict(stats=torch.zeros(3, device=DEV)), dict(out=out.cpu()), dict(stats=stats.double()),
                dict(out=torch.zeros(16, device=DEV)[::2])):
        kw = dict(out=out, stats=stats)
        kw.update(bad)
        with pytest.raises(_lib.SgrlError, match="batch_stats"):
            mlp_hip.batch_stats(r, 0.3, kw["out"], kw["stats"])
    mlp_hip.batch_stats(r, 0.5, out, stats)                               # the well-formed call goes through
    assert torch.equal(out, r * 0.5) and float(stats[0]) == 3.5 and float(stats[1]) == 0.0


# ---- agents ------------------------------------------------------------------------------------------------------------------
def _graph(L):
    from sgrl_amd import graph as G, mjcf
    return G.getGraphDict(mjcf.load_asset(MORPHS[L]).parents, TRAV, [], device=torch.device(DEV))


def _agent(L, hidden, capturable=False, seed=3):
    from sgrl_amd.td3 import Agent, default_train_args
    args = default_train_args(actor_type="mlp", critic_type="mlp", mlp_num_limbs=L, policy_freq=2)
    args.agent.policy_network = {"hidden_dims": list(hidden)}
    args.agent.q_network = {"hidden_dims": list(hidden)}
    args.agent.reward_scale = SCALE
    torch.manual_seed(seed)
    a = Agent(args, device=torch.device(DEV), mlp_hip_grads=True, mlp_hip_optim=True)
    for mod, sd in ((a.actor, 3), (a.critic, 4), (a.actor_target, 5), (a.critic_target, 6)):
        apply_seeded_(mod, sd)
    if capturable:
        for opt in (a.actor_optimizer, a.critic_optimizer):
            opt.param_groups[0]["capturable"] = True
    a.change_morphology(_graph(L))
    a.models2train()
    return a


def _batch(g, n, L):
    batch = {"obs": torch.randn((n, 41 * L), generator=g), "next_obs": torch.randn((n, 41 * L), generator=g),
             "action": torch.rand((n, 3 * L), generator=g) * 2 - 1, "reward": torch.randn((n, 1), generator=g) * 0.5 + 1.0,
             "done": (torch.rand((n, 1), generator=g) < 0.2).float()}
    return {k: v.to(DEV) for k, v in batch.items()}, (torch.randn((n, 3 * L), generator=g) * 0.2).to(DEV)


class Pair(object):
    """A GraphedMlpUpdates and an eager deep copy of its agent, fed the same batches and the same noise."""

    def __init__(self, L, hidden, B, capturable=False):
        from sgrl_amd.td3 import GraphedMlpUpdates
        self.L, self.B, self.graph = L, B, _graph(L)
        agent = _agent(L, hidden, capturable)
        agent.use_mlp_hip_optim = False                        # the construction turns it on
        self.gu = GraphedMlpUpdates(agent, B)
        assert agent.use_mlp_hip_grads and agent.use_mlp_hip_optim
        self.ref = copy.deepcopy(agent)
        self.ref.change_morphology(self.graph)
        self.gen = torch.Generator().manual_seed(77)
        self.it = 0
        self.noise = None
        load = self.gu._load

        def load_then_noise(sl, data_batch):                   # the slot's noise by hand, after _load has drawn its own
            load(sl, data_batch)
            sl["noise"].copy_(self.noise)
        self.gu._load = load_then_noise

    def step(self, replay=None):
        """One update on both sides, compared; replay: whether the graphed side must (True) / must not (False) have replayed."""
        batch, self.noise = _batch(self.gen, self.B, self.L)
        before = self.gu.replays
        got = self.gu.update(0, self.graph, self.L, batch, self.it)
        want = self.ref.update(batch, self.it, noise=self.noise, lazy_stats=True)
        if replay is not None:
            assert self.gu.replays - before == (1 if replay else 0), (self.it, replay)
        assert set(got) == set(want) and ("loss/actor_loss" in got) == (self.it % 2 == 0)
        for k in ("loss/critic_loss", "loss/actor_loss"):
            if k in want:
                assert got[k].dim() == 0 and torch.equal(got[k], want[k]), (self.it, k, float(got[k]), float(want[k]))
        r = batch["reward"].cpu().numpy().reshape(-1)
        mean64, var64 = batch_stats_f64(r, SCALE)
        mean_bar, var_bar = bars(r, SCALE)
        assert abs(float(got["misc/train_reward_mean"]) - mean64) <= mean_bar and abs(float(got["misc/train_reward_var"]) - var64) <= var_bar
        assert abs(float(want["misc/train_reward_mean"]) - mean64) <= mean_bar
        self.it += 1

    def both(self, fn):
        for a in (self.gu.agent, self.ref):
            fn(a)

    def check_state(self, critic_steps, actor_steps):
        a, b = self.gu.agent, self.ref
        for nm in NETS:
            for (name, p), q in zip(getattr(a, nm).named_parameters(), getattr(b, nm).parameters()):
                assert torch.equal(p, q), (nm, name, float((p - q).abs().max()))
        for opt_a, opt_b, net, n in ((a.critic_optimizer, b.critic_optimizer, "critic", critic_steps), (a.actor_optimizer, b.actor_optimizer, "actor", actor_steps)):
            pa, pb = list(getattr(a, net).parameters()), list(getattr(b, net).parameters())
            for p, q in zip(pa, pb):
                sa, sb = opt_a.state[p], opt_b.state[q]
                assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), net
                assert sa["step"].device == sb["step"].device and float(sa["step"]) == float(sb["step"]) == float(n), (net, float(sa["step"]), float(sb["step"]), n)
            ma, mb = opt_a.__dict__.get("_sgrl_step_class"), opt_b.__dict__.get("_sgrl_step_class")
            assert (ma is None) == (mb is None)
            if ma is not None:
                assert [ma[id(p)] for p in pa] == [mb[id(q)] for q in pb] == [n] * len(pa), net
        for side, n in (("_critic", critic_steps), ("_actor", actor_steps)):
            sa, sb = getattr(a._mlp_optim, side), getattr(b._mlp_optim, side)
            assert (sa.counter is None) == (sb.counter is None) and sa.host_step == sb.host_step
            if sa.counter is not None:                          # plain groups: the device counter each side owns, and its host mirror
                assert float(sa.counter) == float(sb.counter) == float(n) == sa.host_step, (side, float(sa.counter), float(sb.counter), n, sa.host_step)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,hidden,B,capturable", [(3, (40, 72), 33, False), (3, (40, 72), 33, True), (7, (256, 256), 66, False)],
                         ids=["L3-40x72-B33-plain", "L3-40x72-B33-capturable", "L7-256x256-B66-plain"])
def test_graphed_against_eager_bit_for_bit(L, hidden, B, capturable):
    pr = Pair(L, hidden, B, capturable)
    gu = pr.gu
    assert gu.stale(0) and gu.stale(1) and 0 not in gu.warmed
    pr.step(replay=False)
    pr.step(replay=False)
    assert 0 in gu.warmed and "anything" in gu.warmed and gu.stale(0) and gu.stale(1)        # warmed, nothing captured yet
    versions = [p._version for nm in NETS for p in getattr(gu.agent, nm).parameters()]
    grad_versions = [p.grad._version for nm in ("actor", "critic") for p in getattr(gu.agent, nm).parameters()]
    for k in range(6):
        pr.step(replay=True)
        assert not gu.stale(k % 2)
    assert gu.replays == 6 and set(gu.slots[None]["graphs"]) == {0, 1} and list(gu.slots) == [None]
    assert gu.launches(1) == 9 and gu.launches(0) == 15
    pr.check_state(critic_steps=8, actor_steps=4)
    # a replay announces its writes: parameters, targets and gradients
    assert all(p._version > v for p, v in zip([p for nm in NETS for p in getattr(gu.agent, nm).parameters()], versions))
    assert all(p.grad._version > v for p, v in zip([p for nm in ("actor", "critic") for p in getattr(gu.agent, nm).parameters()], grad_versions))
    # fewer rows than B: the eager update
    batch, noise = _batch(pr.gen, B - 5, L)
    out = gu.update(0, pr.graph, L, batch, 9)
    assert np.isfinite(float(out["loss/critic_loss"])) and gu.replays == 6


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def test_live_values_and_by_value_scalars():
    pr = Pair(3, (40, 72), 33)
    gu = pr.gu
    for k in range(4):
        pr.step(replay=k >= 2)
    assert not gu.stale(0) and not gu.stale(1)

    def scale_target_weight(a):
        with torch.no_grad():
            w = a.critic_target.critic1.networks[0].weight
            w.copy_(w * 1.5)
    pr.both(scale_target_weight)
    assert not gu.stale(0) and not gu.stale(1)                    # an in-place write moves nothing
    pr.step(replay=True)                                          # ... and the replay reads it: the losses and everything after agree
    pr.step(replay=True)
    pr.check_state(critic_steps=6, actor_steps=3)

    def new_lr(a):
        a.critic_optimizer.param_groups[0]["lr"] = 3e-4
    pr.both(new_lr)
    assert gu.stale(0) and gu.stale(1)                            # lr is baked by value
    pr.step(replay=False)
    pr.step(replay=False)
    pr.step(replay=True)
    pr.step(replay=True)
    pr.check_state(critic_steps=10, actor_steps=5)


def test_a_library_error_under_capture_ends_it_and_the_update_runs_eagerly():
    """The routine raises an SgrlError under the first capture, AFTER it has recorded the whole update (the host half of every step has
    then run, none of their kernels): the capture ends cleanly, the host-side step counts are taken back, that update runs eagerly, and
    the next one of its kind captures and replays -- all bit-identical to the eager copy, counters included."""
    from sgrl_amd import _lib
    pr = Pair(3, (40, 72), 33)
    gu = pr.gu
    pr.step(replay=False)
    pr.step(replay=False)
    run, raised = gu._run, []

    def run_then_refuse(sl, hs, policy_it):
        run(sl, hs, policy_it)
        if torch.cuda.is_current_stream_capturing() and not raised:
            raised.append(policy_it)
            raise _lib.SgrlError("sgrl_mlp_critic_step_grads failed (-1): the training workspace must grow, which a capture cannot record (simulated)")
    gu._run = run_then_refuse
    pr.step(replay=False)                                         # it = 2: the capture is refused, the update runs eagerly
    assert raised == [True] and 0 not in gu.slots[None]["graphs"] and not torch.cuda.is_current_stream_capturing()
    pr.check_state(critic_steps=3, actor_steps=2)
    pr.step(replay=True)
    pr.step(replay=True)                                          # it = 4: this time the capture stands
    pr.step(replay=True)
    assert set(gu.slots[None]["graphs"]) == {0, 1}
    pr.check_state(critic_steps=6, actor_steps=3)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def test_moved_storage_and_regrowth_make_the_graphs_stale():
    pr = Pair(3, (40, 72), 33)
    gu = pr.gu
    for k in range(4):
        pr.step(replay=k >= 2)
    assert not gu.stale(0) and not gu.stale(1)

    def move(a):
        p = a.critic.critic1.networks[0].weight
        p.data = p.data.clone()
    pr.both(move)
    assert gu.stale(0) and gu.stale(1)
    pr.step(replay=False)
    pr.step(replay=False)
    pr.step(replay=True)
    pr.step(replay=True)
    pr.check_state(critic_steps=8, actor_steps=4)
    # one eager update at 2 B rows: the training workspace grows, the handles' generation moves
    batch, noise = _batch(pr.gen, 2 * pr.B, pr.L)
    gens = [h.generation() for h in (gu.agent._mlp_grads.actor, gu.agent._mlp_grads.critic)]
    outs = [a.update(batch, pr.it, noise=noise, lazy_stats=True) for a in (gu.agent, pr.ref)]
    assert torch.equal(outs[0]["loss/critic_loss"], outs[1]["loss/critic_loss"])
    pr.it += 1
    assert [h.generation() for h in (gu.agent._mlp_grads.actor, gu.agent._mlp_grads.critic)] != gens
    assert gu.stale(0) and gu.stale(1)
    pr.step(replay=False)
    pr.step(replay=False)
    pr.step(replay=True)
    pr.step(replay=True)
    pr.check_state(critic_steps=13, actor_steps=7)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def test_update_from_equals_update_fed_the_predicted_batch():
    """walker_7, B = 32, a ring of 500 rows, it = 0 .. 3 (two eager updates, then both graphs): update_from against update on a deep
    copy of the agent, fed the rows and the noise the restatement predicts for the same (seed, draw)."""
    from oracle.formula import synth_obs
    from sgrl_amd.replay import DeviceReplayBuffer
    from sgrl_amd.td3 import GraphedMlpUpdates
    L, B, fill, seed = 7, 32, 500, 77
    gd = _graph(L)
    a_new = _agent(L, (256, 256))
    a_old = copy.deepcopy(a_new)
    a_old.change_morphology(gd)
    g_new, g_old = GraphedMlpUpdates(a_new, B), GraphedMlpUpdates(a_old, B)
    rng = np.random.RandomState(1)
    buf = DeviceReplayBuffer(41 * L, 3 * L, fill, device=torch.device(DEV))
    buf.add_transitions(torch.from_numpy(synth_obs(L, fill, 1).astype(np.float32)), torch.from_numpy(rng.uniform(-1, 1, (fill, 3 * L)).astype(np.float32)),
                        torch.from_numpy(synth_obs(L, fill, 2).astype(np.float32)), torch.from_numpy(rng.normal(1, 0.5, fill).astype(np.float32)),
                        torch.from_numpy((rng.uniform(size=fill) < 0.1).astype(np.float32)))
    assert buf.max_sample_size == fill
    state = {}
    load = g_old._load

    def load_then_noise(sl, data_batch):
        load(sl, data_batch)
        sl["noise"].copy_(state["noise"])
    g_old._load = load_then_noise
    for it in range(4):
        draw = 10 + it
        idx = torch.from_numpy(draw_rows(fill, B, seed, draw)[0]).to(DEV)
        batch = dict(obs=buf.obs_buffer[idx], action=buf.action_buffer[idx], next_obs=buf.next_obs_buffer[idx],
                     reward=buf.reward_buffer[idx].reshape(-1, 1), done=buf.done_buffer[idx].reshape(-1, 1))
        state["noise"] = torch.from_numpy(draw_noise(B, 3 * L, seed, draw, a_old.args.policy_noise)).to(DEV)
        out_new = g_new.update_from(0, gd, L, buf, it, seed, draw)
        out_old = g_old.update(0, gd, L, batch, it)
        assert torch.equal(g_new.slots[None]["noise"], g_old.slots[None]["noise"]), it
        for name in batch:
            assert torch.equal(g_new.slots[None]["batch"][name], g_old.slots[None]["batch"][name]), (it, name)
        assert set(out_new) == set(out_old)
        for name in out_old:
            assert torch.equal(out_new[name], out_old[name]), (it, name)
    assert g_new.replays == g_old.replays == 2 and set(g_new.slots[None]["graphs"]) == {0, 1}
    for nm in NETS:
        for p, q in zip(getattr(a_new, nm).parameters(), getattr(a_old, nm).parameters()):
            assert torch.equal(p, q), nm
    # a buffer shorter than the batch: the eager update on the k rows there are
    short = DeviceReplayBuffer(41 * L, 3 * L, 64, device=torch.device(DEV))
    short.add_transitions(buf.obs_buffer[:20], buf.action_buffer[:20], buf.next_obs_buffer[:20], buf.reward_buffer[:20], buf.done_buffer[:20])
    out = g_new.update_from(0, gd, L, short, 1, seed, 9)
    assert np.isfinite(float(out["loss/critic_loss"])) and g_new.replays == 2


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def test_graphed_trainer_equals_the_eager_trainer():
    from sgrl_amd.td3 import GraphedMlpUpdates, default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    names = ["3d_hopper_3_shin", "3d_walker_3_left_knee_right_knee"]

    def trainer(graphed):
        args = default_train_args(actor_type="mlp", critic_type="mlp", max_episode_steps=30, mlp_hip_grads=True)
        args.mlp_hip_optim = True
        tr = DeviceTrainer(names, [4, 4], args=args, seed=3, device=DEV, max_buffer_size=256, batch_size=16, device_sampler=True,
                           graph_updates=graphed)                  # graph_updates=True no longer raises
        tr.warmup(30)
        for _ in range(40):                                        # the collection of train_round
            if tr.collect_step():
                break
        return tr
    eager, graphed = trainer(False), trainer(True)
    assert isinstance(graphed.graphed, GraphedMlpUpdates) and eager.graphed is None
    for be, bg in zip(eager.buffers, graphed.buffers):             # the precondition: both collected the same transitions
        assert be.max_sample_size == bg.max_sample_size >= 16
        for name in ("obs_buffer", "action_buffer", "next_obs_buffer", "reward_buffer", "done_buffer"):
            assert torch.equal(getattr(be, name), getattr(bg, name)), name
    for nm in NETS:
        for p, q in zip(getattr(eager.agent, nm).parameters(), getattr(graphed.agent, nm).parameters()):
            assert torch.equal(p, q), nm
    n_e, n_g = eager.update_after_round(max_iters=6), graphed.update_after_round(max_iters=6)
    assert n_e == n_g >= 2, (n_e, n_g)
    assert eager.draw == graphed.draw == eager._updates == graphed._updates == 2 * n_e
    assert graphed.graphed.replays == 2 * n_e - 2                  # the shared slot: only the very first two updates are eager
    for nm in NETS:
        for p, q in zip(getattr(eager.agent, nm).parameters(), getattr(graphed.agent, nm).parameters()):
            assert torch.equal(p, q), nm
    for name in names:
        le, lg = eager.last_losses[name], graphed.last_losses[name]
        assert torch.equal(torch.as_tensor(le["loss/critic_loss"]).cpu(), torch.as_tensor(lg["loss/critic_loss"]).cpu()), name
