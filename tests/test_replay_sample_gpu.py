"""sgrl_replay_sample on the GPU (include/sgrl_replay.h, sgrl_amd/csrc/replay_sample.hip) against the NumPy restatement of
tests/test_replay_sample.py: the drawn rows bit for bit, the gather exactly, the noise to float32 rounding, the call recorded into
a hipGraph, the argument errors; then GraphedUpdates.update_from against update fed the predicted batch, and
DeviceTrainer(device_sampler=True).  Rings hold row * 1000 + column patterns, so a wrong row or column shows in the value."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from sgrl_amd import _lib
from tests.test_replay_sample import PAIRS, draw_noise, draw_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = (1, 0xDEADBEEFCAFEF00D)
DRAWS = (0, 1, 2 ** 32 + 5)
NAN = float("nan")
# (obs_dim, act_dim) per (fill, batch): widths that are and are not multiples of four, rows longer than a wavefront's 64 lanes and
# than its 256 floats of 16-byte accesses; the million-row ring is 54 MB at (5, 3)
DIMS = {(1, 1): (8, 4), (5, 8): (41, 3), (256, 256): (123, 9), (300, 256): (615, 45), (1024, 1024): (8, 4), (1000003, 256): (5, 3)}
_rings = {}


def _ring(fill, obs_dim, act_dim):
    """A buffer of exactly `fill` filled rows (shared between the tests, never written again)."""
    from sgrl_amd.replay import DeviceReplayBuffer
    key = (fill, obs_dim, act_dim)
    if key not in _rings:
        buf = DeviceReplayBuffer(obs_dim, act_dim, fill, device=DEV)
        step = 1000 if fill <= 2048 else 8             # exact in float32 either way
        row = torch.arange(fill, device=DEV, dtype=torch.float32)[:, None] * step
        buf.obs_buffer.copy_(row + torch.arange(obs_dim, device=DEV))
        buf.next_obs_buffer.copy_(row + torch.arange(obs_dim, device=DEV) + 0.5)
        buf.action_buffer.copy_(-(row + torch.arange(act_dim, device=DEV)) - 0.25)
        buf.reward_buffer.copy_(row[:, 0] + 0.125)
        buf.done_buffer.copy_((torch.arange(fill, device=DEV) % 2).float())
        buf.max_sample_size, buf.curr = fill, 0
        _rings[key] = buf
    return _rings[key]


def _outputs(batch, obs_dim, act_dim, pad=(3, 1, 5, 2), flat=False):
    f = lambda *s: torch.full(s, NAN, device=DEV)
    out = {"obs": f(batch, obs_dim + pad[0]), "action": f(batch, act_dim + pad[1]), "next_obs": f(batch, obs_dim + pad[2]),
           "reward": f(batch) if flat else f(batch, 1), "done": f(batch, 1)}
    return out, f(batch, act_dim + pad[3]), torch.full((batch,), -7, dtype=torch.int64, device=DEV)


def _check_gather(buf, out, idx, k):
    o, a = buf.obs_dim, buf.action_dim
    assert torch.equal(out["obs"][:k, :o], buf.obs_buffer[idx])
    assert torch.equal(out["next_obs"][:k, :o], buf.next_obs_buffer[idx])
    assert torch.equal(out["action"][:k, :a], buf.action_buffer[idx])
    assert torch.equal(out["reward"].reshape(-1)[:k], buf.reward_buffer[idx])
    assert torch.equal(out["done"].reshape(-1)[:k], buf.done_buffer[idx])
    # columns between the dimension and the stride, and rows from k on, keep their prefill
    for name, d in (("obs", o), ("next_obs", o), ("action", a)):
        assert bool(torch.isnan(out[name][:, d:]).all()) and bool(torch.isnan(out[name][k:]).all()), name
    assert bool(torch.isnan(out["reward"].reshape(-1)[k:]).all()) and bool(torch.isnan(out["done"][k:]).all())


@pytest.mark.parametrize("fill, batch", PAIRS)
def test_rows_equal_the_restatement_and_the_gather_is_exact(fill, batch):
    obs_dim, act_dim = DIMS[(fill, batch)]
    buf = _ring(fill, obs_dim, act_dim)
    k = min(fill, batch)
    for n, (seed, draw) in enumerate((s, d) for s in SEEDS for d in DRAWS):
        out, noise, idx_out = _outputs(batch, obs_dim, act_dim, flat=bool(n & 1))
        assert buf.sample_into(out, batch, seed, draw, noise=noise, noise_std=0.2, idx_out=idx_out) == k
        want, _ = draw_rows(fill, batch, seed, draw)
        got = idx_out.cpu().numpy()
        assert np.array_equal(got[:k], want), (seed, draw)
        assert (got[k:] == -7).all()
        _check_gather(buf, out, torch.from_numpy(want).to(DEV), k)
        ref = draw_noise(k, act_dim, seed, draw, 0.2)
        z = noise.cpu().numpy()
        err = float(np.abs(z[:k, :act_dim] - ref).max())
        assert err <= 1e-6 * 0.2, (seed, draw, err)
        big = np.abs(ref) > 1e-6
        assert np.array_equal(np.sign(z[:k, :act_dim])[big], np.sign(ref)[big])
        assert np.isnan(z[:, act_dim:]).all() and np.isnan(z[k:]).all()


def test_forced_fallback_is_the_restatements():
    buf = _ring(64, 41, 3)
    for seed in SEEDS:
        out, _, idx_out = _outputs(64, 41, 3)
        assert buf.sample_into(out, 64, seed, 2, idx_out=idx_out, max_candidates=64) == 64
        want, looked = draw_rows(64, 64, seed, 2, max_candidates=64)
        assert looked == 64 and sorted(want.tolist()) == list(range(64))
        assert np.array_equal(idx_out.cpu().numpy(), want)
        _check_gather(buf, out, torch.from_numpy(want).to(DEV), 64)
    # a cap that ends in the middle of a round of candidates
    out, _, idx_out = _outputs(256, 123, 9)
    buf = _ring(256, 123, 9)
    buf.sample_into(out, 256, 5, 0, idx_out=idx_out, max_candidates=300)
    assert np.array_equal(idx_out.cpu().numpy(), draw_rows(256, 256, 5, 0, max_candidates=300)[0])


@pytest.mark.parametrize("dims", [(41, 3), (123, 9), (8, 4), (615, 45)])
def test_gather_only_with_given_rows(dims):
    fill = 300
    buf = _ring(fill, *dims)
    idx = torch.tensor([0, fill - 1, 17, 17, 299, 1, 0, 150, 2], dtype=torch.int64, device=DEV)
    k = idx.numel()
    out, noise, idx_out = _outputs(k + 2, *dims)
    assert buf.sample_into(out, k, 1, 0, idx_out=idx_out, idx_in=idx) == k
    assert torch.equal(idx_out[:k], idx) and bool((idx_out[k:] == -7).all())
    _check_gather(buf, out, idx, k)
    assert bool(torch.isnan(noise).all())              # noise = NULL: a prefilled tensor is left alone
    # unpadded, 16-byte aligned outputs (the vector path where the width allows it) give the same rows
    out2, _, _ = _outputs(k, *dims, pad=(0, 0, 0, 0))
    buf.sample_into(out2, k, 1, 0, idx_in=idx)
    _check_gather(buf, out2, idx, k)
    # ... and so do outputs whose rows start off a 16-byte boundary (the element path)
    base = torch.full((k * dims[0] + 1,), NAN, device=DEV)
    out2["obs"] = base[1:].view(k, dims[0])
    buf.sample_into(out2, k, 1, 0, idx_in=idx)
    _check_gather(buf, out2, idx, k)
    assert bool(torch.isnan(base[0]))


def test_zero_prefilled_noise_padding_stays_zero_and_noise_scales():
    buf = _ring(300, 41, 3)
    out, _, _ = _outputs(16, 41, 3)
    noise = torch.zeros(16, 8, device=DEV)
    buf.sample_into(out, 16, 9, 3, noise=noise, noise_std=1.0)
    assert bool((noise[:, 3:] == 0).all()) and bool((noise[:, :3] != 0).all())
    ref = draw_noise(16, 3, 9, 3, 1.0)
    assert float(np.abs(noise[:, :3].cpu().numpy() - ref).max()) <= 1e-6
    half = torch.zeros(16, 8, device=DEV)
    buf.sample_into(out, 16, 9, 3, noise=half, noise_std=0.5)
    assert torch.equal(half, noise * 0.5)


def test_captured_call_replays_the_eager_result():
    buf = _ring(300, 123, 9)
    eager, enoise, eidx = _outputs(64, 123, 9)
    buf.sample_into(eager, 64, 4, 6, noise=enoise, noise_std=0.2, idx_out=eidx)
    out, noise, idx_out = _outputs(64, 123, 9)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.sample_into(out, 64, 4, 6, noise=noise, noise_std=0.2, idx_out=idx_out)
    assert bool((idx_out == -7).all())                 # capturing records the work without running it
    for _ in range(2):                                 # the draw is an argument: both replays repeat it
        for t in list(out.values()) + [noise]:
            t.fill_(NAN)
        idx_out.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx_out, eidx)
        for name in out:
            assert torch.equal(torch.nan_to_num(out[name], nan=-1.0), torch.nan_to_num(eager[name], nan=-1.0)), name
        assert torch.equal(torch.nan_to_num(noise, nan=-1.0), torch.nan_to_num(enoise, nan=-1.0))


def test_argument_errors_launch_nothing():
    from sgrl_amd.replay import _Ring, _bind
    L = _lib.lib()
    _bind(L)
    buf = _ring(300, 41, 3)
    out, noise, idx_out = _outputs(8, 41, 3, pad=(0, 0, 0, 0))
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    ring = _Ring(buf.obs_buffer.data_ptr(), buf.action_buffer.data_ptr(), buf.next_obs_buffer.data_ptr(), buf.reward_buffer.data_ptr(),
                 buf.done_buffer.data_ptr(), 41, 3)
    no_obs = _Ring(None, buf.action_buffer.data_ptr(), buf.next_obs_buffer.data_ptr(), buf.reward_buffer.data_ptr(),
                   buf.done_buffer.data_ptr(), 41, 3)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ring=ring, fill=300, batch=8, cand=0, obs=vp(out["obs"]), ld=(41, 3, 41), reward=vp(out["reward"]), nz=None, ldn=0):
        return L.sgrl_replay_sample(ctypes.byref(ring) if ring is not None else None, fill, batch, 1, 0, cand, None, obs, ld[0],
                                    vp(out["action"]), ld[1], vp(out["next_obs"]), ld[2], reward, vp(out["done"]), vp(idx_out), nz, ldn,
                                    0.2, stream)
    cases = [dict(ring=None), dict(ring=no_obs), dict(obs=None), dict(reward=None), dict(fill=0), dict(fill=-3), dict(batch=0),
             dict(batch=1025), dict(ld=(40, 3, 41)), dict(ld=(41, 2, 41)), dict(ld=(41, 3, 40)), dict(nz=vp(noise), ldn=2), dict(cand=-1)]
    for kw in cases:
        assert call(**kw) == -1, kw                    # SGRL_ERR_ARG
        assert b"sgrl_replay_sample" in L.sgrl_replay_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in list(out.values()) + [noise]) and bool((idx_out == -7).all())
    assert call() == 0                                 # the same call with nothing wrong
    torch.cuda.synchronize()
    assert np.array_equal(idx_out.cpu().numpy(), draw_rows(300, 8, 1, 0)[0])
    assert L.sgrl_replay_sample_launches() in (1, 2)
    # the Python surface refuses what the library could not address
    with pytest.raises(_lib.SgrlError, match="out\\['obs'\\]"):
        buf.sample_into(dict(out, obs=out["obs"].cpu()), 8, 1, 0)
    with pytest.raises(_lib.SgrlError, match="noise"):
        buf.sample_into(out, 8, 1, 0, noise=torch.zeros(8, 2, device=DEV))


def test_update_from_equals_update_fed_the_predicted_batch():
    """walker_7, B = 32, a ring of 500 rows, it = 0 and 1 (both graphs): GraphedUpdates.update_from against GraphedUpdates.update on
    a deep copy of the agent, fed the rows and the noise the restatement predicts for the same (seed, draw)."""
    from oracle.formula import synth_obs
    from sgrl_amd import graph as G, mjcf
    from sgrl_amd.replay import DeviceReplayBuffer
    from sgrl_amd.rollout import TRAV
    from sgrl_amd.td3 import Agent, GraphedUpdates, default_train_args
    dev = torch.device(DEV)
    B, fill, seed = 32, 500, 77
    m = mjcf.load_asset("3d_walker_7_full")
    L = m.num_limbs
    assert L == 7
    gd = G.getGraphDict(m.parents, TRAV, [], device=dev)
    torch.manual_seed(4)
    a_new = Agent(default_train_args(), device=dev)
    a_old = copy.deepcopy(a_new)
    for a in (a_new, a_old):
        a.models2train()
    g_new, g_old = GraphedUpdates(a_new, B), GraphedUpdates(a_old, B)
    rng = np.random.RandomState(1)
    buf = DeviceReplayBuffer(41 * L, 3 * L, fill, device=dev)
    buf.add_transitions(torch.from_numpy(synth_obs(L, fill, 1).astype(np.float32)), torch.from_numpy(rng.uniform(-1, 1, (fill, 3 * L)).astype(np.float32)),
                        torch.from_numpy(synth_obs(L, fill, 2).astype(np.float32)), torch.from_numpy(rng.normal(1, 0.5, fill).astype(np.float32)),
                        torch.from_numpy((rng.uniform(size=fill) < 0.1).astype(np.float32)))
    assert buf.max_sample_size == fill

    def predicted(draw, std):
        idx = torch.from_numpy(draw_rows(fill, B, seed, draw)[0]).to(dev)
        batch = dict(obs=buf.obs_buffer[idx], action=buf.action_buffer[idx], next_obs=buf.next_obs_buffer[idx],
                     reward=buf.reward_buffer[idx].reshape(-1, 1), done=buf.done_buffer[idx].reshape(-1, 1))
        return batch, torch.from_numpy(draw_noise(B, 3 * L, seed, draw, std)).to(dev)

    state = {}
    load = g_old._load

    def load_then_noise(sl, data_batch):               # the slot's noise by hand, after _load has drawn its own
        load(sl, data_batch)
        sl["noise"].copy_(state["noise"])
    g_old._load = load_then_noise
    # the eager run every capture needs is a real update: draw 0 on both sides
    batch, state["noise"] = predicted(0, a_old.args.policy_noise)
    w_new = g_new.warm_from(0, gd, L, buf, seed, 0, iters=1, first_it=0)
    w_old = g_old.warm(0, gd, L, batch, iters=1, first_it=0)
    assert torch.equal(w_new[0]["loss/critic_loss"], w_old[0]["loss/critic_loss"])
    for it in range(2):
        draw = 1 + it
        batch, state["noise"] = predicted(draw, a_old.args.policy_noise)
        out_new = g_new.update_from(0, gd, L, buf, it, seed, draw)
        out_old = g_old.update(0, gd, L, batch, it)
        assert torch.equal(g_new.slots[0]["noise"], g_old.slots[0]["noise"]), it
        for name in batch:
            assert torch.equal(g_new.slots[0]["batch"][name], g_old.slots[0]["batch"][name]), (it, name)
        assert set(out_new) == set(out_old)
        for name in out_old:
            assert torch.equal(torch.as_tensor(out_new[name]), torch.as_tensor(out_old[name])), (it, name)
    assert set(g_new.slots[0]["graphs"]) == {0, 1}
    for nm in ("actor", "critic", "actor_target", "critic_target"):
        for p, q in zip(getattr(a_new, nm).parameters(), getattr(a_old, nm).parameters()):
            assert torch.equal(p, q), nm
    # a buffer shorter than the batch: the eager update on the k rows there are
    short = DeviceReplayBuffer(41 * L, 3 * L, 64, device=dev)
    short.add_transitions(buf.obs_buffer[:20], buf.action_buffer[:20], buf.next_obs_buffer[:20], buf.reward_buffer[:20], buf.done_buffer[:20])
    out = g_new.update_from(0, gd, L, short, 1, seed, 9)
    assert np.isfinite(float(out["loss/critic_loss"]))


TRAINER_NAMES = ["3d_hopper_3_shin", "3d_walker_7_full"]


def _trainer(**kw):
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    args = default_train_args(max_episode_steps=30)
    tr = DeviceTrainer(TRAINER_NAMES, [4, 4], args=args, seed=3, device=DEV, max_buffer_size=256, batch_size=16, **kw)
    tr.warmup(30)
    return tr


@pytest.mark.parametrize("graphed", [False, True])
def test_trainer_with_the_device_sampler(graphed):
    tr = _trainer(device_sampler=True, graph_updates=graphed)
    gen0 = tr.gen.get_state().clone()
    assert all(b.max_sample_size >= 16 for b in tr.buffers)
    out = tr.train_round(max_steps=40, max_iters=2)
    assert out["per_morph_iter"] >= 1
    for name in TRAINER_NAMES:
        loss = tr.last_losses[name]
        assert np.isfinite(float(loss["loss/critic_loss"])) and np.isfinite(float(loss["misc/train_reward_mean"]))
    assert tr.draw == tr._updates == 2 * out["per_morph_iter"]       # one draw number per update
    assert torch.equal(tr.gen.get_state(), gen0)                       # the torch generator is not consulted
    if graphed:
        assert tr.graphed.warmed == {0, 1}
    tr.tot_env_steps = 12345                                           # a resumed run restarts the counter there
    assert tr.draw == 12345


def test_trainer_without_the_flag_consumes_its_generator_as_before():
    states = []
    for _ in range(2):
        tr = _trainer()
        assert tr.device_sampler is False
        gen0 = tr.gen.get_state().clone()
        out = tr.train_round(max_steps=40, max_iters=2)
        assert out["per_morph_iter"] >= 1 and tr.draw == 0
        assert not torch.equal(tr.gen.get_state(), gen0)               # sample(generator=self.gen) drew from it
        states.append(tr.gen.get_state().clone())
    assert torch.equal(states[0], states[1])
