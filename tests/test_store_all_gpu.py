"""Continuous collection on the device: the round record that keeps every episode as one library call (include/sgrl.h
sgrl_round_record_all) against its tensor form, and DeviceTrainer(store_all_episodes=, true_next_obs=) against a Python-side
recorder of what every collection step produced.  Three hoppers x 4 environments, time limit 20, two warm-up rounds of random
actions: a few dozen steps per test."""
import numpy as np
import pytest

from helpers import HOPPERS

pytestmark = pytest.mark.gpu

PER = 4
LIMIT = 20


@pytest.mark.parametrize("max_steps", [2, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_fused_record_all_equals_the_tensor_form(n, max_steps):
    """(e) 40 steps of random reward / done streams around the kernel's workgroup size of 256; a finished round takes one more step
    (the late step of a lagged flag: nothing stored) on every second round before it begins anew.  Every output and every state
    array, exactly."""
    import torch
    from sgrl_amd import rollout
    g = torch.Generator(device="cuda").manual_seed(100 * n + max_steps)
    a = rollout.RoundCollector(n, max_episode_steps=max_steps, device="cuda:0", store_all=True)
    b = rollout.RoundCollector(n, max_episode_steps=max_steps, device="cpu", store_all=True)
    rounds, late, stored_none = 0, False, 0
    for t in range(40):
        rew = torch.randn(n, device="cuda", generator=g)
        done = (torch.rand(n, device="cuda", generator=g) < 0.3).to(torch.uint8)
        assert rollout.FUSED_RECORD
        sa, da, fa = a.record(rew, done)
        sb, db, fb = b.record(rew.cpu(), done.cpu())
        assert torch.equal(sa.cpu(), sb) and torch.equal(da.cpu(), db) and fa == fb, t
        for name in ("done_list", "episode_timesteps", "episode_reward", "_reward_buf", "cur_steps"):
            assert torch.equal(getattr(a, name).cpu(), getattr(b, name)), (name, t)
        assert bool(sb.all()) != late and bool(sb.any()) != late
        if late:
            stored_none += 1
        if fa and (late or rounds % 2 == 0):
            rounds += 1
            late = False
            a.begin_round()
            b.begin_round()
        elif fa:
            late = True
    assert rounds >= 4 and stored_none >= 2
    # the same collector with the tensor form on the device (FUSED_RECORD = False, as CPU ranks run it)
    c = rollout.RoundCollector(n, max_episode_steps=max_steps, device="cuda:0", store_all=True)
    d = rollout.RoundCollector(n, max_episode_steps=max_steps, device="cuda:0", store_all=True)
    for t in range(2 * max_steps + 1):
        rew = torch.randn(n, device="cuda", generator=g)
        done = (torch.rand(n, device="cuda", generator=g) < 0.3).to(torch.uint8)
        sc, dc, fc = c.record(rew, done)
        sc, dc = sc.clone(), dc.clone()
        rollout.FUSED_RECORD = False
        try:
            sd, dd, fd = d.record(rew, done)
        finally:
            rollout.FUSED_RECORD = True
        assert torch.equal(sc, sd) and torch.equal(dc, dd) and fc == fd, t
        assert torch.equal(c.cur_steps, d.cur_steps) and torch.equal(c.episode_timesteps, d.episode_timesteps)
    assert fc and not bool(sc.any())                       # the limit ended the round long ago: the last steps stored nothing


# ---- (f) DeviceTrainer ---------------------------------------------------------------------------------------------------------------
def _trainer(seed=3, **kw):
    import torch
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer
    assert torch.cuda.is_available()
    args = default_train_args(max_episode_steps=LIMIT, batch_size=16)
    kw.setdefault("lag_flag", False)
    return DeviceTrainer(HOPPERS, PER, args=args, seed=seed, device="cuda:0", max_buffer_size=1024, batch_size=16, **kw)


class _Recorder(object):
    """Host copies of what went into TransitionSink.push at every step: (prev_obs, action, next_obs, reward, done)."""

    def __init__(self, trainer):
        self.steps = []
        orig = trainer.sink.push

        def push(prev_obs, action, next_obs, reward, done):
            self.steps.append(tuple(t.detach().cpu().numpy().copy() for t in (prev_obs, action, next_obs, reward, done)))
            return orig(prev_obs, action, next_obs, reward, done)
        trainer.sink.push = push


TOPPLE = {3: [0, 5, 10], 8: [1, 5]}      # step of the round -> environments laid on their side before it (4 k .. 4 k + 3: hopper k)


def _topple(env, which):
    """Uniform actions end no hopper episode within 20 steps: every round would be one episode of 20 steps per environment and the
    two modes would store the same rows.  Environments laid on their side, at rest, 5 cm above the floor (records + refresh, the
    set_state path) terminate by themselves in their next step and run a second and a third episode inside the round."""
    import torch
    torch.cuda.synchronize()
    rec, cnt = env.get_records()
    for i in which:
        m = env.models[env.env_morph[i]]
        rec[i, 2] = 0.05
        rec[i, 3:7] = [0.70710678, 0.70710678, 0, 0]
        rec[i, m.nq:m.nq + m.nv] = 0
    env.set_records(rec, cnt)
    env.refresh_device()


def _warm_rounds(tr, rounds=2, before_step=None, after_step=None):
    """`rounds` warm-up rounds of random actions with the TOPPLE events.  Returns the index of the step that ended each round and
    the statistics train_round would report for it."""
    ends, stats, t = [], [], 0
    while len(ends) < rounds:
        if tr._steps_in_round in TOPPLE:
            _topple(tr.ro.env, TOPPLE[tr._steps_in_round])
        if before_step:
            before_step(t)
        fin = tr.collect_step(random_actions=True)
        if after_step:
            after_step(t)
        if fin:
            ends.append(t)
            c = tr.sink.collector
            stats.append((tr.sink.total_episode_timesteps() // tr.num_envs_global, c.episode_reward.mean().item(),
                          c.episode_timesteps.float().mean().item()))
            tr.begin_round()
        t += 1
        assert t < 4 * (LIMIT + 2)
    return ends, stats


def _expected_rows(steps, ends, env_morph, limbs, store_all, late):
    """The rule per environment, scalar code: rows per morphology in step-then-environment order.  `late`: the step that ended a
    round was taken after the round was complete (a flag read one step late) and stores nothing."""
    n = len(env_morph)
    rows = [[] for _ in limbs]
    first, cur = [True] * n, [0] * n
    for t, (obs, act, nxt, rew, done) in enumerate(steps):
        for i in range(n):
            timeout = cur[i] + 1 == LIMIT
            done_bool = 1.0 if (done[i] and not timeout) else 0.0
            if (store_all or first[i]) and not (late and t in ends):
                k = env_morph[i]
                L = limbs[k]
                rows[k].append((obs[i, :41 * L], act[i, :3 * L], nxt[i, :41 * L], rew[i], done_bool, t, i))
            if done[i] or timeout:
                first[i], cur[i] = False, 0
            else:
                cur[i] += 1
        if t in ends:
            first, cur = [True] * n, [0] * n
    return rows


def _assert_rings(tr, rows):
    for k, b in enumerate(tr.buffers):
        st = b.state_arrays()
        assert st["curr"] == st["max_sample_size"] == len(rows[k]) < 1024, k
        for j, (o, a, nx, rw, d, t, i) in enumerate(rows[k]):
            assert np.array_equal(st["obs_buffer"][j], o) and np.array_equal(st["action_buffer"][j], a), (k, t, i)
            assert np.array_equal(st["next_obs_buffer"][j], nx), (k, t, i)
            assert st["reward_buffer"][j] == rw and st["done_buffer"][j] == d, (k, t, i)
    assert tr.tot_env_steps == tr.sink.stored == sum(len(r) for r in rows)


@pytest.mark.parametrize("lag", [False, True])
def test_store_all_episodes_keeps_every_row_of_the_round(lag):
    tr = _trainer(store_all_episodes=True, lag_flag=lag)
    assert tr.sink.store_all and tr.sink.collector.store_all and tr.sink.lag_flag == lag
    rec = _Recorder(tr)
    ends, _ = _warm_rounds(tr)
    env = tr.ro.env
    rows = _expected_rows(rec.steps, ends, list(env.env_morph), env.num_limbs, True, lag)
    kept_steps = len(rec.steps) - (len(ends) if lag else 0)
    assert all(len(rows[k]) == kept_steps * PER for k in range(len(HOPPERS)))      # steps x environments
    assert kept_steps > len(ends)
    dones = np.concatenate([np.array([r[4] for r in rows[k]]) for k in range(len(HOPPERS))])
    assert (dones == 1).any()                                                      # some episode ended by itself inside a round
    _assert_rings(tr, rows)


def test_default_keeps_first_episodes_and_both_modes_report_the_same_round():
    few, every = _trainer(), _trainer(store_all_episodes=True)
    assert not few.store_all_episodes and not few.true_next_obs and not few.sink.store_all
    rec_few, rec_all = _Recorder(few), _Recorder(every)
    ends_few, stats_few = _warm_rounds(few)
    ends_all, stats_all = _warm_rounds(every)
    assert ends_few == ends_all and stats_few == stats_all                         # per_morph_iter, train_return, train_length
    for x, y in zip(rec_few.steps, rec_all.steps):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))                     # the rollout itself is untouched
    env = few.ro.env
    rows = _expected_rows(rec_few.steps, ends_few, list(env.env_morph), env.num_limbs, False, False)
    _assert_rings(few, rows)                                                       # what the parent commit stores: first episodes
    assert few.sink.stored < every.sink.stored == len(rec_all.steps) * env.num_envs
    # and one policy round on top: the same summary from both
    out_few, out_all = few.train_round(max_iters=2), every.train_round(max_iters=2)
    for key in ("steps", "per_morph_iter", "performance/train_return", "performance/train_length"):
        assert out_few[key] == out_all[key], key
    assert out_all["tot_env_steps"] > out_few["tot_env_steps"]


def test_true_next_obs_stores_the_observation_the_episode_ended_on():
    """The pre-reset observation comes from a twin engine that takes the trainer's records before every step and steps the same
    actions with auto_reset=False."""
    import torch
    from sgrl_amd.vec_env import BatchedModularVecEnv
    tr = _trainer(store_all_episodes=True, true_next_obs=True)
    plain = _trainer(store_all_episodes=True)
    rec, rec_plain = _Recorder(tr), _Recorder(plain)
    env = tr.ro.env
    twin = BatchedModularVecEnv(HOPPERS, PER, seed=3, device="cuda:0", max_episode_steps=LIMIT)
    pre_reset, after = [], []

    def before_step(t):
        torch.cuda.synchronize()
        twin.set_records(*env.get_records())

    def after_step(t):
        twin.step_device(tr.ro.actions.clone(), auto_reset=False)
        torch.cuda.synchronize()
        pre_reset.append((twin.obs.cpu().numpy().copy(), twin.done.cpu().numpy().astype(bool)))
        after.append(env.obs.cpu().numpy().copy())
    ends, _ = _warm_rounds(tr, before_step=before_step, after_step=after_step)
    _warm_rounds(plain)
    rows = _expected_rows(rec.steps, ends, list(env.env_morph), env.num_limbs, True, False)
    _assert_rings(tr, rows)                                                        # the rings hold what the recorder saw pushed
    ended = 0
    for k, L in enumerate(env.num_limbs):
        for (o, a, nx, rw, d, t, i) in rows[k]:
            fin = bool(rec.steps[t][4][i])
            assert fin == bool(pre_reset[t][1][i])
            if fin:
                ended += 1
                assert np.array_equal(nx, pre_reset[t][0][i, :41 * L]), (k, t, i)      # the observation the episode ended on
                assert not np.array_equal(nx, after[t][i, :41 * L]), (k, t, i)         # never the next episode's first
                if t + 1 < len(rec.steps) and t not in ends:
                    assert np.array_equal(rec.steps[t + 1][0][i, :41 * L], after[t][i, :41 * L])
                    assert not np.array_equal(rec.steps[t + 1][0][i, :41 * L], nx)
            else:
                assert np.array_equal(nx, after[t][i, :41 * L]), (k, t, i)             # every other row: the post-step observation,
                assert np.array_equal(nx, pre_reset[t][0][i, :41 * L]), (k, t, i)      # which is also the next row's obs
    assert ended >= 2 * env.num_envs
    # against the default next_obs on the same seeds: until the first episode ends the two runs store the very same rows
    first_end = min(t for t, s in enumerate(rec.steps) if s[4].any())
    assert first_end > 0
    for t in range(first_end):
        assert all(np.array_equal(p, q) for p, q in zip(rec.steps[t], rec_plain.steps[t])), t
    x, y = rec.steps[first_end], rec_plain.steps[first_end]
    assert all(np.array_equal(x[j], y[j]) for j in (0, 1, 3, 4))
    fin = x[4].astype(bool)
    assert np.array_equal(x[2][~fin], y[2][~fin]) and not np.array_equal(x[2][fin], y[2][fin])
    twin.close()


def test_true_next_obs_needs_a_driver_with_reset_where():
    import torch
    from sgrl_amd.rollout import Rollout
    from sgrl_amd.td3 import default_train_args
    from sgrl_amd.train_loop import DeviceTrainer

    class Driver(object):
        """The Rollout surface without the partial reset."""

        def __init__(self, ro):
            self.ro = ro

        def __getattr__(self, name):
            if name == "reset_where":
                raise AttributeError(name)
            return getattr(self.ro, name)
    args = default_train_args(max_episode_steps=LIMIT, batch_size=16)
    make = lambda policy, rank: Driver(Rollout(HOPPERS[:1], 2, policy=policy, seed=1, device="cuda:0", max_episode_steps=LIMIT))
    with pytest.raises(ValueError):
        DeviceTrainer(HOPPERS[:1], 2, args=args, seed=1, device="cuda:0", max_buffer_size=64, rollout=make, true_next_obs=True)
    DeviceTrainer(HOPPERS[:1], 2, args=args, seed=1, device="cuda:0", max_buffer_size=64, rollout=make, store_all_episodes=True)
    assert torch.cuda.is_available()


def test_a_training_round_with_both_switches_on():
    tr = _trainer(store_all_episodes=True, true_next_obs=True, lag_flag=True, graph_updates=False)
    tr.warmup(2 * LIMIT + 2)
    assert all(b.max_sample_size >= 16 for b in tr.buffers)
    out = tr.train_round(max_iters=2)
    assert out["per_morph_iter"] == 2 and 1 <= out["steps"] <= LIMIT + 1
    for name in HOPPERS:
        losses = tr.last_losses[name]
        assert all(np.isfinite(float(losses[key])) for key in losses if key.startswith("loss/")) and "loss/critic_loss" in losses, name
    assert tr.rounds == 1 and tr.graphed is None
