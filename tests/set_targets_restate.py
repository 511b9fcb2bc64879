"""Shared by tests/test_set_targets.py and tests/test_set_targets_gpu.py: a float64 restatement of the no-grad half of a TD3 update
(reference src/agent.py:126-148) over CPU `SEPolicy` / `SECritic` modules, the weights and inputs both files use, and the mutants
that say what the restatement can tell apart.

Written from the reference's lines, not from the kernels:
    noise       = noise.clamp(-noise_clip, noise_clip)                                   agent.py:129
    next_action = (actor_target(next_obs) + noise).clamp(-max_action, max_action)        agent.py:130-133
    Q1, Q2      = critic_target(next_obs, next_action)                                   agent.py:136
    target      = reward + (1 - done) * discount * min(Q1, Q2)                           agent.py:137-139
The modules' forwards go through the tests/set_full_rank_ref.py helpers (float64 modules at oracle.formula full-rank weights).

Weights of weight set `seed`: the actor is apply_full_rank_(policy, seed).  The critic's seed is seed + 10; critic1 takes its own
full-rank values, critic2 a 0.7 / 0.3 mix of critic1's and its own: two independent networks differ by about their own scale, and
then one of them is the smaller one on almost every limb -- the mix keeps the pair close enough that the minimum changes sides.
Inputs: observations oracle.formula.synth_obs, noise N(0, 1) against noise_clip 0.9 and max_action 1 (so that both the clip and the
clamp act on a good share of the entries: tests/test_set_targets.py counts them), reward N(1, 0.5), done = 1 on two rows."""
import numpy as np
import torch

import set_full_rank_ref as R
from oracle.formula import apply_full_rank_, full_rank_values, synth_obs

NOISE_CLIP, MAX_ACTION, DISCOUNT = 0.9, 1.0, 0.99
SEED = 3                                                  # the weight set of the GPU file (qualified by tests/test_set_targets.py)
WALKER = (["3d_walker_7_full"], [5])                      # 35 nodes
CHEETAH = (["3d_cheetah_14_full"], [5])                   # 70 nodes (the GPU file's large batch is 147 rows of the same generator)
MIXED = (["3d_hopper_3_shin", "3d_cheetah_14_full", "3d_walker_7_full"], [3, 2, 1])     # 9 + 28 + 7 = 44 nodes
CASES = {"walker": WALKER, "cheetah": CHEETAH, "mixed": MIXED}
MUTANTS = ["no_noise_clip", "no_action_clamp", "done_ignored", "done_on_reward", "min_first", "min_second", "no_discount"]


def apply_actor(seed):
    return lambda m: apply_full_rank_(m, seed)


def apply_critic(seed):
    """critic1 = full_rank_values(critic1.<name>, seed + 10); critic2 = 0.7 x those values + 0.3 x full_rank_values(critic2.<name>)."""
    def apply(m):
        with torch.no_grad():
            sd = m.state_dict()
            for name, p in sd.items():
                v = full_rank_values(name, tuple(p.shape), seed + 10)
                if name.startswith("critic2."):
                    v = 0.7 * full_rank_values("critic1." + name[len("critic2."):], tuple(p.shape), seed + 10) + 0.3 * v
                p.copy_(torch.from_numpy(v).to(p.dtype))
        return m
    return apply


def cpu_pair(seed, dtype=torch.float64):
    """(SEPolicy, SECritic) on the CPU in `dtype` at weight set `seed`."""
    return R.cpu_modules("actor", apply_actor(seed), dtype), R.cpu_modules("critic", apply_critic(seed), dtype)


def inputs(names, counts, seed=0):
    """Per morphology block (name, L, c, next_obs [c, 41 L], noise [c, 3 L]) and the batch's reward, done [B] -- all float32, the
    dtype the replay buffer hands out.  done = 1 on rows 1 and B - 2 (two of five at B = 5); B = 1: the single row is not done."""
    B = int(sum(counts))
    rng = np.random.RandomState(4200 + seed)
    blocks = []
    for k, (n, c) in enumerate(zip(names, counts)):
        L = R.num_limbs(n)
        blocks.append((n, L, c, synth_obs(L, c, 900 + 31 * seed + k).astype(np.float32), rng.standard_normal((c, 3 * L)).astype(np.float32)))
    reward = rng.normal(1.0, 0.5, size=B).astype(np.float32)
    done = np.zeros(B, dtype=np.float32)
    if B > 1:
        done[[1, B - 2]] = 1.0
    return blocks, reward, done


def restate(pol, crit, name, next_obs, noise, reward, done, noise_clip=NOISE_CLIP, max_action=MAX_ACTION, discount=DISCOUNT,
            mutant=None):
    """agent.py:126-148 in float64 for one morphology block; reward, done [c].  Returns a dict: target [c, L] and the intermediate
    quantities the qualification counts (the raw action, the noisy one before its clamp, both critics' values)."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    next_obs, noise, reward, done = f(next_obs), f(noise), f(reward).reshape(-1, 1), f(done).reshape(-1, 1)
    nz = noise if mutant == "no_noise_clip" else np.clip(noise, -noise_clip, noise_clip)
    a, _ = R.actor_forward(pol, name, next_obs)
    noisy = a + nz
    na = noisy if mutant == "no_action_clamp" else np.clip(noisy, -max_action, max_action)
    (q1, q2), _ = R.critic_forward(crit, name, next_obs, na)
    m = q1 if mutant == "min_first" else q2 if mutant == "min_second" else np.minimum(q1, q2)
    nd = np.ones_like(done) if mutant == "done_ignored" else 1.0 - done
    g = 1.0 if mutant == "no_discount" else discount
    target = nd * (reward + g * m) if mutant == "done_on_reward" else reward + nd * g * m
    return dict(target=target, action=a, noise=noise, noisy=noisy, q1=q1, q2=q2)


def restate_case(pol, crit, names, counts, seed=0, mutant=None, **kw):
    """The restatement over every block of a batch: [(name, row 0, c, L, dict)]."""
    blocks, reward, done = inputs(names, counts, seed)
    out, r = [], 0
    for n, L, c, obs, noise in blocks:
        out.append((n, r, c, L, restate(pol, crit, n, obs, noise, reward[r:r + c], done[r:r + c], mutant=mutant, **kw)))
        r += c
    return out
