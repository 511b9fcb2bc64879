"""The replay draw of include/sgrl_replay.h restated in NumPy / Python integers -- Philox4x32-10, the multiply-shift candidates,
sequential rejection of repeats, the candidate cap and its fallback, Box-Muller in float64 -- with the Random123 known answers,
the properties the definition promises, its uniformity, and the host side of the library: the header's names are exported, there
is no CPU fallback.  tests/test_replay_sample_gpu.py holds the kernel to this restatement bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from sgrl_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
PAIRS = [(1, 1), (5, 8), (256, 256), (300, 256), (1024, 1024), (1000003, 256)]      # (fill, batch)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(M32) for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(M32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(M32)]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [x.astype(np.uint32) for x in c]


def stream_words(seed, draw, stream, start, count):
    """Words x_start .. x_(start + count - 1) of `stream`: key (seed lo, seed hi), counter (i >> 2, draw lo, draw hi, stream), word i & 3."""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    i = np.arange(start, start + count, dtype=np.uint64)
    out = philox4x32_10((i >> np.uint64(2), draw & M32, draw >> 32, stream), (seed & M32, seed >> 32))
    return np.stack(out, axis=1)[np.arange(count), (i & np.uint64(3)).astype(np.int64)]


def draw_rows(fill, batch, seed, draw, max_candidates=0):
    """idx[j] = the j-th distinct value of c_i = (x_i * fill) >> 32, i = 0, 1, ...; after `max_candidates` candidates (0 = 64 k) the
    remaining positions take the smallest rows not yet taken, ascending.  Returns (int64 [k], candidates looked at)."""
    k = min(int(fill), int(batch))
    cap = 64 * k if max_candidates == 0 else int(max_candidates)
    rows, seen, i = [], set(), 0
    while len(rows) < k and i < cap:
        n = min(cap - i, 4096)
        x = stream_words(seed, draw, 0, i, n).astype(np.uint64)
        for j, c in enumerate(((x * np.uint64(fill)) >> np.uint64(32)).tolist()):
            if c not in seen:
                seen.add(c)
                rows.append(c)
                if len(rows) == k:
                    return np.asarray(rows, dtype=np.int64), i + j + 1
        i += n
    r = 0
    while len(rows) < k:
        if r not in seen:
            rows.append(r)
        r += 1
    return np.asarray(rows, dtype=np.int64), min(i, cap)


def draw_noise(k, act_dim, seed, draw, noise_std):
    """[k, act_dim] float32: element e = j * act_dim + c takes words 2 e and 2 e + 1 of stream 1, u = (x + 0.5) / 2^32,
    z = sqrt(-2 ln u1) cos(2 pi u2) in float64, rounded once to float32, times noise_std in float32."""
    x = stream_words(seed, draw, 1, 0, 2 * k * act_dim).astype(np.float64).reshape(k * act_dim, 2)
    u = (x + 0.5) / 4294967296.0
    z = np.sqrt(-2.0 * np.log(u[:, 0])) * np.cos(2.0 * np.pi * u[:, 1])
    return (z.astype(np.float32) * np.float32(noise_std)).reshape(k, act_dim)


# ---- known answers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_gives_the_random123_known_answers(counter, key, want):
    assert tuple(int(x) for x in philox4x32_10(counter, key)) == want


def test_stream_words_follow_the_counter_layout():
    seed, draw = 0x299f31d0a4093822, 0x1319_8a2e_85a3_08d3
    # block 0x243f6a88 of stream 0x03707344 is the third known answer: its four words are x_(4 b) .. x_(4 b + 3)
    got = stream_words(seed, draw, 0x03707344, 4 * 0x243f6a88, 4)
    assert [int(x) for x in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    assert int(stream_words(seed, draw, 0x03707344, 4 * 0x243f6a88 + 2, 1)[0]) == 0x5001e420


# ---- properties of the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill, batch", PAIRS)
def test_k_distinct_rows_below_fill(fill, batch):
    k = min(fill, batch)
    for seed, draw in ((1, 0), (0xDEADBEEFCAFE, 2 ** 32 + 5)):
        idx, looked = draw_rows(fill, batch, seed, draw)
        assert idx.shape == (k,) and idx.dtype == np.int64
        assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < fill
        assert k <= looked <= 64 * k
    if fill == k:
        assert sorted(idx.tolist()) == list(range(fill))


def test_another_draw_gives_other_rows():
    a, _ = draw_rows(200000, 256, 7, 0)
    b, _ = draw_rows(200000, 256, 7, 1)
    c, _ = draw_rows(200000, 256, 8, 0)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, draw_rows(200000, 256, 7, 0)[0])
    # the draw number is 64 bits wide: 2^32 + 5 is not draw 5
    assert not np.array_equal(draw_rows(200000, 256, 7, 5)[0], draw_rows(200000, 256, 7, 2 ** 32 + 5)[0])


def test_the_candidate_cap_reaches_the_fallback_and_still_returns_a_permutation():
    idx, looked = draw_rows(64, 64, 3, 0, max_candidates=64)
    assert looked == 64
    assert sorted(idx.tolist()) == list(range(64))
    free, _ = draw_rows(64, 64, 3, 0)
    # the head is the uncapped draw's, as far as 64 candidates reach; the tail ascends through the rows not yet taken
    x = stream_words(3, 0, 0, 0, 64).astype(np.uint64)
    n_distinct = len(set(((x * np.uint64(64)) >> np.uint64(32)).tolist()))
    assert 1 < n_distinct < 64
    assert np.array_equal(idx[:n_distinct], free[:n_distinct])
    tail = idx[n_distinct:].tolist()
    assert tail == sorted(tail) == sorted(set(range(64)) - set(idx[:n_distinct].tolist()))


def test_noise_restatement_is_standard_normal_and_scaled():
    z = draw_noise(256, 45, 11, 4, 1.0)
    assert z.dtype == np.float32 and z.shape == (256, 45)
    assert abs(float(z.mean())) < 5 / np.sqrt(z.size) and abs(float(z.std()) - 1.0) < 5 / np.sqrt(2 * z.size)
    assert np.array_equal(draw_noise(256, 45, 11, 4, 0.2), z * np.float32(0.2))
    # element e depends on (seed, draw, e) alone: fewer rows are a prefix
    assert np.array_equal(draw_noise(3, 45, 11, 4, 1.0), z[:3])


# ---- uniformity ------------------------------------------------------------------------------------------------------------------
UNIFORMITY_SEED = 2024      # committed: the restatement itself satisfies the bound below with this seed


def test_every_row_is_equally_likely_in_every_position():
    """4 000 draws of batch 4 from fill 16: the count of each row in each position is Binomial(4 000, 1 / 16); the bound is five of
    its standard deviations (a condition on the definition, not a tuned number)."""
    n, fill, batch = 4000, 16, 4
    count = np.zeros((batch, fill), dtype=np.int64)
    for d in range(n):
        idx, _ = draw_rows(fill, batch, UNIFORMITY_SEED, d)
        count[np.arange(batch), idx] += 1
    mean, sd = n / fill, np.sqrt(n * (1 / fill) * (1 - 1 / fill))
    dev = np.abs(count - mean).max()
    print("largest deviation %.1f of mean %.1f (5 sd = %.1f)" % (dev, mean, 5 * sd))
    assert dev <= 5 * sd


# ---- header and library ------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sgrl_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_name_the_header_declares():
    so = ctypes.CDLL(_lib.build())
    names = _declared("sgrl_replay.h")
    assert names == ["sgrl_replay_last_error", "sgrl_replay_sample", "sgrl_replay_sample_launches"]
    for n in names:
        assert hasattr(so, n), n
    assert "replay_sample.hip" in _lib.SOURCES
    # bound from its own module: sgrl.h and _lib.EXPORTS do not list them
    assert not set(names) & set(_lib.EXPORTS) and not set(names) & set(_declared("sgrl.h"))


def test_launch_count_and_argument_errors_need_no_device():
    from sgrl_amd.replay import _Ring, _bind
    L = _lib.lib()
    _bind(L)
    assert L.sgrl_replay_sample_launches() in (1, 2)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ring = _Ring(p, p, p, p, p, 8, 4)
    call = lambda ring, fill, batch, cand, lds, noise, ldn: L.sgrl_replay_sample(
        ring, fill, batch, 1, 0, cand, None, p, lds[0], p, lds[1], p, lds[2], p, p, None, noise, ldn, 0.2, None)
    assert call(None, 4, 4, 0, (8, 4, 8), None, 0) == -1
    assert b"sgrl_replay_sample" in L.sgrl_replay_last_error()
    assert call(ctypes.byref(ring), 0, 4, 0, (8, 4, 8), None, 0) == -1
    assert call(ctypes.byref(ring), 4, 0, 0, (8, 4, 8), None, 0) == -1
    assert call(ctypes.byref(ring), 4, 1025, 0, (8, 4, 8), None, 0) == -1
    assert call(ctypes.byref(ring), 4, 4, 0, (7, 4, 8), None, 0) == -1
    assert call(ctypes.byref(ring), 4, 4, 0, (8, 3, 8), None, 0) == -1
    assert call(ctypes.byref(ring), 4, 4, 0, (8, 4, 7), None, 0) == -1
    assert call(ctypes.byref(ring), 4, 4, 0, (8, 4, 8), p, 3) == -1
    assert call(ctypes.byref(ring), 4, 4, -1, (8, 4, 8), None, 0) == -1


def test_no_cpu_fallback_without_a_device():
    from sgrl_amd.replay import DeviceReplayBuffer, _Ring, _bind
    buf = DeviceReplayBuffer(8, 4, 16, device="cpu")
    buf.add_transitions(torch.ones(4, 8), torch.ones(4, 4), torch.ones(4, 8), torch.ones(4), torch.zeros(4))
    out = dict(obs=torch.zeros(4, 8), action=torch.zeros(4, 4), next_obs=torch.zeros(4, 8), reward=torch.zeros(4, 1),
               done=torch.zeros(4, 1))
    with pytest.raises(_lib.SgrlError, match="no CPU fallback"):
        buf.sample_into(out, 4, 1, 0)
    assert all(float(t.abs().sum()) == 0 for t in out.values())
    if torch.cuda.is_available():
        return                          # the library call below is the no-device case
    L = _lib.lib()
    _bind(L)
    host = (ctypes.c_float * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)
    ring = _Ring(p, p, p, p, p, 8, 4)
    rc = L.sgrl_replay_sample(ctypes.byref(ring), 4, 4, 1, 0, 0, None, p, 8, p, 4, p, 8, p, p, None, None, 0, 0.0, None)
    assert rc == -3                     # SGRL_ERR_HIP
    assert b"no CPU fallback" in L.sgrl_replay_last_error()
    assert all(v == 0 for v in host)
