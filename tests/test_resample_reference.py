"""CPU tests of oracle/resample_np.py, the plain reference of the device-drawn bootstrap resample
(oem_bootstrap_weights): philox4x32-10 against the known answers published with Random123
(kat_vectors), the two forms of it against each other, the multiply-high against big integers, and
the properties of the draw that do not need a device.  tests/test_bootstrap_draw_gpu.py holds the
kernel to this reference bit for bit."""
import numpy as np
import pytest

from oracle import resample_np as rs

# Random123 kat_vectors, "philox4x32 10": counter, key, output
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers_scalar(ctr, key, want):
    assert rs.philox4x32_10(ctr, key) == want


def test_philox_known_answers_vectorised():
    ctr = np.array([k[0] for k in KAT], dtype=np.uint64)
    key = np.array([k[1] for k in KAT], dtype=np.uint64)
    want = np.array([k[2] for k in KAT], dtype=np.uint64)
    got = rs.philox4x32_10_np(ctr, key)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    for c, k, w in KAT:   # one block, and one key broadcast over the blocks
        assert np.array_equal(rs.philox4x32_10_np(np.array(c), np.array(k)), np.array(w, dtype=np.uint64))
        assert np.array_equal(rs.philox4x32_10_np(np.array([c, c]), np.array(k)), np.array([w, w], dtype=np.uint64))


def test_philox_scalar_and_vectorised_forms_agree():
    rng = np.random.default_rng(2011)
    ctr = rng.integers(0, 1 << 32, size=(2000, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(2000, 2), dtype=np.uint64)
    ctr[:8] = [[0, 0, 0, 0], [0xffffffff] * 4, [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1],
               [0xffffffff, 0, 0xffffffff, 0], [0, 0xffffffff, 0, 0xffffffff]]
    got = rs.philox4x32_10_np(ctr, key)
    for i in range(len(ctr)):
        assert tuple(int(x) for x in got[i]) == rs.philox4x32_10(ctr[i], key[i]), i
    assert int(got.max()) < 1 << 32
    # every input word matters: flipping one bit of any counter or key word changes the block
    base = rs.philox4x32_10((1, 2, 3, 4), (5, 6))
    for w in range(4):
        c = [1, 2, 3, 4]
        c[w] ^= 1 << 31
        assert rs.philox4x32_10(c, (5, 6)) != base
    assert rs.philox4x32_10((1, 2, 3, 4), (5 ^ 1, 6)) != base
    assert rs.philox4x32_10((1, 2, 3, 4), (5, 6 ^ 1)) != base


@pytest.mark.parametrize("n", [1, 3, 10_000_001, 2**40 + 12345, 2**64 - 1])
def test_mulhi64_matches_big_integers(n):
    rng = np.random.default_rng(n % 1000)
    a = rng.integers(0, 1 << 64, size=5000, dtype=np.uint64)
    a[:6] = [0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1]
    got = rs.mulhi64(a, n)
    assert got.dtype == np.uint64
    want = [(int(x) * n) >> 64 for x in a]
    assert [int(x) for x in got] == want
    assert int(got.max()) < n


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 4097, 200_001])
@pytest.mark.parametrize("seed,replica", [(0, 0), (0x123456789abcdef0, 4), (2**64 - 1, 2**32 - 1)])
def test_draw_sums_to_the_read_count(n, seed, replica):
    w = rs.bootstrap_weights(n, seed, replica)
    assert w.dtype == np.uint32 and w.shape == (n,)
    assert int(w.sum()) == n


def test_one_read_store_draws_that_read_once():
    for seed, replica in [(0, 0), (11, 1), (2**64 - 1, 2**32 - 1)]:
        assert rs.bootstrap_weights(1, seed, replica).tolist() == [1]
        assert rs.bootstrap_weights_scalar(1, seed, replica).tolist() == [1]


@pytest.mark.parametrize("n", [2, 3, 257, 1000, 1001])
def test_vectorised_draw_equals_the_draw_by_draw_form(n):
    for seed, replica in [(11, 0), (0x1_0000_0000, 1), (0x123456789abcdef0, 2**32 - 1)]:
        full = rs.bootstrap_weights(n, seed, replica)
        assert np.array_equal(full, rs.bootstrap_weights_scalar(n, seed, replica))
        off, cnt = n // 3, n - n // 3 - 1
        assert np.array_equal(rs.bootstrap_weights(n, seed, replica, off, cnt),
                              rs.bootstrap_weights_scalar(n, seed, replica, off, cnt))


def test_draw_crosses_the_chunk_boundary_of_the_vectorised_form(monkeypatch):
    n = 10_001
    want = rs.bootstrap_weights(n, 7, 3)
    monkeypatch.setattr(rs, "_CHUNK", 257)   # odd chunk, last chunk partial, odd store
    assert np.array_equal(rs.bootstrap_weights(n, 7, 3), want)


@pytest.mark.parametrize("n,cuts", [(10, [0, 1, 2, 9, 10]), (200_001, [0, 1, 66_667, 66_668, 199_999, 200_001]),
                                    (4097, [0, 4096, 4097]), (1001, [0, 0, 333, 1001, 1001])])
def test_shard_slices_concatenate_to_the_full_draw(n, cuts):
    full = rs.bootstrap_weights(n, 0xdeadbeef_00000005, 9)
    parts = [rs.bootstrap_weights(n, 0xdeadbeef_00000005, 9, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [len(p) for p in parts] == [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), full)
    assert np.array_equal(rs.bootstrap_weights(n, 0xdeadbeef_00000005, 9, 0, n), full)
    with pytest.raises(ValueError):
        rs.bootstrap_weights(n, 1, 0, n - 1, 2)


def test_every_part_of_the_stream_key_matters():
    """(seed low, seed high, replica) each select a different stream, and the draw is reproducible."""
    n = 20_000
    a = rs.bootstrap_weights(n, 11, 0)
    assert np.array_equal(a, rs.bootstrap_weights(n, 11, 0))
    others = [rs.bootstrap_weights(n, 12, 0), rs.bootstrap_weights(n, 11 + (1 << 32), 0),
              rs.bootstrap_weights(n, 11 << 32, 0), rs.bootstrap_weights(n, 11 + (11 << 32), 0),
              rs.bootstrap_weights(n, 11, 1), rs.bootstrap_weights(n, 0, 11)]
    for i, b in enumerate(others):
        assert not np.array_equal(a, b), i
        for j in range(i):
            assert not np.array_equal(others[j], b), (i, j)


def test_draw_has_the_moments_of_the_multinomial():
    """bootstrap.rs:7-16: Multinomial(n; 1/n) -- the reference itself is a sound resample."""
    n = 200_000
    w0, w1 = rs.bootstrap_weights(n, 11, 0), rs.bootstrap_weights(n, 11, 1)
    for w in (w0, w1):
        assert abs(w.var() - (1 - 1 / n)) < 0.02
        assert abs((w == 0).mean() - np.exp(-1)) < 0.01
        assert abs((w == 1).mean() - np.exp(-1)) < 0.01
        assert abs((w == 2).mean() - np.exp(-1) / 2) < 0.01
    assert abs(np.corrcoef(w0, w1)[0, 1]) < 0.02
