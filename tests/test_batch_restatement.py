"""tests/batch_restatement.py pinned on the definition of batching, at every width of the ladder (N = 2^12): the plaintext m of a
message v satisfies m(psi^(5^i)) = v_i and m(psi^-(5^i)) = v_(N/2 + i) modulo t, psi the minimal primitive 2N-th root; products are
slot-wise, the Galois element 5^s rotates both rows by s and 2N - 1 swaps them.  No GPU."""
import numpy as np
import pytest

import batch_restatement as R
from oracle import oracle as O

LOG_N = 12
N = 1 << LOG_N


def _eval(poly, x, t):
    acc = 0
    for c in reversed([int(c) for c in poly]):
        acc = (acc * x + c) % t
    return acc


def _message(rng, t, size=N):
    return rng.integers(0, t, size, dtype=np.uint64)


def test_index_map_is_a_permutation_with_the_reference_corners():
    for log_n in (1, 2, 5, 12, 15):
        m = R.index_map(log_n)
        assert sorted(int(v) for v in m) == list(range(1 << log_n))
        assert int(m[0]) == 0                                                  # (5^0 - 1) / 2 = 0
        assert int(m[(1 << log_n) >> 1]) == (1 << log_n) - 1                   # (2N - 1 - 1) / 2 = N - 1, all ones
    assert [int(v) for v in R.index_map(3)] == [0, 2, 1, 3, 7, 5, 6, 4]      # 5^i = 1, 5, 9, 13 mod 16


@pytest.mark.parametrize("bits", sorted(R.LADDER))
def test_slots_are_the_evaluations_at_the_odd_powers_of_psi(bits):
    t = R.LADDER[bits]
    assert O.is_prime(t) and (t - 1) % (2 * N) == 0 and t.bit_length() == bits
    b = R.batch(LOG_N, t)
    rng = np.random.default_rng(bits)
    v = _message(rng, t)
    m = b.encode(v)
    assert int(m.max()) < t
    psi = O.minimal_primitive_root(2 * N, t)
    for i in (0, 1, 2, 77, N // 2 - 1):
        g = pow(5, i, 2 * N)
        assert _eval(m, pow(psi, g, t), t) == int(v[i]), i
        assert _eval(m, pow(psi, 2 * N - g, t), t) == int(v[N // 2 + i]), i
    assert np.array_equal(b.decode(m), v)


def test_every_slot_at_a_small_degree():
    log_n, n = 6, 64
    t = R.batching_prime(log_n, 20)
    b = R.batch(log_n, t)
    v = _message(np.random.default_rng(6), t, n)
    m = b.encode(v)
    psi = O.minimal_primitive_root(2 * n, t)
    for i in range(n // 2):
        g = pow(5, i, 2 * n)
        assert _eval(m, pow(psi, g, t), t) == int(v[i])
        assert _eval(m, pow(psi, 2 * n - g, t), t) == int(v[n // 2 + i])


@pytest.mark.parametrize("bits", sorted(R.LADDER))
def test_short_messages_sign_rule_product_rotation_and_swap(bits):
    t = R.LADDER[bits]
    b = R.batch(LOG_N, t)
    rng = np.random.default_rng(1000 + bits)
    a, c = _message(rng, t), _message(rng, t)
    # zero padding
    for size in (0, 1, N // 2, N - 1):
        padded = np.zeros(N, dtype=np.uint64)
        padded[:size] = a[:size]
        assert np.array_equal(b.encode(a[:size]), b.encode(padded)), size
        assert np.array_equal(b.decode(b.encode(a[:size])), padded), size
    # the sign rule: -x in two's complement encodes t - x
    small = rng.integers(1, min(t, 1 << 62), N, dtype=np.int64)
    assert np.array_equal(b.encode(-small), b.encode((t - small.astype(object)).astype(np.uint64)))
    # slot-wise product
    want = np.array([(int(x) * int(y)) % t for x, y in zip(a, c)], dtype=np.uint64)
    assert np.array_equal(b.decode(b.multiply(b.encode(a), b.encode(c))), want)
    # rotation of both rows by s, and the row swap
    rows = a.reshape(2, N // 2)
    for s in (1, 5, N // 2 - 1):
        got = b.decode(b.galois(b.encode(a), pow(5, s, 2 * N)))
        assert np.array_equal(got.reshape(2, N // 2), np.roll(rows, -s, axis=1)), s
    got = b.decode(b.galois(b.encode(a), 2 * N - 1))
    assert np.array_equal(got.reshape(2, N // 2), rows[::-1])
