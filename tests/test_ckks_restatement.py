"""The numpy restatement of the CKKS encoder (tests/ckks_restatement.py) against the definition -- no GPU, no library.

Encoding is the canonical embedding: the polynomial with the rounded coefficients takes the value scale * z_i at zeta^(5^i), zeta =
e^{2 pi i / 2N}.  Evaluated in np.longdouble at N = 2^10 the unrounded coefficients reproduce it within relative 2^-44 (128 times the
2^-51 measured when this was written; an index or root error gives order 1), and the round trip through rounding stays within
N / (2 scale) (the worst case of the rounding) + 2^-40 max |z| (floating-point slack)."""
import numpy as np

import ckks_restatement as R

LOG_N = 10
N = 1 << LOG_N
SLOTS = N // 2
M = 2 * N
SCALE = 2.0 ** 40


def _tables():
    return R.roots_table(M), R.group_table(M, SLOTS // 2)


def test_tables():
    roots, group = _tables()
    assert R.roots_ulp_error(roots) <= 2.0
    assert R.roots_ulp_error(R.roots_table(1 << 14)) <= 2.0
    assert roots[0].tolist() == [1.0, 0.0] and roots[M // 4].tolist() == [0.0, 1.0] and roots[M // 2][0] == -1.0
    assert [int(g) for g in group[:4]] == [1, 5, 25, 125] and all(int(g) == pow(5, i, M) for i, g in enumerate(group))


def test_encoding_is_the_canonical_embedding():
    rng = np.random.default_rng(0xCCE5)
    roots, group = _tables()
    z = rng.uniform(0.5, 1, SLOTS) * np.exp(1j * rng.uniform(0, 2 * np.pi, SLOTS))   # moduli away from 0: the error is relative
    coeffs = R.encode_coeffs(z, SLOTS, roots, group, SCALE)
    # evaluate sum_j c_j zeta^(5^i j) in long double, with exactly reduced exponents
    two_pi = 2 * np.arccos(np.longdouble(-1))
    zeta = np.exp(1j * (two_pi * np.arange(M, dtype=np.longdouble) / M)).astype(np.clongdouble)
    c = coeffs.astype(np.longdouble)
    j = np.arange(N, dtype=np.int64)
    worst = 0.0
    for i in range(SLOTS):
        e = (pow(5, i, M) * j) % M
        got = np.sum(c * zeta[e])
        worst = max(worst, float(abs(got - np.clongdouble(z[i]) * SCALE) / (abs(z[i]) * SCALE)))
    print("canonical embedding, worst relative error:", worst)
    assert worst < 2.0 ** -44


def test_round_trip_within_the_rounding_bound():
    rng = np.random.default_rng(0xCCE6)
    roots, group = _tables()
    for size in (1, SLOTS // 2 + 1, SLOTS):
        z = rng.uniform(-1, 1, size) + 1j * rng.uniform(-1, 1, size)
        coeffs = R.encode_coeffs(z, SLOTS, roots, group, SCALE)
        rounded = np.array([float(v) for v in R.round_coeffs(coeffs)])
        back = R.decode_values(rounded / SCALE, SLOTS, roots, group)
        want = np.concatenate([z, np.zeros(SLOTS - size)])
        err = float(np.max(np.abs(back - want)))
        print("round trip, size", size, "max error", err)
        assert err <= N / (2 * SCALE) + 2.0 ** -40 * float(np.max(np.abs(z)))


def test_exact_rounding_and_bit_count():
    assert [R.round_exact(x) for x in (0.5, -0.5, 1.5, -1.5, 2.5, 0.49999999999999994, -0.49999999999999994, -0.2)] == \
        [1, -1, 2, -2, 3, 0, 0, 0]
    xs = [0.5, -0.5, 2.0 ** 52 + 1, -(2.0 ** 52 + 1), 2.0 ** 63 - 1024, 4503599627370495.5, -4503599627370495.5, 1e300, -3.7]
    assert R.round_coeffs(xs) == [R.round_exact(x) for x in xs]
    assert R.bit_count(np.array([0.3])) == 1 and R.bit_count(np.array([1.0])) == 1 and R.bit_count(np.array([-2.0])) == 2
    assert R.bit_count(np.array([2.0 ** 40])) == 41 and R.bit_count(np.array([np.nextafter(2.0 ** 40, np.inf)])) == 42
    assert R.bit_count(np.array([np.inf])) > 4096


def test_compose_double_is_the_centred_value():
    primes = [1099511590913, 1099511592961, 1152921504606830593]
    big_q = primes[0] * primes[1] * primes[2]
    for v in (0, 1, -1, 12345678901234567890123, -12345678901234567890123, big_q // 2, -(big_q // 2)):
        got = R.compose_double(v % big_q, big_q, 3, 1.0)
        assert abs(got - float(v)) <= abs(float(v)) * 2.0 ** -50, (v, got)


def test_compose_array_is_compose_double_on_arrays():
    from oracle import oracle as O
    primes = [int(q) for q in O.coeff_modulus_create(1 << 10, [60, 40, 40, 50])]
    rng = np.random.default_rng(3)
    for size in (1, 2, 4):
        res = np.stack([rng.integers(0, q, 300, dtype=np.uint64) for q in primes[:size]])
        res[:, :4] = 0
        res[:, 4] = [q - 1 for q in primes[:size]]
        x, big_q = R.crt_values(res, primes[:size])
        want = np.array([R.compose_double(int(v), big_q, size, 2.0 ** -40) for v in x])
        assert np.array_equal(R.compose_array(res, primes[:size], 2.0 ** -40).view(np.uint64), want.view(np.uint64))
