"""The per-thread programs of the noise kernels (phantom-fhe_amd/csrc/pha_noise.h: host/device functions, the very source the
kernels call) and their host-built tables (pha_rns_tables.h noise_tables / noise_level_tables) compiled for the host and compared
with Python integers -- no GPU needed.  Harness: tests/emu/emu_noise.cpp (test-only).

Chains: ladder12 (every width, 41 .. 61 bits) and the same reversed (61-bit limbs first, so digits exceed the later moduli), L = 1,
2, 4, 14; scalars 1, 65537 and a 59-bit t above the 41-bit limbs.  Values: uniform v and the constructed 0, 1, Q - 1, (Q - 1) / 2,
(Q + 1) / 2, 2^k - 1, 2^k and Q - 2^k for every k at a 64-bit word boundary and at bitcount(Q) - 2.  Expected: the digits are
Python's mixed-radix digits; the sign decision, the magnitude's digits, the Horner words, the bit count and the budget are exact;
the lexicographic maximum of a set is max of the integers, ties and sets that differ only in the lowest digit included.

The harness is also built ONCE as a stand-alone program (its own main) with -fsanitize=undefined and run on the CPU: the bit count
must not shift by the word size."""
import ctypes as C
import os
import subprocess
from math import prod

import numpy as np
import pytest

from oracle import oracle as O
from util import primes_of, rng_for

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)
LADDER = [int(q) for q in primes_of("ladder12")[1]]
WIDE = LADDER[::-1]
CHAINS = {"ladder": LADDER, "wide": WIDE}
T59 = int(O.get_primes(1 << 12, 59, 3)[2])                  # a 59-bit prime that is no limb of ladder12
SCALARS = [1, 65537, T59]
LIMB_COUNTS = [1, 2, 4, 14]
CASES = [(name, L, s) for name in CHAINS for L in LIMB_COUNTS for s in SCALARS]
UNIFORM = 256


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_noise") / "libemu_noise.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "emu", "emu_noise.cpp")])
    L = C.CDLL(out)
    L.emu_noise_max_limbs.restype = C.c_uint32
    L.emu_noise_tables.argtypes = [u64p, C.c_uint32, u64p, u64p]
    L.emu_noise_tables.restype = None
    L.emu_noise_level.argtypes = [u64p, C.c_uint32, u64p]
    L.emu_noise_level.restype = C.c_int
    L.emu_noise_columns.argtypes = [u64p, C.c_uint32, C.c_uint32, C.c_uint64, u64p, C.c_size_t, u64p, u64p, u32p, u64p, u32p, i32p]
    L.emu_noise_columns.restype = None
    L.emu_noise_argmax.argtypes = [u64p, C.c_size_t, C.c_uint32]
    L.emu_noise_argmax.restype = C.c_size_t
    L.emu_noise_bits.argtypes = [u64p, C.c_uint32]
    L.emu_noise_bits.restype = C.c_uint32
    return L


def p(a):
    return a.ctypes.data_as(u64p)


def a64(v):
    return np.array([int(x) for x in v], dtype=np.uint64)


def mixed_radix(v, primes):
    """v in [0, prod(primes)) -> its digits a_i < q_i, v = a_0 + a_1 q_0 + a_2 q_0 q_1 + ..."""
    out = []
    for q in primes:
        out.append(v % q)
        v //= q
    assert v == 0
    return out


def words_of(v, L):
    return [(v >> (64 * w)) & ((1 << 64) - 1) for w in range(L)]


def constructed(Q):
    """The values of the module docstring that lie in [0, Q)."""
    bits = Q.bit_length()
    vals = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2]
    for k in sorted(set(list(range(64, bits, 64)) + [bits - 2])):
        if k >= 1:
            vals += [(1 << k) - 1, 1 << k, Q - (1 << k)]
    return [v for v in vals if 0 <= v < Q]


def run_columns(emu, primes, L, scalar, values):
    """values: integers in [0, Q) whose RESIDUES go in; returns the harness' (digits, mag, neg, words, bits, budget)."""
    x = np.array([[v % q for v in values] for q in primes[:L]], dtype=np.uint64)
    n = len(values)
    digits, mag, words = (np.zeros((n, L), dtype=np.uint64) for _ in range(3))
    neg, bits, budget = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    emu.emu_noise_columns(p(a64(primes)), len(primes), L, scalar, p(np.ascontiguousarray(x)), n, p(digits), p(mag),
                          neg.ctypes.data_as(u32p), p(words), bits.ctypes.data_as(u32p), budget.ctypes.data_as(i32p))
    return digits, mag, neg, words, bits, budget


@pytest.mark.parametrize("name,L", [(n, L) for n in CHAINS for L in LIMB_COUNTS])
def test_tables_equal_python_integers(emu, name, L):
    primes = CHAINS[name]
    size = len(primes)
    assert emu.emu_noise_max_limbs() == 64
    inv, lift = np.zeros(size * size * 2, dtype=np.uint64), np.zeros(size, dtype=np.uint64)
    emu.emu_noise_tables(p(a64(primes)), size, p(inv), p(lift))
    inv = inv.reshape(size, size, 2)
    for j, qj in enumerate(primes):
        assert int(lift[j]) % qj == 0 and (1 << 61) <= int(lift[j]) < (1 << 61) + qj
        for i in range(size):
            if i < j:
                w = pow(primes[i], -1, qj)
                assert (int(inv[i, j, 0]), int(inv[i, j, 1])) == (w, (w << 64) // qj), (i, j)
            else:
                assert (int(inv[i, j, 0]), int(inv[i, j, 1])) == (0, 0)
    Q = prod(primes[:L])
    half = np.zeros(L, dtype=np.uint64)
    assert emu.emu_noise_level(p(a64(primes)), L, p(half)) == Q.bit_length()
    assert [int(h) for h in half] == mixed_radix((Q - 1) // 2, primes[:L])


@pytest.mark.parametrize("name,L,scalar", CASES)
def test_every_stage_equals_python_integers(emu, name, L, scalar):
    primes = CHAINS[name]
    qs = primes[:L]
    Q = prod(qs)
    rng = rng_for(9400 + 100 * list(CHAINS).index(name) + 10 * LIMB_COUNTS.index(L) + SCALARS.index(scalar))
    uniform = [int(sum(int(rng.integers(0, 1 << 62)) << (62 * k) for k in range(L + 1)) % Q) for _ in range(UNIFORM)]
    special = constructed(Q)
    # the constructed values are meant for the number the norm is taken of: feed x with scalar * x == v (mod Q)
    back = pow(scalar, -1, Q)
    values = uniform + [v * back % Q for v in special]
    digits, mag, neg, words, bits, budget = run_columns(emu, primes, L, scalar, values)
    for j, x in enumerate(values):
        v = x * scalar % Q
        if j >= UNIFORM:
            assert v == special[j - UNIFORM]
        assert [int(d) for d in digits[j]] == mixed_radix(v, qs), (j, v)
        want_neg = v >= (Q + 1) // 2
        m = Q - v if want_neg else v
        assert m == min(v, Q - v)
        assert bool(neg[j]) == want_neg, (j, v)
        assert [int(d) for d in mag[j]] == mixed_radix(m, qs), (j, v)
        assert [int(w) for w in words[j]] == words_of(m, L), (j, v)
        assert int(bits[j]) == m.bit_length(), (j, v)
        assert int(budget[j]) == max(0, Q.bit_length() - m.bit_length() - 1), (j, v)


@pytest.mark.parametrize("name,L", [(n, L) for n in CHAINS for L in LIMB_COUNTS])
def test_lexicographic_maximum_is_the_integer_maximum(emu, name, L):
    qs = CHAINS[name][:L]
    Q = prod(qs)
    rng = rng_for(9500 + 10 * list(CHAINS).index(name) + LIMB_COUNTS.index(L))

    def argmax(vals):
        d = np.array([mixed_radix(v, qs) for v in vals], dtype=np.uint64)
        return int(emu.emu_noise_argmax(p(np.ascontiguousarray(d)), len(vals), L))

    for _ in range(20):
        vals = [int(sum(int(rng.integers(0, 1 << 62)) << (62 * k) for k in range(L + 1)) % Q) for _ in range(33)]
        assert vals[argmax(vals)] == max(vals)
    base = Q // 3
    low = [base - base % qs[0] + d for d in (0, 2, 1, 2, 0)]          # differ only in the lowest digit; the maximum twice
    assert [mixed_radix(v, qs)[1:] for v in low] == [mixed_radix(low[0], qs)[1:]] * 5
    assert argmax(low) == 1, "the first maximum is kept"
    assert argmax([5, 5, 5]) == 0
    assert argmax([0, Q - 1, 1]) == 1
    if L > 1:                                                           # a larger low digit must not beat a larger high digit
        assert argmax([qs[0] - 1, qs[0]]) == 1


def test_bit_count_at_word_boundaries(emu):
    for v in [0, 1, (1 << 63), (1 << 64) - 1, 1 << 64, (1 << 127), 1 << 128, (1 << 192) - 1]:
        w = a64(words_of(v, 3))
        assert emu.emu_noise_bits(p(w), 3) == v.bit_length(), v


def test_stand_alone_program_under_ubsan(tmp_path):
    """The same source as a program of its own, built with -fsanitize=undefined (no recovery: a report ends it) and run here."""
    exe = str(tmp_path / "emu_noise_ubsan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEMU_NOISE_MAIN", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "emu", "emu_noise.cpp")])
    for chain in (LADDER, WIDE):
        r = subprocess.run([exe] + [str(q) for q in chain], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        assert r.stdout.startswith("emu_noise ok") and "runtime error" not in r.stderr
