"""The per-thread program of plain_sum_kernel (phantom-fhe_amd/csrc/pha_plain_sum.h: host/device functions, the very source the
kernel calls) compiled for the host and compared with Python integers -- no GPU needed.  Harness: tests/emu/emu_plain_sum.cpp
(test-only), built once with -ffp-contract=off like the library and once with -ffp-contract=fast (the header states the rule as a
pragma, so the flag must not matter).

One "thread" is two adjacent coefficients of both polynomials: four sums acc + sum over k of plain[k] * ct[k].  Moduli at every bit
length from 36 to 50 run the FP64 back end (and the integer one, which must give the same words), 51 to 61 the integer back end.
Term counts sit around each limb's own flush interval T (T - 1, T, T + 1, 2 T, 2 T + 1), plus 1 and 1000.

The second test checks the derivation itself, not only its outcome: the value every accumulator holds just before it is reduced
stays inside the bound the header's comment derives -- (q - 1) + T (q - 1)^2 < 2^128 on the integer side (reached exactly by
operands that are all q - 1), q (1 + 0.875 T) <= 1.4 * 2^52 on the FP64 side -- so a too-generous T cannot pass by luck on random
data."""
import ctypes as C
import os
import subprocess
from operator import mul

import numpy as np
import pytest

from oracle import oracle as O
from util import rng_for

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = C.POINTER(C.c_uint64)
FP_BITS = list(range(36, 51))
INT_BITS = list(range(51, 62))
CAP = 1 << 16
PATTERNS = ["max", "zero", "alternating", "random", "half"]


@pytest.fixture(scope="module", params=["off", "fast"])
def emu(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_plain_sum_" + request.param) / "libemu_plain_sum.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=" + request.param, "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "emu", "emu_plain_sum.cpp")])
    L = C.CDLL(out)
    L.emu_plain_sum_per.argtypes = [C.c_uint64, C.c_int]
    L.emu_plain_sum_per.restype = C.c_uint32
    L.emu_plain_sum.argtypes = [C.c_uint64, C.c_int, C.c_uint32, u64p, u64p, u64p, u64p, u64p, u64p]
    L.emu_plain_sum.restype = None
    return L


def p(a):
    return a.ctypes.data_as(u64p)


def prime_of(bits):
    q = int(O.get_primes(1 << 12, bits, 1)[0])
    assert q.bit_length() == bits
    return q


def per_int(bits):
    """T = 2^(128 - 2 b), capped: (q - 1) + T (q - 1)^2 < 2^128 for q < 2^b."""
    return min(1 << (128 - 2 * bits), CAP)


def per_fp(bits):
    """T = floor((56 * 2^(52 - b) - 40) / 35), capped: 2^b (1 + 0.875 T) <= 1.4 * 2^52."""
    return min((56 * (1 << (52 - bits)) - 40) // 35, CAP)


def term_counts(t):
    return sorted({1, 1000, t - 1, t, t + 1, 2 * t, 2 * t + 1} - {0})


def operands(pattern, q, terms, rng):
    """plain, ct0, ct1: [terms][2] canonical words."""
    shape = (terms, 2)
    if pattern == "max":
        return tuple(np.full(shape, q - 1, dtype=np.uint64) for _ in range(3))
    if pattern == "zero":
        return tuple(np.zeros(shape, dtype=np.uint64) for _ in range(3))
    if pattern == "alternating":            # 0 / q - 1 by term and by coefficient, out of step between the operands
        k = np.arange(terms)[:, None] + np.arange(2)[None, :]
        a = np.where(k % 2 == 0, q - 1, 0).astype(np.uint64)
        b = np.where(k % 3 != 0, q - 1, 0).astype(np.uint64)
        return np.full(shape, q - 1, dtype=np.uint64), a, b
    if pattern == "half":                   # every reduced product is (q - 1) / 2 or -(q - 1) / 2: the centred sums run one way
        return (np.ones(shape, dtype=np.uint64), np.full(shape, (q - 1) // 2, dtype=np.uint64),
                np.full(shape, (q + 1) // 2, dtype=np.uint64))
    return tuple(rng.integers(0, q, shape, dtype=np.uint64) for _ in range(3))


def expect(q, plain, ct0, ct1, acc):
    out = []
    for c, a in ((ct0, acc[:2]), (ct1, acc[2:])):
        for j in range(2):
            out.append((int(a[j]) + sum(map(mul, plain[:, j].tolist(), c[:, j].tolist()))) % q)
    return out


def run(emu, q, fp, plain, ct0, ct1, acc):
    out, peak = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    plain, ct0, ct1 = (np.ascontiguousarray(x) for x in (plain, ct0, ct1))
    emu.emu_plain_sum(q, fp, plain.shape[0], p(plain), p(ct0), p(ct1), p(acc) if acc is not None else None, p(out), p(peak))
    return [int(v) for v in out], peak


def check_peak(q, bits, fp, terms, peak, worst):
    t = per_fp(bits) if fp else per_int(bits)
    assert int(peak[3]) == 4 * -(-terms // t), "one probe per accumulator and interval"
    if fp:
        bound = q * (8 + 7 * t) // 8                        # q (1 + 0.875 T)
        assert bound <= 14 * (1 << 52) // 10, (bits, t)     # the derivation's ceiling, 1.4 * 2^52
        assert int(peak[2]) <= bound, f"{bits} bits, {terms} terms: |sum| reached {int(peak[2])} > q (1 + 0.875 T) = {bound}"
    else:
        bound = (q - 1) + t * (q - 1) ** 2
        assert bound < 1 << 128, (bits, t)
        got = (int(peak[1]) << 64) | int(peak[0])
        assert got <= bound, f"{bits} bits, {terms} terms: accumulator reached {got} > {bound}"
        if worst:                                           # all q - 1 with acc q - 1: the bound is reached exactly, unwrapped
            assert got == (q - 1) + min(t, terms) * (q - 1) ** 2, (bits, terms, got)


@pytest.mark.parametrize("bits", FP_BITS + INT_BITS)
def test_program_equals_python_integers(emu, bits):
    q = prime_of(bits)
    fp_limb = bits <= 50
    assert emu.emu_plain_sum_per(q, 0) == per_int(bits)
    if fp_limb:
        assert emu.emu_plain_sum_per(q, 1) == per_fp(bits)
    # the limb's own back end around its own T; the integer back end on an FP64 limb at the same counts (bit-identical words)
    counts = term_counts(per_fp(bits) if fp_limb else per_int(bits))
    rng = rng_for(7300 + bits)
    for terms in counts:
        for pattern in PATTERNS:
            plain, ct0, ct1 = operands(pattern, q, terms, rng)
            for acc in (None, np.full(4, q - 1, dtype=np.uint64)):
                want = expect(q, plain, ct0, ct1, acc if acc is not None else [0] * 4)
                for fp in ((1, 0) if fp_limb else (0,)):
                    got, peak = run(emu, q, fp, plain, ct0, ct1, acc)
                    assert got == want, f"{bits} bits, q = {q}, {'fp64' if fp else 'integer'} back end, {terms} terms, {pattern}, " \
                                        f"acc {'q - 1' if acc is not None else 'none'}: got {got}, want {want}"
                    check_peak(q, bits, fp, terms, peak, worst=pattern == "max" and acc is not None)


def test_stated_terms_per_flush():
    """The figures the kernel's comment and DESIGN.md state."""
    assert [per_int(b) for b in (61, 60, 50, 49, 40)] == [64, 256, CAP, CAP, CAP]
    assert [per_fp(b) for b in (50, 49, 40)] == [5, 11, 6552]
    for b in range(20, 51):     # one more term would leave the derivation's ceiling (where the cap does not bind)
        t = (56 * (1 << (52 - b)) - 40) // 35
        assert 10 * (8 + 7 * t) <= 8 * 14 * (1 << (52 - b)) < 10 * (8 + 7 * (t + 1))
    for b in range(51, 65):
        t = 1 << (128 - 2 * b)
        assert (2 ** b - 2) + t * (2 ** b - 2) ** 2 < 2 ** 128 <= (2 ** b - 2) + 2 * t * (2 ** b - 2) ** 2


@pytest.mark.parametrize("bits", FP_BITS + INT_BITS)
def test_magnitude_before_each_flush_stays_inside_the_derived_bound(emu, bits):
    """Long sums (several intervals) of the operands that push an accumulator furthest: all q - 1 with an acc of q - 1 for the
    128-bit integers (the bound is met exactly, so a wrapped accumulator cannot hide), one-signed halves and random words for the
    doubles."""
    q = prime_of(bits)
    fp_limb = bits <= 50
    t = per_fp(bits) if fp_limb else per_int(bits)
    terms = 3 * t + 2
    rng = rng_for(7400 + bits)
    acc = np.full(4, q - 1, dtype=np.uint64)
    for pattern in ("max", "half", "random", "alternating"):
        plain, ct0, ct1 = operands(pattern, q, terms, rng)
        got, peak = run(emu, q, 1 if fp_limb else 0, plain, ct0, ct1, acc)
        check_peak(q, bits, 1 if fp_limb else 0, terms, peak, worst=pattern == "max")
        assert got == expect(q, plain, ct0, ct1, acc)
    if fp_limb:
        # the one-signed halves come within one term of the per-term allowance: the sum after T terms is acc + T (q - 1) / 2
        plain, ct0, ct1 = operands("half", q, t, rng)
        _, peak = run(emu, q, 1, plain, ct0, ct1, acc)
        assert int(peak[2]) == (q - 1) + t * ((q - 1) // 2)
