"""The per-thread programs of the decryption kernels (phantom-fhe_amd/csrc/pha_decrypt.h: host/device functions, the very source the
kernels call) and their tables (pha_rns_tables.h) compiled for the host and compared with Python integers -- no GPU needed.
Harness: tests/emu/emu_decrypt.cpp (test-only), built once with -ffp-contract=off like the library and once with
-ffp-contract=fast (pha_arith.h states the rule as a pragma, so the flag must not matter).

Phase program: one "thread" is two adjacent coefficients of one limb of a group of G <= 4 ciphertexts of k polynomials.  Every
width of ladder12 (41 .. 61 bits), k = 2, 3, 4 (2 and 3 in the instantiation the kernel launches for them and in the run-time
loop), and k around each limb's first flush (k - 1 = T and T + 1 terms) where that is at most 300; the words must equal Python's and
the value every accumulator holds just before it is reduced must stay inside the bound the header derives.

Scale-and-round program: against floor(t x / Q + 1/2) mod t in Python integers for uniform x; a coefficient is excluded only where
|frac(t x / Q) - 1/2| < L * 2^-14 (the header's margin), and at most 1 % of a case may be excluded (uniform x puts an expected
2 * L * 2^-14 <= 0.18 % there, so the cap can only trip on a broken margin).  The fraction sum itself is held against exact
rationals within the header's L (2^-15 + 2^-20).  Constructed x = Q - 1 and t x / Q = t - 0.3 give 0, never t."""
import ctypes as C
import os
import subprocess
from fractions import Fraction
from math import prod

import numpy as np
import pytest

from oracle import oracle as O
from util import primes_of, rng_for

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = C.POINTER(C.c_uint64)
f64p = C.POINTER(C.c_double)
CAP = 1 << 16
LADDER = [int(q) for q in primes_of("ladder12")[1]]        # 50 .. 41, 51 .. 60 bits, then the two 61-bit special primes
WIDE = LADDER[::-1]                                         # 61-bit limbs first: the 31-bit split
T59 = int(O.get_primes(1 << 12, 59, 3)[2])                  # a 59-bit prime that is no limb of ladder12
PLAIN_MODULI = [65537, 1032193, T59]
LIMB_COUNTS = [1, 2, 4, 14]
COUNT = 2048


@pytest.fixture(scope="module", params=["off", "fast"])
def emu(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_decrypt_" + request.param) / "libemu_decrypt.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=" + request.param, "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "emu", "emu_decrypt.cpp")])
    L = C.CDLL(out)
    L.emu_phase_group.restype = C.c_int
    L.emu_phase.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, u64p, u64p, u64p, u64p]
    L.emu_phase.restype = None
    L.emu_round_tables.argtypes = [u64p, C.c_uint32, C.c_uint64, f64p, u64p]
    L.emu_round_tables.restype = C.c_int
    L.emu_scale_round.argtypes = [u64p, C.c_uint32, C.c_uint64, u64p, C.c_size_t, u64p, f64p]
    L.emu_scale_round.restype = None
    L.emu_mod_t_tables.argtypes = [u64p, C.c_uint32, C.c_uint64, u64p, u64p]
    L.emu_mod_t_tables.restype = C.c_uint64
    L.emu_mod_t.argtypes = [u64p, C.c_uint32, C.c_uint64, C.c_uint64, u64p, C.c_size_t, u64p]
    L.emu_mod_t.restype = None
    return L


def p(a):
    return a.ctypes.data_as(u64p)


def a64(v):
    return np.array([int(x) for x in v], dtype=np.uint64)


# ---- phase ----------------------------------------------------------------------------------------------------------------------
def per_int(bits):
    return min(1 << (128 - 2 * bits), CAP)


def per_fp(bits):
    return min((56 * (1 << (52 - bits)) - 40) // 35, CAP)


def phase_sizes(per):
    """k = 2, 3, 4 and, where it stays short, the largest k before the first flush (k - 1 = T terms) and one past it."""
    ks = [2, 3, 4]
    if per + 2 <= 300:
        ks += [per + 1, per + 2]
    return ks


def run_phase(emu, q, fp, G, k, specialised, with_c0, ct, sk):
    out, peak = np.zeros(2 * G, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    emu.emu_phase(q, fp, G, k, specialised, int(with_c0), p(np.ascontiguousarray(ct)), p(np.ascontiguousarray(sk)), p(out), p(peak))
    return out.reshape(G, 2), peak


def phase_expect(q, k, with_c0, ct, sk):
    G = ct.shape[0]
    want = np.zeros((G, 2), dtype=np.uint64)
    for g in range(G):
        for j in range(2):
            v = int(ct[g, 0, j]) if with_c0 else 0
            v += sum(int(ct[g, i, j]) * int(sk[i - 1, j]) for i in range(1, k))
            want[g, j] = v % q
    return want


def check_phase_peak(q, bits, fp, G, k, with_c0, peak, worst):
    t = per_fp(bits) if fp else per_int(bits)
    assert int(peak[3]) == 2 * G * -(-(k - 1) // t), "one probe per accumulator and interval"
    if fp:
        bound = q * (8 + 7 * t) // 8
        assert bound <= 14 * (1 << 52) // 10, (bits, t)
        assert int(peak[2]) <= bound, f"{bits} bits, k = {k}: |sum| reached {int(peak[2])} > q (1 + 0.875 T) = {bound}"
    else:
        bound = (q - 1) + t * (q - 1) ** 2
        assert bound < 1 << 128, (bits, t)
        got = (int(peak[1]) << 64) | int(peak[0])
        assert got <= bound, f"{bits} bits, k = {k}: accumulator reached {got} > {bound}"
        if worst and with_c0:       # every word q - 1: the bound is reached exactly, so a wrapped accumulator cannot hide
            assert got == (q - 1) + min(t, k - 1) * (q - 1) ** 2, (bits, k, got)


@pytest.mark.parametrize("limb", range(len(LADDER)))
def test_phase_program_equals_python_integers(emu, limb):
    q = LADDER[limb]
    bits = q.bit_length()
    fp_limb = bits <= 50
    assert emu.emu_phase_group() == 4
    rng = rng_for(9100 + limb)
    back_ends = (1, 0) if fp_limb else (0,)      # an FP64 limb also runs the integer program: the same words
    for fp in back_ends:
        for k in phase_sizes(per_fp(bits) if fp else per_int(bits)):
            for G in (1, 2, 3, 4):
                for pattern in ("max", "random"):
                    if pattern == "max":
                        ct, sk = np.full((G, k, 2), q - 1, dtype=np.uint64), np.full((k - 1, 2), q - 1, dtype=np.uint64)
                    else:
                        ct, sk = rng.integers(0, q, (G, k, 2), dtype=np.uint64), rng.integers(0, q, (k - 1, 2), dtype=np.uint64)
                    for with_c0 in (True, False):
                        want = phase_expect(q, k, with_c0, ct, sk)
                        for specialised in ((1, 0) if k <= 3 else (0,)):
                            got, peak = run_phase(emu, q, fp, G, k, specialised, with_c0, ct, sk)
                            assert np.array_equal(got, want), \
                                f"{bits} bits, q = {q}, {'fp64' if fp else 'integer'} program, G = {G}, k = {k}, {pattern}, " \
                                f"c0 {'kept' if with_c0 else 'dropped'}, specialised {specialised}: got {got.tolist()}, want {want.tolist()}"
                            check_phase_peak(q, bits, fp, G, k, with_c0, peak, worst=pattern == "max")


def test_phase_flush_figures(emu):
    """The figures pha_decrypt.h states, asked of the header's own functions: no flush up to k = 65 at 61 bits and k = 257 at 60; 5
    and 11 terms on FP64 limbs of 50 and 49 bits; every ladder width agrees with the formulas this file derives its cases from."""
    emu.emu_phase_per.argtypes, emu.emu_phase_per.restype = [C.c_uint64, C.c_int], C.c_uint32
    by_bits = {q.bit_length(): q for q in LADDER}
    assert [emu.emu_phase_per(by_bits[b], 0) for b in (61, 60)] == [64, 256]
    assert [emu.emu_phase_per(by_bits[b], 1) for b in (50, 49)] == [5, 11]
    for q in LADDER:
        assert emu.emu_phase_per(q, 0) == per_int(q.bit_length())
        if q.bit_length() <= 50:
            assert emu.emu_phase_per(q, 1) == per_fp(q.bit_length())
    emu.emu_decrypt_max_limbs.restype = C.c_uint32
    assert emu.emu_decrypt_max_limbs() == 64
    assert 65 in phase_sizes(per_int(61)) and 66 in phase_sizes(per_int(61))
    assert 257 in phase_sizes(per_int(60)) and 258 in phase_sizes(per_int(60))


# ---- scale-and-round ------------------------------------------------------------------------------------------------------------
def crt_weights(primes):
    Q = prod(primes)
    return Q, [(Q // q) * pow(Q // q, -1, q) for q in primes]


def compose(x, primes):
    """x [L][count] -> Python integers in [0, Q)."""
    Q, w = crt_weights(primes)
    cols = [[int(v) for v in row] for row in x]
    return Q, [sum(c[j] * wi for c, wi in zip(cols, w)) % Q for j in range(len(cols[0]))]


def residues(values, primes):
    return np.array([[v % q for v in values] for q in primes], dtype=np.uint64)


def scale_round(emu, primes, t, x):
    x = np.ascontiguousarray(x)
    out, fsum = np.zeros(x.shape[1], dtype=np.uint64), np.zeros(x.shape[1], dtype=np.float64)
    emu.emu_scale_round(p(a64(primes)), len(primes), t, p(x), x.shape[1], p(out), fsum.ctypes.data_as(f64p))
    return out, fsum


def round_tables(emu, primes, t):
    L = len(primes)
    frac, itab = np.zeros(2 * L, dtype=np.float64), np.zeros(2 * L, dtype=np.uint64)
    h = emu.emu_round_tables(p(a64(primes)), L, t, frac.ctypes.data_as(f64p), p(itab))
    return h, frac, itab


def exact_tables(primes, t):
    """h and, per limb, the big integers A_i = t [qhat_i^-1]_{q_i}, B_i = t [qhat_i^-1 2^h]_{q_i}."""
    Q = prod(primes)
    h = (max(q.bit_length() for q in primes) + 1) // 2
    ab = []
    for q in primes:
        inv = pow(Q // q, -1, q)
        ab.append((q, t * inv, t * (inv * (1 << h) % q)))
    return h, ab


CASES = [(name, t, L) for name in ("ladder", "wide") for t in PLAIN_MODULI for L in LIMB_COUNTS]


@pytest.mark.parametrize("name,t,L", CASES)
def test_scale_round_equals_exact_rounding(emu, name, t, L):
    primes = (LADDER if name == "ladder" else WIDE)[:L]
    rng = rng_for(9200 + 100 * PLAIN_MODULI.index(t) + 10 * LIMB_COUNTS.index(L) + (name == "wide"))
    x = np.stack([rng.integers(0, q, COUNT, dtype=np.uint64) for q in primes])
    got, fsum = scale_round(emu, primes, t, x)
    assert int(got.max()) < t, "a word equal to t (or above) was written"
    Q, X = compose(x, primes)
    excluded, bad = 0, []
    for j, v in enumerate(X):
        r = t * v % Q                                    # frac(t x / Q) = r / Q
        if abs(2 * r - Q) * (1 << 14) < 2 * L * Q:       # |frac - 1/2| < L * 2^-14
            excluded += 1
            continue
        want = (2 * t * v + Q) // (2 * Q) % t
        if int(got[j]) != want:
            bad.append((j, int(got[j]), want))
    print(f"{name} t = {t} L = {L}: {excluded} of {COUNT} coefficients excluded")
    assert excluded * 100 <= COUNT, f"{excluded} of {COUNT} coefficients inside the margin: more than 1 %"
    assert not bad, f"{len(bad)} coefficients differ outside the margin, first (index, got, want): {bad[:3]}"
    # the fraction sum against exact rationals, on the first coefficients: the header's L (2^-15 + 2^-20)
    h, ab = exact_tables(primes, t)
    bound = L * (Fraction(1, 1 << 15) + Fraction(1, 1 << 20))
    for j in range(48):
        f = Fraction(0)
        for i, (q, a, b) in enumerate(ab):
            w = int(x[i, j])
            f += (w & ((1 << h) - 1)) * Fraction(a % q, q) + (w >> h) * Fraction(b % q, q)
        assert abs(Fraction(float(fsum[j])) - f) <= bound, (j, float(fsum[j]), float(f))
        assert (f - Fraction(t * X[j] % Q, Q)).denominator == 1, "the fraction sum is t x / Q up to an integer"


@pytest.mark.parametrize("name,t,L", CASES)
def test_scale_round_never_writes_t(emu, name, t, L):
    """x = Q - 1 (t x / Q = t - t / Q: rounds to t) and x with t x / Q = t - 0.3 give 0 -- the reference's llround can store t."""
    primes = (LADDER if name == "ladder" else WIDE)[:L]
    Q = prod(primes)
    near = ((10 * t - 3) * Q + 5 * t) // (10 * t)        # round((t - 0.3) Q / t)
    values = [Q - 1, near, 0, 1]
    got, _ = scale_round(emu, primes, t, residues(values, primes))
    if 2 * t < Q:                                        # t / Q < 1/2: both round up to t
        assert [int(v) for v in got[:2]] == [0, 0], got
    for v, g in zip(values, got):
        assert int(g) == (2 * t * v + Q) // (2 * Q) % t
        assert int(g) < t


# ---- tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,t,L", CASES)
def test_tables_equal_python_big_integers(emu, name, t, L):
    primes = (LADDER if name == "ladder" else WIDE)[:L]
    Q = prod(primes)
    h, frac, itab = round_tables(emu, primes, t)
    want_h, ab = exact_tables(primes, t)
    assert h == want_h and h <= 31
    for i, (q, a, b) in enumerate(ab):
        for k, v in enumerate((a, b)):
            assert int(itab[2 * i + k]) == v // q % t, (i, k)
            assert abs(Fraction(float(frac[2 * i + k])) - Fraction(v % q, q)) <= Fraction(1, 1 << 52), (i, k)
    hat_inv, mat = np.zeros(2 * L, dtype=np.uint64), np.zeros(L, dtype=np.uint64)
    q_mod_t = emu.emu_mod_t_tables(p(a64(primes)), L, t, p(hat_inv), p(mat))
    assert q_mod_t == Q % t
    for i, q in enumerate(primes):
        inv = pow(Q // q, -1, q)
        assert (int(hat_inv[2 * i]), int(hat_inv[2 * i + 1])) == (inv, (inv << 64) // q)
        assert int(mat[i]) == (Q // q) % t


# ---- the bgv tail ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,t,L", [c for c in CASES if c[1] != 1032193])
def test_mod_t_conversion_equals_the_centred_value(emu, name, t, L):
    """exact_convert_array delivers the centred representative of x modulo t (its rounded quotient picks x or x - Q), except where
    x / Q is within the double sum's error of 1/2; then times the inverse correction factor."""
    primes = (LADDER if name == "ladder" else WIDE)[:L]
    rng = rng_for(9300 + 100 * PLAIN_MODULI.index(t) + 10 * LIMB_COUNTS.index(L) + (name == "wide"))
    x = np.stack([rng.integers(0, q, 512, dtype=np.uint64) for q in primes])
    Q, X = compose(x, primes)
    for factor in (1, 3, t - 1):
        out = np.zeros(x.shape[1], dtype=np.uint64)
        emu.emu_mod_t(p(a64(primes)), L, t, factor, p(np.ascontiguousarray(x)), x.shape[1], p(out))
        assert int(out.max()) < t
        for j, v in enumerate(X):
            if abs(2 * v - Q) * (1 << 40) < Q:
                continue
            centred = v - Q if 2 * v > Q else v
            assert int(out[j]) == centred * factor % t, (j, factor)
