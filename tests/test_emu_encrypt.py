"""The per-thread programs of the encryption kernels (phantom-fhe_amd/csrc/pha_encrypt.h and apply_epilogue_muladd of pha_ntt_core.h:
host/device functions, the very source the kernels call) compiled for the host and compared with Python integers -- no GPU needed.
Harness: tests/emu/emu_encrypt.cpp (test-only), built once with -ffp-contract=off like the library and once with
-ffp-contract=fast (pha_arith.h states the rule as a pragma, so the flag must not matter).

Load prologue (PRO_SMALL): every limb width of ladder12 (41 .. 61 bits), samples v in {0, +-1, +-21, +-2^16} and random ones in the
reference's range, factors k in {1, 65537, a 59-bit t}: the word is [k v] mod q, canonical, and on an FP64 limb the double the first
round starts from has that value.
Store epilogues (EPI_FWD_MULADD, EPI_FWD_NEG_MULADD with and without the plaintext): x spans the lazy range the last round hands over
-- integers in [0, 8 q) on the integer back end, doubles in (-8 q, 8 q) on the FP64 one -- the factors and the plaintext span [0, q);
the word is [+-(a b + x) + p] mod q and every FP64 intermediate stays inside the bound the header derives (1.375 q + 2, 2.375 q + 2)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from util import primes_of, rng_for

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = C.POINTER(C.c_uint64)
f64p = C.POINTER(C.c_double)
LADDER = [int(q) for q in primes_of("ladder12")[1]]        # 50 .. 41, 51 .. 60 bits, then the two 61-bit special primes
T59 = int(O.get_primes(1 << 12, 59, 3)[2])                  # a 59-bit prime that is no limb of ladder12
FACTORS = [1, 65537, T59]
SAMPLES = [0, 1, -1, 21, -21, 1 << 16, -(1 << 16)]


@pytest.fixture(scope="module", params=["off", "fast"])
def emu(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_encrypt_" + request.param) / "libemu_encrypt.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=" + request.param, "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "emu", "emu_encrypt.cpp")])
    L = C.CDLL(out)
    L.emu_small_sample_max.restype = C.c_uint64
    L.emu_small_lift.argtypes = [C.c_uint64, C.c_uint64, C.c_int, u64p, C.c_size_t, u64p, f64p]
    L.emu_small_lift.restype = None
    L.emu_muladd.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_size_t, u64p, u64p, u64p, u64p, u64p, f64p]
    L.emu_muladd.restype = None
    return L


def p(a):
    return a.ctypes.data_as(u64p)


def a64(v):
    return np.array([int(x) % (1 << 64) for x in v], dtype=np.uint64)


def test_constants(emu):
    assert emu.emu_small_sample_max() == 1 << 16
    assert emu.emu_small_min_prime_bits() == 18          # primes from 2^17: |v| <= 2^16 < q
    assert [emu.emu_muladd_bound(w) for w in (0, 1)] == [1375, 2375]
    assert min(q.bit_length() for q in LADDER) == 41 and max(q.bit_length() for q in LADDER) == 61


@pytest.mark.parametrize("limb", range(len(LADDER)))
def test_small_lift_equals_python_integers(emu, limb):
    q = LADDER[limb]
    fp = q.bit_length() <= 50
    rng = rng_for(9400 + limb)
    v = SAMPLES + [int(x) for x in rng.integers(-21, 22, 64)] + [int(x) for x in rng.integers(-(1 << 16), (1 << 16) + 1, 64)]
    w = a64(v)                                           # two's complement
    for k in FACTORS:
        out, outf = np.zeros(len(v), dtype=np.uint64), np.zeros(len(v), dtype=np.float64)
        emu.emu_small_lift(q, 0 if k == 1 else k, int(fp), p(w), len(v), p(out), outf.ctypes.data_as(f64p))
        want = [(k * x) % q for x in v]
        assert [int(x) for x in out] == want, f"{q.bit_length()} bits, k = {k}"
        if fp:
            assert [int(x) for x in outf] == want and all(float(int(x)) == x for x in outf), f"{q.bit_length()} bits, k = {k}: the FP64 form"
    # a factor of exactly 1 passed as a factor (not as "absent") multiplies by 1
    out, outf = np.zeros(len(v), dtype=np.uint64), np.zeros(len(v), dtype=np.float64)
    emu.emu_small_lift(q, 1, int(fp), p(w), len(v), p(out), outf.ctypes.data_as(f64p))
    assert [int(x) for x in out] == [x % q for x in v]


def lazy_inputs(rng, q, fp, count):
    """x as the last round leaves it: the corners of the lazy range, then random values over all of it."""
    if fp:
        corners = [0, 1, -1, q // 2, -(q // 2), q - 1, -(q - 1), q, 4 * q, -4 * q, (15 * q) // 2, -((15 * q) // 2), 8 * q - 1, -(8 * q - 1)]
        vals = corners + [int(x) for x in rng.integers(-(8 * q - 1), 8 * q, count - len(corners))]
        return vals, np.array([float(x) for x in vals], dtype=np.float64).view(np.uint64)
    corners = [0, 1, q - 1, q, 2 * q - 1, 2 * q, 4 * q - 1, 4 * q, 8 * q - 1]
    vals = corners + [int(x) for x in rng.integers(0, 8 * q, count - len(corners), dtype=np.uint64)]
    return vals, a64(vals)


def operand(rng, q, count):
    """canonical words: the corners of [0, q) in every pairing position, then random"""
    corners = [0, 1, q - 1, q // 2, q - 1, q - 1, 0, q - 1]
    return corners + [int(x) for x in rng.integers(0, q, count - len(corners), dtype=np.uint64)]


@pytest.mark.parametrize("limb", range(len(LADDER)))
def test_muladd_epilogues_equal_python_integers(emu, limb):
    q = LADDER[limb]
    bits = q.bit_length()
    rng = rng_for(9500 + limb)
    count = 512
    back_ends = (1, 0) if bits <= 50 else (0,)           # an FP64 limb also runs the integer program: the same words
    for fp in back_ends:
        for pattern in ("max", "random"):
            xv, xw = lazy_inputs(rng, q, fp, count)
            if pattern == "max":                         # every operand at q - 1, x over its whole range
                a, b, pl = [q - 1] * count, [q - 1] * count, [q - 1] * count
            else:
                a, b, pl = operand(rng, q, count), operand(rng, q, count)[::-1], operand(rng, q, count)
            for neg, has_p in ((0, 0), (1, 0), (1, 1)):
                out, peak = np.zeros(count, dtype=np.uint64), np.zeros(2, dtype=np.float64)
                emu.emu_muladd(q, fp, neg, has_p, count, p(xw), p(a64(a)), p(a64(b)), p(a64(pl)), p(out), peak.ctypes.data_as(f64p))
                if neg:
                    want = [(-(ai * bi + xi) + (pi if has_p else 0)) % q for ai, bi, xi, pi in zip(a, b, xv, pl)]
                else:
                    want = [(ai * bi + xi) % q for ai, bi, xi in zip(a, b, xv)]
                got = [int(v) for v in out]
                bad = [i for i in range(count) if got[i] != want[i]]
                assert not bad, f"{bits} bits, q = {q}, {'fp64' if fp else 'integer'} program, neg {neg}, plain {has_p}, {pattern}: " \
                                f"{len(bad)} words differ, first x = {xv[bad[0]]}, a = {a[bad[0]]}, b = {b[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"
                if fp:
                    s_bound = emu.emu_muladd_bound(0) * q / 1000 + 2
                    r_bound = (emu.emu_muladd_bound(1) if has_p else emu.emu_muladd_bound(0)) * q / 1000 + 2
                    assert r_bound < 2 ** 52.6
                    assert peak[0] <= s_bound, f"{bits} bits: |a b + x| reached {peak[0]} > 1.375 q + 2 = {s_bound}"
                    assert peak[1] <= r_bound, f"{bits} bits: |r| reached {peak[1]} > {r_bound}"
                    assert peak[0] > 0 and peak[1] > 0, "the probe saw nothing"
