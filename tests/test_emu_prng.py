"""The per-thread programs of the seeded samplers (phantom-fhe_amd/csrc/pha_prng.h: host/device functions, the very source the
kernels call) compiled for the host with g++ and compared with the numpy restatement (tests/prng_restatement.py) -- no GPU needed.
Harness: tests/emu/emu_prng.cpp (test-only).

Blocks (nonces on both sides of 2^16, 2^32, up to 2^64 - 1), the quarter-round's hand-worked value, the three value rules, the
acceptance bound and the exactness of the stored reduction for every prime of ladder12 (41 .. 61 bits) and reject12, and full
uniform groups of reject12 (where 5.88 % of the words are redrawn) with the number of blocks each group drew."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import prng_restatement as R
from util import primes_of

HERE = os.path.dirname(os.path.abspath(__file__))
u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
LADDER = [int(q) for q in primes_of("ladder12")[1]]
REJECT = [int(q) for q in R.REJECT12[1]]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_prng") / "libemu_prng.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "emu", "emu_prng.cpp")])
    L = C.CDLL(out)
    L.emu_quarter_round.argtypes = [u32p]
    L.emu_blocks.argtypes = [u8p, u64p, C.c_size_t, u32p]
    L.emu_small.argtypes = [u8p, C.c_int, C.c_uint64, C.c_size_t, u64p, u64p]
    L.emu_max_multiple.argtypes = [C.c_uint64]
    L.emu_max_multiple.restype = C.c_uint64
    L.emu_reduce.argtypes = [C.c_uint64, u64p, C.c_size_t, u64p]
    L.emu_uniform.argtypes = [u8p, u64p, C.c_size_t, C.c_size_t, u64p, u32p]
    for f in (L.emu_quarter_round, L.emu_blocks, L.emu_small, L.emu_reduce, L.emu_uniform):
        f.restype = None
    return L


def p(a, t):
    return a.ctypes.data_as(t)


def seed_of(tag):
    return np.ascontiguousarray(R.STAT_SEED_ARRAY if tag is None else R.seed_bytes(tag))


def test_constants_and_quarter_round(emu):
    assert emu.emu_prng_seed_bytes() == 64 and emu.emu_prng_group_words() == 8
    v = np.array([1, 0, 0, 0], dtype=np.uint32)
    emu.emu_quarter_round(p(v, u32p))
    assert [int(x) for x in v] == [0x08008145, 0x00000080, 0x00010200, 0x20500000]


@pytest.mark.parametrize("tag", [None, 0, 1])
def test_blocks_equal_the_restatement(emu, tag):
    seed = seed_of(tag)
    rng = np.random.default_rng(77)
    nonces = np.concatenate([np.array([0, 1, 7, 65535, 65536, (1 << 17) - 1, 1 << 17, (1 << 32) - 1, 1 << 32, (1 << 64) - 1], dtype=np.uint64),
                             rng.integers(0, 1 << 63, 200, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                             np.arange(4096, dtype=np.uint64)])
    out = np.zeros((nonces.size, 16), dtype=np.uint32)
    emu.emu_blocks(p(seed, u8p), p(nonces, u64p), nonces.size, p(out, u32p))
    assert np.array_equal(out, R.block(seed, nonces))
    zero = np.zeros(64, dtype=np.uint8)
    emu.emu_blocks(p(zero, u8p), p(np.zeros(1, dtype=np.uint64), u64p), 1, p(out, u32p))
    assert not out[0].any()                                   # all-zero input, all-zero output


@pytest.mark.parametrize("which,fn", [(0, R.ternary_signed), (1, R.error_signed)])
def test_value_rules_equal_the_restatement(emu, which, fn):
    n = 4096
    for tag in (None, 5):
        seed = seed_of(tag)
        want = fn(seed, n)
        for q in (LADDER[0], LADDER[-1], REJECT[0]):
            s, r = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
            emu.emu_small(p(seed, u8p), which, q, n, p(s, u64p), p(r, u64p))
            assert np.array_equal(s.view(np.int64), want)
            assert np.array_equal(r, R.residues(want, [q])[0])
        assert np.max(np.abs(want)) <= (1 if which == 0 else 21)


@pytest.mark.parametrize("q", LADDER + REJECT)
def test_acceptance_bound_and_reduction_are_exact(emu, q):
    bound = R.max_multiple(q)
    assert emu.emu_max_multiple(q) == bound
    rng = np.random.default_rng(q % (1 << 32))
    corners = [0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, bound - 1, bound, bound + 1, (1 << 64) - 1, (1 << 63), (1 << 63) - 1]
    words = np.array(corners + [((1 << 64) // q) * q - 1, ((1 << 64) // q) * q] + [k * q for k in (3, 15, 16) if k * q < (1 << 64)],
                     dtype=np.uint64)
    words = np.concatenate([words, rng.integers(0, 1 << 63, 512, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 512, dtype=np.uint64)])
    out = np.zeros(words.size, dtype=np.uint64)
    emu.emu_reduce(q, p(words, u64p), words.size, p(out, u64p))
    assert [int(x) for x in out] == [int(w) % q for w in words], f"{q.bit_length()} bits"


@pytest.mark.parametrize("name", ["reject12", "ladder12"])
def test_uniform_groups_equal_the_restatement(emu, name):
    primes = REJECT if name == "reject12" else LADDER[:4] + LADDER[-2:]
    n = 4096
    for tag in (None, 6):
        seed = seed_of(tag)
        log = []
        want = R.uniform(seed, primes, n, log)
        ps = np.array(primes, dtype=np.uint64)
        out, tries = np.zeros((len(primes), n), dtype=np.uint64), np.zeros((len(primes), n // 8), dtype=np.uint32)
        emu.emu_uniform(p(seed, u8p), p(ps, u64p), len(primes), n, p(out, u64p), p(tries, u32p))
        assert np.array_equal(out, want)
        drawn = np.ones((len(primes), n // 8), dtype=np.int64)
        for y, j, _, r in log:
            drawn[y, j] += r
        assert np.array_equal(tries, drawn)
        if name == "reject12":
            assert len(log) > 300 and any(r >= 2 for _, _, _, r in log)
        else:
            assert not log                                    # primes just below a power of two: about 10^-14 of the words
