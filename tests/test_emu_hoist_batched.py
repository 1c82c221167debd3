"""The per-thread program of hoist_inner_prod_batched_kernel (phantom-fhe_amd/csrc/pha_hoist_batched.h: host/device functions, the
very source the kernel calls) compiled for the host and compared with Python integers -- no GPU needed.  Harness:
tests/emu/emu_hoist_batched.cpp (test-only): it replays every thread of a toy launch on ordinary host arrays.

Toy launch: N = 1024, three limbs of [Q_l || P] (50, 61 and 61 bits; the last one maps to another row of the prime table than its
own index, as a special limb does), random permutation tables.  Covered: every (BETA, CB) the library instantiates -- the harness
reports the library's CB per (beta, form) -- and the run-time digit loop at beta = 5; plain and weighted; groups of CB - 1, CB, CB + 1
and 2 CB + 1 ciphertexts (the guarded tail); `accumulate` off and on.

Random operands check the indexing (which digit, key, weight and table word meets which).  The capacity test takes every operand
at q - 1 and exactly the elements one launch may carry (63 // beta plain, 63 weighted: 63 products of 61-bit residues on top of a
seed is what a 128-bit sum holds); a wrapped accumulator cannot give the expected word.

Canary words before and after cx -- the region after it is as large as the ciphertexts a full last group would have -- show that
a tail group stores nothing for a ciphertext it does not have; the operands are compared with their copies afterwards."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from util import rng_for

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
N, LIMBS = 1024, 3
CANARY = 0xC0FFEE0DDBA11ABC
MARGIN = 64                      # words (even: the buffers stay 16-byte aligned)
BETAS = [1, 2, 3, 4, 5]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_hoist_batched") / "libemu_hoist_batched.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "emu", "emu_hoist_batched.cpp")])
    L = C.CDLL(out)
    L.emu_hoist_batched_cb.argtypes = [C.c_int, C.c_int]
    L.emu_hoist_batched_cb.restype = C.c_int
    L.emu_hoist_batched.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                    u64p, u64p, u64p, u32p, u64p, u64p, u32p]
    L.emu_hoist_batched.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def moduli():
    """Prime table [50, 61, 50, 61 bits]; the launch's limbs use rows 0, 1 and 3."""
    p50 = [int(p) for p in O.get_primes(1 << 12, 50, 2)]
    p61 = [int(p) for p in O.get_primes(1 << 12, 61, 2)]
    primes = [p50[0], p61[0], p50[1], p61[1]]
    assert [p.bit_length() for p in primes] == [50, 61, 50, 61]
    return primes, [0, 1, 3]


def aligned(words, dtype=np.uint64):
    """Zeroed array whose data starts on a 16-byte boundary."""
    raw = np.zeros(words * np.dtype(dtype).itemsize + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + words * np.dtype(dtype).itemsize].view(dtype)


def per_limb(shape_head, qs, fill):
    """[..., limb, N] array, limb l filled by fill(q_l, shape)."""
    a = aligned(int(np.prod(shape_head)) * len(qs) * N).reshape(tuple(shape_head) + (len(qs), N))
    for l, q in enumerate(qs):
        a[..., l, :] = fill(q, tuple(shape_head) + (N,))
    return a


def operands(rng, primes, rows, beta, n_elts, n_ct, maximal):
    qs = [primes[r] for r in rows]
    if maximal:
        fill = lambda q, shape: np.full(shape, q - 1, dtype=np.uint64)
    else:
        fill = lambda q, shape: rng.integers(0, q, shape, dtype=np.uint64)
    mu = per_limb((n_ct, beta), qs, fill)                       # [n_ct][beta][limb][N]
    keys = per_limb((n_elts, beta, 2), primes, fill)            # [n_elts][beta][2][prime][N]
    w = per_limb((n_elts,), qs, fill)                           # [n_elts][limb][N]
    seed = per_limb((n_ct, 2), qs, fill)                        # [n_ct][2][limb][N]
    tables = aligned(n_elts * N, np.uint32).reshape(n_elts, N)
    for e in range(n_elts):
        tables[e] = rng.permutation(N).astype(np.uint32)
    return mu, keys, w, seed, tables


def expect_random(primes, rows, beta, weighted, accumulate, mu, keys, w, seed, tables):
    """[n_ct][2][limb][N] as Python integers."""
    n_ct, n_elts = mu.shape[0], keys.shape[0]
    out = np.zeros((n_ct, 2, LIMBS, N), dtype=object)
    for l, r in enumerate(rows):
        q = primes[r]
        for b in range(n_ct):
            for c in range(2):
                acc = seed[b, c, l].astype(object) if accumulate else np.zeros(N, dtype=object)
                for e in range(n_elts):
                    part = np.zeros(N, dtype=object)
                    for i in range(beta):
                        part = part + mu[b, i, l][tables[e]].astype(object) * keys[e, i, c, r].astype(object)
                    acc = acc + (part % q) * w[e, l].astype(object) if weighted else acc + part
                out[b, c, l] = acc % q
    return out


def launch(emu, primes, rows, beta, cb, weighted, accumulate, n_ct, mu, keys, w, seed, tables):
    """Runs the first n_ct ciphertexts of the operands; returns cx [n_ct][2][limb][N] after checking the canaries."""
    n_elts = keys.shape[0]
    words = n_ct * 2 * LIMBS * N
    after = cb * 2 * LIMBS * N + MARGIN          # room for the ciphertexts a full last group would have
    buf = aligned(MARGIN + words + after)
    buf[:] = CANARY
    cx = buf[MARGIN:MARGIN + words]
    if accumulate:
        cx[:] = seed[:n_ct].reshape(-1)
    ins = [np.ascontiguousarray(mu[:n_ct]), keys, w, tables]
    assert ins[0].ctypes.data % 16 == 0 and cx.ctypes.data % 16 == 0
    copies = [a.copy() for a in ins]
    pr = np.array(primes, dtype=np.uint64)
    rw = np.array(rows, dtype=np.uint32)
    rc = emu.emu_hoist_batched(beta, cb, int(weighted), N, LIMBS, len(primes), n_elts, n_ct, int(accumulate), cx.ctypes.data_as(u64p),
                               ins[0].ctypes.data_as(u64p), keys.ctypes.data_as(u64p), tables.ctypes.data_as(u32p),
                               w.ctypes.data_as(u64p), pr.ctypes.data_as(u64p), rw.ctypes.data_as(u32p))
    assert rc == 0, f"no instantiation for beta {beta}, CB {cb}"
    assert np.all(buf[:MARGIN] == CANARY), "words before cx were written"
    assert np.all(buf[MARGIN + words:] == CANARY), "words after the last ciphertext of the launch were written (tail group)"
    for a, b in zip(ins, copies):
        assert np.array_equal(a, b), "an operand was written"
    return cx.reshape(n_ct, 2, LIMBS, N).copy()


def group_sizes(cb):
    return sorted({cb - 1, cb, cb + 1, 2 * cb + 1} - {0})


def test_library_group_widths(emu):
    """CB per instantiation: 1, 2 or 4, and 2 where the issue's register budget asks for it."""
    for beta in BETAS:
        for weighted in (0, 1):
            assert emu.emu_hoist_batched_cb(beta, weighted) in (1, 2, 4)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("beta", BETAS)
def test_every_word_equals_python_integers(emu, moduli, beta, weighted):
    primes, rows = moduli
    cb = emu.emu_hoist_batched_cb(beta, int(weighted))
    rng = rng_for(8800 + 2 * beta + int(weighted))
    n_elts, n_max = 3, 2 * cb + 1
    mu, keys, w, seed, tables = operands(rng, primes, rows, beta, n_elts, n_max, maximal=False)
    for accumulate in (False, True):
        want = expect_random(primes, rows, beta, weighted, accumulate, mu, keys, w, seed, tables)
        for n_ct in group_sizes(cb):
            got = launch(emu, primes, rows, beta, cb, weighted, accumulate, n_ct, mu, keys, w, seed, tables)
            bad = np.argwhere(got.astype(object) != want[:n_ct])
            assert bad.size == 0, f"beta {beta}, CB {cb}, {n_ct} ciphertexts, accumulate {accumulate}: first wrong word at " \
                                  f"[ct, poly, limb, k] = {bad[0].tolist()}"


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("beta", BETAS)
def test_full_capacity_at_q_minus_one(emu, moduli, beta, weighted):
    """Every operand q - 1, the seed q - 1, and exactly the elements one launch may carry: 63 // beta (plain: beta products per
    element) or 63 (weighted: one product per element) -- at 61 bits the 128-bit sums are then as full as they ever get."""
    primes, rows = moduli
    cb = emu.emu_hoist_batched_cb(beta, int(weighted))
    n_elts = 63 if weighted else 63 // beta
    rng = rng_for(8900 + 2 * beta + int(weighted))
    n_max = 2 * cb + 1
    mu, keys, w, seed, tables = operands(rng, primes, rows, beta, n_elts, n_max, maximal=True)
    for accumulate in (False, True):
        for n_ct in group_sizes(cb):
            got = launch(emu, primes, rows, beta, cb, weighted, accumulate, n_ct, mu, keys, w, seed, tables)
            for l, r in enumerate(rows):
                q = primes[r]
                s = (q - 1) if accumulate else 0
                if weighted:
                    want = (s + n_elts * ((beta * (q - 1) ** 2 % q) * (q - 1))) % q
                    assert s + n_elts * (q - 1) ** 2 < 1 << 128
                else:
                    want = (s + n_elts * beta * (q - 1) ** 2) % q
                    assert s + n_elts * beta * (q - 1) ** 2 < 1 << 128
                assert np.all(got[:, :, l, :] == np.uint64(want)), \
                    f"beta {beta}, CB {cb}, {n_ct} ciphertexts, accumulate {accumulate}, {q.bit_length()}-bit limb {l}"


def test_other_group_widths_give_the_same_words(emu, moduli):
    """CB is a tuning choice: 1, 2 and 4 ciphertexts per thread give identical words (beta = 3 and the run-time loop)."""
    primes, rows = moduli
    rng = rng_for(8990)
    for beta in (3, 5):
        for weighted in (False, True):
            mu, keys, w, seed, tables = operands(rng, primes, rows, beta, 2, 5, maximal=False)
            ref = launch(emu, primes, rows, beta, 1, weighted, True, 5, mu, keys, w, seed, tables)
            for cb in (2, 4):
                assert np.array_equal(launch(emu, primes, rows, beta, cb, weighted, True, 5, mu, keys, w, seed, tables), ref)
