"""The per-thread program of hoist_bsgs_batched_kernel (phantom-fhe_amd/csrc/pha_hoist_bsgs_batched.h: host/device functions, the
very source the kernel calls) compiled for the host and compared with Python integers -- no GPU needed.  Harness:
tests/emu/emu_hoist_bsgs_batched.cpp (test-only): it replays every thread of a toy launch on ordinary host arrays.  It is built
twice, with -ffp-contract=off and -ffp-contract=fast: the FP body must not depend on the flag.

Toy launch: N = 1024, random permutation tables, two data limbs -- 40 bits (the FP body) and 60 bits (the integer body) -- and one
61-bit special limb that maps to another row of the prime table than its own index.  Covered: every (NG, CB, BETA) the library
instantiates (the harness reports the library's CB per (BETA, NG)); keyed baby steps with an identity baby step in first and in
middle position; the P c0 / P c1 terms on the data limbs and nothing on the special limb; groups of CB - 1, CB, CB + 1 and 2 CB + 1
ciphertexts (the guarded tail); a non-zero first accumulator g0; a missing weight through the zero plane.

The capacity test takes every operand at q - 1 and 62 baby entries, the single entry's limit for 61-bit primes (nb + 1 <= 63): the
128-bit sums are as full as they ever get and the FP limb goes through seven re-centrings; a wrapped sum or an inexact double cannot
give the expected word.

Canary words before acc, in the accumulators below g0 and after acc -- that region is as large as the ciphertexts a full last group
would have -- show that a tail group stores nothing for a ciphertext it does not have; the operands are compared with their copies
afterwards."""
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
u8p = C.POINTER(C.c_uint8)
N, LIMBS, QL = 1024, 3, 2
CANARY = 0xC0FFEE0DDBA11ABC
MARGIN = 64
BETAS = [1, 2, 3, 4]
NGS = [1, 2, 4, 8, 16]
G0 = 1                           # first accumulator of the launch: the accumulators below it stay untouched


@pytest.fixture(scope="module", params=["off", "fast"], ids=["contract_off", "contract_fast"])
def emu(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_hoist_bsgs_batched_" + request.param) / "libemu_hoist_bsgs_batched.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-ffp-contract=" + request.param, "-fPIC", "-shared",
                           "-o", out, os.path.join(HERE, "emu", "emu_hoist_bsgs_batched.cpp")])
    L = C.CDLL(out)
    L.emu_hoist_bsgs_batched_cb.argtypes = [C.c_int, C.c_int]
    L.emu_hoist_bsgs_batched_cb.restype = C.c_int
    L.emu_hoist_bsgs_batched.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_uint32] * 8 + \
        [u64p, u64p, u64p, u8p, u32p, u64p, u8p, u64p, u64p, u32p, u64p]
    L.emu_hoist_bsgs_batched.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def moduli():
    """Prime table [40, 60, 50, 61 bits]; the launch's limbs use rows 0, 1 (data) and 3 (special)."""
    primes = [int(O.get_primes(1 << 12, b, 1)[0]) for b in (40, 60, 50, 61)]
    assert [p.bit_length() for p in primes] == [40, 60, 50, 61]
    return primes, [0, 1, 3]


def per_limb(shape_head, qs, fill):
    """[..., limb, N] array, limb l filled by fill(q_l, shape)."""
    a = np.zeros(tuple(shape_head) + (len(qs), N), dtype=np.uint64)
    for l, q in enumerate(qs):
        a[..., l, :] = fill(q, tuple(shape_head) + (N,))
    return a


def operands(rng, primes, rows, beta, nb, g_total, n_ct, maximal):
    qs = [primes[r] for r in rows]
    if maximal:
        fill = lambda q, shape: np.full(shape, q - 1, dtype=np.uint64)
    else:
        fill = lambda q, shape: rng.integers(0, q, shape, dtype=np.uint64)
    mu = per_limb((n_ct, beta), qs, fill)                       # [n_ct][beta][limb][N]
    keys = per_limb((nb, beta, 2), primes, fill)                # [nb][beta][2][prime][N]
    w = per_limb((g_total, nb), qs, fill)                       # [g_total][nb][limb][N]
    cc = per_limb((n_ct, 2), qs[:QL], fill)                     # [n_ct][2][data limb][N]
    tables = np.stack([rng.permutation(N).astype(np.uint32) for _ in range(nb)])
    return mu, keys, w, cc, tables


def expect(primes, rows, beta, keyed, has_w, mu, keys, w, cc, tables):
    """acc [n_ct][g_total][2][limb][N] as Python integers."""
    n_ct, nb, g_total = mu.shape[0], keys.shape[0], w.shape[0]
    P = primes[rows[-1]]
    out = np.zeros((n_ct, g_total, 2, LIMBS, N), dtype=object)
    for l, r in enumerate(rows):
        q = primes[r]
        for b in range(n_ct):
            for c in range(2):
                x = []
                for j in range(nb):
                    tab = tables[j]
                    part = np.zeros(N, dtype=object)
                    if keyed[j]:
                        for i in range(beta):
                            part = part + mu[b, i, l][tab].astype(object) * keys[j, i, c, r].astype(object)
                        if l < QL and c == 0:
                            part = part + P * cc[b, 0, l][tab].astype(object)
                    elif l < QL:
                        part = P * cc[b, c, l][tab].astype(object)
                    x.append(part % q)
                for g in range(g_total):
                    acc = np.zeros(N, dtype=object)
                    for j in range(nb):
                        if has_w[g * nb + j]:
                            acc = acc + x[j] * w[g, j, l].astype(object)
                    out[b, g, c, l] = acc % q
    return out


def launch(emu, primes, rows, ng, cb, beta, n_ct, keyed, has_w, mu, keys, w, cc, tables):
    """Runs the accumulators [G0, G0 + ng) of the first n_ct ciphertexts; returns acc [n_ct][ng][2][limb][N] after checking the canaries."""
    nb, g_total = keys.shape[0], w.shape[0]
    assert g_total == G0 + ng
    words = n_ct * g_total * 2 * LIMBS * N
    after = cb * g_total * 2 * LIMBS * N + MARGIN          # room for the ciphertexts a full last group would have
    buf = np.full(MARGIN + words + after, CANARY, dtype=np.uint64)
    acc = buf[MARGIN:MARGIN + words]
    ins = [np.ascontiguousarray(mu[:n_ct]), keys, w, np.ascontiguousarray(cc[:n_ct]), tables]
    copies = [a.copy() for a in ins]
    pr = np.array(primes, dtype=np.uint64)
    rw = np.array(rows, dtype=np.uint32)
    pq = np.array([primes[rows[-1]] % primes[r] for r in rows[:QL]], dtype=np.uint64)
    kd = np.array(keyed, dtype=np.uint8)
    hw = np.array(has_w, dtype=np.uint8)
    rc = emu.emu_hoist_bsgs_batched(ng, cb, beta, N, LIMBS, QL, len(primes), nb, g_total, G0, n_ct, acc.ctypes.data_as(u64p),
                                    ins[0].ctypes.data_as(u64p), keys.ctypes.data_as(u64p), kd.ctypes.data_as(u8p),
                                    tables.ctypes.data_as(u32p), w.ctypes.data_as(u64p), hw.ctypes.data_as(u8p),
                                    ins[3].ctypes.data_as(u64p), pr.ctypes.data_as(u64p), rw.ctypes.data_as(u32p), pq.ctypes.data_as(u64p))
    assert rc == 0, f"no instantiation for NG {ng}, CB {cb}, beta {beta}"
    assert np.all(buf[:MARGIN] == CANARY), "words before acc were written"
    assert np.all(buf[MARGIN + words:] == CANARY), "words after the last ciphertext of the launch were written (tail group)"
    got = acc.reshape(n_ct, g_total, 2, LIMBS, N)
    assert np.all(got[:, :G0] == CANARY), "accumulators below g0 were written"
    for a, b in zip(ins, copies):
        assert np.array_equal(a, b), "an operand was written"
    return got[:, G0:].copy()


def group_sizes(cb):
    return sorted({cb - 1, cb, cb + 1, 2 * cb + 1} - {0})


def test_library_group_widths(emu):
    """CB per instantiation: 1, 2 or 4."""
    for beta in BETAS:
        for ng in NGS:
            assert emu.emu_hoist_bsgs_batched_cb(beta, ng) in (1, 2, 4)


@pytest.mark.parametrize("ng", NGS)
@pytest.mark.parametrize("beta", BETAS)
def test_every_word_equals_python_integers(emu, moduli, beta, ng):
    primes, rows = moduli
    cb = emu.emu_hoist_bsgs_batched_cb(beta, ng)
    rng = rng_for(7700 + 32 * beta + ng)
    nb, g_total, n_max = 3, G0 + ng, 2 * cb + 1
    mu, keys, w, cc, tables = operands(rng, primes, rows, beta, nb, g_total, n_max, maximal=False)
    has_w = [1] * (g_total * nb)
    has_w[G0 * nb + 2] = 0                                    # a missing weight in the first accumulator of the launch
    for keyed in ([0, 1, 1], [1, 0, 1]):                      # the identity baby step first, and in the middle
        want = expect(primes, rows, beta, keyed, has_w, mu, keys, w, cc, tables)[:, G0:]
        for n_ct in group_sizes(cb):
            got = launch(emu, primes, rows, ng, cb, beta, n_ct, keyed, has_w, mu, keys, w, cc, tables)
            bad = np.argwhere(got.astype(object) != want[:n_ct])
            assert bad.size == 0, f"NG {ng}, CB {cb}, beta {beta}, {n_ct} ciphertexts, keyed {keyed}: first wrong word at " \
                                  f"[ct, giant, poly, limb, k] = {bad[0].tolist()}"


@pytest.mark.parametrize("ng", NGS)
@pytest.mark.parametrize("beta", BETAS)
def test_full_capacity_at_q_minus_one(emu, moduli, beta, ng):
    """Every operand q - 1 and 62 baby entries (61 keyed, one identity): nb + 1 = 63 is what the driver admits for 61-bit primes."""
    primes, rows = moduli
    cb = emu.emu_hoist_bsgs_batched_cb(beta, ng)
    nb, g_total, n_ct = 62, G0 + ng, cb + 1
    rng = rng_for(7900 + 32 * beta + ng)
    mu, keys, w, cc, tables = operands(rng, primes, rows, beta, nb, g_total, n_ct, maximal=True)
    keyed = [1] * nb
    keyed[17] = 0
    got = launch(emu, primes, rows, ng, cb, beta, n_ct, keyed, [1] * (g_total * nb), mu, keys, w, cc, tables)
    P = primes[rows[-1]]
    for l, r in enumerate(rows):
        q = primes[r]
        pc = P * (q - 1) % q if l < QL else 0
        inner = beta * (q - 1) ** 2 % q
        for c in range(2):
            s_keyed = (inner + pc) % q if c == 0 else inner
            assert (nb - 1) * s_keyed * (q - 1) + pc * (q - 1) < 1 << 128
            want = ((nb - 1) * s_keyed * (q - 1) + pc * (q - 1)) % q
            assert np.all(got[:, :, c, l, :] == np.uint64(want)), f"NG {ng}, CB {cb}, beta {beta}, {q.bit_length()}-bit limb {l}, poly {c}"


def test_other_group_widths_give_the_same_words(emu, moduli):
    """CB is a tuning choice: 1, 2 and 4 ciphertexts per thread give identical words (NG = 2)."""
    primes, rows = moduli
    rng = rng_for(7990)
    ng, nb, n_ct = 2, 10, 5                                   # 10 baby entries: one FP re-centring inside the loop
    for beta in (1, 3):
        mu, keys, w, cc, tables = operands(rng, primes, rows, beta, nb, G0 + ng, n_ct, maximal=False)
        keyed = [0] + [1] * (nb - 1)
        has_w = [1] * ((G0 + ng) * nb)
        ref = launch(emu, primes, rows, ng, 1, beta, n_ct, keyed, has_w, mu, keys, w, cc, tables)
        for cb in (2, 4):
            assert np.array_equal(launch(emu, primes, rows, ng, cb, beta, n_ct, keyed, has_w, mu, keys, w, cc, tables), ref), \
                f"beta {beta}, CB {cb}"
