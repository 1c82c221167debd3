"""The one-word centred lift of a BFV plaintext (phantom-fhe_amd/csrc/pha_bfv_lift.h: host/device functions, the very source the
load prologue of the forward transform calls) compiled for the host and compared with Python integers -- no GPU needed.  Harness:
tests/emu/emu_bfv_lift.cpp (test-only).

A word w below t stands for the centred residue w (w < (t + 1) / 2) or w - t; its lift into the limb of q is that residue modulo
q.  Every w in [0, t) for t = 65537, and the words around 0, the threshold and t - 1 for a 20-bit and a 36-bit t, for one prime
of each bit length the parameter sets use."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
u64p = C.POINTER(C.c_uint64)
PRIME_BITS = [36, 37, 40, 45, 46, 49, 50, 60, 61]       # every bit length of a prime in tests/util.py's sets
T_SMALL = 65537
T_EDGE = [(1 << 20) - 3, 1032193, (1 << 36) - 5]      # 20-bit (one of them the reference's batching prime) and 36-bit plain moduli


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_bfv_lift") / "libemu_bfv_lift.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "emu", "emu_bfv_lift.cpp")])
    L = C.CDLL(out)
    L.emu_bfv_lift.argtypes = [C.c_uint64, C.c_uint64, u64p, C.c_size_t, u64p]
    L.emu_bfv_lift.restype = None
    L.emu_bfv_lift_threshold.argtypes = [C.c_uint64]
    L.emu_bfv_lift_threshold.restype = C.c_uint64
    return L


def prime_of(bits):
    q = int(O.get_primes(1 << 12, bits, 1)[0])
    assert q.bit_length() == bits
    return q


def lift(emu, q, t, words):
    w = np.array(words, dtype=np.uint64)
    out = np.full(len(w), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    emu.emu_bfv_lift(q, t, w.ctypes.data_as(u64p), len(w), out.ctypes.data_as(u64p))
    return [int(v) for v in out]


def want(w, q, t):
    centred = w if w < (t + 1) // 2 else w - t
    return centred % q


@pytest.mark.parametrize("bits", PRIME_BITS)
def test_every_word_below_65537(emu, bits):
    q, t = prime_of(bits), T_SMALL
    assert emu.emu_bfv_lift_threshold(t) == (t + 1) // 2
    got = lift(emu, q, t, range(t))
    ref = [want(w, q, t) for w in range(t)]
    assert got == ref
    assert max(got) < q and got[(t - 1) // 2] == (t - 1) // 2 and got[(t + 1) // 2] == q - (t - 1) // 2 and got[t - 1] == q - 1


# (the lift needs t below q: the entries refuse any other level)
@pytest.mark.parametrize("bits,t", [(b, t) for b in PRIME_BITS for t in T_EDGE if t.bit_length() < b])
def test_boundary_words_of_wider_plain_moduli(emu, bits, t):
    q = prime_of(bits)
    assert t < q
    half = (t + 1) // 2
    words = sorted({0, 1, 2, half - 2, half - 1, half, half + 1, t - 2, t - 1})
    assert lift(emu, q, t, words) == [want(w, q, t) for w in words]
