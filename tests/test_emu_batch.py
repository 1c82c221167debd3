"""The arithmetic, the index math and the pass phases of the BFV / BGV batch encoder (phantom-fhe_amd/csrc/pha_batch.h: host/device
functions, the very source the kernels of pha_batch.hip run) compiled for the host with g++ and compared with the restatement
(tests/batch_restatement.py) word for word -- no GPU needed.  Harness: tests/emu/emu_batch.cpp (test-only).  Every pass of N = 2^12
(one pass) and N = 2^15 (two passes) is walked thread index by thread index: gather, stages, scale and scatter."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batch_restatement as R
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
IN_PLAIN, IN_GATHER = 0, 1
OUT_CANON, OUT_SCATTER = 1, 2
POISON = 0xDEADBEEFDEADBEEF


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_batch") / "libemu_batch.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "emu", "emu_batch.cpp")])
    L = C.CDLL(out)
    L.emu_batch_index_map.argtypes = [C.c_uint32, u64p]
    L.emu_batch_index_map.restype = None
    L.emu_batch_sign_rule.argtypes = [C.c_uint64, C.c_uint64]
    L.emu_batch_sign_rule.restype = C.c_uint64
    L.emu_batch_threads.argtypes = [C.c_uint32]
    L.emu_batch_threads.restype = C.c_uint32
    L.emu_batch_nwt.argtypes = [C.c_int, C.c_uint32, C.c_uint64, u64p, C.c_uint64, C.c_uint64, u32p, u64p, C.c_int, C.c_uint32, u64p, u64p,
                                C.c_int, C.c_uint32]
    L.emu_batch_nwt.restype = C.c_uint32
    L.emu_batch_gather.argtypes = [u64p, u64p, u32p, C.c_uint32]
    L.emu_batch_gather.restype = None
    L.emu_batch_permute.argtypes = [u64p, u64p, u32p, C.c_uint32, C.c_uint64, C.c_uint32]
    L.emu_batch_permute.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(u64p)


def _tables(log_n, t):
    """(forward pairs, inverse pairs, N^-1, its Shoup quotient): slot brev(k) holds psi^(+-k) with its Shoup quotient, slot 1 of the
    inverse table NOT folded with N^-1 -- what pha_batch_encoder_create builds."""
    n = 1 << log_n
    psi = O.minimal_primitive_root(2 * n, t)
    ipsi = pow(psi, t - 2, t)
    tw, itw = np.zeros(2 * n, dtype=np.uint64), np.zeros(2 * n, dtype=np.uint64)
    pw = ipw = 1
    for k in range(n):
        at = R.reverse_bits(k, log_n)
        tw[2 * at], tw[2 * at + 1] = pw, (pw << 64) // t
        itw[2 * at], itw[2 * at + 1] = ipw, (ipw << 64) // t
        pw, ipw = pw * psi % t, ipw * ipsi % t
    ninv = pow(n, t - 2, t)
    return tw, itw, ninv, (ninv << 64) // t


def _run(emu, inverse, log_n, t, tabs, perm, src, in_mode, values_size, out_mode, nthreads=0):
    n = 1 << log_n
    tw, itw, ninv, ninv_s = tabs
    mid, out = np.full(n, POISON, dtype=np.uint64), np.full(n, POISON, dtype=np.uint64)
    src = np.ascontiguousarray(src, dtype=np.uint64)
    passes = emu.emu_batch_nwt(inverse, log_n, t, _p(itw if inverse else tw), ninv, ninv_s, perm.ctypes.data_as(u32p), _p(src), in_mode,
                               values_size, _p(mid), _p(out), out_mode, nthreads)
    return out, passes


def test_index_map_sign_rule_and_thread_counts(emu):
    for log_n in (1, 2, 3, 7, 12, 15, 17):
        got = np.zeros(1 << log_n, dtype=np.uint64)
        emu.emu_batch_index_map(log_n, _p(got))
        assert np.array_equal(got, R.index_map(log_n)), log_n
    t = R.LADDER[59]
    for v in (0, 1, t - 1, (1 << 63) - 1):
        assert emu.emu_batch_sign_rule(v, t) == v
    for x in (1, 2, t - 1):
        assert emu.emu_batch_sign_rule((1 << 64) - x, t) == t - x
    assert [emu.emu_batch_threads(k) for k in (3, 9, 12, 13, 14)] == [64, 64, 512, 1024, 1024]


@pytest.mark.parametrize("log_n", [12, 15])
@pytest.mark.parametrize("bits", [16, 59])
def test_every_pass_against_the_restatement(emu, log_n, bits):
    t = R.batching_prime(log_n, bits) if (log_n, bits) != (15, 16) else R.smallest_batching_prime(15)   # 40961 at 2^12, 65537 at 2^15
    n = 1 << log_n
    b = R.batch(log_n, t)
    tabs = _tables(log_n, t)
    imap = R.index_map(log_n)
    perm = np.zeros(n, dtype=np.uint32)
    perm[imap.astype(np.int64)] = np.arange(n, dtype=np.uint32)
    rng = np.random.default_rng(log_n * 100 + bits)
    v = rng.integers(0, t, n, dtype=np.uint64)
    # the plain transforms (no permutation): the reference's launchers over gpu_plain_tables()
    got, passes = _run(emu, 0, log_n, t, tabs, perm, v, IN_PLAIN, 0, OUT_CANON)
    assert passes == (1 if log_n <= 14 else 2)
    assert np.array_equal(got, b.nwt_forward(v))
    got, _ = _run(emu, 1, log_n, t, tabs, perm, v, IN_PLAIN, 0, OUT_CANON)
    assert np.array_equal(got, b.nwt_backward(v))
    # encode: gather in the first load, zero padding, the sign rule, N^-1 and the canonical reduction in the last store
    signed = v.copy()
    neg = rng.integers(0, n, 64)
    signed[neg] = (np.uint64(0) - (np.uint64(t) - v[neg])) * (v[neg] != 0) + v[neg] * (v[neg] == 0)   # -(t - x): encodes x again
    for size in (0, 1, n // 2, n - 1, n):
        want = b.encode(v[:size])
        got, _ = _run(emu, 1, log_n, t, tabs, perm, signed, IN_GATHER, size, OUT_CANON)
        assert np.array_equal(got, want), size
        assert int(got.max()) < t
        # the same with the permutation as a pass of its own in front of the plain transform
        buf = np.full(n, POISON, dtype=np.uint64)
        emu.emu_batch_permute(_p(buf), _p(signed), perm.ctypes.data_as(u32p), size, t, n)
        got, _ = _run(emu, 1, log_n, t, tabs, perm, buf, IN_PLAIN, 0, OUT_CANON)
        assert np.array_equal(got, want), size
    # a thread count that does not divide the tile's work evenly takes the same walk
    got, _ = _run(emu, 1, log_n, t, tabs, perm, v, IN_GATHER, n, OUT_CANON, nthreads=96)
    assert np.array_equal(got, b.encode(v))
    # decode: scatter in the last store, and the plain store followed by the gather
    plain = b.encode(v)
    got, _ = _run(emu, 0, log_n, t, tabs, perm, plain, IN_PLAIN, 0, OUT_SCATTER)
    assert np.array_equal(got, v)
    ntt, _ = _run(emu, 0, log_n, t, tabs, perm, plain, IN_PLAIN, 0, OUT_CANON)
    out = np.full(n, POISON, dtype=np.uint64)
    emu.emu_batch_gather(_p(out), _p(ntt), imap.astype(np.uint32).ctypes.data_as(u32p), n)
    assert np.array_equal(out, v)


def test_stand_alone_program_builds_and_runs(tmp_path):
    """The same harness with its own main(): the program a sanitizer build of the host-compilable header runs (add
    -fsanitize=address,undefined to this line; the suite builds it plain)."""
    exe = str(tmp_path / "emu_batch")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEMU_BATCH_MAIN", "-o", exe, os.path.join(HERE, "emu", "emu_batch.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "round trips OK" in r.stdout
