"""The arithmetic and the pass phases of the CKKS encoder (phantom-fhe_amd/csrc/pha_ckks_fft.h: host/device functions, the very
source the kernels of pha_ckks.hip run) compiled for the host with g++ and compared with the numpy restatement
(tests/ckks_restatement.py) bit for bit -- no GPU needed.  Harness: tests/emu/emu_ckks_fft.cpp (test-only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ckks_restatement as R
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
u64p, u32p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
PRIME_BITS = [30, 36, 37, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 55, 59, 60, 61]   # every bit length of a prime in tests/util.py (CONFIGS and MIXED_BITS)
IN_INTERLEAVED, IN_GATHER, IN_SPLIT = 0, 1, 2
OUT_INTERLEAVED, OUT_SPLIT, OUT_SCATTER = 0, 1, 2


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_ckks_fft") / "libemu_ckks_fft.so")
    # -ffp-contract=fast on purpose: the header states the no-contraction rule itself
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=fast", "-march=native", "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "emu", "emu_ckks_fft.cpp")])
    L = C.CDLL(out)
    L.emu_ckks_bfly.argtypes = [C.c_int, f64p, f64p, f64p]
    L.emu_ckks_bfly.restype = None
    L.emu_ckks_psi_all.argtypes = [u32p, C.c_uint32, C.c_uint32, u32p]
    L.emu_ckks_psi_all.restype = None
    L.emu_ckks_brev.argtypes = [C.c_uint32, C.c_uint32]
    L.emu_ckks_brev.restype = C.c_uint32
    L.emu_ckks_round.argtypes = [C.c_double]
    L.emu_ckks_round.restype = C.c_double
    L.emu_ckks_bit_count.argtypes = [C.c_uint64]
    L.emu_ckks_bit_count.restype = C.c_int
    L.emu_ckks_round_reduce.argtypes = [C.c_int, f64p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, u64p]
    L.emu_ckks_round_reduce.restype = None
    L.emu_ckks_fft.argtypes = [C.c_int, C.c_uint32, C.c_uint32, f64p, u32p, f64p, C.c_int, C.c_uint32, f64p, f64p, C.c_int, C.c_double,
                               C.c_uint32, u64p]
    L.emu_ckks_fft.restype = C.c_uint32
    return L


def _f(a):
    return a.ctypes.data_as(f64p)


def test_butterflies_round_every_operation_on_its_own(emu):
    rng = np.random.default_rng(0xB0F1)
    for _ in range(2000):
        a, b, w = (rng.standard_normal(2) * 2.0 ** rng.integers(-30, 30) for _ in range(3))
        ar, ai, br, bi, wr, wi = (np.float64(v) for v in (*a, *b, *w))
        x, y = a.copy(), b.copy()
        emu.emu_ckks_bfly(0, _f(x), _f(y), _f(w))
        dr, di = ar - br, ai - bi
        assert x.tolist() == [ar + br, ai + bi] and y.tolist() == [dr * wr - di * wi, dr * wi + di * wr]
        x, y = a.copy(), b.copy()
        emu.emu_ckks_bfly(1, _f(x), _f(y), _f(w))
        tr, ti = br * wr - bi * wi, br * wi + bi * wr
        assert x.tolist() == [ar + tr, ai + ti] and y.tolist() == [ar - tr, ai - ti]


@pytest.mark.parametrize("log_n", range(1, 17))
def test_psi_of_every_stage_and_butterfly(emu, log_n):
    m = 4 << log_n
    group = R.group_table(m, max(1, 1 << (log_n - 1)))
    half = 1 << (log_n - 1)
    got = np.zeros((log_n, half), dtype=np.uint32)
    emu.emu_ckks_psi_all(group.ctypes.data_as(u32p), log_n, m, got.ctypes.data_as(u32p))
    t = np.arange(half, dtype=np.int64)
    for lp in range(log_n):
        want = R.psi(group, log_n, lp, t >> lp, m)
        assert np.array_equal(got[lp].astype(np.int64), want), (log_n, lp)
        assert want.min() > 0 and want.max() < m           # m - psi stays inside the table
    assert all(emu.emu_ckks_brev(i, log_n) == int(R.brev(i, log_n)) for i in (0, 1, 2, 3, (1 << log_n) - 1, (1 << log_n) // 3))


def _edge_values():
    big = [float(2 ** 53 - 1), float(2 ** 53 - 3), float(2 ** 53 - 5)]           # the largest odd integers below 2^53
    vals = [0.5, 1.5, 2.5, float(2 ** 52 + 1), float(2 ** 63 - 1024), 0.49999999999999994, 4503599627370495.5, 3.0, 0.0,
            1e-300, 123456789.5] + big
    return np.array(vals + [-v for v in vals] + [-0.25, -0.4999, -1e-9], dtype=np.float64)


@pytest.mark.parametrize("bits", PRIME_BITS)
def test_round_and_reduce_one_word(emu, bits):
    q = int(O.get_primes(1 << 12, bits, 1)[0])
    ratio = (1 << 128) // q
    x = _edge_values()
    rng = np.random.default_rng(bits)
    x = np.concatenate([x, rng.standard_normal(500) * 2.0 ** rng.integers(0, 62, 500)])
    for wide in (0, 1):
        out = np.full(len(x), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        emu.emu_ckks_round_reduce(wide, _f(x), len(x), q, ratio & (2 ** 64 - 1), ratio >> 64, out.ctypes.data_as(u64p))
        want = [R.round_exact(v) % q for v in x]
        assert [int(v) for v in out] == want, wide
        assert int(out.max()) < q
    for v in (-0.25, -0.4999, -1e-9, -0.0):           # a coefficient that rounds to -0.0 gives 0, not q
        one = np.array([v])
        out = np.zeros(1, dtype=np.uint64)
        emu.emu_ckks_round_reduce(0, _f(one), 1, q, ratio & (2 ** 64 - 1), ratio >> 64, out.ctypes.data_as(u64p))
        assert int(out[0]) == 0
    assert all(emu.emu_ckks_round(float(v)) == float(R.round_exact(v)) for v in x)


@pytest.mark.parametrize("bits", [36, 50, 61])
def test_round_and_reduce_wide(emu, bits):
    """Coefficients of 65 .. 128 bits and far above: mantissa and exponent against Python integers."""
    q = int(O.get_primes(1 << 12, bits, 1)[0])
    ratio = (1 << 128) // q
    rng = np.random.default_rng(100 + bits)
    x = rng.standard_normal(600) * 2.0 ** rng.integers(60, 700, 600)
    x = np.concatenate([x, [2.0 ** 64, -(2.0 ** 64), 2.0 ** 127, 2.0 ** 128, -(2.0 ** 600), float(q) * 2.0 ** 70, -float(q) * 2.0 ** 70]])
    out = np.zeros(len(x), dtype=np.uint64)
    emu.emu_ckks_round_reduce(1, _f(x), len(x), q, ratio & (2 ** 64 - 1), ratio >> 64, out.ctypes.data_as(u64p))
    assert [int(v) for v in out] == [int(v) % q for v in x]


def test_bit_count_from_the_bit_pattern(emu):
    for v in (0.0, 0.3, 1.0, 1.5, 2.0, 3.0, 2.0 ** 40, float(np.nextafter(2.0 ** 40, np.inf)), 2.0 ** 63 - 1024, 1e300, np.inf):
        bits = int(np.array([v]).view(np.uint64)[0])
        assert emu.emu_ckks_bit_count(bits) == R.bit_count(np.array([v])), v
    assert emu.emu_ckks_bit_count(int(np.array([np.nan]).view(np.uint64)[0])) > 4096


def _transform(emu, inverse, log_n, roots, group, src, in_mode, values_size, out_mode, fix, nthreads):
    n = 1 << log_n
    mid, out = np.zeros(2 * n), np.full(2 * n, np.nan)
    mx = C.c_uint64()
    passes = emu.emu_ckks_fft(inverse, log_n, 4 * n, _f(roots), group.ctypes.data_as(u32p), _f(src), in_mode, values_size, _f(mid), _f(out),
                              out_mode, fix, nthreads, C.byref(mx))
    return out, passes, mx.value


# one workgroup holds the whole array up to 2^13 points; 2^14 takes the two passes.  The thread counts include one that does not
# divide the tile's work evenly.
@pytest.mark.parametrize("log_n,nthreads", [(1, 64), (2, 64), (3, 7), (5, 64), (9, 256), (13, 512), (14, 512), (14, 96)])
def test_whole_transform_through_the_kernel_phases(emu, log_n, nthreads):
    n = 1 << log_n
    m = 4 * n
    roots, group = R.roots_table(m), R.group_table(m, max(1, n // 2))
    rng = np.random.default_rng(log_n)
    z = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    inter = np.stack([z.real, z.imag], axis=1).reshape(-1).copy()
    # the reference's launchers: in place order, interleaved, with and without the scalar
    for fix in (2.0 ** 40 / n, 0.0):
        got, passes, _ = _transform(emu, 1, log_n, roots, group, inter, IN_INTERLEAVED, 0, OUT_INTERLEAVED, fix, nthreads)
        re, im = R.special_ifft(z.real, z.imag, roots, group, m, fix if fix else 1.0)
        assert passes == (1 if log_n <= 13 else 2)
        assert np.array_equal(got.reshape(n, 2)[:, 0].view(np.uint64), re.view(np.uint64))
        assert np.array_equal(got.reshape(n, 2)[:, 1].view(np.uint64), im.view(np.uint64))
    got, _, _ = _transform(emu, 0, log_n, roots, group, inter, IN_INTERLEAVED, 0, OUT_INTERLEAVED, 0.0, nthreads)
    re, im = R.special_fft(z.real, z.imag, roots, group, m)
    assert np.array_equal(got.view(np.uint64), np.stack([re, im], axis=1).reshape(-1).view(np.uint64))
    # encode's form: gathered, zero-padded input; split, scaled output; the maximum
    for size in sorted({1, n // 2 + 1, n}):
        got, _, mx = _transform(emu, 1, log_n, roots, group, inter, IN_GATHER, size, OUT_SPLIT, 2.0 ** 40 / n, nthreads)
        want = R.encode_coeffs(z[:size], n, roots, group, 2.0 ** 40)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), size
        assert mx == int(np.max(np.abs(want)).view(np.uint64))
        assert emu.emu_ckks_bit_count(mx) == R.bit_count(want)
    # decode's form: split input, scattered output
    coeffs = rng.standard_normal(2 * n)
    got, _, _ = _transform(emu, 0, log_n, roots, group, coeffs, IN_SPLIT, 0, OUT_SCATTER, 0.0, nthreads)
    want = R.decode_values(coeffs, n, roots, group)
    assert np.array_equal(got.view(np.uint64), np.stack([want.real, want.imag], axis=1).reshape(-1).view(np.uint64))
