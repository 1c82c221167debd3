"""GPU parity of the CKKS encoder (csrc/pha_ckks.hip) with the numpy / Python-integer restatement (tests/ckks_restatement.py), word
for word and bit for bit unless stated.  The restatement is fed the library's own root table, so libm plays no part.

A. tables: every root within 2 ulp per component of np.longdouble cos / sin, group exact;
B. pha_special_fft_backward / _forward at every log N from 12 to 17 (slot counts 2^11 .. 2^16: one LDS-resident pass up to 2^13
   points, two passes above);
C. pha_ckks_encode_batched = restatement -> exact rounding -> Python-integer residues -> oracle forward NTT: hyb12_a2 (all levels,
   with and without the special limbs), p61_a2, wide_p33, c2_ckks14, c3_ckks16 at 3 limbs and once at 45 with the special limbs;
   counts 1, 3, 8; 1, n / 2 + 1 and n values; scales 2^40, 2^70, 2^140 and 1.0 (the negative-zero case); every word canonical;
   the special-limb form equals rows [0, l) u P of the key-level encoding; bit counts equal the restatement's; the fused and the
   unfused path of word-sized coefficients forced in turn at every degree from 2^12 to 2^17;
D. refusals;
E. pha_compose_array / pha_ckks_decode_batched on uniform random canonical plaintexts: hyb12_a2 (every level), c2_ckks14, c3_ckks16
   at 2 and 45 limbs.  Over more than 16 limbs a uniform plaintext's value over the scale is beyond the double range, where the
   reference's arithmetic gives infinities and NaN: compared as such (any NaN equals any NaN, see _same_doubles), and a 45-limb
   batch of 45-limb plaintexts made by encode (finite values, so the FFT is compared bit for bit) is decoded as well.  Every
   coefficient of every message is compared with the Python integers;
F. end to end without keys through pha_plain_inner_product_rescale_batched."""
import functools
import gc

import numpy as np
import pytest

import ckks_restatement as R
from oracle import oracle as O
from util import oracle_ctx, primes_of, uniform_poly

pytestmark = pytest.mark.gpu

POISON = -0x2152411021524111          # 0xDEADBEEFDEADBEEF as int64


@functools.lru_cache(maxsize=2)
def _setup(name):
    import torch
    import phantom_fhe_amd as P
    log_n, primes, size_p = primes_of(name)
    ctx = P.PhantomContext(log_n, list(primes), size_p, device=torch.device("cuda:0"))
    enc = ctx.ckks_encoder()
    roots, group = enc.tables()
    roots = np.stack([roots.real, roots.imag], axis=1).copy()
    return P, ctx, enc, roots, group


def _release():
    import torch
    _setup.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _messages(rng, count, size):
    return rng.uniform(-1, 1, (count, size)) + 1j * rng.uniform(-1, 1, (count, size))


def _first_diff(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    idx = tuple(int(v) for v in np.argwhere(got != ref)[0])
    raise AssertionError(f"{what}: {int(np.count_nonzero(got != ref))} words differ, first at {idx}: got {got[idx]!r}, want {ref[idx]!r}")


def _same_doubles(got, want, what):
    """Bit for bit, except that any NaN equals any NaN: which sign and payload an invalid operation (inf - inf, 0 * inf) gives is
    the hardware's choice (x86 sets the sign bit, gfx950 does not), and IEEE 754 leaves it open.  Infinities and zeros keep their
    signs.  NaN arises only where the plaintext's value over the scale is beyond the double range (uniform random plaintexts over
    more than 16 limbs)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN at different places"
    ok = ~np.isnan(want)
    _first_diff(got[ok].view(np.uint64), want[ok].view(np.uint64), what)


def _reference_plain(name, roots, group, z, scale, rows):
    """Restatement -> exact rounding -> residues -> oracle forward NTT over the prime-table rows `rows`; and the bit count."""
    log_n, primes, _ = primes_of(name)
    n = 1 << (log_n - 1)
    coeffs = R.encode_coeffs(z, n, roots, group, scale)
    res = R.residues(R.round_coeffs(coeffs), [primes[r] for r in rows])
    return oracle_ctx(name).nwt_forward_map(res, rows), R.bit_count(coeffs)


def _encode(gpu, P, ctx, enc, size_Ql, z, size, scale, with_special):
    import torch
    count = z.shape[0]
    limbs = size_Ql + (ctx.size_P if with_special else 0)
    d_z = torch.from_numpy(np.ascontiguousarray(z)).to(gpu)
    dst = torch.full((count, limbs, ctx.n), POISON, dtype=torch.int64, device=gpu)
    bits = enc.encode_batched(size_Ql, d_z, size, scale, dst, with_special=with_special)
    assert ctx.check_canonical(dst, limbs, 0, ctx.size_P if with_special else 0, count, limbs * ctx.n) == 0
    return dst, bits


def _check_encode(gpu, name, size_Ql, with_special, count, size, scale, seed, amplitude=1.0):
    P, ctx, enc, roots, group = _setup(name)
    rng = np.random.default_rng(seed)
    n = ctx.n // 2
    z = _messages(rng, count, n) * amplitude          # rows longer than `size`: the tail must not be read
    dst, bits = _encode(gpu, P, ctx, enc, size_Ql, z, size, scale, with_special)
    got = P.to_host(dst)
    rows = list(range(size_Ql)) + (list(range(ctx.size_Q, ctx.size_QP)) if with_special else [])
    for k in range(count):
        want, want_bits = _reference_plain(name, roots, group, z[k, :size], scale, rows)
        _first_diff(got[k], want, f"{name} Ql={size_Ql} special={with_special} count={count} size={size} message {k}")
        assert bits[k] == want_bits
    return dst


# ---- A ----------------------------------------------------------------------------------------------------------------------------
def test_tables(gpu):
    _, ctx, enc, roots, group = _setup("hyb12_a2")
    m = 2 * ctx.n
    assert roots.shape == (m, 2) and group.shape == (ctx.n // 4,)
    worst = R.roots_ulp_error(roots)
    print("roots, worst error in ulp:", worst)
    assert worst <= 2.0
    assert np.array_equal(group, R.group_table(m, ctx.n // 4))
    _release()


# ---- B ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hyb12_a2", "hyb13_a3", "c2_ckks14", "c4_bfv15", "c3_ckks16", "hyb17_a2"])
def test_special_fft_launchers(gpu, name):
    import torch
    _, ctx, enc, roots, group = _setup(name)
    n, m = ctx.n // 2, 2 * ctx.n
    log_n = n.bit_length() - 1
    rng = np.random.default_rng(ctx.log_n)
    z = _messages(rng, 1, n)[0]
    fix = 2.0 ** 40 / n
    d = torch.from_numpy(z.copy()).to(gpu)
    enc.special_fft_backward(d, log_n, fix)
    re, im = R.special_ifft(z.real, z.imag, roots, group, m, fix)
    got = d.cpu().numpy()
    _first_diff(got.real.view(np.uint64), re.view(np.uint64), f"{name} backward re")
    _first_diff(got.imag.view(np.uint64), im.view(np.uint64), f"{name} backward im")
    d = torch.from_numpy(z.copy()).to(gpu)
    enc.special_fft_forward(d, log_n)
    re, im = R.special_fft(z.real, z.imag, roots, group, m)
    got = d.cpu().numpy()
    _first_diff(got.real.view(np.uint64), re.view(np.uint64), f"{name} forward re")
    _first_diff(got.imag.view(np.uint64), im.view(np.uint64), f"{name} forward im")
    if log_n > 3:   # a sparse transform: fewer points than slots, same table
        zs = z[:n // 4].copy()
        d = torch.from_numpy(zs.copy()).to(gpu)
        enc.special_fft_backward(d, log_n - 2, 0.0)
        re, im = R.special_ifft(zs.real, zs.imag, roots, group, m, 1.0)
        got = d.cpu().numpy()
        assert np.array_equal(got.real.view(np.uint64), re.view(np.uint64)) and np.array_equal(got.imag.view(np.uint64), im.view(np.uint64))
    _release()


# ---- C ----------------------------------------------------------------------------------------------------------------------------
def test_encode_hyb12_every_level_with_and_without_special(gpu):
    name = "hyb12_a2"
    _, ctx, enc, _, _ = _setup(name)
    n = ctx.n // 2
    counts, sizes = [1, 3, 8], [1, n // 2 + 1, n]
    case = 0
    for size_Ql in range(1, ctx.size_Q + 1):
        for with_special in (False, True):
            scale = 2.0 ** 40 if size_Ql > 1 else 2.0 ** 30
            _check_encode(gpu, name, size_Ql, with_special, counts[case % 3], sizes[(case // 2) % 3], scale, 1000 + case)
            case += 1
    # every (count, size) pair at one level
    for count in counts:
        for size in sizes:
            _check_encode(gpu, name, 3, True, count, size, 2.0 ** 40, 2000 + 10 * count + size)
    _release()


def test_encode_special_rows_equal_the_key_level_encoding(gpu):
    import torch
    name = "hyb12_a2"
    P, ctx, enc, _, _ = _setup(name)
    rng = np.random.default_rng(77)
    z = _messages(rng, 3, ctx.n // 2)
    key, _ = _encode(gpu, P, ctx, enc, ctx.size_Q, z, ctx.n // 2, 2.0 ** 40, True)
    for size_Ql in (2, 4, ctx.size_Q):
        got, _ = _encode(gpu, P, ctx, enc, size_Ql, z, ctx.n // 2, 2.0 ** 40, True)
        assert torch.equal(got[:, :size_Ql], key[:, :size_Ql]) and torch.equal(got[:, size_Ql:], key[:, ctx.size_Q:])
    _release()


@pytest.mark.parametrize("name,size_Ql,with_special,count,size_kind,scale", [
    ("p61_a2", 6, True, 3, 2, 2.0 ** 40),            # 61-bit special primes
    ("p61_a2", 2, False, 1, 1, 2.0 ** 40),
    ("wide_p33", 6, True, 3, 1, 2.0 ** 40),          # 36-bit primes: |c| >> q
    ("wide_p33", 1, False, 8, 0, 2.0 ** 30),
    ("c2_ckks14", 8, True, 3, 2, 2.0 ** 40),
    ("c2_ckks14", 4, False, 1, 1, 2.0 ** 40),
    ("c3_ckks16", 3, False, 3, 1, 2.0 ** 40),
    ("c3_ckks16", 45, True, 1, 2, 2.0 ** 40),
    ("hyb13_a3", 9, False, 3, 2, 2.0 ** 70),         # 65 .. 128-bit coefficients
    ("hyb13_a3", 9, True, 1, 1, 2.0 ** 140),         # beyond 128 bits
])
def test_encode_other_sets_and_scales(gpu, name, size_Ql, with_special, count, size_kind, scale):
    _, ctx, _, _, _ = _setup(name)
    n = ctx.n // 2
    _check_encode(gpu, name, size_Ql, with_special, count, [1, n // 2 + 1, n][size_kind], scale, 3000 + size_Ql + count)
    _release()


@pytest.mark.parametrize("name,size_Ql,with_special,count", [
    ("hyb12_a2", 6, True, 3), ("hyb13_a3", 4, False, 2), ("c2_ckks14", 8, True, 3), ("c4_bfv15", 2, False, 2), ("c3_ckks16", 3, True, 2),
    ("hyb17_a2", 2, True, 2), ("p61_a2", 6, True, 1), ("wide_p33", 6, False, 8)])
def test_encode_paths_agree(gpu, name, size_Ql, with_special, count):
    """Coefficients that fit a word take one of two paths, chosen per launch shape: round-and-reduce as the load prologue of the
    forward transform's first pass (the decomposed form is never written), or the decompose kernel followed by the plain transform.
    Both forced in turn (the measurement hook), at every degree's transform plan: each equals the restatement, word for word."""
    import torch
    P, ctx, _, _, _ = _setup(name)
    n = ctx.n // 2
    try:
        outs = []
        for mode in (1, 0):
            P.set_ckks_encode_path(mode)
            outs.append(_check_encode(gpu, name, size_Ql, with_special, count, n // 2 + 1, 2.0 ** 40, 7000 + size_Ql))
        assert torch.equal(outs[0], outs[1])
    finally:
        P.set_ckks_encode_path(-1)
    with pytest.raises(ValueError):
        P.set_ckks_encode_path(2)
    _release()


def test_encode_scale_one_gives_canonical_zeros(gpu):
    """Scale 1.0 and |values| < 0.4: every coefficient rounds to +0.0 or -0.0, and -0.0 gives the word 0, not q."""
    import torch
    name = "hyb12_a2"
    P, ctx, enc, roots, group = _setup(name)
    n = ctx.n // 2
    rng = np.random.default_rng(5)
    z = _messages(rng, 1, n) * 0.28                   # |z| < 0.4
    coeffs = R.encode_coeffs(z[0], n, roots, group, 1.0)
    assert np.max(np.abs(coeffs)) < 0.5 and np.any(np.signbit(coeffs)), "the case needs coefficients in (-0.5, 0)"
    dst = _check_encode(gpu, name, 3, True, 1, n, 1.0, 5, amplitude=0.28)
    assert int(torch.count_nonzero(dst)) == 0
    # the launcher on its own, before any transform
    d_c = torch.from_numpy(np.ascontiguousarray(coeffs[:n] + 1j * coeffs[n:])).to(gpu)
    out = torch.full((3, ctx.n), POISON, dtype=torch.int64, device=gpu)
    ctx.decompose_array(3, out, d_c, 1)
    assert int(torch.count_nonzero(out)) == 0
    _release()


# ---- D ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    import torch
    name = "hyb12_a2"
    P, ctx, enc, roots, group = _setup(name)
    n = ctx.n // 2
    rng = np.random.default_rng(9)
    z = _messages(rng, 1, n)
    d_z = torch.from_numpy(z).to(gpu)
    dst = torch.full((1, 3, ctx.n), POISON, dtype=torch.int64, device=gpu)

    def refused(match, size_Ql, values, size, scale):
        with pytest.raises(ValueError, match=match):
            enc.encode_batched(size_Ql, values, size, scale, dst[:, :size_Ql].contiguous() if size_Ql < 3 else dst)
        assert int((dst != POISON).sum()) == 0

    refused("empty", 3, d_z, 0, 2.0 ** 40)
    refused("exceeds max slots", 3, torch.cat([d_z, d_z], dim=1).contiguous(), n + 1, 2.0 ** 40)
    refused("scale out of bounds", 3, d_z, n, 0.0)
    refused("scale out of bounds", 3, d_z, n, -1.0)
    refused("scale out of bounds", 1, d_z, n, 2.0 ** 59)              # q_0 has 60 bits: (int) log2 + 1 = 60
    big = torch.full((1, n), 100.0, dtype=torch.complex128, device=gpu)
    refused("too large", 1, big, n, 2.0 ** 55)                          # coefficient 0 = 100 * 2^55: 63 bits against 60
    inf = d_z.clone()
    inf[0, 5] = complex(float("inf"), 0.0)
    refused("too large", 3, inf, n, 2.0 ** 40)
    with pytest.raises(ValueError, match="scale out of bounds"):
        enc.decode_batched(3, dst, 0.0, torch.zeros((1, n), dtype=torch.complex128, device=gpu))
    torch.cuda.synchronize()
    _check_encode(gpu, name, 3, False, 1, n, 2.0 ** 40, 9)            # the library still computes
    _release()


# ---- E ----------------------------------------------------------------------------------------------------------------------------
def _check_decode(gpu, name, size_Ql, count, scale, seed, encoded=False):
    """Every coefficient of every message against the Python integers.  encoded: the plaintexts are encodings of random messages
    (small centred values: finite doubles at any level) instead of uniform residues (values up to Q / 2: beyond the double range
    over more than 16 limbs, where the reference's arithmetic gives infinities and NaN -- compared as such)."""
    import torch
    P, ctx, enc, roots, group = _setup(name)
    log_n, primes, _ = primes_of(name)
    n = ctx.n // 2
    rng = np.random.default_rng(seed)
    if encoded:
        d_plain = torch.empty((count, size_Ql, ctx.n), dtype=torch.int64, device=gpu)
        enc.encode_batched(size_Ql, torch.from_numpy(_messages(rng, count, n)).to(gpu), n, scale, d_plain)
        plain = P.to_host(d_plain)
    else:
        plain = np.stack([uniform_poly(rng, primes[:size_Ql], ctx.n) for _ in range(count)])
        d_plain = P.to_device(plain, gpu)
    coeff = np.stack([oracle_ctx(name).nwt_backward(plain[k], size_Ql, 0) for k in range(count)])
    want_coeffs = [R.compose_array(coeff[k], primes[:size_Ql], 1.0 / scale) for k in range(count)]
    finite = all(bool(np.all(np.isfinite(c))) for c in want_coeffs)
    assert finite == (encoded or size_Ql <= 16), "the case is meant to be finite exactly when encoded or within 16 limbs"
    # the launcher: coefficient form in, n complex numbers out
    for k in range(count):
        d_out = torch.full((n,), complex(np.nan, np.nan), dtype=torch.complex128, device=gpu)
        ctx.compose_array(size_Ql, d_out, P.to_device(coeff[k], gpu), 1.0 / scale)
        got = d_out.cpu().numpy()
        _same_doubles(np.concatenate([got.real, got.imag]), want_coeffs[k], f"{name} compose Ql={size_Ql} message {k}")
    # decode of the batch
    d_vals = torch.full((count, n), complex(np.nan, np.nan), dtype=torch.complex128, device=gpu)
    enc.decode_batched(size_Ql, d_plain, scale, d_vals)
    vals = d_vals.cpu().numpy()
    assert np.array_equal(P.to_host(d_plain), plain), "decode changed its input"
    for k in range(count):
        want = R.decode_values(want_coeffs[k], n, roots, group)
        _same_doubles(vals[k].real, want.real, f"{name} decode Ql={size_Ql} message {k} re")
        _same_doubles(vals[k].imag, want.imag, f"{name} decode Ql={size_Ql} message {k} im")


def test_decode_hyb12_every_level(gpu):
    for size_Ql in range(1, 7):
        _check_decode(gpu, "hyb12_a2", size_Ql, [1, 3, 2][size_Ql % 3], 2.0 ** 40 if size_Ql > 1 else 2.0 ** 30, 4000 + size_Ql)
    _release()


@pytest.mark.parametrize("name,size_Ql,count,encoded", [("c2_ckks14", 8, 2, False), ("c3_ckks16", 2, 1, False),
                                                        ("c3_ckks16", 45, 2, False), ("c3_ckks16", 45, 2, True)])
def test_decode_other_sets(gpu, name, size_Ql, count, encoded):
    _check_decode(gpu, name, size_Ql, count, 2.0 ** 40, 5000 + size_Ql, encoded)
    _release()


# ---- F ----------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_plain_inner_product(gpu):
    """Trivial ciphertexts (c0 = encode(x_k), c1 = 0) times encoded weights a_k, summed and rescaled by the library; decoding c0 at
    scale^2 / q_last gives sum a_k o x_k within 2^-20 (worst case K * 2 * 2^-27 from the encodings plus N / scale from the rescale,
    below 2^-23)."""
    import torch
    name, K, size_Ql, scale = "c2_ckks14", 4, 3, 2.0 ** 40
    P, ctx, enc, _, _ = _setup(name)
    _, primes, _ = primes_of(name)
    n = ctx.n // 2
    rng = np.random.default_rng(0xE2E)
    r, phi = np.sqrt(rng.uniform(0, 1, (2, K, n))), rng.uniform(0, 2 * np.pi, (2, K, n))
    x, a = r[0] * np.exp(1j * phi[0]), r[1] * np.exp(1j * phi[1])          # |values| <= 1
    ct = torch.zeros((K, 2, size_Ql, ctx.n), dtype=torch.int64, device=gpu)
    c0 = torch.empty((K, size_Ql, ctx.n), dtype=torch.int64, device=gpu)
    enc.encode_batched(size_Ql, torch.from_numpy(x).to(gpu), n, scale, c0)
    ct[:, 0] = c0
    plain = torch.empty((K, size_Ql, ctx.n), dtype=torch.int64, device=gpu)
    enc.encode_batched(size_Ql, torch.from_numpy(a).to(gpu), n, scale, plain)
    dst = torch.full((1, 2, size_Ql - 1, ctx.n), POISON, dtype=torch.int64, device=gpu)
    ctx.plain_inner_product_rescale_batched(size_Ql, plain, ct, None, K, 1, P.scheme_type.ckks, dst)
    out = torch.empty((1, n), dtype=torch.complex128, device=gpu)
    enc.decode_batched(size_Ql - 1, dst[:, 0].contiguous(), scale * scale / float(primes[size_Ql - 1]), out)
    err = float(np.max(np.abs(out.cpu().numpy()[0] - np.sum(a * x, axis=0))))
    print("end to end, max error:", err)
    assert err < 2.0 ** -20
    assert int(torch.count_nonzero(dst[:, 1])) == 0
    _release()
