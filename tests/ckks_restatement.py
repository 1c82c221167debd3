"""numpy / Python-integer restatement of the CKKS encoder (the reference's src/ckks.cu, src/fft.cu, src/rns_base.cu:49-253), written
from their description: tables, the special FFT in both directions, round-and-reduce, CRT composition into doubles.

Every butterfly is separate real multiplies and adds on float64 arrays (numpy never contracts them), so the result is the
"bit-exact" reference of the library's kernels: a complex product is (ar*br - ai*bi, ar*bi + ai*br), every operation rounded on its
own, in the radix-2 butterfly graph.  The transforms take the root table as an argument, so libm differences between the machine
that built a table and the one that checks it cannot matter."""
import math
from fractions import Fraction

import numpy as np

TWO64 = 18446744073709551616.0
PI = 3.1415926535897932384626433832795028842


def brev(x, bits):
    """The low `bits` bits of x (array or int) reversed."""
    x = np.asarray(x, dtype=np.uint64)
    out = np.zeros_like(x)
    for b in range(bits):
        out |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(bits - 1 - b)
    return out.astype(np.int64)


def group_table(m, count):
    """group[i] = 5^i mod m."""
    out, pos = np.empty(count, dtype=np.uint32), 1
    for i in range(count):
        out[i] = pos
        pos = pos * 5 % m
    return out


def roots_table(m):
    """roots[i] = e^{2 pi i * i / m} the way the reference builds it: polar() over an eighth of the circle, then the 8-fold
    symmetry.  [m][2] float64 (re, im)."""
    eighth = [(math.cos(2 * PI * i / m), math.sin(2 * PI * i / m)) for i in range(m // 8 + 1)]

    def root(i):
        i &= m - 1
        if i <= m // 8:
            return eighth[i]
        if i <= m // 4:
            re, im = eighth[m // 4 - i]
            return (im, re)
        if i <= m // 2:
            re, im = root(m // 2 - i)
            return (0.0 - re, 0.0 - (-im))
        if i <= 3 * m // 4:
            re, im = root(i - m // 2)
            return (0.0 - re, 0.0 - im)
        re, im = root(m - i)
        return (re, -im)

    return np.array([root(i) for i in range(m)], dtype=np.float64)


def roots_ulp_error(roots):
    """Largest distance, in units in the last place of the true component, of a [m][2] root table from np.longdouble cos / sin.
    The long-double reference folds every index into the first eighth of the circle first (the symmetries are exact), so its
    angle is at most pi / 4 and its own error (2^-64 relative in the angle) stays far below a double's ulp for every component,
    the small ones included; no slack is taken off."""
    m = len(roots)
    i = np.arange(m, dtype=np.int64)
    q, r = i // (m // 8), i % (m // 8)               # octant and offset
    k = np.where(q % 2 == 0, r, m // 8 - r)          # angle folded into [0, pi / 4]
    ang = 2 * np.arccos(np.longdouble(-1)) * k.astype(np.longdouble) / m
    c, s = np.cos(ang), np.sin(ang)
    swap = (q % 4 == 1) | (q % 4 == 2)               # octants 1, 2, 5, 6: |cos| and |sin| trade places
    mag = [np.where(swap, s, c), np.where(swap, c, s)]
    sign = [np.where((q >= 2) & (q <= 5), -1, 1), np.where(q >= 4, -1, 1)]
    worst = 0.0
    for col in (0, 1):
        want = mag[col] * sign[col]
        ulp = np.spacing(np.abs(want.astype(np.float64))).astype(np.longdouble)
        worst = max(worst, float(np.max(np.abs(roots[:, col].astype(np.longdouble) - want) / ulp)))
    return worst


def psi(group, log_n, log_pairs, k, m):
    """Root index of butterfly group(s) k of the stage whose pairs are 2^log_pairs apart in a transform of 2^log_n points."""
    k = np.asarray(k, dtype=np.int64)
    at = brev(k << log_pairs, log_n - 1) if log_n >= 2 else np.zeros_like(k)
    return (group[at].astype(np.int64) << log_pairs) & (m - 1)


def _stage(log_n, it):
    """(indices of the upper elements, log_pairs, butterfly groups k) of stage `it`."""
    n = 1 << log_n
    log_pairs = log_n - it - 1
    pairs = 1 << log_pairs
    t = np.arange(n // 2, dtype=np.int64)
    k, j = t >> log_pairs, t & (pairs - 1)
    return 2 * k * pairs + j, log_pairs, pairs, k


def special_ifft(re, im, roots, group, m, fix):
    """Inverse special FFT (encode) of 2^log_n points, in natural order as the reference's launcher sees them (no bit reversal);
    every element times `fix` after the last stage."""
    re, im = np.array(re, dtype=np.float64), np.array(im, dtype=np.float64)
    log_n = int(len(re)).bit_length() - 1
    for it in range(log_n - 1, -1, -1):
        g, log_pairs, pairs, k = _stage(log_n, it)
        w = roots[m - psi(group, log_n, log_pairs, k, m)]
        wr, wi = w[:, 0], w[:, 1]
        ar, ai, br, bi = re[g], im[g], re[g + pairs], im[g + pairs]
        sr, si, dr, di = ar + br, ai + bi, ar - br, ai - bi
        re[g], im[g] = sr, si
        re[g + pairs] = dr * wr - di * wi
        im[g + pairs] = dr * wi + di * wr
    return re * fix, im * fix


def special_fft(re, im, roots, group, m):
    """Forward special FFT (decode), natural order in and out."""
    re, im = np.array(re, dtype=np.float64), np.array(im, dtype=np.float64)
    log_n = int(len(re)).bit_length() - 1
    for it in range(log_n):
        g, log_pairs, pairs, k = _stage(log_n, it)
        w = roots[psi(group, log_n, log_pairs, k, m)]
        wr, wi = w[:, 0], w[:, 1]
        ar, ai, br, bi = re[g], im[g], re[g + pairs], im[g + pairs]
        with np.errstate(invalid="ignore"):       # infinite coefficients (values beyond the double range) give NaN, silently
            tr = br * wr - bi * wi
            ti = br * wi + bi * wr
            re[g], im[g] = ar + tr, ai + ti
            re[g + pairs], im[g + pairs] = ar - tr, ai - ti
    return re, im


def encode_coeffs(values, n, roots, group, scale):
    """The [2 n] float64 coefficients of a message of at most n complex values, before rounding."""
    values = np.asarray(values, dtype=np.complex128)
    assert 0 < len(values) <= n
    log_n = n.bit_length() - 1
    re, im = np.zeros(n), np.zeros(n)
    at = brev(np.arange(len(values)), log_n)
    re[at], im[at] = values.real, values.imag
    re, im = special_ifft(re, im, roots, group, 4 * n, scale / float(n))
    return np.concatenate([re, im])


def bit_count(coeffs):
    """max_coeff_bit_count = ceil(log2(max(max |coefficient|, 1))) + 1, exact (from mantissa and exponent)."""
    mx = float(np.max(np.abs(coeffs)))
    if not math.isfinite(mx):
        return 1 << 20
    if mx < 1.0:
        return 1
    man, exp = math.frexp(mx)          # mx = man * 2^exp, 0.5 <= man < 1
    return (exp - 1 if man == 0.5 else exp) + 1


def round_exact(x):
    """C round() of one double as a Python integer: nearest, halves away from zero -- from the exact rational value."""
    f = Fraction(float(x))
    r = (abs(f) + Fraction(1, 2)).__floor__()
    return -r if f < 0 else r


def round_coeffs(coeffs):
    """round_exact over an array, as a list of Python integers."""
    out = []
    for x in np.asarray(coeffs, dtype=np.float64).tolist():
        t = int(x)                       # truncation, exact
        if abs(x) < 4503599627370496.0 and abs(x - t) >= 0.5:   # x - t is exact below 2^52; above, x is integral
            t += 1 if x > 0 else -1
        out.append(t)
    return out


def residues(ints, primes):
    """[len(primes)][len(ints)] uint64: the exact integers modulo every prime, canonical."""
    if max(abs(v) for v in ints) < 1 << 62:
        a = np.array(ints, dtype=np.int64)
        return np.stack([np.mod(a, np.int64(int(q))).astype(np.uint64) for q in primes])
    return np.stack([np.array([v % int(q) for v in ints], dtype=np.uint64) for q in primes])


def compose_double(x, big_q, size, inv_scale):
    """One CRT-composed integer x in [0, Q) as the double the reference's compose kernel forms: word by word from the low word up,
    the factor 2^64 per word folded into the scale; below (Q + 1) / 2 the words of x, otherwise the signed per-word differences
    against Q's words (strictly greater: add, else subtract), in that order."""
    mask = (1 << 64) - 1
    res, f = 0.0, float(inv_scale)
    if x >= (big_q + 1) >> 1:
        for w in range(size):
            a, q = (x >> (64 * w)) & mask, (big_q >> (64 * w)) & mask
            if a > q:
                res += float(a - q) * f
            else:
                res -= float(q - a) * f if q - a else 0.0
            f *= TWO64
    else:
        for w in range(size):
            a = (x >> (64 * w)) & mask
            res += float(a) * f if a else 0.0
            f *= TWO64
    return res


def crt_values(coeff_form, primes):
    """[L][N] canonical residues -> ([N] object array of the Python integers in [0, Q), Q)."""
    primes = [int(q) for q in primes]
    big_q = 1
    for q in primes:
        big_q *= q
    terms = [(big_q // q) * pow(big_q // q, -1, q) % big_q for q in primes]
    cols = np.asarray(coeff_form, dtype=np.uint64).astype(object)
    return sum(cols[i] * terms[i] for i in range(len(primes))) % big_q, big_q


def compose_array(coeff_form, primes, inv_scale):
    """[L][N] canonical residues in coefficient form -> [N] float64: compose_double over every coefficient, word by word on arrays
    (a + (-b) is a - b, and adding the 0.0 of a skipped word changes nothing, so the bits are compose_double's)."""
    x, big_q = crt_values(coeff_form, primes)
    size, mask, half = len(primes), (1 << 64) - 1, (big_q + 1) >> 1
    upper = np.array([v >= half for v in x], dtype=bool)
    # the little-endian 64-bit words of every x, [N][size]
    words = np.frombuffer(b"".join(int(v).to_bytes(8 * size, "little") for v in x), dtype="<u8").reshape(len(x), size)
    res, f = np.zeros(len(x)), float(inv_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        for w in range(size):
            a = words[:, w].astype(np.uint64)
            q = np.uint64((big_q >> (64 * w)) & mask)
            gt = a > q
            hi = np.where(gt, a - q, np.uint64(0))
            lo = np.where(gt, np.uint64(0), q - a)
            up = np.where(gt, res + np.where(hi != 0, hi.astype(np.float64) * f, 0.0),
                          res - np.where(lo != 0, lo.astype(np.float64) * f, 0.0))
            down = res + np.where(a != 0, a.astype(np.float64) * f, 0.0)
            res = np.where(upper, up, down)
            f *= TWO64
    return res


def decode_values(coeffs, n, roots, group):
    """[2 n] float64 coefficients -> n complex values."""
    log_n = n.bit_length() - 1
    re, im = special_fft(coeffs[:n], coeffs[n:], roots, group, 4 * n)
    at = brev(np.arange(n), log_n)
    return re[at] + 1j * im[at]
