"""Parameter sets on moduli that coeff_modulus_create never draws (tests/test_modulus_shapes.py on the CPU, tests/test_gpu_modulus_shapes.py
on the GPU): NTT primes at the BOTTOM of a bit width (the first ones above 2^(b-1), among them the far side of every value threshold
the kernels branch on: 2^41 / 2^42 and 2^46 / 2^47 in make_fpmod, 2^49 / 2^50 in build_prime_tables), limbs of 16 .. 30 bits, and
the plain moduli that go with them.

The primes are committed as literals (SETS), as util.C1_PRIMES is; RECIPES says where each comes from ("the k-th prime = 1 (mod 2N)
above 2^b") and derive() re-derives them with the Miller-Rabin test below, which shares no code with the oracle."""
import functools

import numpy as np

from oracle import oracle as O

_MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)   # deterministic below 3.3 * 10^24 (Sorenson, Webster 2015), so below 2^64


def is_prime(n):
    """Deterministic Miller-Rabin for n < 2^64."""
    n = int(n)
    if n < 2:
        return False
    for p in _MR_BASES:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in _MR_BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def primes_above(lo, two_n, count, skip=0):
    """The primes = 1 (mod two_n) greater than lo, ascending: `count` of them after the first `skip`."""
    out, c = [], (int(lo) // two_n) * two_n + 1
    if c <= lo:
        c += two_n
    while len(out) < skip + count:
        if is_prime(c):
            out.append(c)
        c += two_n
    return out[skip:]


def primes_below(hi, two_n, count):
    """The `count` largest primes = 1 (mod two_n) smaller than hi, descending."""
    out, c = [], ((int(hi) - 2) // two_n) * two_n + 1
    while len(out) < count and c > 1:
        if is_prime(c):
            out.append(c)
        c -= two_n
    return out


# name: (log_n, data limbs, special limbs); a limb group is (b, k, count): the k-th .. (k + count - 1)-th prime = 1 (mod 2N) above 2^b
_EDGE = [(59, 1, 1), (49, 1, 2), (47, 1, 1), (46, 1, 1), (42, 1, 1), (41, 1, 1), (50, 1, 1)]
RECIPES = {
    "edge12": (12, _EDGE, [(60, 1, 2)]),        # the far side of every threshold; alpha 2, beta 4, lower levels have a short digit
    "edge14": (14, _EDGE, [(60, 1, 2)]),        # the same at N = 2^14: other NTT plan, other FP64 re-centring schedule
    "small12": (12, [(29, 9, 6)], [(59, 1, 2)]),   # 30-bit limbs at the bottom of their width
    "tiny12": (12, [(18, 1, 4)], [(59, 1, 2)]),    # 19-bit limbs
    "pair12": (12, [(15, 1, 2)], []),           # 40961 and 65537 as the limbs of a chain of their own (NTT and dyadic rows only)
    "low50": (12, [(49, 9, 4)], [(59, 1, 2)]),     # BFV with all three multiplies possible
    "low60": (12, [(59, 9, 3)], [(59, 12, 2)]),    # BFV, all-integer back end
    "bottom50": (12, [(49, 1, 3)], [(59, 1, 2)]),  # no room for the HPS base R below the data primes
}


def derive(name):
    """(log_n, primes of QP, special count) of a set from its recipe."""
    log_n, data, special = RECIPES[name]
    two_n = 2 << log_n
    qp = [p for b, k, count in data + special for p in primes_above(1 << b, two_n, count, k - 1)]
    return log_n, qp, sum(count for _, _, count in special)


SETS = {
    "edge12": (12, [576460752303439873, 562949954093057, 562949954142209, 140737488486401, 70368744210433, 4398046568449, 2199023288321,
                    1125899906949121, 1152921504606904321, 1152921504606994433], 2),
    "edge14": (14, [576460752304439297, 562949954142209, 562949954961409, 140737488486401, 70368744210433, 4398047232001, 2199023288321,
                    1125899908022273, 1152921504607338497, 1152921504608747521], 2),
    "small12": (12, [537444353, 537542657, 537591809, 537673729, 537722881, 537763841, 576460752303439873, 576460752303702017], 2),
    "tiny12": (12, [270337, 286721, 319489, 417793, 576460752303439873, 576460752303702017], 2),
    "pair12": (12, [40961, 65537], 0),
    "low50": (12, [562949954838529, 562949954879489, 562949954961409, 562949955010561, 576460752303439873, 576460752303702017], 2),
    "low60": (12, [576460752305569793, 576460752305799169, 576460752305872897, 576460752305889281, 576460752305922049], 2),
    "bottom50": (12, [562949954093057, 562949954142209, 562949954224129, 576460752303439873, 576460752303702017], 2),
}

# Plain moduli.  T40: the largest prime = 1 (mod 8192) below 2^40; T59: the third largest below 2^59 (tests/test_emu_decrypt.py's T59);
# "below": the largest batching prime (= 1 mod 8192) below 2^(b - 1), b the bit length of the set's smallest data prime -- under every
# data prime, yet within a factor two of it.
T40 = 1099511480321
T59 = 576460752303185921
PLAIN_BELOW = {"edge12": 2199023190017, "small12": 536813569, "tiny12": 188417, "low50": 562949953216513, "low60": 576460752303415297}


def plain_modulus(name, label):
    """A plain modulus by label: "2", "257", "40961", "t40", "below" (of the set `name`), "T59"."""
    return PLAIN_BELOW[name] if label == "below" else {"2": 2, "257": 257, "40961": 40961, "t40": T40, "T59": T59}[label]


def data_primes(name):
    log_n, qp, size_p = SETS[name]
    return qp[:len(qp) - size_p]


def primes_of(name):
    """(log_n, primes of QP, special count) of a set of this file or of util.CONFIGS."""
    if name not in SETS:
        import util
        return util.primes_of(name)
    log_n, qp, size_p = SETS[name]
    return log_n, tuple(qp), size_p


@functools.lru_cache(maxsize=None)
def oracle_ctx(name):
    log_n, qp, size_p = primes_of(name)
    return O.Ctx(log_n, list(qp), size_p)


def seed_of(name, *tag):
    return [0x5AFE] + [int.from_bytes(str(x).encode(), "little") % (1 << 32) for x in (name,) + tag]


def edge_inputs(rng, primes, n):
    """[3][L][n]: uniform residues, every word q - 1, and q - 1 - r with r < 2^10 (the top of the range, where a lazy reduction
    that is one subtraction short shows)."""
    q = np.array([int(p) for p in primes], dtype=np.uint64)[:, None]
    uni = np.stack([rng.integers(0, int(p), n, dtype=np.uint64) for p in primes])
    top = np.broadcast_to(q - np.uint64(1), uni.shape).copy()
    near = q - np.uint64(1) - rng.integers(0, 1 << 10, uni.shape, dtype=np.uint64)
    return np.stack([uni, top, near])


def compose(coeff, primes, at=None):
    """CRT in Python integers of coeff [L][N] at the positions `at` (default all): (list of values in [0, Q), Q)."""
    primes = [int(p) for p in primes]
    big = 1
    for p in primes:
        big *= p
    w = [(big // p) * pow(big // p, -1, p) % big for p in primes]
    at = range(coeff.shape[1]) if at is None else at
    return [sum(int(coeff[l, k]) * w[l] for l in range(len(primes))) % big for k in at], big


def negacyclic_ints(a, b, modulus):
    """a b mod (X^N + 1, modulus) of two length-N sequences of integers in [0, modulus), exactly, as a list of Python integers:
    Kronecker substitution (one big-integer product)."""
    n, modulus = len(a), int(modulus)
    width = (2 * (modulus - 1).bit_length() + n.bit_length() + 7) // 8 + 1           # bytes per packed coefficient
    pack = lambda v: int.from_bytes(b"".join(int(x).to_bytes(width, "little") for x in v), "little")
    raw = (pack(a) * pack(b)).to_bytes(2 * n * width, "little")
    c = [int.from_bytes(raw[i * width:(i + 1) * width], "little") for i in range(2 * n)]
    return [(c[i] - c[i + n]) % modulus for i in range(n)]


def negacyclic_product(a, b, t):
    """The same for words below t < 2^63, as a uint64 array."""
    return np.array(negacyclic_ints(a, b, t), dtype=np.uint64)


class Keyed:
    """One set (of this file or util.CONFIGS) with a ternary secret key: encryption through encrypt_restatement.Restatement with noise
    in [-21, 21], and a decryption that uses the oracle only for the phase (transforms, dyadic products, sums -- pinned by their
    definitions in tests/test_modulus_shapes.py): the CRT, the scaling and the rounding are Python integers."""
    NOISE = 21

    def __init__(self, name, spec=None):
        """spec: (log_n, primes of QP, special count) of a chain that is no named set; `name` then only seeds the randomness."""
        from encrypt_restatement import residues
        self.name = name
        self.log_n, self.primes, self.size_p = primes_of(name) if spec is None else (spec[0], tuple(spec[1]), spec[2])
        self.n, self.size_q = 1 << self.log_n, len(self.primes) - self.size_p
        self.oc = oracle_ctx(name) if spec is None else O.Ctx(self.log_n, list(self.primes), self.size_p)
        self.sk = np.random.default_rng(seed_of(name, "sk")).integers(-1, 2, self.n)
        res = residues(self.sk, self.primes)
        self.sk_ntt = np.concatenate([self.oc.nwt_forward(res[:self.size_q], self.size_q, 0)] +
                                     ([self.oc.nwt_forward(res[self.size_q:], self.size_p, self.size_q)] if self.size_p else []))

    def messages(self, t, count, tag="m"):
        """[count][N] below t: the first four coefficients t - 1, the rest uniform."""
        m = np.random.default_rng(seed_of(self.name, tag, t)).integers(0, int(t), (count, self.n), dtype=np.uint64)
        m[:, :4] = int(t) - 1
        return m

    def encrypt(self, kind, t, plain, level, tag):
        from encrypt_restatement import Restatement
        rng = np.random.default_rng(seed_of(self.name, "enc", tag, t))
        a = np.stack([rng.integers(0, int(q), self.n, dtype=np.uint64) for q in self.primes[:level]])
        e = rng.integers(-self.NOISE, self.NOISE + 1, self.n)
        return Restatement(self.oc, kind, t).symmetric(self.sk_ntt, a, e, np.ascontiguousarray(plain, dtype=np.uint64), level)

    def phase(self, kind, ct, level):
        """c0 + sum_i c_i s^i in coefficient form, [level][N] (bv_semantics.BvScheme.phase)."""
        oc, s = self.oc, np.ascontiguousarray(self.sk_ntt[:level])
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        ntt = ct if kind == O.BGV else np.stack([oc.nwt_forward(c, level, 0) for c in ct])
        acc, power = None, s
        for i in range(1, len(ct)):
            term = oc.multiply(ntt[i], power, level)
            acc = term if acc is None else oc.add(acc, term, level)
            power = oc.multiply(power, s, level)
        if kind == O.BGV:
            return oc.nwt_backward(oc.add(ntt[0], acc, level), level, 0)
        return oc.add(ct[0], oc.nwt_backward(acc, level, 0), level)

    def decrypt(self, kind, t, ct, level, with_norm=False):
        """-> (plaintext [N] below t -- BGV: before any correction factor --, margin in bits, as bv_semantics.BvScheme.decrypt);
        with_norm: also the exact noise norm (BFV: of t * phase, BGV: of the phase) and Q_l."""
        import math
        t = int(t)
        v, big = compose(self.phase(kind, ct, level), self.primes[:level])
        if kind == O.BGV:
            centred = [x - big if x > big // 2 else x for x in v]
            worst = max(abs(x) for x in centred)
            plain = [x % t for x in centred]
        else:
            scaled = [x * t for x in v]
            worst = max(min(x % big, big - x % big) for x in scaled)
            plain = [((x + big // 2) // big) % t for x in scaled]
        margin = math.log2(big // 2) - (math.log2(worst) if worst else 0.0)
        plain = np.array(plain, dtype=np.uint64)
        return (plain, margin, worst, big) if with_norm else (plain, margin)


@functools.lru_cache(maxsize=None)
def keyed(name):
    return Keyed(name)


# ---- the BFV matrix ------------------------------------------------------------------------------------------------------------------
VARIANTS = ("behz", "hps", "overq")
IN, OUT, REFUSED = "in-domain", "out-of-domain", "refused"
_NO_ROOM = "base R has no room for the scaled product: t sqrt(2N) 4/3 >= R / Q (DESIGN.md 4.8a1)"
_NO_BASE = "no base R: the walk down from the smallest data prime to 2^(bits - 1) finds too few primes"
# (set, plain modulus label): {variant: (status, reason)}; a variant that is not named is in-domain
_HPS_OUT = {"hps": (OUT, _NO_ROOM)}
_TINY = {"hps": (REFUSED, _NO_BASE), "overq": (REFUSED, _NO_BASE)}
BFV_CELLS = {
    ("low50", "t40"): {}, ("low50", "below"): _HPS_OUT, ("low50", "T59"): _HPS_OUT,
    ("small12", "2"): {}, ("small12", "257"): {}, ("small12", "40961"): {}, ("small12", "below"): _HPS_OUT,
    ("low60", "40961"): {}, ("low60", "t40"): {}, ("low60", "T59"): _HPS_OUT,
    ("tiny12", "2"): _TINY, ("tiny12", "257"): _TINY, ("tiny12", "40961"): _TINY,
    ("hyb12_a2", "T59"): _HPS_OUT,
}


# hps_overq_leveled one level down (low50, low60): in-domain at every plain modulus of the matrix but this one, where the product
# keeps 40 bits of margin at the full level and the dropped limb has 59: the scaled product's noise does not fit Q_l / (2 t).
LEVELED_OUT = {("low60", "T59"): "no noise room one level down: margin 40 bits at the full level, the dropped limb has 59"}


def hps_has_room(q, r, t, n):
    """The room condition of plain HPS: the scaled tensor t d / Q must stay inside (-R / 2, R / 2).  A coefficient of
    d = c0 c1' + c1 c0' is a sum of 2N products of residues uniform in (-Q / 2, Q / 2): standard deviation sqrt(2N) Q^2 / 12; eight
    of them scaled by t / Q are t sqrt(2N) Q 2 / 3, which has to stay below R / 2: 16 t^2 2N Q^2 < 9 R^2."""
    big_q = big_r = 1
    for p in q:
        big_q *= int(p)
    for p in r:
        big_r *= int(p)
    return 16 * int(t) ** 2 * 2 * n * big_q ** 2 < 9 * big_r ** 2


def cell_status(name, label, variant):
    return BFV_CELLS[(name, label)].get(variant, (IN, ""))


def in_domain_cells():
    return [(name, label, v) for (name, label) in BFV_CELLS for v in VARIANTS if cell_status(name, label, v)[0] == IN]


def multiplier(variant, oc, t, size_ql=None):
    if variant == "behz":
        return O.Behz(oc, t)
    if variant == "hps":
        return O.Hps(oc, t)
    return O.HpsOverQ(oc, t, size_ql) if size_ql else O.HpsOverQ(oc, t)


@functools.lru_cache(maxsize=None)
def bfv_operands(name, label):
    """(t, messages [2][N], fresh ciphertexts [2][2][Q][N], the exact negacyclic product of the messages modulo t)."""
    k = keyed(name)
    t = plain_modulus(name, label)
    m = k.messages(t, 2)
    cts = np.stack([k.encrypt(O.BFV, t, m[i], k.size_q, i) for i in range(2)])
    return t, m, cts, negacyclic_product(m[0], m[1], t)


# ---- operands and references of the sum kernels (tests/test_gpu_modulus_shapes.py) ---------------------------------------------------------
BLOCK = 64


def planted(rng, primes, lead, n):
    """[*lead][L][N] uniform residues with, in every polynomial at the same positions, blocks of q - 1, (q - 1) / 2, (q + 1) / 2 and 0
    at both ends (the extreme products line up across the terms of a sum) and next to them a block of floor(sqrt(q / 2)), whose
    square is just below q / 2 with the same sign in every term: an FP64 accumulator grows fastest there."""
    import math
    out = np.empty(tuple(lead) + (len(primes), n), dtype=np.uint64)
    for j, q in enumerate(primes):
        q = int(q)
        out[..., j, :] = rng.integers(0, q, tuple(lead) + (n,), dtype=np.uint64)
        for at in (0, n - 4 * BLOCK):
            for i, v in enumerate((q - 1, (q - 1) // 2, (q + 1) // 2, 0)):
                out[..., j, at + i * BLOCK:at + (i + 1) * BLOCK] = v
        for at in (4 * BLOCK, n - 5 * BLOCK):
            out[..., j, at:at + BLOCK] = math.isqrt(q // 2)
    return out


def tensor_sums(oc, a, b, limbs, upto):
    """{k: sum over the first k terms of tensor_prod_2x2(a[i], b[i])} for k in upto, with the oracle's product and add."""
    acc, out = None, {}
    for k in range(max(upto)):
        p = oc.tensor_prod_2x2(a[k], b[k], limbs)
        acc = p if acc is None else np.stack([oc.add(acc[i], p[i], limbs) for i in range(3)])
        if k + 1 in upto:
            out[k + 1] = acc.copy()
    return out


def plain_sums(oc, plain, ct, limbs, upto):
    """{k: sum over the first k terms of plain[i] (.) ct[i][p], both polynomials} for k in upto."""
    s, out = None, {}
    for k in range(max(upto)):
        prod = [oc.multiply(plain[k], ct[k][p], limbs) for p in range(2)]
        s = prod if s is None else [oc.add(s[p], prod[p], limbs) for p in range(2)]
        if k + 1 in upto:
            out[k + 1] = np.stack(s)
    return out


def add_ct(oc, a, b, limbs):
    return np.stack([oc.add(a[p], b[p], limbs) for p in range(2)])
