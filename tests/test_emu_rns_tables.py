"""The constants of the RNS tools (phantom-fhe_amd/csrc/pha_rns_tables.h: what Context::tool / hps / hps_overq / behz upload), held on
the CPU against their definitions -- no GPU needed.  Harness: tests/emu/emu_rns_tables.cpp (test-only).

The expected values are NOT read off the code under test: Python integers compute them from the definitions (qhat_i = prod / q_i,
exact rationals for the scale-and-round tables), and the carry-free form of a converter is the rule written in front of
BConv::split_kind (pha_internal.h) and beside BConvTables (pha_rns_tables.h).
"""
import ctypes as C
import os
import subprocess
from fractions import Fraction
from math import prod

import numpy as np
import pytest

from util import chain_primes, primes_of

HERE = os.path.dirname(os.path.abspath(__file__))
T = 65537
U64, U32 = np.uint64, np.uint32


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_rns_tables") / "libemu_rns_tables.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "emu", "emu_rns_tables.cpp")])
    L = C.CDLL(out)
    L.emu_behz_size_b.restype = C.c_uint32
    L.emu_digit.restype = C.c_int
    return L


def a64(v):
    return np.array([int(x) for x in v], dtype=U64)


def a32(v):
    return np.array([int(x) for x in v], dtype=U32)


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def sz(n):
    return C.c_size_t(n)


def shoup(v, q):
    return (v << 64) // q


def pairs(flat):
    return [(int(flat[2 * i]), int(flat[2 * i + 1])) for i in range(len(flat) // 2)]


def is_prime(n):
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:                    # these twelve bases decide every n < 2^64
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


def primes_down(start, step, count):
    out = []
    while len(out) < count:
        if is_prime(start):
            out.append(start)
        start -= step
    return out


# ---- converters --------------------------------------------------------------------------------------------------------------------
def split_rule(P, ip, op, family=0):
    """(kind, mont, r90, row_pad, cut of the matrix entries): the comment in front of BConv::split_kind."""
    widest = max(len(ip), family)
    by = max((P[r] - 1).bit_length() for r in ip)      # residues of the inputs are below 2^by
    bm = max((P[r] - 1).bit_length() for r in op)      # matrix entries are residues of the outputs
    if widest <= 16 and by <= 60 and bm <= 60:
        kind = 1
    elif widest <= 32 and by <= 60 and bm <= 62:
        kind = 2
    elif widest <= 32 and by <= 62 and bm <= 60:
        kind = 3
    else:
        kind = 0
    row_pad = 32 if kind >= 2 and len(ip) > 16 else 16
    mont = (kind == 1 or (kind != 0 and sum(P[r] for r in ip) < 2 ** 64)) and all(P[r] & 1 for r in op)
    r90 = mont and kind == 1 and widest <= 15
    return kind, mont, r90, row_pad, 31 if kind == 2 else 30


def run_bconv(emu, P, ip, op, out_scale=None, in_scale=1, family=0, var1=False):
    isz, osz = len(ip), len(op)
    hat, mat, mat30, oninv, meta = np.zeros(2 * isz, U64), np.zeros(osz * isz, U64), np.zeros(osz * 32 * 2, U32), np.zeros(osz, U64), np.zeros(4, U32)
    pa, ia, oa = a64(P), a32(ip), a32(op)
    osa = a64(out_scale) if out_scale is not None else None
    emu.emu_bconv(ptr(pa), sz(len(P)), ptr(ia), sz(isz), ptr(oa), sz(osz), ptr(osa) if osa is not None else None, C.c_uint64(in_scale),
                  C.c_uint32(family), C.c_int(1 if var1 else 0), ptr(hat), ptr(mat), ptr(mat30), ptr(oninv), ptr(meta))
    return hat, mat, mat30, oninv, meta


def check_conv(P, ip, op, got, out_scale=None, in_scale=1, family=0, var1=False):
    """Every table of one converter against the definitions.  Returns the kind."""
    hat, mat, mat30, oninv, meta = got
    isz, osz = len(ip), len(op)
    Q = prod(P[r] for r in ip)
    want_hat, want_mat = [], [[0] * isz for _ in range(osz)]
    for i, r in enumerate(ip):
        q = P[r]
        inv = pow(Q // q, -1, q)
        v = (q - prod(P[o] for o in op) * inv % q) % q if var1 else in_scale * inv % q
        want_hat.append((v, shoup(v, q)))
    for j, o in enumerate(op):
        p = P[o]
        for i, r in enumerate(ip):
            want_mat[j][i] = pow(P[r], -1, p) if var1 else (Q // P[r]) * (out_scale[j] if out_scale is not None else 1) % p
    assert pairs(hat) == want_hat
    assert [int(x) for x in mat] == [v for row in want_mat for v in row]
    kind, mont, r90, row_pad, cut = split_rule(P, ip, op, family)
    assert [int(x) for x in meta] == [kind, int(mont), int(r90), row_pad]
    for j, o in enumerate(op):
        p = P[o]
        assert int(oninv[j]) == ((-pow(p, -1, 2 ** 64)) % 2 ** 64 if mont else 0)
        if mont:
            assert int(oninv[j]) * p % 2 ** 64 == 2 ** 64 - 1
    m30 = mat30[:osz * row_pad * 2].reshape(osz, row_pad, 2)
    assert not mat30[osz * row_pad * 2:].any()
    if isz <= row_pad:
        radix = (2 ** 90 if r90 else 2 ** 64) if mont else 1
        for j, o in enumerate(op):
            for i in range(row_pad):
                lo, hi = int(m30[j, i, 0]), int(m30[j, i, 1])
                assert lo < 2 ** cut
                assert lo + (hi << cut) == (want_mat[j][i] * radix % P[o] if i < isz else 0)
    else:
        assert not m30.any()
    return kind


def level(name, size_ql):
    """(prime table, rows of Ql, rows of P, limb -> row of [Ql || P])"""
    _, primes, size_p = primes_of(name)
    size_q = len(primes) - size_p
    data, special = list(range(size_ql)), list(range(size_q, size_q + size_p))
    return [int(p) for p in primes], data, special, data + special


# (set, data limbs, kinds of the digits, kind of P -> Ql): the smallest sets that reach each branch
_LEVELS = [
    ("hyb12_a2", 6, [1, 1, 1], 1),
    ("hyb12_a2", 5, [1, 1, 1], 1),          # short last digit
    ("c1_bfv4096", 2, [1, 1], 1),           # alpha = 1
    ("p61_a2", 6, [2, 2, 2], 3),            # 61-bit special primes: 30 / 31 cuts going up, 31 / 30 coming down
    ("wide_p20", 24, [2, 2], 2),            # row pitch 32; digits of 20 and 4 limbs
    ("wide_p33", 6, [0], 0),                # more than 32 inputs: no carry-free form
]
_LEVEL_IDS = [f"{c[0]}-{c[1]}" for c in _LEVELS]


@pytest.mark.parametrize("name,size_ql,digit_kinds,down_kind", _LEVELS, ids=_LEVEL_IDS)
def test_digit_converters_and_part_hat_inv(emu, name, size_ql, digit_kinds, down_kind):
    P, data, special, qlp = level(name, size_ql)
    alpha = len(special)
    beta = -(-size_ql // alpha)
    assert beta == len(digit_kinds)
    want_part = []
    for b in range(beta):
        own = list(range(b * alpha, min((b + 1) * alpha, size_ql)))
        ip = [qlp[j] for j in own]
        op = [qlp[j] for j in range(len(qlp)) if j not in own]
        isz, osz = len(ip), len(op)
        gi, go, cnt = np.zeros(len(qlp), U32), np.zeros(len(qlp), U32), np.zeros(2, U32)
        hat, mat, mat30, oninv, meta = np.zeros(2 * isz, U64), np.zeros(osz * isz, U64), np.zeros(osz * 32 * 2, U32), np.zeros(osz, U64), np.zeros(4, U32)
        part = np.zeros(2 * size_ql, U64)
        pa, qa = a64(P), a32(qlp)
        n = emu.emu_digit(ptr(pa), sz(len(P)), ptr(qa), sz(len(qlp)), C.c_uint32(size_ql), C.c_uint32(alpha), C.c_uint32(b), ptr(gi), ptr(go),
                          ptr(cnt), ptr(hat), ptr(mat), ptr(mat30), ptr(oninv), ptr(meta), ptr(part))
        assert n == beta
        assert [int(x) for x in cnt] == [isz, osz]
        assert [int(x) for x in gi[:isz]] == ip and [int(x) for x in go[:osz]] == op
        assert check_conv(P, ip, op, (hat, mat, mat30, oninv, meta), family=alpha) == digit_kinds[b]
        Qd = prod(P[r] for r in ip)
        want_part += [(pow(Qd // P[r], -1, P[r]), shoup(pow(Qd // P[r], -1, P[r]), P[r])) for r in ip]
    assert pairs(part) == want_part and len(want_part) == size_ql     # the digits' phase-1 factors, concatenated by data limb
    if name == "wide_p20":
        assert int(meta[3]) == 16         # the 4-limb last digit keeps the 16-entry pitch next to the 20-limb one's 32


@pytest.mark.parametrize("name,size_ql,digit_kinds,down_kind", _LEVELS, ids=_LEVEL_IDS)
def test_p_to_ql_pinv_and_the_level_constants(emu, name, size_ql, digit_kinds, down_kind):
    P, data, special, _ = level(name, size_ql)
    big_p = prod(P[r] for r in special)
    pa, sa = a64(P), a32(special)
    p_mod_q, p_inv = np.zeros(size_ql, U64), np.zeros(size_ql, U64)
    emu.emu_prod_mod_limbs(ptr(pa), sz(len(P)), ptr(sa), sz(len(special)), C.c_uint32(size_ql), C.c_int(0), ptr(p_mod_q))
    emu.emu_prod_mod_limbs(ptr(pa), sz(len(P)), ptr(sa), sz(len(special)), C.c_uint32(size_ql), C.c_int(1), ptr(p_inv))
    assert [int(x) for x in p_mod_q] == [big_p % P[i] for i in data]
    assert [int(x) for x in p_inv] == [pow(big_p, -1, P[i]) for i in data]
    last = a32([size_ql - 1])
    inv_q_last = np.zeros(size_ql - 1, U64)
    emu.emu_prod_mod_limbs(ptr(pa), sz(len(P)), ptr(last), sz(1), C.c_uint32(size_ql - 1), C.c_int(1), ptr(inv_q_last))
    assert [int(x) for x in inv_q_last] == [pow(P[size_ql - 1], -1, P[i]) for i in range(size_ql - 1)]
    assert check_conv(P, special, data, run_bconv(emu, P, special, data)) == down_kind
    scale = [int(x) for x in p_inv]
    assert check_conv(P, special, data, run_bconv(emu, P, special, data, out_scale=scale), out_scale=scale) == down_kind


def test_the_sets_reach_every_form():
    """kinds 0..3, Montgomery with both radices and without, both row pitches: what the cases above are chosen for."""
    seen = set()
    for name, size_ql, _, _ in _LEVELS:
        P, data, special, qlp = level(name, size_ql)
        alpha = len(special)
        seen.add(split_rule(P, special, data)[:4])
        for b in range(-(-size_ql // alpha)):
            own = list(range(b * alpha, min((b + 1) * alpha, size_ql)))
            seen.add(split_rule(P, [qlp[j] for j in own], [qlp[j] for j in range(len(qlp)) if j not in own], alpha)[:4])
    assert {s[0] for s in seen} == {0, 1, 2, 3}
    assert {s[3] for s in seen} == {16, 32}
    assert (1, True, True, 16) in seen and any(s[1] and not s[2] for s in seen) and any(not s[1] for s in seen)


# ---- plain-modulus constants ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size_ql", [("c1_bfv4096", 2), ("bfv13_50", 4), ("bfv13_50", 3)])
def test_plain_modulus_constants(emu, name, size_ql):
    P, data, special, _ = level(name, size_ql)
    scal, qlq, phat, tinv, inc = np.zeros(6, U64), np.zeros(size_ql - 1, U64), np.zeros(len(special), U64), np.zeros(size_ql, U64), np.zeros(size_ql, U64)
    pa, sa = a64(P), a32(special)
    emu.emu_plain(ptr(pa), sz(len(P)), C.c_uint32(size_ql), ptr(sa), sz(len(special)), C.c_uint64(T), ptr(scal), ptr(qlq), ptr(phat), ptr(tinv), ptr(inc))
    q_last, big_p, big_q = P[size_ql - 1], prod(P[r] for r in special), prod(P[i] for i in data)
    want = [pow(q_last, -1, T), pow(big_p, -1, T), (-big_q) % T]
    assert pairs(scal) == [(v, shoup(v, T)) for v in want]
    assert [int(x) for x in qlq] == [q_last % P[i] for i in range(size_ql - 1)]
    assert [int(x) for x in phat] == [big_p // P[r] % T for r in special]
    assert [int(x) for x in tinv] == [pow(T, -1, P[i]) for i in data]
    assert [int(x) for x in inc] == [P[i] - T for i in data]


# ---- BFV multiply: HPS, HPS over Q, BEHZ on bfv13_50 with t = 65537 ---------------------------------------------------------------------
def bfv_set():
    log_n, primes, size_p = primes_of("bfv13_50")
    P = [int(p) for p in primes]
    return log_n, P, len(P) - size_p


def hps_table(P0, size_q, log_n):
    """the prime table after Context::hps: |Q| + 1 primes below the smallest q_i, descending in steps of 2N (get_primes_below)"""
    r = primes_down(min(P0[:size_q]) - (2 << log_n), 2 << log_n, size_q + 1)
    return P0 + r, list(range(len(P0), len(P0) + size_q + 1))


def check_alpha(emu, P, ib, ob):
    out = np.zeros((len(ib) + 1) * len(ob), U64)
    pa, ia, oa = a64(P), a32(ib), a32(ob)
    emu.emu_alpha_table(ptr(pa), sz(len(P)), ptr(ia), sz(len(ib)), ptr(oa), sz(len(ob)), ptr(out))
    big = prod(P[r] for r in ib)
    assert [int(x) for x in out] == [a * big % P[o] for a in range(len(ib) + 1) for o in ob]


def check_scale_round(emu, P, away, keep, factor):
    """x_s = factor prod(keep) ((S / s)^-1 mod s) over S = away u keep; the tables are the parts of the exact rational x_s / s."""
    na, nk = len(away), len(keep)
    frac, tab = np.zeros(na, np.float64), np.zeros(nk * (na + 1), U64)
    pa, aa, ka = a64(P), a32(away), a32(keep)
    emu.emu_scale_round(ptr(pa), sz(len(P)), ptr(aa), sz(na), ptr(ka), sz(nk), C.c_uint64(factor), ptr(frac), ptr(tab))
    S = prod(P[r] for r in away + keep)
    K = prod(P[r] for r in keep)
    tab = tab.reshape(nk, na + 1)
    for a, r in enumerate(away):
        s = P[r]
        x = Fraction(factor * K * pow(S // s, -1, s), s)
        whole = x.numerator // x.denominator
        rest = x - whole
        # the harness divides two doubles: three roundings of relative 2^-53 on a value below 1
        assert abs(Fraction(float(frac[a])) - rest) <= Fraction(1, 2 ** 51)
        assert float(frac[a]) == float(rest.numerator) / float(s)
        assert [int(tab[k, a]) for k in range(nk)] == [whole % P[kr] for kr in keep]
    for k, r in enumerate(keep):
        s = P[r]
        assert int(tab[k, na]) == (factor * K * pow(S // s, -1, s) // s) % s


def test_hps_tables(emu):
    log_n, P0, size_q = bfv_set()
    P, R = hps_table(P0, size_q, log_n)
    Q = list(range(size_q))
    assert all(is_prime(P[r]) and P[r] % (2 << log_n) == 1 and P[r] < min(P0[:size_q]) for r in R)
    for ib, ob in ((Q, R), (R, Q)):
        check_conv(P, ib, ob, run_bconv(emu, P, ib, ob))
        check_alpha(emu, P, ib, ob)
    check_scale_round(emu, P, Q, R, T)          # t R / (Q R) into R


@pytest.mark.parametrize("size_ql", [4, 3], ids=["top", "one-level-dropped"])
def test_hps_overq_tables(emu, size_ql):
    log_n, P0, size_q = bfv_set()
    assert size_q == 4
    P, R = hps_table(P0, size_q, log_n)
    Ql, Rl, dropped = list(range(size_ql)), R[:size_ql], list(range(size_ql, size_q))
    for ib, ob in ((Ql, Rl), (Rl, Ql)):
        check_conv(P, ib, ob, run_bconv(emu, P, ib, ob))
        check_alpha(emu, P, ib, ob)
    full = list(range(size_q)) if dropped else Ql
    check_conv(P, full, Rl, run_bconv(emu, P, full, Rl, var1=True), var1=True)
    check_scale_round(emu, P, Rl, Ql, T)        # t Ql / (Ql Rl) into Ql
    if dropped:
        check_scale_round(emu, P, dropped, Ql, 1)   # Ql / Q into Ql
        out = np.zeros(size_ql, U64)
        pa, da = a64(P), a32(dropped)
        emu.emu_prod_mod_limbs(ptr(pa), sz(len(P)), ptr(da), sz(len(dropped)), C.c_uint32(size_ql), C.c_int(0), ptr(out))
        assert [int(x) for x in out] == [prod(P[r] for r in dropped) % P[i] for i in Ql]


def test_behz_tables(emu):
    log_n, P0, size_q = bfv_set()
    two_n = 2 << log_n
    # |B| = |Q|, plus one when 32 + |t| + |prod q| bits reach 61 |Q| + 61
    big_q = prod(P0[:size_q])
    size_b = size_q + (1 if 32 + T.bit_length() + big_q.bit_length() >= 61 * size_q + 61 else 0)
    pq = a64(P0[:size_q])
    assert emu.emu_behz_size_b(ptr(pq), C.c_uint32(size_q), C.c_uint64(T)) == size_b == size_q
    wide = [int(p) for p in chain_primes(12, (61, 61))]      # the other side of the rule: two 61-bit primes and a 40-bit t
    t40 = (1 << 39) + 1
    assert 32 + t40.bit_length() + (wide[0] * wide[1]).bit_length() >= 61 * 2 + 61
    pw = a64(wide)
    assert emu.emu_behz_size_b(ptr(pw), C.c_uint32(2), C.c_uint64(t40)) == 3
    # m_sk, then B: 61-bit primes descending from 2^61 - 2N + 1; the table holds B, m_sk, m_tilde = 2^32
    found = primes_down(2 ** 61 - two_n + 1, two_n, size_b + 1)
    m_sk, B, mt = found[0], found[1:], 2 ** 32
    aux0 = len(P0)
    P = P0 + B + [m_sk, mt]
    Q, rB, rBsk, r_msk, r_mt = list(range(size_q)), list(range(aux0, aux0 + size_b)), list(range(aux0, aux0 + size_b + 1)), aux0 + size_b, aux0 + size_b + 1
    # Q -> Bsk u {m_tilde}: the phase-1 factors carry m_tilde (= Behz::mt_qhatinv); the even output keeps Barrett rows
    got = run_bconv(emu, P, Q, rBsk + [r_mt], in_scale=mt)
    check_conv(P, Q, rBsk + [r_mt], got, in_scale=mt)
    assert int(got[4][1]) == 0
    assert pairs(got[0]) == [(mt * pow(big_q // P[i], -1, P[i]) % P[i], shoup(mt * pow(big_q // P[i], -1, P[i]) % P[i], P[i])) for i in Q]
    for ib, ob in ((Q, rBsk), (rB, Q), (rB, [r_msk])):
        check_conv(P, ib, ob, run_bconv(emu, P, ib, ob))
    nbsk = size_b + 1
    pb, wb, wq, tqb, sc = np.zeros(4 * nbsk, U64), np.zeros(nbsk, U64), np.zeros(size_q, U64), np.zeros(2 * (size_q + nbsk), U64), np.zeros(4, U64)
    pa = a64(P)
    emu.emu_behz(ptr(pa), sz(len(P)), C.c_uint32(size_q), C.c_uint32(aux0), C.c_uint32(size_b), C.c_uint64(T), ptr(pb), ptr(wb), ptr(wq), ptr(tqb), ptr(sc))
    big_b = prod(B)
    bsk = [P[r] for r in rBsk]
    assert [int(x) for x in wb] == [big_q % p for p in bsk]
    assert pairs(pb[:2 * nbsk]) == [(pow(big_q, -1, p), shoup(pow(big_q, -1, p), p)) for p in bsk]
    assert pairs(pb[2 * nbsk:]) == [(pow(mt, -1, p), shoup(pow(mt, -1, p), p)) for p in bsk]
    assert [int(x) for x in wq] == [big_b % P[i] for i in Q]
    limbs = [P[i] for i in Q] + bsk
    assert [int(x) for x in tqb] == [T] * len(limbs) + [shoup(T, p) for p in limbs]
    neg = (-pow(big_q, -1, mt)) % mt
    inv = pow(big_b, -1, m_sk)
    assert pairs(sc) == [(neg, shoup(neg, mt)), (inv, shoup(inv, m_sk))]


def test_behz_scale_by_a_plain_modulus_above_the_data_primes(emu):
    """t = T59 (59 bits) on a chain with 40-bit limbs: the per-limb factor of the scaled inverse transform is t mod q_i with ITS Shoup
    quotient, floor((t mod q_i) 2^64 / q_i) < 2^64.  The reference keeps t itself, whose quotient floor(t 2^64 / q_i) needs 83 bits
    there.  For a limb above t (the 60-bit one, and the 61-bit Bsk primes) the words are t and its quotient, as before."""
    log_n, chain, size_p = primes_of("hyb12_a2")
    P0, size_q, two_n = [int(p) for p in chain], len(chain) - size_p, 2 << log_n
    t59 = primes_down(2 ** 59 - two_n + 1, two_n, 3)[2]
    assert t59.bit_length() == 59 and sum(1 for q in P0[:size_q] if q < t59) == 5 and P0[0] > t59
    big_q = prod(P0[:size_q])
    size_b = size_q + (1 if 32 + t59.bit_length() + big_q.bit_length() >= 61 * size_q + 61 else 0)
    pq = a64(P0[:size_q])
    assert emu.emu_behz_size_b(ptr(pq), C.c_uint32(size_q), C.c_uint64(t59)) == size_b
    found = primes_down(2 ** 61 - two_n + 1, two_n, size_b + 1)
    aux0 = len(P0)
    P = P0 + found[1:] + [found[0], 2 ** 32]
    nbsk = size_b + 1
    pb, wb, wq, tqb, sc = np.zeros(4 * nbsk, U64), np.zeros(nbsk, U64), np.zeros(size_q, U64), np.zeros(2 * (size_q + nbsk), U64), np.zeros(4, U64)
    pa = a64(P)
    emu.emu_behz(ptr(pa), sz(len(P)), C.c_uint32(size_q), C.c_uint32(aux0), C.c_uint32(size_b), C.c_uint64(t59), ptr(pb), ptr(wb), ptr(wq), ptr(tqb), ptr(sc))
    limbs = P0[:size_q] + [P[aux0 + j] for j in range(nbsk)]
    want = [t59 % p for p in limbs]
    assert [int(x) for x in tqb] == want + [shoup(v, p) for v, p in zip(want, limbs)]
    assert all(shoup(t59, p) >= 2 ** 64 for p in P0[1:size_q]) and all(shoup(v, p) < 2 ** 64 for v, p in zip(want, limbs))
    # what the pair is for: x * (t mod q) by Shoup's method equals x t mod q for the extreme and some random x
    r = np.random.default_rng(59)
    for v, p in zip(want, limbs):
        for x in [0, 1, p - 1] + [int(y) for y in r.integers(0, p, 5)]:
            hi = (x * shoup(v, p)) >> 64
            got = (x * v - hi * p) % 2 ** 64
            assert (got - p if got >= p else got) == x * t59 % p
