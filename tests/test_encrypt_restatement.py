"""tests/encrypt_restatement.py pinned by decryption: the restated sequences of src/secretkey.cu produce ciphertexts whose phase under
the secret key is the plaintext plus exactly the noise the construction implies.  CPU only (oracle steps and Python integers).

Symmetric, NTT form: c0 + c1 (.) s = plain - NTT(k e), so the inverse transform of (phase - plain) is the residues of -k e, exactly.
Symmetric, bfv: the phase decrypts to m in all N coefficients.
Asymmetric: with pk = (-(a s + k e_pk), a) over QP, the ciphertext over Q_l u P has phase k nu with
    nu = -u e_pk + e_0 + e_1 s                        (products in Z[X] / (X^N + 1))
and the mod-down of polynomial j subtracts r_j = (c_j mod P) + eps_j P -- the fast base conversion of the P residues, a sum of |P| = alpha
terms each in [0, P), so 0 <= eps_j <= alpha - 1 -- and divides by P.  Under ckks therefore, with X = phase - plain (centred, composed
by CRT) and rho_j = c_j mod P in [0, P):
    P X = k nu - (rho_0 + rho_1 s) - P (eps_0 + eps_1 s)
Every coefficient of rho_1 s is a signed sum of N values in [0, P) (s is ternary), so |rho_0 + rho_1 s| < (N + 1) P and
|eps_0 + eps_1 s| <= (alpha - 1) (N + 1):
    |P X - k nu| < alpha (N + 1) P                    per coefficient -- the bound asserted, in exact integers.
bgv's mod-down subtracts a multiple of t as well and bfv's divides in coefficient form; both decrypt to m exactly."""
import numpy as np
import pytest

import ckks_semantics as S
from encrypt_restatement import Restatement, residues
from oracle import oracle as O
from util import crt_compose

T = 65537
HYB, C1 = "hyb12_a2", "c1_bfv4096"
LEVELS = {HYB: (6, 3, 1), C1: (2, 1)}
NOISE = 21          # the reference's samplers: |e| <= 21


def scheme_of(name):
    return S.scheme(name)


def draws(sch, tag, l, special=False):
    """(a over the rows, e, a second e pair, u) for one encryption; extremes of the reference's range in the first words."""
    rng = sch._rng("encrypt", tag, l, int(special))
    rows = sch.rows(l, special)
    a = sch._uniform(rng, [sch.primes[r] for r in rows])
    e = rng.integers(-NOISE, NOISE + 1, (3, sch.n))
    e[:, 0], e[:, 1] = NOISE, -NOISE
    u = rng.integers(-1, 2, sch.n)
    return a, e[0], e[1:], u


def negacyclic(a, b):
    """a b in Z[X] / (X^N + 1) for small integer vectors (exact in int64: |sums| < N * 2^40)."""
    n = len(a)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    out = np.zeros(n, dtype=np.int64)
    for i in np.nonzero(a)[0]:
        out[i:] += a[i] * b[:n - i]
        out[:i] -= a[i] * b[n - i:]
    return out


def centred(res, primes):
    """[L][N] residues -> N Python integers in (-Q / 2, Q / 2]."""
    out = []
    for k in range(res.shape[1]):
        v, big = crt_compose([res[i, k] for i in range(len(primes))], primes)
        out.append(v - big if 2 * v > big else v)
    return out


def small_plain_ntt(sch, l, tag):
    """An NTT-form plaintext [l][N] of a small integer polynomial (what a ckks encoding is)."""
    m = sch._rng("plain", tag).integers(-(1 << 30), 1 << 30, sch.n)
    return sch.oc.nwt_forward(residues(m, sch.primes[:l]), l, 0)


def raw_plain(sch, tag):
    return sch._rng("raw", tag).integers(0, T, sch.n).astype(np.uint64)


def phase_coeff(sch, ct, l, ntt_form):
    """c0 + c1 s of a size-2 ciphertext, in coefficient form."""
    oc = sch.oc
    if ntt_form:
        return oc.nwt_backward(sch.decrypt(ct, l), l, 0)
    c1s = oc.nwt_backward(oc.multiply(oc.nwt_forward(ct[1], l, 0), sch.sk_ntt[:l], l), l, 0)
    return oc.add(ct[0], c1s, l)


def bfv_decrypt(sch, ct, l):
    primes = [int(q) for q in sch.primes[:l]]
    big = 1
    for q in primes:
        big *= q
    out = []
    for v in centred(phase_coeff(sch, ct, l, False), primes):
        out.append(((v % big) * T + big // 2) // big % T)
    return np.array(out, dtype=np.uint64)


def bgv_decrypt(sch, ct, l):
    primes = [int(q) for q in sch.primes[:l]]
    return np.array([v % T for v in centred(phase_coeff(sch, ct, l, True), primes)], dtype=np.uint64)


@pytest.mark.parametrize("scheme", [O.CKKS, O.BGV], ids=["ckks", "bgv"])
@pytest.mark.parametrize("l", LEVELS[HYB])
def test_symmetric_phase_is_plain_minus_the_noise(scheme, l):
    sch = scheme_of(HYB)
    r = Restatement(sch.oc, scheme, 0 if scheme == O.CKKS else T)
    a, e, _, _ = draws(sch, "sym", l)
    if scheme == O.CKKS:
        plain = small_plain_ntt(sch, l, l)
        plain_ntt = plain
    else:
        plain = raw_plain(sch, l)
        plain_ntt = sch.oc.bgv_lift_plain(plain, l)
    ct = r.symmetric(sch.sk_ntt, a, e, plain, l)
    assert np.array_equal(ct[1], a), "c1 is the uniform a, untouched"
    diff = sch.oc.nwt_backward(sch.oc.sub(sch.decrypt(ct, l), plain_ntt, l), l, 0)
    k = T if scheme == O.BGV else 1
    assert np.array_equal(diff, residues(-k * e, sch.primes[:l])), "phase - plain is not -k e"
    if scheme == O.BGV:
        assert np.array_equal(bgv_decrypt(sch, ct, l), plain)


@pytest.mark.parametrize("special", [False, True], ids=["data", "special"])
def test_zero_symmetric_both_forms_and_the_public_key(special):
    """The coefficient form is the inverse transform of the NTT form (k = 1), rows [0, l) u P included; the public key is the zero
    encryption over all QP rows."""
    sch = scheme_of(HYB)
    r = Restatement(sch.oc, O.CKKS)
    l = 3
    a, e, _, _ = draws(sch, "zero", l, special)
    ntt = r.zero_symmetric(sch.sk_ntt, a, e, l, special, True)
    coeff = r.zero_symmetric(sch.sk_ntt, a, e, l, special, False)
    assert np.array_equal(np.stack([r.backward(ntt[j], l, special) for j in range(2)]), coeff)
    if special:
        a, e, _, _ = draws(sch, "pk", sch.size_q, True)
        pk = r.public_key(sch.sk_ntt, a, e)
        assert pk.shape == (2, sch.size_qp, sch.n)
        assert np.array_equal(pk, r.zero_symmetric(sch.sk_ntt, a, e, sch.size_q, True, True))
        # over all QP rows: p0 + p1 s = -NTT(e)
        oc, qp = sch.oc, sch.size_qp
        lhs = oc.nwt_backward(oc.add(pk[0], oc.multiply(pk[1], sch.sk_ntt, qp), qp), qp, 0)
        assert np.array_equal(lhs, residues(-e, sch.primes))


@pytest.mark.parametrize("l", LEVELS[C1])
def test_bfv_symmetric_decrypts_to_m(l):
    sch = scheme_of(C1)
    r = Restatement(sch.oc, O.BFV, T)
    a, e, _, _ = draws(sch, "bfv", l)
    m = raw_plain(sch, l)
    ct = r.symmetric(sch.sk_ntt, a, e, m, l)
    assert np.array_equal(bfv_decrypt(sch, ct, l), m)


@pytest.mark.parametrize("l", LEVELS[HYB])
def test_asymmetric_ckks_noise_is_nu_over_p_up_to_the_mod_down(l):
    sch = scheme_of(HYB)
    r = Restatement(sch.oc, O.CKKS)
    a_pk, e_pk, _, _ = draws(sch, "pk", sch.size_q, True)
    pk = r.public_key(sch.sk_ntt, a_pk, e_pk)
    _, _, e, u = draws(sch, "asym", l)
    plain = small_plain_ntt(sch, l, 10 + l)
    ct = r.asymmetric(pk, u, e, plain, l)
    assert ct.shape == (2, l, sch.n)
    x = centred(sch.oc.nwt_backward(sch.oc.sub(sch.decrypt(ct, l), plain, l), l, 0), [int(q) for q in sch.primes[:l]])
    nu = -negacyclic(u, e_pk) + e[0] + negacyclic(e[1], sch.s_small)
    big_p = 1
    for q in sch.primes[sch.size_q:]:
        big_p *= int(q)
    bound = sch.size_p * (sch.n + 1) * big_p
    worst = max(abs(big_p * xv - int(nv)) for xv, nv in zip(x, nu))
    print(f"level {l}: max |P X - nu| / P = {worst / big_p:.1f}, bound alpha (N + 1) = {sch.size_p * (sch.n + 1)}")
    assert worst < bound


@pytest.mark.parametrize("name,scheme", [(HYB, O.BGV), (C1, O.BFV)], ids=["bgv", "bfv"])
def test_asymmetric_bgv_and_bfv_decrypt_to_m(name, scheme):
    sch = scheme_of(name)
    r = Restatement(sch.oc, scheme, T)
    a_pk, e_pk, _, _ = draws(sch, "pk", sch.size_q, True)
    pk = r.public_key(sch.sk_ntt, a_pk, e_pk)
    for l in LEVELS[name]:
        _, _, e, u = draws(sch, "asym", l)
        m = raw_plain(sch, 20 + l)
        ct = r.asymmetric(pk, u, e, m, l)
        got = bgv_decrypt(sch, ct, l) if scheme == O.BGV else bfv_decrypt(sch, ct, l)
        assert np.array_equal(got, m), f"level {l}"
