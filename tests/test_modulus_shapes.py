"""The CPU oracle on the sets of tests/modulus_shapes.py (primes at the bottom of a bit width, limbs of 16 .. 30 bits, plain moduli up to
59 bits), pinned by DEFINITIONS, not by itself -- tests/test_gpu_modulus_shapes.py then holds the kernels against the oracle.

1. the committed primes against their recipes, Miller-Rabin against O.is_prime;
2. forward and inverse NTT against X[k] = sum_j x[j] psi^((2 brev(k) + 1) j): every output of every limb below 2^31 in numpy uint64
   (every product fits: exact, and no code of oracle.c), 16 outputs of the wider limbs in Python integers;
3. mod-up, mod-down, rescale and the BGV modulus switch at 16 coefficients against the CRT in Python integers;
4. the BFV matrix: every (set, plain modulus, multiply) cell encrypts two messages, multiplies on the oracle, decrypts by phase + CRT +
   round(t x / Q) in Python integers and compares with the exact negacyclic product modulo t.  In-domain cells are asserted by name
   with margin >= bv_semantics.MIN_MARGIN; every other cell is listed in modulus_shapes.BFV_CELLS with its reason and must behave as
   listed (a refusal refuses, a cell without room in base R is the one the room rule names).  Margins are printed (pytest -s).
5. the plain-HPS carry: the three cells the fix settles."""
import functools
import math
import operator

import numpy as np
import pytest

import modulus_shapes as M
from bv_semantics import MIN_MARGIN
from oracle import oracle as O
from util import brev

NTT_SETS = ["edge12", "edge14", "small12", "tiny12", "pair12"]
POSITIONS = 16


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_committed_primes_are_their_recipes():
    for name in M.RECIPES:
        assert M.derive(name) == M.SETS[name], name
        log_n, qp, size_p = M.SETS[name]
        assert len(set(qp)) == len(qp) and all(O.is_prime(p) and (p - 1) % (2 << log_n) == 0 for p in qp), name
    assert M.T40 == M.primes_below(1 << 40, 8192, 1)[0]
    assert M.T59 == M.primes_below(1 << 59, 8192, 3)[2] == int(O.get_primes(4096, 59, 3)[2])
    for name, t in M.PLAIN_BELOW.items():
        smallest = min(M.data_primes(name))
        assert t == M.primes_below(1 << (smallest.bit_length() - 1), 8192, 1)[0] and t < smallest, name


def test_miller_rabin_agrees_with_the_oracle():
    """On every committed prime, its neighbours in the progression 1 + k 2N, and the top of five widths against get_primes."""
    for name, (log_n, qp, _) in M.SETS.items():
        for p in qp:
            for c in range(p - 8 * (2 << log_n), p + 9 * (2 << log_n), 2 << log_n):
                assert M.is_prime(c) == O.is_prime(c), c
    for bits in (20, 30, 42, 50, 61):
        assert M.primes_below(1 << bits, 8192, 3) == [int(p) for p in O.get_primes(4096, bits, 3)], bits
    assert [M.is_prime(c) for c in (0, 1, 2, 3, 4, 37, 561, 3215031751, 2 ** 61 - 1, 2 ** 61 + 1)] == \
        [False, False, True, True, False, True, False, False, True, False]     # Carmichael, a strong pseudoprime to 2, 3, 5, 7


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def minimal_root(q, two_n):
    """The smallest primitive two_n-th root of unity modulo q (the reference's choice of psi), in Python integers."""
    a = 2
    while pow(a, (q - 1) // two_n * (two_n // 2), q) != q - 1:
        a += 1
    g = pow(a, (q - 1) // two_n, q)
    best, w, g2 = g, g, g * g % q
    for _ in range(two_n // 2 - 1):
        w = w * g2 % q
        best = min(best, w)
    return best


def ntt_inputs(name, limb_rows):
    log_n, qp, _ = M.primes_of(name)
    return M.edge_inputs(np.random.default_rng(M.seed_of(name, "ntt")), [qp[i] for i in limb_rows], 1 << log_n)


@functools.lru_cache(maxsize=2)
def _exponents(log_n):
    """[N][N] int32: (2 brev(k) + 1) j mod 2N."""
    n = 1 << log_n
    odd = np.array([2 * brev(k, log_n) + 1 for k in range(n)], dtype=np.int64)
    return ((odd[:, None] * np.arange(n, dtype=np.int64)[None, :]) % (2 * n)).astype(np.int32)


def definition_small(x, q, psi, log_n):
    """For q < 2^31 and x [M][N]: (forward, inverse) [M][N] in uint64, every output.  Forward X[k] = sum_j x[j] psi^((2 brev(k) + 1) j);
    inverse x[j] = N^-1 sum_k X[k] psi^(-(2 brev(k) + 1) j).  The inputs are cut at 16 bits, so a sum of N products (power below
    2^31 times half below 2^16) stays below 2^59: no reduction inside a sum."""
    n, uq = 1 << log_n, np.uint64(q)
    halves = np.concatenate([x & np.uint64(0xFFFF), x >> np.uint64(16)])            # [2M][N]
    out = []
    for base in (psi, pow(psi, -1, q)):
        pw = np.ones(2 * n, dtype=np.uint64)
        for e in range(1, 2 * n):
            pw[e] = int(pw[e - 1]) * base % q
        s = np.zeros_like(halves)
        for k0 in range(0, n, 512):
            w = pw[_exponents(log_n)[k0:k0 + 512]]                                   # [512][N], row k column j
            for h in range(len(halves)):
                if base == psi:
                    s[h, k0:k0 + 512] = (w * halves[h][None, :]).sum(axis=1)         # forward: over j
                else:
                    s[h] += (w * halves[h][k0:k0 + 512, None]).sum(axis=0)           # inverse: over k
        s %= uq
        lo, hi = s[:len(x)], s[len(x):]
        out.append((lo + hi * np.uint64(1 << 16) % uq) % uq)
    return out[0], out[1] * np.uint64(pow(n, -1, q)) % uq


def definition_at(xs, q, psi, log_n, at):
    """(forward, inverse) outputs of the inputs xs [M][N] at the positions `at`, in Python integers: forward position k is
    sum_j x[j] psi^((2 brev(k) + 1) j), inverse position j is N^-1 sum_k x[k] psi^(-(2 brev(k) + 1) j).  Both read one table of the
    2N powers of psi; exponent rows come from _exponents."""
    n = 1 << log_n
    pw = [1] * (2 * n)
    for e in range(1, 2 * n):
        pw[e] = pw[e - 1] * psi % q
    ex, n_inv = _exponents(log_n), pow(n, -1, q)
    rows = [[int(v) for v in x] for x in xs]
    fwd_w = [[pw[e] for e in ex[k].tolist()] for k in at]                          # row k: every j
    inv_w = [[pw[(2 * n - e) % (2 * n)] for e in ex[:, j].tolist()] for j in at]      # column j: every k, negative exponent
    dot = lambda a, b: sum(map(operator.mul, a, b))
    return ([[dot(x, w) % q for w in fwd_w] for x in rows], [[dot(x, w) % q * n_inv % q for w in inv_w] for x in rows])


@pytest.mark.parametrize("name", NTT_SETS)
def test_ntt_is_its_definition(name):
    log_n, qp, size_p = M.primes_of(name)
    n = 1 << log_n
    oc = M.oracle_ctx(name)
    rows = list(range(len(qp)))
    x = ntt_inputs(name, rows)
    rng = np.random.default_rng(M.seed_of(name, "at"))
    at = [0, 1, n - 1, n // 2] + [int(v) for v in rng.choice(np.arange(2, n // 2), POSITIONS - 4, replace=False)]
    psis = [minimal_root(q, 2 * n) for q in qp]
    assert psis == [O.minimal_primitive_root(2 * n, q) for q in qp]
    small = {i: definition_small(x[:, i], q, psis[i], log_n) for i, q in enumerate(qp) if q < 1 << 31}
    wide = {i: definition_at(x[:, i], q, psis[i], log_n, at) for i, q in enumerate(qp) if i not in small}
    assert len(at) == POSITIONS
    for kind in range(3):
        fwd, inv = oc.nwt_forward_map(x[kind], rows), oc.nwt_backward_map(x[kind], rows)
        for i, q in enumerate(qp):
            if i in small:
                assert np.array_equal(fwd[i], small[i][0][kind]), (name, q, kind, "forward")
                assert np.array_equal(inv[i], small[i][1][kind]), (name, q, kind, "inverse")
            else:
                assert [int(fwd[i, k]) for k in at] == wide[i][0][kind], (name, q, kind, "forward")
                assert [int(inv[i, k]) for k in at] == wide[i][1][kind], (name, q, kind, "inverse")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
CONV_LEVELS = [("edge12", 8), ("edge12", 7), ("edge12", 3), ("edge12", 1), ("edge14", 8), ("edge14", 2), ("small12", 6), ("small12", 3),
               ("tiny12", 4), ("tiny12", 3)]


def _coeffs(name, ql, tag):
    """[2][ql + |P|][N] coefficient-form residues over Ql u P: every word q - 1 first, then uniform; the positions to check."""
    log_n, qp, size_p = M.primes_of(name)
    size_q = len(qp) - size_p
    rows = list(range(ql)) + list(range(size_q, len(qp)))
    x = M.edge_inputs(np.random.default_rng(M.seed_of(name, tag, ql)), [qp[i] for i in rows], 1 << log_n)
    at = [0, 1, (1 << log_n) - 1] + [int(v) for v in np.random.default_rng(M.seed_of(name, "pos", ql)).integers(0, 1 << log_n, POSITIONS - 3)]
    return x[[1, 0]], rows, at


def _centre(v, mod):
    return v - mod if v > mod // 2 else v


@pytest.mark.parametrize("name,ql", CONV_LEVELS)
def test_modup_is_the_fast_conversion_of_each_digit(name, ql):
    """Digit d (alpha limbs, the last one shorter) holds X_d in [0, Q_d); every other limb p of Ql u P gets X_d + u Q_d for ONE u in
    [0, digit size) (the fast conversion's overflow), the digit's own limbs their words."""
    log_n, qp, size_p = M.primes_of(name)
    oc, tool = M.oracle_ctx(name), O.Tool(M.oracle_ctx(name), ql)
    xs, rows, at = _coeffs(name, ql, "modup")
    for x in xs:
        c = np.ascontiguousarray(x[:ql])
        up = tool.modup(oc.nwt_forward(c, ql, 0), O.CKKS)
        assert up.shape[0] == tool.beta == -(-ql // size_p)
        for d in range(tool.beta):
            own = list(range(d * size_p, min((d + 1) * size_p, ql)))
            coeff = oc.nwt_backward_map(up[d], rows)
            vals, big = M.compose(c[own], [qp[i] for i in own], at)
            for v, k in zip(vals, at):
                us = set()
                for r, row in enumerate(rows):
                    if row in own:
                        assert int(coeff[r, k]) == int(c[row, k])
                    else:
                        us.add((int(coeff[r, k]) - v) * pow(big, -1, qp[row]) % qp[row])
                assert len(us) <= 1 and all(u < len(own) for u in us), (name, ql, d, k, us)


@pytest.mark.parametrize("name,ql", CONV_LEVELS)
def test_moddown_is_the_division_by_p(name, ql):
    """moddown_from_NTT (ckks): floor(X / P) - u for one u in [0, alpha), X the value over Ql u P."""
    log_n, qp, size_p = M.primes_of(name)
    oc, tool = M.oracle_ctx(name), O.Tool(M.oracle_ctx(name), ql)
    xs, rows, at = _coeffs(name, ql, "moddown")
    big_p = math.prod(qp[len(qp) - size_p:])
    for x in xs:
        down = oc.nwt_backward(tool.moddown_from_ntt(oc.nwt_forward_map(x, rows), O.CKKS), ql, 0)
        vals, _ = M.compose(x, [qp[i] for i in rows], at)
        got, big_q = M.compose(down, qp[:ql], at)
        for v, g, k in zip(vals, got, at):
            assert 0 <= (v // big_p - g) % big_q < size_p, (name, ql, k)


@pytest.mark.parametrize("name,ql", [c for c in CONV_LEVELS if c[1] > 1])
def test_rescale_and_mod_switch_divide_by_the_last_prime(name, ql):
    """rescale_ntt: floor(X / q_last) exactly (the reference's rescale floors).  mod_t_divide_q_last_ntt: (X + delta) / q_last with delta = -X (mod q_last), delta = 0 (mod t), |delta| < t q_last -- for every plain modulus below the smallest live limb, and T59 (below the 60-bit
    limb only) where the set has one."""
    log_n, qp, size_p = M.primes_of(name)
    oc = M.oracle_ctx(name)
    xs, rows, at = _coeffs(name, ql, "rescale")
    q_last = qp[ql - 1]
    ts = [t for t in (2, 257, 40961, M.T40, M.PLAIN_BELOW.get(name, 65537)) if t < min(qp[:ql])] + ([M.T59] if name.startswith("edge") else [])
    ts = [t for t in ts if 4 * t * q_last < math.prod(qp[:ql])]      # delta itself must fit the level: a switch needs t q_last << Q_l
    assert len(ts) >= (1 if ql == 2 else 3)
    for x in xs:
        c = np.ascontiguousarray(x[:ql])
        ntt = oc.nwt_forward(c, ql, 0)
        vals, big = M.compose(c, qp[:ql], at)
        got, low = M.compose(oc.nwt_backward(O.Tool(oc, ql).rescale_ntt(ntt[None], 1)[0], ql - 1, 0), qp[:ql - 1], at)
        assert got == [v // q_last % low for v in vals], (name, ql)
        for t in ts:
            tool = O.Tool(oc, ql).set_plain_modulus(t)
            got, low = M.compose(oc.nwt_backward(tool.mod_t_divide_q_last_ntt(ntt[None], 1)[0], ql - 1, 0), qp[:ql - 1], at)
            for v, g in zip(vals, got):
                delta = _centre((g * q_last - v) % big, big)
                assert delta % t == 0 and abs(delta) < t * q_last and (v + delta) % q_last == 0, (name, ql, t)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def _multiply(name, label, variant):
    """(message matches, margin) of one cell on the oracle alone; raises ValueError where the oracle refuses."""
    k = M.keyed(name)
    t, m, cts, want = M.bfv_operands(name, label)
    got, margin = k.decrypt(O.BFV, t, M.multiplier(variant, k.oc, t).multiply(cts[0], cts[1]), k.size_q)
    return bool(np.array_equal(got, want)), margin


@pytest.mark.parametrize("name,label", list(M.BFV_CELLS), ids=[f"{n}-{l}" for n, l in M.BFV_CELLS])
def test_bfv_matrix(name, label):
    k = M.keyed(name)
    t, m, cts, want = M.bfv_operands(name, label)
    for i in range(2):                                   # the fresh operands decrypt to their messages
        plain, margin = k.decrypt(O.BFV, t, cts[i], k.size_q)
        assert np.array_equal(plain, m[i]) and margin >= MIN_MARGIN
    assert int(want[0]) != int(m[0][0]) or t == 2       # the product is not an operand
    for variant in M.VARIANTS:
        status, reason = M.cell_status(name, label, variant)
        if status == M.REFUSED:
            with pytest.raises(ValueError, match="cannot set up the HPS bases"):
                M.multiplier(variant, k.oc, t)
            print(f"{name} t={label} {variant}: refused ({reason})")
            continue
        exact, margin = _multiply(name, label, variant)
        print(f"{name} t={label} {variant}: {'exact' if exact else 'WRONG'}, margin {margin:.1f} bits [{status}]")
        if variant == "hps":                             # the listed status of a plain-HPS cell is the room rule's, not a choice
            assert (status == M.IN) == M.hps_has_room(k.primes[:k.size_q], O.Hps(k.oc, t).r, t, k.n), (name, label)
        if status == M.IN:
            assert exact, f"{name} t={label} {variant}: the product decrypts to something else (margin {margin:.1f})"
            assert margin >= MIN_MARGIN, f"{name} t={label} {variant}: margin {margin:.1f} bits"
        else:
            assert variant == "hps" and not exact, f"{name} t={label} {variant} is listed as {status} ({reason}) but decrypts"


def test_every_behz_and_overq_cell_is_in_domain():
    for (name, label), cell in M.BFV_CELLS.items():
        for variant in ("behz", "overq"):
            assert M.cell_status(name, label, variant)[0] == (M.REFUSED if name == "tiny12" and variant == "overq" else M.IN)
    assert ("hyb12_a2", "T59", "behz") in M.in_domain_cells() and ("low50", "T59", "behz") in M.in_domain_cells()


@pytest.mark.parametrize("name,label", [c for c in M.BFV_CELLS if c[0] in ("low50", "low60")], ids=lambda v: str(v))
def test_bfv_leveled_one_level_down(name, label):
    """hps_overq_leveled with one level dropped: in-domain but for the cell modulus_shapes.LEVELED_OUT names."""
    k = M.keyed(name)
    t, m, cts, want = M.bfv_operands(name, label)
    got, margin = k.decrypt(O.BFV, t, O.HpsOverQ(k.oc, t, k.size_q - 1).multiply(cts[0], cts[1]), k.size_q)
    exact = bool(np.array_equal(got, want))
    print(f"{name} t={label} overq one level down: {'exact' if exact else 'WRONG'}, margin {margin:.1f} bits")
    if (name, label) in M.LEVELED_OUT:
        assert not exact, f"{name} t={label} is listed as out-of-domain one level down but decrypts"
    else:
        assert exact and margin >= MIN_MARGIN, f"{name} t={label}: margin {margin:.1f} bits"


def test_bottom50_has_no_hps_base_but_multiplies_by_behz():
    oc = M.oracle_ctx("bottom50")
    for cls in (O.Hps, O.HpsOverQ):
        with pytest.raises(ValueError, match="cannot set up the HPS bases"):
            cls(oc, 65537)
    k = M.keyed("bottom50")
    mm = k.messages(65537, 2)
    cts = [k.encrypt(O.BFV, 65537, mm[i], k.size_q, i) for i in range(2)]
    got, margin = k.decrypt(O.BFV, 65537, O.Behz(oc, 65537).multiply(cts[0], cts[1]), k.size_q)
    assert np.array_equal(got, M.negacyclic_product(mm[0], mm[1], 65537)) and margin >= MIN_MARGIN


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain(label, log_n, qp, size_p):
    """A keyed chain of explicit primes that is no named set (qp a tuple)."""
    return M.Keyed(label, (log_n, qp, size_p))


def _temporary_set(label, log_n, qp, size_p):
    return _chain(label, log_n, tuple(int(p) for p in qp), size_p)


@pytest.mark.parametrize("label,bits,low,count", [("top30x4", 30, False, 4), ("low30x6", 30, True, 6), ("low36x4", 36, True, 4)])
def test_plain_hps_carry_reaches_every_limb_consistently(label, bits, low, count):
    """scaleAndRound_HPS_QR_R on a value of the size a tensor product has, against round(t v / Q) in Python integers: the result over
    R differs from it by the carry's first reduction only, a multiple of r_0 below |Q| r_0 + 1 -- in EVERY coefficient.  With the
    reference's in-place reduction (rns.cu:1733) about N (r_0 - r_|Q|) / r_0 coefficients per polynomial were noise of R's size: one
    to three here at 30 bits, which is what made the t = 2 cells of these shapes wrong."""
    n, t = 4096, 2
    sp = M.primes_above(1 << 59, 2 * n, 2)
    q = M.primes_above(1 << (bits - 1), 2 * n, count, 8) if low else M.primes_below(1 << bits, 2 * n, count)
    k = _temporary_set(label, 12, q + sp, 2)
    hps = O.Hps(k.oc, t)
    r, big_q, big_r = hps.r, math.prod(q), math.prod(hps.r)
    assert r == sorted(r, reverse=True) and M.hps_has_room(q, r, t, n)
    rng = np.random.default_rng(M.seed_of(label, "carry"))
    e = 2 * big_q.bit_length() + 4                       # |d| < 2^(e - 1): about N Q^2 / 2, well inside Q R
    assert (1 << e) < big_q * big_r
    d = [int.from_bytes(rng.bytes((e + 7) // 8), "little") % (1 << e) - (1 << (e - 1)) for _ in range(n)]
    x = np.array([[v % s for v in d] for s in q + r], dtype=np.uint64)
    got, _ = M.compose(hps.scale_round_qr_r(x), r)
    worst = 0
    for g, v in zip(got, d):
        err = _centre((g - (2 * t * v + big_q) // (2 * big_q)) % big_r, big_r)
        assert abs(err) <= count * r[0] + 1 and min(err % r[0], -err % r[0]) <= 1, (label, err)
        worst = max(worst, abs(err))
    print(f"{label}: largest error of the scaled value {worst} = {worst / r[0]:.2f} r_0")


@pytest.mark.parametrize("label,bits,low,count", [("top30x4", 30, False, 4), ("low36x4", 36, True, 4)])
def test_plain_hps_decrypts_at_the_settled_cells(label, bits, low, count):
    n, t = 4096, 2
    sp = M.primes_above(1 << 59, 2 * n, 2)
    q = M.primes_above(1 << (bits - 1), 2 * n, count, 8) if low else M.primes_below(1 << bits, 2 * n, count)
    k = _temporary_set(label, 12, q + sp, 2)
    mm = k.messages(t, 2)
    cts = [k.encrypt(O.BFV, t, mm[i], k.size_q, i) for i in range(2)]
    got, margin = k.decrypt(O.BFV, t, O.Hps(k.oc, t).multiply(cts[0], cts[1]), k.size_q)
    print(f"{label} t=2 hps: margin {margin:.1f} bits")
    assert np.array_equal(got, M.negacyclic_product(mm[0], mm[1], t)) and margin >= MIN_MARGIN


# ---- the kernels' thread program on these limbs, replayed on the CPU (tests/emu/emu_ntt.cpp, as tests/test_emu_ntt.py does) -----------
@pytest.fixture(scope="module")
def emu_ntt(tmp_path_factory):
    import ctypes as C
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path_factory.mktemp("emu_shapes") / "libemu_ntt.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(here, "emu", "emu_ntt.cpp")])
    lib = C.CDLL(out)
    u64p = C.POINTER(C.c_uint64)
    lib.emu_ntt.argtypes = [C.c_int, C.c_int, C.c_int, u64p, u64p, C.c_uint64] + [u64p] * 5
    return lib, (lambda a: a.ctypes.data_as(u64p))


@pytest.mark.parametrize("name", NTT_SETS)
def test_ntt_thread_program_on_the_edge_limbs(emu_ntt, name):
    """pha_ntt_core.h's thread program with make_fpmod's constants for q, forward and inverse, both back ends (FP64 below 2^50, where
    the light butterflies switch on q >> 47 and q >> 42), on the three inputs, against the oracle that section 2 pins.  This pins the words on the far
    side of each switch and that a switch exists: with both thresholds taken away (q >> 55) edge12 and edge14 fail; moved by one to
    four bits they do not -- a pass has 6 or 7 stages at N = 2^12 / 2^14 and the thresholds are sized for 9."""
    lib, p = emu_ntt
    log_n, qp, size_p = M.primes_of(name)
    n = 1 << log_n
    x = ntt_inputs(name, list(range(len(qp))))
    z = np.zeros(2, dtype=np.uint64)
    f = lambda w: np.ascontiguousarray(w.astype(np.float64)).view(np.uint64).copy()
    f1 = lambda v: np.array([float(v), 0.0], dtype=np.float64).view(np.uint64).copy()
    pair = lambda v, q: np.array([v, O.compute_shoup(v, q)], dtype=np.uint64)
    for i, q in enumerate(qp):
        tw, tws, itw, itws, ni, nis = O.ntt_tables(log_n, q)
        c = O.Ctx(log_n, [q], 0)
        itw_p, itws_p = itw.copy(), itws.copy()
        itw_p[1] = int(itw[1]) * n % q
        itws_p[1] = O.compute_shoup(int(itw_p[1]), q)
        twi = np.ascontiguousarray(np.stack([tw, tws], axis=1).reshape(-1))
        itwi = np.ascontiguousarray(np.stack([itw_p, itws_p], axis=1).reshape(-1))
        for variant in (0, 6):                           # the two-pass plan and the one-launch plan of N = 2^12 / 2^14
            code = log_n | (variant << 8)
            for kind in range(3):
                y = np.ascontiguousarray(x[kind, i])
                fwd, inv = c.nwt_forward(y.reshape(1, n), 1)[0], c.nwt_backward(y.reshape(1, n), 1)[0]
                got = np.zeros(n, dtype=np.uint64)
                what = (name, q, q.bit_length(), variant, kind)
                assert lib.emu_ntt(code, 1, 1, p(y), p(got), q, p(twi), p(z), p(z), p(z), p(z)) == 0
                assert np.array_equal(got, fwd), what + ("forward",)
                assert lib.emu_ntt(code, 0, 3, p(y), p(got), q, p(itwi), p(pair(ni, q)), p(pair(int(itw[1]), q)), p(z), p(z)) == 0
                assert np.array_equal(got, inv), what + ("inverse",)
                if q >> 50 == 0:
                    fcode = code | (1 << 16)
                    assert lib.emu_ntt(fcode, 1, 1, p(y), p(got), q, p(f(tw)), p(z), p(z), p(z), p(z)) == 0
                    assert np.array_equal(got, fwd), what + ("forward fp64",)
                    assert lib.emu_ntt(fcode, 0, 3, p(y), p(got), q, p(f(itw_p)), p(f1(ni)), p(f1(int(itw[1]))), p(z), p(z)) == 0
                    assert np.array_equal(got, inv), what + ("inverse fp64",)


def test_plain_hps_carry_on_a_36_bit_chain_at_2_14():
    """Four 36-bit data primes at N = 2^14, t = 786433 (a chain tests/test_gpu_fuzz_batched.py draws): the scaled value is within
    |Q| r_0 of round(t v / Q) in every one of 8 x 16384 coefficients.  With the reference's chained reduction about one coefficient
    in 50000 on this chain (N (r_0 - r_4) / r_0 = 0.3 per polynomial) was off by 2^172 .. 2^177, R having 180 bits; those are the
    only words the fix changes."""
    log_n, t = 14, 786433
    qp = [68718428161, 68717740033, 68716036097, 68714954753, 1152921504606748673, 1152921504606683137]
    n, q = 1 << log_n, qp[:4]
    assert all(M.is_prime(p) and p % (2 * n) == 1 for p in qp)
    k = _temporary_set("fuzz36x4_14", log_n, qp, 2)
    hps = O.Hps(k.oc, t)
    r, big_q, big_r = hps.r, math.prod(q), math.prod(hps.r)
    rng = np.random.default_rng(M.seed_of("fuzz36x4_14", "carry"))
    e = 2 * big_q.bit_length() + 4
    assert (1 << e) < big_q * big_r
    for rep in range(8):
        d = [int.from_bytes(rng.bytes((e + 7) // 8), "little") % (1 << e) - (1 << (e - 1)) for _ in range(n)]
        got = hps.scale_round_qr_r(np.array([[v % s for v in d] for s in q + r], dtype=np.uint64))
        vals, _ = M.compose(got, r)
        for i, (g, v) in enumerate(zip(vals, d)):
            err = _centre((g - (2 * t * v + big_q) // (2 * big_q)) % big_r, big_r)
            assert abs(err) <= 4 * r[0] + 1 and min(err % r[0], -err % r[0]) <= 1, (rep, i, err)


def _overq_noisy(q, sp, t, reps, label):
    """Coefficients of scaleAndRound_HPS_QlRl_Ql whose result over Q is further than (|R| + 1) max q from round(t v / R)."""
    n = 4096
    hq = O.HpsOverQ(O.Ctx(12, list(q) + list(sp), len(sp)), t)
    r, big_q, big_r = hq.r, math.prod(q), math.prod(hq.r)
    e = (big_q * big_r).bit_length() - 3
    rng = np.random.default_rng(M.seed_of(label, "overq carry"))
    noisy = 0
    for _ in range(reps):
        d = [int.from_bytes(rng.bytes((e + 7) // 8), "little") % (1 << e) - (1 << (e - 1)) for _ in range(n)]
        got, _ = M.compose(hq.scale_round_qlrl_ql(np.array([[v % s for v in d] for s in list(q) + r], dtype=np.uint64)), q)
        noisy += sum(1 for g, v in zip(got, d) if abs(_centre((g - (2 * t * v + big_r) // (2 * big_r)) % big_q, big_q)) > (len(r) + 1) * max(q))
    return noisy


def test_overq_carry_is_consistent_on_ascending_chains_only():
    """scaleAndRound_HPS_QlRl_Ql chains its carry across the Q limbs as the reference does (rns.cu:1783; restated, not changed here).
    On a chain whose data primes ASCEND no later reduction subtracts anything and all 8 x 4096 coefficients are within a few q of
    round(t v / R).  The same primes in DESCENDING order lose about N (q_0 - q_last) / q_0 coefficients per polynomial to noise (1.5
    expected in these 8 polynomials at 30 bits): the open defect DESIGN.md 4.8a1 records for hps_overq.  When it is fixed the second
    assertion turns into `== 0`."""
    n = 4096
    sp = M.primes_above(1 << 59, 2 * n, 2)
    down = M.primes_below(1 << 30, 2 * n, 4)
    assert _overq_noisy(down[::-1], sp, 2, 8, "ascending") == 0
    assert 1 <= _overq_noisy(down, sp, 2, 8, "descending") <= 8
