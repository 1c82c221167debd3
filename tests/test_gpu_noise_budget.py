"""Noise as a device-side quantity (pha_poly_infty_norm_batched, pha_invariant_noise_budget_batched), at N = 2^12:

A. the norm kernel on constructed polynomials: ladder12 at 1, 2, 3 and 14 limbs and hyb12_a2 at 6 -- uniform values below some 2^k
   (half of the polynomials with both signs) plus one planted extreme (0, 1, Q - 1, (Q - 1) / 2, (Q + 1) / 2, 2^k - 1, 2^k, Q - 2^k
   at the word boundaries and at bitcount(Q) - 2) at coefficient 0, at N - 1, at the last or first coefficient of a workgroup, or
   twice; one polynomial all zero, one all == Q - 1 (norm 1); about 20 polynomials at a padded stride, destinations poisoned;
   scalars 1, 65537 and a 59-bit t; norm and bits word for word against Python integers;
B. uniform residues (full-range v), ladder12 at 14 limbs, 3 polynomials, exact;
C. end to end against BvScheme.phase + compose of tests/bv_semantics.py: hyb12_a2 under bfv (fresh encryptions, their size-3 HPS
   products with n_powers = 2, the relinearized products, one leveled ciphertext, one ciphertext pushed to budget 0), under bgv
   (fresh, and after pha_keyswitch_mod_switch at the lower level) and one ckks encryption of an encoding; batch 1, 5, 9 at a padded
   stride, chunk 1, 3, 0 the same words, the ciphertexts unchanged; |budget - margin| < 1 with the margin BvScheme.decrypt reports
   (budget = floor(log2 Q) - floor(log2 norm) - 1 against log2(Q // 2) - log2(norm)); fresh > product everywhere, and
   product > 0 for BEHZ products on hyb12_a2 and HPS products on c1_bfv4096 -- an HPS product on hyb12_a2 has no room left by the
   CPU pipeline either (margin 0.0012 bits: its auxiliary base sits below the 40-bit limbs, next to a 60-bit one), so there the
   budget is held exactly against the reference, which is 0;
   the one front end behind three tails: on a strided batch of uniform ciphertexts the budget entry's norm and the decrypt entries'
   plaintexts equal the single-step entries applied to the phase built from the earlier entries, bfv and bgv, chunk 0, 1, 2;
D. refusals with poisoned outputs untouched, batch == 0, norm == NULL, strict mode;
E. workloads.noise_budget_batch gives the C entry's budgets."""
import gc
from math import prod

import numpy as np
import pytest

import bv_semantics as S
import ckks_semantics as CS
from oracle import oracle as O
from util import primes_of, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

POISON = -0x2152411021524111
POISON32 = -0x21524111
T = S.T
T59 = int(O.get_primes(1 << 12, 59, 3)[2])
MASK = (1 << 64) - 1


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _ctx(name, gpu, plain_t=0):
    import phantom_fhe_amd as P
    log_n, primes, size_p = primes_of(name)
    ctx = P.PhantomContext(log_n, [int(p) for p in primes], size_p, device=gpu)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    return P, ctx


def _p64(shape, gpu):
    import torch
    return torch.full(shape, POISON, dtype=torch.int64, device=gpu)


def _p32(shape, gpu):
    import torch
    return torch.full(shape, POISON32, dtype=torch.int32, device=gpu)


def _words(v, L):
    return [(v >> (64 * w)) & MASK for w in range(L)]


def _norm_of(values, Q):
    return max(min(int(v), Q - int(v)) for v in values)


def _budget_of(norm, Q):
    return max(0, Q.bit_length() - norm.bit_length() - 1)


def _extremes(Q):
    bits = Q.bit_length()
    vals = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2]
    for k in sorted(set(list(range(64, bits, 64)) + [bits - 2])):
        vals += [(1 << k) - 1, 1 << k, Q - (1 << k)]
    return [v for v in vals if 0 <= v < Q]


def _big_uniform(rng, bound, n):
    """n uniform Python integers below `bound` (a power of two or not), as an object array."""
    limbs = bound.bit_length() // 62 + 2
    acc = np.zeros(n, dtype=object)
    for k in range(limbs):
        acc = acc + (rng.integers(0, 1 << 62, n).astype(object) << (62 * k))
    return acc % bound


def _residues(values, qs):
    return np.stack([(values % q).astype(np.uint64) for q in qs])


def _run_norm(P, ctx, gpu, x, L, n, scalar, pad=16):
    """x [count][L][N] uint64 -> (norm [count][L], bits [count]) from poisoned destinations, at a padded stride."""
    count, stride = x.shape[0], L * n + pad
    src = _p64((count * stride,), gpu)
    for c in range(count):
        src[c * stride:c * stride + L * n] = P.to_device(np.ascontiguousarray(x[c]), gpu).reshape(-1)
    before = src.clone()
    norm, bits = _p64((count, L), gpu), _p32((count,), gpu)
    ctx.poly_infty_norm_batched(L, src, bits, norm, scalar=scalar, count=count, stride=stride)
    assert bool((src == before).all()), "the source was written to"
    return P.to_host(norm), bits.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# A, B: the norm kernel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", [("ladder12", 1), ("ladder12", 2), ("ladder12", 3), ("ladder12", 14), ("hyb12_a2", 6)])
def test_norm_of_constructed_polynomials(name, L, gpu):
    P, ctx = _ctx(name, gpu)
    n = ctx.n
    qs = [int(q) for q in primes_of(name)[1]][:L]
    Q = prod(qs)
    rng = rng_for(9600 + 20 * L + len(name))
    ext = _extremes(Q)
    places = [[0], [n - 1], [127], [128], [5, 3000], [n - 128], [63], [64]]
    polys = []
    for c in range(18):
        k = int(rng.integers(1, Q.bit_length() - 2))
        v = _big_uniform(rng, 1 << k, n)
        if c % 2:                                            # both signs: Q - u in a random half
            v = np.where(rng.integers(0, 2, n).astype(bool), (Q - v) % Q, v)
        for at in places[c % len(places)]:
            v[at] = ext[c % len(ext)]
        polys.append(v)
    polys.append(np.zeros(n, dtype=object))                  # norm 0, bits 0
    polys.append(np.full(n, Q - 1, dtype=object))            # every coefficient == Q - 1: norm 1
    want = [_norm_of(v, Q) for v in polys]
    assert want[-2] == 0 and want[-1] == 1
    for scalar in (1, 65537, T59):
        back = pow(scalar, -1, Q)
        x = np.stack([_residues(v * back % Q, qs) for v in polys])
        norm, bits = _run_norm(P, ctx, gpu, x, L, n, scalar)
        for c, m in enumerate(want):
            assert [int(w) for w in norm[c]] == _words(m, L), f"{name} L {L} scalar {scalar} polynomial {c}: norm {norm[c]}, want {m}"
            assert int(bits[c]) == m.bit_length(), f"{name} L {L} scalar {scalar} polynomial {c}: bits {bits[c]}, want {m.bit_length()}"
    del ctx
    _release()


def test_norm_of_uniform_residues(gpu):
    P, ctx = _ctx("ladder12", gpu)
    L, n = 14, ctx.n
    qs = [int(q) for q in primes_of("ladder12")[1]][:L]
    Q = prod(qs)
    x = np.stack([uniform_poly(rng_for(9650 + c), qs, n) for c in range(3)])
    w = [(Q // q) * pow(Q // q, -1, q) for q in qs]
    for scalar in (1, T59):
        norm, bits = _run_norm(P, ctx, gpu, x, L, n, scalar, pad=0)
        for c in range(3):
            v = sum(x[c, i].astype(object) * wi for i, wi in enumerate(w)) * scalar % Q
            m = _norm_of(v, Q)
            assert [int(t) for t in norm[c]] == _words(m, L), (scalar, c)
            assert int(bits[c]) == m.bit_length(), (scalar, c)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C: end to end
# ------------------------------------------------------------------------------------------------------------------------------
def _reference(sch, ct, level, scalar):
    """(norm, budget, Q) of ciphertext ct from BvScheme.phase + compose: max min(scalar v mod Q, Q - scalar v mod Q)."""
    v, big = S.BvScheme.compose(sch, sch.phase(ct, level), level)
    m = _norm_of(v * scalar % big, big)
    return m, _budget_of(m, big), big


def _budgets(P, ctx, gpu, level, cts, sk, scheme, chunk=0, pad=16):
    """cts: numpy [B][k][level][N] -> (budget [B], norm [B][level]) at a padded ct stride from poisoned destinations."""
    B, k = cts.shape[0], cts.shape[1]
    words = k * level * ctx.n
    stride = words + pad
    buf = _p64((B * stride,), gpu)
    for b in range(B):
        buf[b * stride:b * stride + words] = P.to_device(np.ascontiguousarray(cts[b]), gpu).reshape(-1)
    before = buf.clone()
    budget, norm = _p32((B,), gpu), _p64((B, level), gpu)
    ctx.invariant_noise_budget_batched(level, buf, sk, scheme, budget, norm, cipher_size=k, batch=B, stride=stride, chunk=chunk)
    assert bool((buf == before).all()), "the ciphertexts were written to"
    return budget.cpu().numpy(), P.to_host(norm)


def _check_against(P, ctx, gpu, sch, level, cts, sk, scheme, scalar, what):
    """Every batch size and chunk against the reference; returns (budgets, reference norms, Q)."""
    refs = [_reference(sch, ct, level, scalar) for ct in cts]
    big = refs[0][2]
    first = None
    for B in (1, 5, 9):
        if B > len(cts):
            continue
        for chunk in (1, 3, 0):
            budget, norm = _budgets(P, ctx, gpu, level, np.ascontiguousarray(cts[:B]), sk, scheme, chunk)
            for b in range(B):
                m, bud, _ = refs[b]
                assert [int(w) for w in norm[b]] == _words(m, level), f"{what} B {B} chunk {chunk} ciphertext {b}: norm"
                assert int(budget[b]) == bud, f"{what} B {B} chunk {chunk} ciphertext {b}: budget {budget[b]}, want {bud}"
            if B == len(cts):
                first = (budget, norm) if first is None else first
                assert np.array_equal(first[0], budget) and np.array_equal(first[1], norm), f"{what}: chunk {chunk} gives other words"
    return [r[1] for r in refs], [r[0] for r in refs], big


def _relin_key(P, ctx, gpu, sch, scheme):
    new_key, a, e = sch.relin_randomness()
    dev = lambda x: P.to_device(np.ascontiguousarray(x), gpu)   # noqa: E731
    return ctx.generate_one_kswitch_key(dev(sch.sk_ntt), dev(new_key), dev(a), dev(e), scheme)


def _bfv_products(gpu, name, multiply, room):
    """Fresh encryptions, their size-3 products by `multiply` read with s and s^2, and the relinearized products: norm and budget exact
    against the reference, |budget - margin| < 1, fresh > product; room: the product keeps noise room (product > 0).
    Returns what the caller goes on with."""
    import torch
    sch = S.scheme(name, O.BFV)
    P, ctx = _ctx(name, gpu, T)
    bfv, level, n = P.scheme_type.bfv, sch.size_q, sch.n
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    plain = rng_for(9700).integers(0, T, (9, n), dtype=np.uint64)
    fresh = np.stack([sch.encrypt(plain[b], level, ("noise", b)) for b in range(9)])
    b_fresh, _, big = _check_against(P, ctx, gpu, sch, level, fresh, sk, bfv, T, f"{name} fresh")
    for b in range(9):
        margin = sch.decrypt(fresh[b], level)[1]
        assert abs(b_fresh[b] - margin) < 1, (b, b_fresh[b], margin)
    d_all = P.to_device(fresh, gpu)
    d3 = _p64((9, 3, level, n), gpu)
    getattr(ctx, multiply)(d_all, torch.roll(d_all, -1, 0).contiguous(), d3)
    prod3 = P.to_host(d3)
    b_prod, _, _ = _check_against(P, ctx, gpu, sch, level, prod3, sk, bfv, T, f"{name} {multiply} size-3 products")
    key = _relin_key(P, ctx, gpu, sch, bfv)
    ct2, c2 = d3[:, :2].contiguous(), d3[:, 2].contiguous()
    ctx.keyswitch_inplace_batched(level, ct2, c2, 9, key.public_keys_ptr, bfv)
    relin = P.to_host(ct2)
    b_relin, _, _ = _check_against(P, ctx, gpu, sch, level, relin, sk, bfv, T, f"{name} {multiply} relinearized products")
    print(f"{name} {multiply}: budgets fresh {list(b_fresh)}, product {list(b_prod)}, relinearized {list(b_relin)}")
    for b in range(9):
        assert b_fresh[b] > b_prod[b] and b_fresh[b] > b_relin[b], (b, b_fresh[b], b_prod[b], b_relin[b])
        assert abs(b_prod[b] - sch.decrypt(prod3[b], level)[1]) < 1
        assert abs(b_relin[b] - sch.decrypt(relin[b], level)[1]) < 1
        if room:
            assert b_prod[b] > 0 and b_relin[b] > 0, (b, b_prod[b], b_relin[b])
    del key
    return sch, P, ctx, sk, plain, fresh, b_fresh, big


@pytest.mark.parametrize("name,multiply", [("hyb12_a2", "bfv_multiply_behz_batched"), ("c1_bfv4096", "bfv_multiply_hps_batched")])
def test_bfv_budgets_fresh_product_relinearized_in_order(name, multiply, gpu):
    """fresh budget > product budget > 0 where the multiply suits the parameter set: BEHZ on hyb12_a2, HPS on c1_bfv4096 (the CPU
    pipeline's margins: 238.5 -> 211.0 bits, and 50.5 -> 22.9 bits)."""
    ctx = _bfv_products(gpu, name, multiply, room=True)[2]
    del ctx
    _release()


def test_bfv_budgets_hps_products_leveled_and_pushed_hyb12(gpu):
    """hyb12_a2 under HPS: norm and budget are exact against the reference, but the product itself has no room left -- HPS takes its
    auxiliary base R below the SMALLEST q_i (40 bits here, next to a 60-bit limb), so t / Q times the tensor product does not fit R.
    The CPU pipeline (oracle Hps.multiply + BvScheme.decrypt) reports a margin of 0.0012 bits for the same product: the budget is 0
    by the reference too, and `product > 0` is asserted where the multiply suits the parameters (the test above)."""
    sch, P, ctx, sk, plain, fresh, b_fresh, big = _bfv_products(gpu, "hyb12_a2", "bfv_multiply_hps_batched", room=False)
    bfv, level = P.scheme_type.bfv, sch.size_q
    # a leveled ciphertext: size_Ql < |Q|
    low = 3
    leveled = np.stack([sch.encrypt(plain[0], low, ("noise.low", 0))])
    b_low, _, _ = _check_against(P, ctx, gpu, sch, low, leveled, sk, bfv, T, "bfv leveled")
    assert 0 < b_low[0] < b_fresh[0]
    # floor(Q / (2 t)) added to coefficient 0 of c0: t * phase moves by about Q / 2, no room is left
    pushed = fresh[:1].copy()
    q = [int(p) for p in sch.primes[:level]]
    bump = big // (2 * T)
    for i, p in enumerate(q):
        pushed[0, 0, i, 0] = np.uint64((int(pushed[0, 0, i, 0]) + bump) % p)
    b_pushed, _, _ = _check_against(P, ctx, gpu, sch, level, pushed, sk, bfv, T, "bfv pushed to the edge")
    assert b_pushed[0] == 0
    del ctx
    _release()


def test_bgv_budgets_fresh_and_after_the_mod_switch(gpu):
    import torch
    sch = S.scheme("hyb12_a2", O.BGV)
    P, ctx = _ctx("hyb12_a2", gpu, T)
    bgv, level, n = P.scheme_type.bgv, sch.size_q, sch.n
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    plain = rng_for(9710).integers(0, T, (9, n), dtype=np.uint64)
    fresh = np.stack([sch.encrypt(plain[b], level, ("noise", b)) for b in range(9)])
    b_fresh, _, _ = _check_against(P, ctx, gpu, sch, level, fresh, sk, bgv, 1, "bgv fresh")
    for b in range(9):
        assert abs(b_fresh[b] - sch.decrypt(fresh[b], level)[1]) < 1
    # products, key switch fused with the modulus switch: level - 1
    d_all = P.to_device(fresh, gpu)
    d_rot = torch.roll(d_all, -1, 0).contiguous()
    t3 = _p64((9, 3, level, n), gpu)
    for b in range(9):
        ctx.tensor_prod_2x2_rns_poly(d_all[b], d_rot[b], t3[b], level)
    key = _relin_key(P, ctx, gpu, sch, bgv)
    dst = _p64((9, 2, level - 1, n), gpu)
    ctx.keyswitch_mod_switch_batched(level, t3[:, :2].contiguous(), t3[:, 2].contiguous(), 9, key.public_keys_ptr, dst)
    switched = P.to_host(dst)
    b_sw, _, _ = _check_against(P, ctx, gpu, sch, level - 1, switched, sk, bgv, 1, "bgv after keyswitch_mod_switch")
    for b in range(9):
        assert b_fresh[b] > b_sw[b] > 0, (b, b_fresh[b], b_sw[b])
        assert abs(b_sw[b] - sch.decrypt(switched[b], level - 1)[1]) < 1
    del ctx, key
    _release()


def test_ckks_headroom_of_an_encrypted_encoding(gpu):
    sch = CS.scheme("hyb12_a2")
    P, ctx = _ctx("hyb12_a2", gpu)                           # no plain modulus: ckks needs none
    level, n = sch.size_q, sch.n
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 1)
    pt = CS.cpu_codec("hyb12_a2").encode(CS.messages(77, 1, sch.slots), level, float(1 << 40))[0]
    ct = sch.encrypt(pt, level, "noise")
    coeff = sch.oc.nwt_backward(sch.decrypt(ct, level), level, 0)
    v, big = S.BvScheme.compose(sch, coeff, level)
    m = _norm_of(v, big)
    for chunk in (1, 0):
        budget, norm = _budgets(P, ctx, gpu, level, ct[None], sk, P.scheme_type.ckks, chunk)
        assert [int(w) for w in norm[0]] == _words(m, level)
        assert int(budget[0]) == _budget_of(m, big) and budget[0] > 0
    del ctx
    _release()


@pytest.mark.parametrize("scheme", ["bfv", "bgv"])
def test_the_three_tails_share_one_phase(scheme, gpu):
    """One front end feeds the decrypt entries and the noise budget: on one strided batch of uniform ciphertexts (hyb12_a2, level 3,
    cipher_size 3, batch 5 -- a short last phase group, and under bfv the per-ciphertext forward transforms -- stride 3 L N + 16) the
    norm of the budget entry and the plaintexts of the decrypt entry are, word for word, those of the single-step entries applied to
    the phase built from the earlier entries; chunk 0, 1 and 2."""
    import torch
    P, ctx = _ctx("hyb12_a2", gpu, T)
    level, k, B, n = 3, 3, 5, ctx.n
    ln = level * n
    stride = k * ln + 16
    qs = [int(q) for q in primes_of("hyb12_a2")[1]][:level]
    rng = rng_for(9790 + len(scheme))
    cts = np.stack([np.stack([uniform_poly(rng, qs, n) for _ in range(k)]) for _ in range(B)])
    dense = P.to_device(cts, gpu)                                   # [B][k][L][N]
    buf = _p64((B * stride,), gpu)
    for b in range(B):
        buf[b * stride:b * stride + k * ln] = dense[b].reshape(-1)
    before = buf.clone()
    sk = ctx.secret_key_powers(P.to_device(uniform_poly(rng, [int(q) for q in primes_of("hyb12_a2")[1]], n), gpu), k - 1)
    phase = torch.empty((B, level, n), dtype=torch.int64, device=gpu)
    if scheme == "bfv":     # forward NTT of c1, c2; the phase without c0; inverse NTT; + c0
        ntt = dense.clone()
        ntt[:, 0] = 0
        for i in (1, 2):
            part = ntt[:, i].contiguous()
            ctx.nwt_2d_radix8_forward_inplace_batched(part, level, 0, B, ln)
            ntt[:, i] = part
        ctx.decrypt_phase_batched(level, ntt, sk, phase)
        ctx.nwt_2d_radix8_backward_inplace_batched(phase, level, 0, B, ln)
        for b in range(B):
            ctx.add_rns_poly(phase[b], dense[b, 0].contiguous(), phase[b], level)
    else:                   # the phase; inverse NTT
        ctx.decrypt_phase_batched(level, buf, sk, phase, cipher_size=k, batch=B, strides=(stride, ln))
        ctx.nwt_2d_radix8_backward_inplace_batched(phase, level, 0, B, ln)
    bits, want_norm, want_plain = _p32((B,), gpu), _p64((B, level), gpu), _p64((B, n), gpu)
    ctx.poly_infty_norm_batched(level, phase, bits, want_norm, scalar=T if scheme == "bfv" else 1)
    for b in range(B):
        (ctx.hps_decrypt_scale_and_round if scheme == "bfv" else ctx.decrypt_mod_t)(level, want_plain[b], phase[b])
    decrypt = ctx.bfv_decrypt_batched if scheme == "bfv" else ctx.bgv_decrypt_batched
    for chunk in (0, 1, 2):
        budget, norm, plain = _p32((B,), gpu), _p64((B, level), gpu), _p64((B, n), gpu)
        ctx.invariant_noise_budget_batched(level, buf, sk, getattr(P.scheme_type, scheme), budget, norm, cipher_size=k, batch=B,
                                           stride=stride, chunk=chunk)
        decrypt(level, buf, sk, plain, cipher_size=k, batch=B, strides=(stride, n), chunk=chunk)
        assert torch.equal(norm, want_norm), f"{scheme} chunk {chunk}: the budget entry's norm is not the norm of the phase"
        assert torch.equal(plain, want_plain), f"{scheme} chunk {chunk}: the decrypt entry's plaintexts are not the tail of the phase"
        assert bool((budget != POISON32).all()) and bool((buf == before).all()), f"{scheme} chunk {chunk}"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: refusals, batch == 0, norm == NULL, strict mode
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_empty_batch_and_null_norm(gpu):
    import torch
    sch = S.scheme("hyb12_a2", O.BGV)
    P, ctx = _ctx("hyb12_a2", gpu, T)
    _, bare = _ctx("hyb12_a2", gpu)
    level, k, batch, n = 3, 3, 2, sch.n
    ln = level * n
    rng = rng_for(9720)
    cts = np.stack([np.stack([uniform_poly(rng, sch.primes[:level], n) for _ in range(k)]) for _ in range(batch)])
    ct = P.to_device(cts, gpu)
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    big = _p64((batch * k * ln + 64,), gpu)
    budget, norm, bits = _p32((batch,), gpu), _p64((batch, level), gpu), _p32((batch,), gpu)
    bgv = P.scheme_type.bgv

    def refused(text, fn, *args, **kw):
        with pytest.raises(ValueError) as e:
            fn(*args, **kw)
        assert text in str(e.value), str(e.value)

    nb = ctx.invariant_noise_budget_batched
    shape = dict(cipher_size=k, batch=batch, n_powers=2)
    refused("null", nb, level, None, sk, bgv, budget, norm, **shape)
    refused("null", nb, level, ct, None, bgv, budget, norm, **shape)
    with pytest.raises((ValueError, AttributeError)):
        nb(level, ct, sk, bgv, None, norm, **shape)
    from phantom_fhe_amd import lib as L
    args = [ctx._h, level, ct.data_ptr(), k, batch, k * ln, sk.data_ptr(), 2, int(bgv), None, norm.data_ptr(), 0, None]
    assert L.load().pha_invariant_noise_budget_batched(*args) == -1 and b"null" in L.load().pha_last_error()
    for bad_level in (0, sch.size_q + 1):
        refused("RNSBase is invalid", nb, bad_level, ct, sk, bgv, budget, norm, **shape)
    refused("cipher_size", nb, level, ct, sk, bgv, budget, norm, cipher_size=1, batch=batch, n_powers=2)
    refused("fewer powers", nb, level, ct, sk, bgv, budget, norm, cipher_size=k, batch=batch, n_powers=1)
    refused("ct stride", nb, level, ct, sk, bgv, budget, norm, stride=k * ln - 2)
    refused("even", nb, level, ct, sk, bgv, budget, norm, stride=k * ln + 1)
    refused("aligned", nb, level, big[1:1 + batch * k * ln], sk, bgv, budget, norm, **shape)
    refused("unsupported scheme", nb, level, ct, sk, 7, budget, norm, **shape)
    refused("unsupported scheme", nb, level, ct, sk, 0, budget, norm, **shape)
    for scheme in (P.scheme_type.bfv, bgv):
        refused("plain modulus", bare.invariant_noise_budget_batched, level, ct, sk, scheme, budget, norm, **shape)
    as32 = ct.reshape(-1).view(torch.int32)
    refused("budget must not overlap ct", nb, level, ct, sk, bgv, as32[2 * n:2 * n + batch], norm, **shape)
    refused("budget must not overlap sk_powers", nb, level, ct, sk, bgv, sk.reshape(-1).view(torch.int32)[:batch], norm, **shape)
    refused("norm must not overlap ct", nb, level, ct, sk, bgv, budget, ct.reshape(-1)[n:n + batch * level], **shape)
    refused("norm must not overlap sk_powers", nb, level, ct, sk, bgv, budget, sk.reshape(-1)[:batch * level], **shape)
    # the norm entry
    pn = ctx.poly_infty_norm_batched
    src = ct[:, 0].contiguous()
    refused("null", pn, level, None, bits, norm, count=batch)
    refused("RNSBase is invalid", pn, 0, src, bits, norm)
    refused("RNSBase is invalid", pn, sch.size_q + 1, src, bits, norm)
    refused("src stride", pn, level, src, bits, norm, stride=ln - 1)
    refused("norm must not overlap src", pn, level, src, bits, src.reshape(-1)[8:8 + batch * level])
    refused("bits must not overlap src", pn, level, src, src.reshape(-1).view(torch.int32)[4:4 + batch], norm)
    torch.cuda.synchronize()
    assert bool((budget == POISON32).all()) and bool((bits == POISON32).all()) and bool((norm == POISON).all()), "a refused call wrote"
    assert np.array_equal(P.to_host(ct), cts)
    # batch == 0 / count == 0 do nothing
    nb(level, ct, sk, bgv, budget, norm, cipher_size=k, batch=0, n_powers=2)
    pn(level, src, bits, norm, count=0)
    torch.cuda.synchronize()
    assert bool((budget == POISON32).all()) and bool((bits == POISON32).all()) and bool((norm == POISON).all()), "an empty batch wrote"
    # norm == NULL: the same budgets / bits, nothing else written
    nb(level, ct, sk, bgv, budget, norm)
    alone = _p32((batch,), gpu)
    nb(level, ct, sk, bgv, alone)
    assert bool((alone == budget).all()) and not bool((budget == POISON32).any())
    pn(level, src, bits, norm)
    alone = _p32((batch,), gpu)
    pn(level, src, alone)
    assert bool((alone == bits).all()) and not bool((bits == POISON32).any())
    # ckks needs no plain modulus
    bare_sk = bare.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    alone = _p32((batch,), gpu)
    bare.invariant_noise_budget_batched(level, ct, bare_sk, P.scheme_type.ckks, alone)
    assert bool((alone == budget).all()), "bgv and ckks take the same norm (scalar = 1)"
    del ctx, bare
    _release()


def test_strict_mode_names_the_operand(gpu):
    sch = S.scheme("hyb12_a2", O.BGV)
    P, ctx = _ctx("hyb12_a2", gpu, T)
    level, k, batch, n = 3, 3, 5, sch.n
    rng = rng_for(9730)
    cts = np.stack([np.stack([uniform_poly(rng, sch.primes[:level], n) for _ in range(k)]) for _ in range(batch)])
    bad = cts.copy()
    bad[3, 2, level - 1, n - 1] = np.uint64(sch.primes[level - 1])        # one word == q in ciphertext 3 of 5
    d_ct, d_bad = P.to_device(cts, gpu), P.to_device(bad, gpu)
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    bad_sk = sk.clone()
    bad_sk[1, 0, 5] = int(sch.primes[0]) + 1
    prev = P.set_strict(True)
    try:
        for scheme in (P.scheme_type.bgv, P.scheme_type.bfv, P.scheme_type.ckks):
            budget = _p32((batch,), gpu)
            with pytest.raises(ValueError) as e:
                ctx.invariant_noise_budget_batched(level, d_bad, sk, scheme, budget)
            assert "PHA_STRICT" in str(e.value) and "noise_budget ct" in str(e.value) and "1 word" in str(e.value), str(e.value)
            with pytest.raises(ValueError) as e:
                ctx.invariant_noise_budget_batched(level, d_ct, bad_sk, scheme, budget)
            assert "noise_budget sk_powers" in str(e.value), str(e.value)
            assert bool((budget == POISON32).all())
            ctx.invariant_noise_budget_batched(level, d_ct, sk, scheme, budget)       # canonical operands pass
        bits = _p32((batch,), gpu)
        with pytest.raises(ValueError) as e:
            ctx.poly_infty_norm_batched(level, d_bad[:, 2].contiguous(), bits)
        assert "PHA_STRICT" in str(e.value) and "poly_infty_norm src" in str(e.value) and "1 word" in str(e.value), str(e.value)
        assert bool((bits == POISON32).all())
        ctx.poly_infty_norm_batched(level, d_ct[:, 2].contiguous(), bits)
    finally:
        P.set_strict(prev)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# E: the workload
# ------------------------------------------------------------------------------------------------------------------------------
def test_workload_equals_the_entry(gpu):
    import torch
    from phantom_fhe_amd import workloads as W
    sch = S.scheme("hyb12_a2", O.BFV)
    P, ctx = _ctx("hyb12_a2", gpu, T)
    level, n = sch.size_q, sch.n
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 1)
    plain = rng_for(9740).integers(0, T, (3, n), dtype=np.uint64)
    cts = P.to_device(np.stack([sch.encrypt(plain[b], level, ("noise.w", b)) for b in range(3)]), gpu)
    got = W.noise_budget_batch(ctx, cts, level, sk, P.scheme_type.bfv)
    assert got.dtype == torch.int32 and got.shape == (3,) and got.device == cts.device
    want = _p32((3,), gpu)
    ctx.invariant_noise_budget_batched(level, cts, sk, P.scheme_type.bfv, want)
    assert bool((got == want).all()) and int(got.min()) > 0
    empty = W.noise_budget_batch(ctx, cts[:0], level, sk, P.scheme_type.bfv)
    assert empty.shape == (0,)
    del ctx
    _release()
