"""GPU parity of the BGV key switch fused with mod_switch_to_next: pha_keyswitch_mod_switch(_batched),
pha_inner_product_relin_mod_switch_batched and the mirror's relinearize_mod_switch / multiply_relin_mod_switch.  Bit for bit on
every output word, every output buffer poisoned before the call so that an unwritten word fails.

1. against the oracle's composition keyswitch_inplace(BGV) then mod_t_divide_q_last_ntt, at every shape the path branches on
   (alpha = 1, a short last digit, beta = 5, the split converter, alpha > 32, 61-bit special primes, the batched NTT plan), with the
   operands left untouched, the library's own two calls giving the same words, and the single entry equal to the batch of one;
2. one production-size case (N = 2^15, 30 + 15 limbs);
3. the inner-product entry against the summed tensor product followed by the batched entry, every chunk size, and the oracle;
4. refusals: status, message, dst untouched;
5. semantics independent of the oracle's mod-down: a genuine size-3 encryption of m decrypts to m * q_last^-1 mod t afterwards;
6. the pyPhantom names against mod_switch_to_next(relinearize(...));
7. the single entry replayed from a captured graph.
"""
import gc

import numpy as np
import pytest

from oracle import oracle as O
from util import crt_compose, oracle_ctx, primes_of, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

BGV_T = 65537
POISON = -0x2152411021524111          # 0xDEADBEEFDEADBEEF as int64


def _setup(name, gpu, plain_t=BGV_T):
    import phantom_fhe_amd as P
    log_n, primes, size_p = primes_of(name)
    ctx = P.PhantomContext(log_n, list(primes), size_p, device=gpu)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    return P, ctx, 1 << log_n, primes, size_p, len(primes) - size_p


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _poisoned(shape, gpu):
    import torch
    return torch.full(shape, POISON, dtype=torch.int64, device=gpu)


def _keys(rng, primes, n, size_q, size_p):
    """Uniform synthetic evaluation keys [dnum][2][QP][N], as tests/test_gpu_rns.py makes them."""
    dnum = -(-size_q // size_p)
    return np.stack([np.stack([uniform_poly(rng, primes, n), uniform_poly(rng, primes, n)]) for _ in range(dnum)])


def _first_diff(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    idx = tuple(int(v) for v in np.argwhere(got != ref)[0])
    raise AssertionError(f"{what}: {int(np.count_nonzero(got != ref))} words differ, first at {idx}: got {int(got[idx])}, "
                         f"want {int(ref[idx])}")


def _oracle_fused(tool, ct, c2, keys):
    return tool.mod_t_divide_q_last_ntt(tool.keyswitch_inplace(ct, c2, keys, O.BGV), 2)


def _two_calls(P, ctx, ql, d_ct, d_c2, batch, rlk, n, gpu):
    """the library's existing composition, on a copy: the batched key switch, then the switch"""
    work = d_ct.clone()
    two = _poisoned((batch, 2, ql - 1, n), gpu)
    ctx.keyswitch_inplace_batched(ql, work, d_c2, batch, rlk.public_keys_ptr, O.BGV)
    ctx.mod_t_and_divide_q_last_ntt(ql, work, 2 * batch, two)
    return two


def _check_case(name, ql, batch, gpu, plain_t=BGV_T, extreme=False, rng_id=0, oracle_upto=None):
    import torch
    P, ctx, n, primes, size_p, size_q = _setup(name, gpu, plain_t)
    ql = size_q if ql is None else ql
    oc = oracle_ctx(name)
    tool = O.Tool(oc, ql).set_plain_modulus(plain_t)
    r = rng_for(9700 + rng_id)
    evk = _keys(r, primes, n, size_q, size_p)
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    ct = np.stack([np.stack([uniform_poly(r, primes[:ql], n) for _ in range(2)]) for _ in range(batch)])
    c2 = np.stack([uniform_poly(r, primes[:ql], n) for _ in range(batch)])
    if extreme:                             # every word of the first ciphertext at q - 1
        top = np.stack([np.full(n, int(q) - 1, dtype=np.uint64) for q in primes[:ql]])
        ct[0] = np.stack([top, top])
        c2[0] = top
    d_ct, d_c2 = P.to_device(ct, gpu), P.to_device(c2, gpu)
    dst = _poisoned((batch, 2, ql - 1, n), gpu)
    ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, batch, rlk.public_keys_ptr, dst)
    got = P.to_host(dst)
    keys = [evk[i] for i in range(tool.beta)]
    for b in range(batch if oracle_upto is None else oracle_upto):
        _first_diff(got[b], _oracle_fused(tool, ct[b], c2[b], keys), f"{name} ql={ql} batch={batch}: ciphertext {b} against the oracle")
    assert np.array_equal(P.to_host(d_ct), ct) and np.array_equal(P.to_host(d_c2), c2), "the fused call wrote to an operand"
    two = _two_calls(P, ctx, ql, d_ct, d_c2, batch, rlk, n, gpu)
    _first_diff(got, P.to_host(two), f"{name} ql={ql} batch={batch}: against the library's two calls")
    one = _poisoned((2, ql - 1, n), gpu)
    ctx.keyswitch_mod_switch(ql, d_ct[0], d_c2[0], rlk.public_keys_ptr, one)
    assert torch.equal(one, dst[0]), "the single entry differs from the batched one"
    del ctx, rlk, d_ct, d_c2, dst, two, one
    _release()


# (config, live data limbs (None: the top level), batch): what each covers is in the module docstring and beside the case
CASES = [
    ("hyb12_a2", 6, 1),
    ("hyb12_a2", 5, 1),
    ("hyb12_a2", 2, 1),          # one output limb
    ("hyb12_a2", 6, 3),          # batch > 1
    ("c1_bfv4096", 2, 1),        # alpha = 1
    ("hyb13_a3", 9, 2),
    ("hyb13_a3", 7, 2),          # short last digit
    ("hyb13_b5", 10, 2),         # beta = 5
    ("wide_p20", 20, 1),         # the split converter
    ("wide_p33", None, 1),       # alpha > 32
    ("p61_a2", 6, 1),            # 61-bit special primes
    ("hyb14_a4", 8, 8),          # 16 polynomials: the batched NTT plan
]


@pytest.mark.parametrize("name,ql,batch", CASES)
def test_fused_equals_keyswitch_then_mod_switch(name, ql, batch, gpu):
    _check_case(name, ql, batch, gpu, rng_id=CASES.index((name, ql, batch)))


def test_extreme_residues(gpu):
    _check_case("hyb12_a2", 6, 1, gpu, extreme=True, rng_id=40)


def test_other_plain_modulus(gpu):
    _check_case("hyb12_a2", 6, 1, gpu, plain_t=786433, rng_id=41)


def test_production_size(gpu):
    """N = 2^15, 30 + 15 limbs, t = 786433, two ciphertexts: the whole batch against the device composition, ciphertext 0 against
    the oracle."""
    _check_case("c4_bfv15", 30, 2, gpu, plain_t=786433, rng_id=42, oracle_upto=1)


# ------------------------------------------------------------------------------------------------------------------------------
# 3: inner products
# ------------------------------------------------------------------------------------------------------------------------------
def _operands(rng, primes, shape_front, n):
    out = np.empty(tuple(shape_front) + (2, len(primes), n), dtype=np.uint64)
    for j, q in enumerate(primes):
        out[..., j, :] = rng.integers(0, int(q), tuple(shape_front) + (2, n), dtype=np.uint64)
    return out


def _oracle_sum(oc, a, b, limbs):
    acc = None
    for k in range(a.shape[0]):
        p = oc.tensor_prod_2x2(a[k], b[k], limbs)
        acc = p if acc is None else np.stack([oc.add(acc[i], p[i], limbs) for i in range(3)])
    return acc


@pytest.mark.parametrize("name,ql", [("hyb12_a2", 6), ("hyb13_a3", 9)])
def test_inner_product(name, ql, gpu):
    import torch
    P, ctx, n, primes, size_p, size_q = _setup(name, gpu)
    terms, batch = 3, 3
    r = rng_for(9750 + ql)
    evk = _keys(r, primes, n, size_q, size_p)
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    op1, op2 = _operands(r, primes[:ql], (batch, terms), n), _operands(r, primes[:ql], (batch, terms), n)
    d1, d2 = P.to_device(op1, gpu), P.to_device(op2, gpu)
    keep1, keep2 = d1.clone(), d2.clone()
    s01, s2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    want = _poisoned((batch, 2, ql - 1, n), gpu)
    ctx.tensor_prod_2x2_sum_batched(d1, d2, s01, s2, ql, terms, batch)
    ctx.keyswitch_mod_switch_batched(ql, s01, s2, batch, rlk.public_keys_ptr, want)
    for chunk in (0, 1, 2):
        dst = _poisoned((batch, 2, ql - 1, n), gpu)
        ctx.inner_product_relin_mod_switch_batched(ql, d1, d2, terms, batch, rlk.public_keys_ptr, dst, chunk=chunk)
        assert torch.equal(dst, want), f"chunk {chunk} differs from the sum followed by the batched entry"
    assert torch.equal(d1, keep1) and torch.equal(d2, keep2), "the inner product wrote to an operand"
    oc = oracle_ctx(name)
    tool = O.Tool(oc, ql).set_plain_modulus(BGV_T)
    t3 = _oracle_sum(oc, op1[0], op2[0], ql)
    _first_diff(P.to_host(want[0]), _oracle_fused(tool, t3[:2], t3[2], [evk[i] for i in range(tool.beta)]), f"{name}: group 0 against the oracle")
    if name == "hyb12_a2":       # a shared vector: operand 2 with a batch stride of 0 against the same vector replicated
        shared = d2[0].contiguous()
        rep = shared.unsqueeze(0).repeat(batch, 1, 1, 1, 1).contiguous()
        a, b = _poisoned((batch, 2, ql - 1, n), gpu), _poisoned((batch, 2, ql - 1, n), gpu)
        ctx.inner_product_relin_mod_switch_batched(ql, d1, shared, terms, batch, rlk.public_keys_ptr, a)
        ctx.inner_product_relin_mod_switch_batched(ql, d1, rep, terms, batch, rlk.public_keys_ptr, b, chunk=2)
        assert torch.equal(a, b) and not bool((a == POISON).any())
    del ctx, rlk
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# 4: refusals
# ------------------------------------------------------------------------------------------------------------------------------
def _refused(call, dsts, fragment):
    import torch
    with pytest.raises(ValueError) as e:
        call()
    assert fragment in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for d in dsts:
        assert bool((d == POISON).all()), f"a refused call wrote to its output ({fragment})"


def test_refusals(gpu):
    import torch
    name, ql, batch = "hyb12_a2", 6, 2
    P, ctx, n, primes, size_p, size_q = _setup(name, gpu)
    r = rng_for(9790)
    rlk = P.PhantomRelinKey.from_numpy(_keys(r, primes, n, size_q, size_p), gpu)
    kp = rlk.public_keys_ptr
    d_ct = P.to_device(np.stack([np.stack([uniform_poly(r, primes[:ql], n) for _ in range(2)]) for _ in range(batch)]), gpu)
    d_c2 = P.to_device(np.stack([uniform_poly(r, primes[:ql], n) for _ in range(batch)]), gpu)
    dst = _poisoned((batch, 2, ql - 1, n), gpu)
    for args in ((None, d_c2, batch, kp, dst), (d_ct, None, batch, kp, dst), (d_ct, d_c2, batch, None, dst)):
        _refused(lambda: ctx.keyswitch_mod_switch_batched(ql, *args), [dst], "null device pointer")
    _refused(lambda: ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, batch, kp, None), [dst], "null device pointer")
    _refused(lambda: ctx.keyswitch_mod_switch(ql, d_ct[0], d_c2[0], kp, None), [dst], "null device pointer")
    _refused(lambda: ctx.keyswitch_mod_switch_batched(size_q + 1, d_ct, d_c2, batch, kp, dst), [dst], "size_Ql out of range")
    _refused(lambda: ctx.keyswitch_mod_switch_batched(0, d_ct, d_c2, batch, kp, dst), [dst], "size_Ql out of range")
    _refused(lambda: ctx.keyswitch_mod_switch_batched(1, d_ct, d_c2, batch, kp, dst), [dst], "last remaining modulus")
    _refused(lambda: ctx.keyswitch_mod_switch(1, d_ct[0], d_c2[0], kp, dst[0]), [dst], "last remaining modulus")
    _refused(lambda: ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, 1025, kp, dst), [dst], "batch out of range")
    keep_ct, keep_c2 = d_ct.clone(), d_c2.clone()
    for bad in (d_ct.view(-1)[n:n + batch * 2 * (ql - 1) * n], d_ct.view(-1)[:2 * (ql - 1) * n]):
        with pytest.raises(ValueError, match="dst must not overlap ct or c2"):
            ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, 1, kp, bad)
    with pytest.raises(ValueError, match="dst must not overlap ct or c2"):
        ctx.keyswitch_mod_switch(ql, d_ct[0], d_c2, kp, d_c2.view(-1)[2 * n:2 * n + 2 * (ql - 1) * n])
    torch.cuda.synchronize()
    assert torch.equal(d_ct, keep_ct) and torch.equal(d_c2, keep_c2), "a refused call wrote to an operand"
    ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, 0, kp, dst)          # batch == 0: status 0, nothing happens
    torch.cuda.synchronize()
    assert bool((dst == POISON).all())
    # the inner-product entry: its own refusals and the ones it shares
    op = P.to_device(np.stack([np.stack([np.stack([uniform_poly(r, primes[:ql], n) for _ in range(2)])] * 2)] * batch), gpu)
    _refused(lambda: ctx.inner_product_relin_mod_switch_batched(ql, None, op, 2, batch, kp, dst), [dst], "null device pointer")
    _refused(lambda: ctx.inner_product_relin_mod_switch_batched(ql, op, op, 2, batch, kp, None), [dst], "null device pointer")
    _refused(lambda: ctx.inner_product_relin_mod_switch_batched(1, op, op, 2, batch, kp, dst, strides=(2 * n, 4 * n, 2 * n, 4 * n)),
             [dst], "last remaining modulus")
    _refused(lambda: ctx.inner_product_relin_mod_switch_batched(size_q + 1, op, op, 2, batch, kp, dst, strides=(0, 0, 0, 0)),
             [dst], "size_Ql out of range")
    _refused(lambda: ctx.inner_product_relin_mod_switch_batched(ql, op, op, 0, batch, kp, dst, strides=(0, 0, 0, 0)), [dst], "terms")
    with pytest.raises(ValueError, match="dst must not overlap an operand ciphertext"):
        ctx.inner_product_relin_mod_switch_batched(ql, op, op, 2, batch, kp, op.view(-1)[:batch * 2 * (ql - 1) * n])
    ctx.inner_product_relin_mod_switch_batched(ql, op, op, 2, 0, kp, dst, strides=(2 * ql * n, 4 * ql * n, 2 * ql * n, 4 * ql * n))
    torch.cuda.synchronize()
    assert bool((dst == POISON).all())
    # a fresh context without a plain modulus
    _, bare, *_ = _setup(name, gpu, plain_t=None)
    _refused(lambda: bare.keyswitch_mod_switch_batched(ql, d_ct, d_c2, batch, kp, dst), [dst], "bgv needs a plain modulus (pha_context_set_plain_modulus)")
    _refused(lambda: bare.keyswitch_mod_switch(ql, d_ct[0], d_c2[0], kp, dst[0]), [dst], "bgv needs a plain modulus (pha_context_set_plain_modulus)")
    _refused(lambda: bare.inner_product_relin_mod_switch_batched(ql, op, op, 2, batch, kp, dst), [dst],
             "bgv needs a plain modulus (pha_context_set_plain_modulus)")
    # a context without a special modulus
    log_n2, primes2, size_p2 = primes_of("c2_ntt14")
    assert size_p2 == 0
    nop = P.PhantomContext(log_n2, list(primes2), 0, device=gpu)
    _refused(lambda: nop.keyswitch_mod_switch_batched(4, d_ct, d_c2, 1, kp, dst), [dst], "context has no special modulus")
    _refused(lambda: nop.inner_product_relin_mod_switch_batched(4, op, op, 2, 1, kp, dst, strides=(0, 0, 0, 0)), [dst],
             "context has no special modulus")
    del ctx, bare, nop, rlk
    _release()


def test_strict_mode_names_the_operand(gpu):
    import torch
    name, ql, batch = "hyb12_a2", 6, 2
    P, ctx, n, primes, size_p, size_q = _setup(name, gpu)
    r = rng_for(9791)
    rlk = P.PhantomRelinKey.from_numpy(_keys(r, primes, n, size_q, size_p), gpu)
    kp = rlk.public_keys_ptr
    d_ct = P.to_device(np.stack([np.stack([uniform_poly(r, primes[:ql], n) for _ in range(2)]) for _ in range(batch)]), gpu)
    d_c2 = P.to_device(np.stack([uniform_poly(r, primes[:ql], n) for _ in range(batch)]), gpu)
    dst = _poisoned((batch, 2, ql - 1, n), gpu)
    was = P.set_strict(True)
    try:
        ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, batch, kp, dst)      # canonical operands pass
        torch.cuda.synchronize()
        good = P.to_host(dst).copy()
        dst.fill_(POISON)
        old = int(d_c2[1, 3, 17])
        d_c2[1, 3, 17] = int(primes[3])                                       # one word at its modulus
        _refused(lambda: ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, batch, kp, dst), [dst], "keyswitch c2")
        _refused(lambda: ctx.keyswitch_mod_switch(ql, d_ct[1], d_c2[1], kp, dst[1]), [dst], "keyswitch c2")
        d_c2[1, 3, 17] = old
        d_ct[0, 1, 2, 5] = int(primes[2]) + 1
        _refused(lambda: ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, batch, kp, dst), [dst], "keyswitch ct")
        op = torch.stack([d_ct, d_ct], dim=1).contiguous()                    # [batch][2 terms][2][L][N], the bad word in both terms
        _refused(lambda: ctx.inner_product_relin_mod_switch_batched(ql, op, op, 2, batch, kp, dst), [dst], "tensor_prod_2x2_sum operand1")
        P.set_strict(False)                                                   # accepted with strict mode off
        ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, batch, kp, dst)
        torch.cuda.synchronize()
        assert not bool((dst == POISON).any())
        assert np.array_equal(P.to_host(dst)[1], good[1])
    finally:
        P.set_strict(was)
    del ctx, rlk
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# 5: what the result decrypts to
# ------------------------------------------------------------------------------------------------------------------------------
def test_decrypts_to_the_message_times_q_last_inverse(gpu):
    """A size-3 ciphertext with c0 + c1 s + c2 s^2 = m + t e under a ternary s, keys generated by the library: after the fused call
    the centred lift of c0 + c1 s over the remaining primes is m * q_last^-1 modulo t, coefficient for coefficient -- the
    correction-factor convention of mod_switch_to_next (src/evaluate.cu:1421-1425), checked with big integers."""
    name = "hyb12_a2"
    P, ctx, n, primes, size_p, size_q = _setup(name, gpu)
    ql, nl, dnum, t = size_q, size_q - 1, size_q // size_p, BGV_T
    oc = oracle_ctx(name)
    r = rng_for(9795)
    s_small = r.integers(-1, 2, n)
    sk_ntt = oc.nwt_forward(np.stack([(s_small % int(q)).astype(np.uint64) for q in primes]), len(primes), 0)
    s2_ntt = oc.multiply(sk_ntt[:size_q], sk_ntt[:size_q], size_q)
    a = np.stack([uniform_poly(r, primes, n) for _ in range(dnum)])
    e_small = r.integers(-3, 4, (dnum, n))
    e_key = np.stack([np.stack([(e_small[d] % int(q)).astype(np.uint64) for q in primes]) for d in range(dnum)])
    rlk = ctx.generate_one_kswitch_key(P.to_device(sk_ntt, gpu), P.to_device(s2_ntt, gpu), P.to_device(a, gpu), P.to_device(e_key, gpu),
                                       O.BGV)
    q = primes[:ql]
    m = r.integers(0, t, n)
    noise = r.integers(-3, 4, n)
    me = np.stack([((m + t * noise) % int(p)).astype(np.uint64) for p in q])            # m + t e
    c1, c2 = uniform_poly(r, q, n), uniform_poly(r, q, n)
    s, s2 = sk_ntt[:ql], s2_ntt[:ql]
    c0 = oc.sub(oc.sub(oc.nwt_forward(me, ql, 0), oc.multiply(c1, s, ql), ql), oc.multiply(c2, s2, ql), ql)
    dst = _poisoned((2, nl, n), gpu)
    ctx.keyswitch_mod_switch(ql, P.to_device(np.stack([c0, c1]), gpu), P.to_device(c2, gpu), rlk.public_keys_ptr, dst)
    res = P.to_host(dst)
    phase = oc.nwt_backward(oc.add(res[0], oc.multiply(res[1], sk_ntt[:nl], nl), nl), nl)
    inv = pow(int(q[nl]) % t, -1, t)
    for k in range(n):
        v, Q = crt_compose([phase[l, k] for l in range(nl)], q[:nl])
        v = v - Q if v > Q // 2 else v
        assert v % t == int(m[k]) * inv % t, f"coefficient {k}"
    del ctx, rlk
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# 6: pyPhantom
# ------------------------------------------------------------------------------------------------------------------------------
def test_pyphantom_names(gpu):
    from phantom_fhe_amd import pyPhantom as ph
    name = "hyb12_a2"
    log_n, primes, size_p = primes_of(name)
    n, size_q = 1 << log_n, len(primes) - size_p
    r = rng_for(9796)

    def make(scheme):
        parms = ph.params(scheme)
        parms.set_poly_modulus_degree(n)
        parms.set_special_modulus_size(size_p)
        parms.set_coeff_modulus(ph.create_coeff_modulus(n, [60, 40, 40, 40, 40, 40, 60, 60]))
        if scheme != ph.scheme_type.ckks:
            parms.set_plain_modulus(ph.modulus(BGV_T))
        return ph.context(parms)

    evk = _keys(r, primes, n, size_q, size_p)
    h1 = np.stack([uniform_poly(r, primes[:size_q], n) for _ in range(2)])
    h2 = np.stack([uniform_poly(r, primes[:size_q], n) for _ in range(2)])
    ctx = make(ph.scheme_type.bgv)
    rlk = ph.relin_key(); rlk.load(ctx, evk)
    a, b = ph.ciphertext(), ph.ciphertext()
    a.load(ctx, 1, h1); b.load(ctx, 1, h2)
    a.set_correction_factor(7); b.set_correction_factor(5)
    a.set_scale(3.0)
    prod = ph.multiply(ctx, a, b)
    ref = ph.mod_switch_to_next(ctx, ph.relinearize(ctx, prod, rlk))
    for got in (ph.relinearize_mod_switch(ctx, prod, rlk), ph.multiply_relin_mod_switch(ctx, a, b, rlk)):
        _first_diff(got.to_numpy(), ref.to_numpy(), "pyPhantom")
        assert got.chain_index() == ref.chain_index() == 2 and got.is_ntt_form() and ref.is_ntt_form()
        assert got.scale() == ref.scale() and got.correction_factor() == ref.correction_factor()
    assert ref.correction_factor() == 35 * pow(int(primes[size_q - 1]) % BGV_T, -1, BGV_T) % BGV_T
    with pytest.raises(ValueError):
        ph.relinearize_mod_switch(ctx, a, rlk)                      # size 2
    for scheme in (ph.scheme_type.ckks, ph.scheme_type.bfv):        # other schemes are refused
        other = make(scheme)
        okey = ph.relin_key(); okey.load(other, evk)
        x, y = ph.ciphertext(), ph.ciphertext()
        x.load(other, 1, h1); y.load(other, 1, h2)
        x.set_scale(2.0 ** 40); y.set_scale(2.0 ** 40)
        three = ph.ciphertext(); three.load(other, 1, np.concatenate([h1, h2[:1]]))
        with pytest.raises(ValueError):
            ph.relinearize_mod_switch(other, three, okey)
        if scheme == ph.scheme_type.ckks:
            with pytest.raises(ValueError):
                ph.multiply_relin_mod_switch(other, x, y, okey)


# ------------------------------------------------------------------------------------------------------------------------------
# 7: graph capture
# ------------------------------------------------------------------------------------------------------------------------------
def test_replays_from_a_captured_graph(gpu):
    """The single entry is plain launches on the caller's stream (scratch from the stream's arena, no host synchronisation): captured
    on a side stream after one warm-up call there, it replays on new inputs to what the eager call gives."""
    import torch
    name, ql = "hyb12_a2", 6
    P, ctx, n, primes, size_p, size_q = _setup(name, gpu)
    r = rng_for(9797)
    rlk = P.PhantomRelinKey.from_numpy(_keys(r, primes, n, size_q, size_p), gpu)
    ins = [(np.stack([uniform_poly(r, primes[:ql], n) for _ in range(2)]), uniform_poly(r, primes[:ql], n)) for _ in range(3)]
    want = []
    for ct, c2 in ins:
        dst = _poisoned((2, ql - 1, n), gpu)
        ctx.keyswitch_mod_switch(ql, P.to_device(ct, gpu), P.to_device(c2, gpu), rlk.public_keys_ptr, dst)
        want.append(P.to_host(dst))
    d_ct, d_c2 = P.to_device(ins[0][0], gpu), P.to_device(ins[0][1], gpu)
    out = _poisoned((2, ql - 1, n), gpu)
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        ctx.keyswitch_mod_switch(ql, d_ct, d_c2, rlk.public_keys_ptr, out)      # warm-up: the stream's scratch arena exists before the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ctx.keyswitch_mod_switch(ql, d_ct, d_c2, rlk.public_keys_ptr, out)
    for i in (1, 2, 0):
        d_ct.copy_(P.to_device(ins[i][0], gpu))
        d_c2.copy_(P.to_device(ins[i][1], gpu))
        out.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(P.to_host(out), want[i]), i
    del g, ctx, rlk
    _release()
