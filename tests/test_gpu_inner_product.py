"""GPU parity of the summed tensor product (pha_tensor_prod_2x2_sum_batched) and of the two inner-product entries built on it
(pha_inner_product_relin_rescale_batched, pha_inner_product_relin_batched).  Bit-exact throughout, every output word compared, every
output buffer poisoned before the call so that an unwritten word fails.

A. the kernel against the oracle (tensor_prod_2x2 per term, summed with add): hyb12_a2, p61_a2, c2_ckks14, wide_p20, over every row
   of the prime table (special primes included: that is where p61_a2 has its 61-bit primes); terms 1, 2, 3, 31, 32, 33, 64, 65, 100;
   batch 1 and 3.  Uniform inputs, and in every term of every ciphertext, at the same coefficient positions
   of both operands, blocks of q - 1, (q - 1) / 2, (q + 1) / 2 and 0: the largest products and the largest centred values line up
   across all terms, which is what breaks an accumulator that flushes one term too late (16 terms per flush on the 61-bit limbs of
   p61_a2, 2 on the 50-bit FP64 limbs);
B. terms == 1 against pha_tensor_prod_2x2_batched on the device;
C. strides: a shared operand 2 (batch stride 0) against the same call with it replicated, and operands that are views with gaps
   into larger buffers against the dense call;
D. both whole operations against pha_tensor_prod_2x2_sum_batched followed by the existing batched key switch, on the device:
   hyb13_a3, hyb14_a4, c2_ckks14 (ckks) and hyb12_a2 with a plain modulus (bgv); batch 7 at chunk 1, 3 and 0;
E. the whole operations against the oracle (sum in the oracle, keyswitch_inplace, rescale_ntt), every group at the small sets; at
   c3_ckks16 (45 limbs, 8 terms, 8 groups sharing operand 2) the whole batch against the device composition and the first and last
   group against the oracle;
F. (replaced by the composition in D at hyb13_a3, ckks, no rescale.)  The issue proposed comparing inner_product_relin_batched with
   the device sum of K separate tensor_prod + keyswitch_inplace results, word for word.  That identity does not hold: the hybrid
   key switch is linear only up to its approximation terms.  The mod-up is a FAST base conversion, x -> x + u Q_digit with an
   overshoot u that depends on the input, so modup(a + b) != modup(a) + modup(b), and the mod-down rounds its own input once per
   key switch instead of once per sum.  Both results decrypt to the same message with slightly different noise, and their NTT-form
   words differ everywhere: in the CPU oracle at hyb13_a3 with three terms all 147456 output words of keyswitch(sum) differ from
   the sum of the key switches.  No other test was changed for this;
G. refusals (status -1, the message, poisoned outputs untouched), and operands unchanged by successful calls; every refusal of
   the four entries with its whole message, and which one a call with several defects reports;
H. strict mode: one word >= its modulus in term k of group g of either operand is refused with the operand named, and accepted
   with strict mode off.
"""
import functools
import gc

import numpy as np
import pytest

from oracle import oracle as O
from util import oracle_ctx, primes_of, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

BGV_T = 65537
POISON = -0x2152411021524111          # 0xDEADBEEFDEADBEEF as int64
TERMS = [1, 2, 3, 31, 32, 33, 64, 65, 100]
BLOCK = 64                            # coefficients per special block


def _setup(name, gpu, plain_t=None):
    import phantom_fhe_amd as P
    log_n, primes, size_p = primes_of(name)
    ctx = P.PhantomContext(log_n, list(primes), size_p, device=gpu)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    return P, ctx, log_n, primes, size_p, len(primes) - size_p


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _poisoned(shape, gpu):
    import torch
    return torch.full(shape, POISON, dtype=torch.int64, device=gpu)


def _plant_blocks(ct, primes):
    """ct [..., limb, N]: blocks of q - 1, (q - 1) / 2, (q + 1) / 2 and 0 at the start and at the end of every polynomial."""
    n = ct.shape[-1]
    for j, q in enumerate(primes):
        q = int(q)
        for at in (0, n - 4 * BLOCK):
            for i, v in enumerate((q - 1, (q - 1) // 2, (q + 1) // 2, 0)):
                ct[..., j, at + i * BLOCK:at + (i + 1) * BLOCK] = v
    return ct


def _operands(rng, primes, batch, terms, n, blocks=True):
    """[batch][terms][2][L][N], uniform, with the special blocks planted in every term of every ciphertext."""
    out = np.empty((batch, terms, 2, len(primes), n), dtype=np.uint64)
    for j, q in enumerate(primes):
        out[:, :, :, j] = rng.integers(0, int(q), (batch, terms, 2, n), dtype=np.uint64)
    return _plant_blocks(out, primes) if blocks else out


def _oracle_sum(oc, a, b, limbs, upto=None):
    """sum over k of tensor_prod_2x2(a[k], b[k]) with the oracle's add; upto: also the partial sums after those term counts."""
    acc, partial = None, {}
    for k in range(a.shape[0]):
        p = oc.tensor_prod_2x2(a[k], b[k], limbs)
        acc = p if acc is None else np.stack([oc.add(acc[i], p[i], limbs) for i in range(3)])
        if upto and k + 1 in upto:
            partial[k + 1] = acc.copy()
    return partial if upto else acc


def _first_diff(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    idx = tuple(int(v) for v in np.argwhere(got != ref)[0])
    msg = f"{what}: {int(np.count_nonzero(got != ref))} words differ, first at {idx}: got {int(got[idx])}, want {int(ref[idx])}"
    print(msg)
    raise AssertionError(msg)


def _keys(rng, primes, n, dnum):
    """Synthetic evaluation keys [dnum][2][QP][N], uniform residues."""
    return np.stack([np.stack([uniform_poly(rng, primes, n), uniform_poly(rng, primes, n)]) for _ in range(dnum)])


# ------------------------------------------------------------------------------------------------------------------------------
# A: the kernel against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
A_CONFIGS = ["hyb12_a2", "p61_a2", "c2_ckks14", "wide_p20"]


@functools.lru_cache(maxsize=1)
def _pool(name):
    """Inputs for 3 groups of 100 terms and the oracle's partial sums after every term count of TERMS."""
    log_n, primes, size_p = primes_of(name)
    n, ql = 1 << log_n, len(primes)      # every row of the prime table: the 61-bit primes of p61_a2 are its special primes
    rng = rng_for(9100 + A_CONFIGS.index(name))
    op1, op2 = _operands(rng, primes[:ql], 3, max(TERMS), n), _operands(rng, primes[:ql], 3, max(TERMS), n)
    oc = oracle_ctx(name)
    ref = [_oracle_sum(oc, op1[g], op2[g], ql, upto=set(TERMS)) for g in range(3)]
    return op1, op2, ref


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("name", A_CONFIGS)
def test_sum_kernel_against_oracle(name, terms, batch, gpu):
    P, ctx, log_n, primes, size_p, _ = _setup(name, gpu)
    n, ql = 1 << log_n, len(primes)
    op1, op2, ref = _pool(name)
    d1 = P.to_device(op1[:batch, :terms], gpu)
    d2 = P.to_device(op2[:batch, :terms], gpu)
    keep1, keep2 = d1.clone(), d2.clone()
    r01, r2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    ctx.tensor_prod_2x2_sum_batched(d1, d2, r01, r2, ql, terms, batch)
    g01, g2 = P.to_host(r01), P.to_host(r2)
    for g in range(batch):
        _first_diff(g01[g], ref[g][terms][:2], f"{name} terms={terms} batch={batch} group {g} (c0, c1)")
        _first_diff(g2[g], ref[g][terms][2], f"{name} terms={terms} batch={batch} group {g} c2")
    import torch
    assert torch.equal(d1, keep1) and torch.equal(d2, keep2), "the summed tensor product wrote to an operand"
    del ctx, d1, d2, r01, r2, keep1, keep2
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B: one term is the batched tensor product
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A_CONFIGS)
def test_one_term_equals_the_batched_tensor_product(name, gpu):
    import torch
    P, ctx, log_n, primes, size_p, _ = _setup(name, gpu)
    n, batch, ql = 1 << log_n, 3, len(primes)
    rng = rng_for(9200 + A_CONFIGS.index(name))
    d1 = P.to_device(_operands(rng, primes[:ql], batch, 1, n), gpu)
    d2 = P.to_device(_operands(rng, primes[:ql], batch, 1, n), gpu)
    r01, r2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    w01, w2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    ctx.tensor_prod_2x2_sum_batched(d1, d2, r01, r2, ql, 1, batch)
    ctx.tensor_prod_2x2_batched(d1[:, 0].contiguous(), d2[:, 0].contiguous(), w01, w2, ql, batch)
    assert torch.equal(r01, w01) and torch.equal(r2, w2), f"{name}: terms == 1 differs from pha_tensor_prod_2x2_batched"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C: strides
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hyb12_a2", "p61_a2"])
def test_shared_operand_and_views_with_gaps(name, gpu):
    import torch
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 3, 5
    ct = 2 * ql * n
    rng = rng_for(9300 + A_CONFIGS.index(name))
    op1 = _operands(rng, primes[:ql], batch, terms, n)
    vec = _operands(rng, primes[:ql], 1, terms, n)[0]                 # [terms][2][L][N], shared by all groups
    d1, dv = P.to_device(op1, gpu), P.to_device(vec, gpu)
    drep = dv[None].expand(batch, terms, 2, ql, n).contiguous()
    want01, want2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    ctx.tensor_prod_2x2_sum_batched(d1, drep, want01, want2, ql, terms, batch)
    oc = oracle_ctx(name)
    for g in range(batch):
        ref = _oracle_sum(oc, op1[g], vec, ql)
        _first_diff(P.to_host(want01[g]), ref[:2], f"{name} replicated operand 2, group {g} (c0, c1)")
        _first_diff(P.to_host(want2[g]), ref[2], f"{name} replicated operand 2, group {g} c2")
    # batch stride 0, through the dense default (op2 one dimension short) and through explicit strides
    for strides in (None, (ct, terms * ct, ct, 0)):
        r01, r2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
        ctx.tensor_prod_2x2_sum_batched(d1, dv, r01, r2, ql, terms, batch, strides=strides)
        assert torch.equal(r01, want01) and torch.equal(r2, want2), f"{name}: shared operand 2 (strides={strides}) differs"
    # views with gaps: ciphertext (g, k) at off + g * bs + k * ts of a poisoned buffer, different geometry for the two operands
    views = []
    for src, off, gap_t, gap_b in ((d1, 6, 2 * n + 10, 14), (drep, 2 * n, 4, 2 * ct + 2)):
        ts = ct + gap_t
        bs = terms * ts + gap_b
        big = _poisoned((off + batch * bs + 8,), gpu)
        for g in range(batch):
            for k in range(terms):
                at = off + g * bs + k * ts
                big[at:at + ct] = src[g, k].reshape(-1)
        views.append((big, big[off:], ts, bs))
    (big1, v1, ts1, bs1), (big2, v2, ts2, bs2) = views
    keep1, keep2 = big1.clone(), big2.clone()
    r01, r2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    ctx.tensor_prod_2x2_sum_batched(v1, v2, r01, r2, ql, terms, batch, strides=(ts1, bs1, ts2, bs2))
    assert torch.equal(r01, want01) and torch.equal(r2, want2), f"{name}: operands with gaps differ from the dense call"
    assert torch.equal(big1, keep1) and torch.equal(big2, keep2)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: the whole operations against the composition of existing entries, on the device (and F, see the module docstring)
# ------------------------------------------------------------------------------------------------------------------------------
D_CASES = [("hyb13_a3", O.CKKS), ("hyb14_a4", O.CKKS), ("c2_ckks14", O.CKKS), ("hyb12_a2", O.BGV)]


@pytest.mark.parametrize("name,scheme", D_CASES)
def test_whole_operations_equal_the_composition(name, scheme, gpu):
    import torch
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu, BGV_T if scheme == O.BGV else None)
    n, batch, terms = 1 << log_n, 7, 5
    rng = rng_for(9400 + len(name) + scheme)
    evk = _keys(rng, primes, n, -(-ql // size_p))
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    d1 = P.to_device(_operands(rng, primes[:ql], batch, terms, n), gpu)
    d2 = P.to_device(_operands(rng, primes[:ql], batch, terms, n), gpu)
    keep1, keep2 = d1.clone(), d2.clone()
    s01, s2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    ctx.tensor_prod_2x2_sum_batched(d1, d2, s01, s2, ql, terms, batch)
    if scheme == O.CKKS:
        want = _poisoned((batch, 2, ql - 1, n), gpu)
        ctx.keyswitch_rescale_batched(ql, s01, s2, batch, rlk.public_keys_ptr, want)
        for chunk in (1, 3, 0):
            dst = _poisoned((batch, 2, ql - 1, n), gpu)
            ctx.inner_product_relin_rescale_batched(ql, d1, d2, terms, batch, rlk.public_keys_ptr, dst, chunk=chunk)
            if not torch.equal(dst, want):
                _first_diff(P.to_host(dst), P.to_host(want), f"{name} inner_product_relin_rescale_batched chunk={chunk}")
    want = s01.clone()
    ctx.keyswitch_inplace_batched(ql, want, s2, batch, rlk.public_keys_ptr, scheme)
    for chunk in (1, 3, 0):
        dst = _poisoned((batch, 2, ql, n), gpu)
        ctx.inner_product_relin_batched(ql, d1, d2, terms, batch, rlk.public_keys_ptr, scheme, dst, chunk=chunk)
        if not torch.equal(dst, want):
            _first_diff(P.to_host(dst), P.to_host(want), f"{name} inner_product_relin_batched scheme={scheme} chunk={chunk}")
    assert torch.equal(d1, keep1) and torch.equal(d2, keep2), "a whole operation wrote to an operand"
    del ctx, rlk
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# E: the whole operations against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scheme", D_CASES)
def test_whole_operations_against_oracle(name, scheme, gpu):
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu, BGV_T if scheme == O.BGV else None)
    n, batch, terms = 1 << log_n, 3, 4
    rng = rng_for(9500 + len(name) + scheme)
    oc = oracle_ctx(name)
    tool = O.Tool(oc, ql)
    if scheme == O.BGV:
        tool.set_plain_modulus(BGV_T)
    evk = _keys(rng, primes, n, -(-ql // size_p))
    keys = [evk[i] for i in range(tool.beta)]
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    op1, op2 = _operands(rng, primes[:ql], batch, terms, n), _operands(rng, primes[:ql], batch, terms, n)
    d1, d2 = P.to_device(op1, gpu), P.to_device(op2, gpu)
    dst = _poisoned((batch, 2, ql, n), gpu)
    ctx.inner_product_relin_batched(ql, d1, d2, terms, batch, rlk.public_keys_ptr, scheme, dst)
    got = P.to_host(dst)
    if scheme == O.CKKS:
        dres = _poisoned((batch, 2, ql - 1, n), gpu)
        ctx.inner_product_relin_rescale_batched(ql, d1, d2, terms, batch, rlk.public_keys_ptr, dres)
        gres = P.to_host(dres)
    for g in range(batch):
        s = _oracle_sum(oc, op1[g], op2[g], ql)
        ref = tool.keyswitch_inplace(s[:2], s[2], keys, scheme)
        _first_diff(got[g], ref, f"{name} inner_product_relin_batched scheme={scheme} group {g}")
        if scheme == O.CKKS:
            _first_diff(gres[g], tool.rescale_ntt(ref, 2), f"{name} inner_product_relin_rescale_batched group {g}")
    del ctx, rlk
    _release()


def test_whole_operation_c3(gpu):
    """c3_ckks16, 45 limbs: 8 terms, 8 groups sharing operand 2 (rows of a matrix against one vector).  The whole batch against the
    device composition; the first and the last group against the oracle (two oracle key switches)."""
    import torch
    name, scheme = "c3_ckks16", O.CKKS
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 8, 8
    rng = rng_for(9600)
    oc = oracle_ctx(name)
    tool = O.Tool(oc, ql)
    evk = _keys(rng, primes, n, ql // size_p)
    keys = [evk[i] for i in range(tool.beta)]
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    # operands generated on the device (the host would hold 3 GB of them); the two groups the oracle sees are copied back
    gen = torch.Generator(device=gpu)
    gen.manual_seed(9600)
    d1 = torch.empty((batch, terms, 2, ql, n), dtype=torch.int64, device=gpu)
    dv = torch.empty((terms, 2, ql, n), dtype=torch.int64, device=gpu)
    for j in range(ql):
        d1[:, :, :, j] = torch.randint(0, int(primes[j]), (batch, terms, 2, n), dtype=torch.int64, device=gpu, generator=gen)
        dv[:, :, j] = torch.randint(0, int(primes[j]), (terms, 2, n), dtype=torch.int64, device=gpu, generator=gen)
    keep1, keepv = d1.clone(), dv.clone()
    dres = _poisoned((batch, 2, ql - 1, n), gpu)
    ctx.inner_product_relin_rescale_batched(ql, d1, dv, terms, batch, rlk.public_keys_ptr, dres)
    dks = _poisoned((batch, 2, ql, n), gpu)
    ctx.inner_product_relin_batched(ql, d1, dv, terms, batch, rlk.public_keys_ptr, scheme, dks)
    assert torch.equal(d1, keep1) and torch.equal(dv, keepv), "a whole operation wrote to an operand"
    del keep1, keepv
    s01, s2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    ctx.tensor_prod_2x2_sum_batched(d1, dv, s01, s2, ql, terms, batch)
    want = _poisoned((batch, 2, ql - 1, n), gpu)
    ctx.keyswitch_rescale_batched(ql, s01, s2, batch, rlk.public_keys_ptr, want)
    if not torch.equal(dres, want):
        _first_diff(P.to_host(dres), P.to_host(want), "c3 inner_product_relin_rescale_batched vs the device composition")
    ctx.keyswitch_inplace_batched(ql, s01, s2, batch, rlk.public_keys_ptr, scheme)
    if not torch.equal(dks, s01):
        _first_diff(P.to_host(dks), P.to_host(s01), "c3 inner_product_relin_batched vs the device composition")
    del s01, s2, want
    vec = P.to_host(dv)
    for g in (0, batch - 1):
        s = _oracle_sum(oc, P.to_host(d1[g]), vec, ql)
        ref = tool.keyswitch_inplace(s[:2], s[2], keys, scheme)
        _first_diff(P.to_host(dks[g]), ref, f"c3 inner_product_relin_batched group {g} vs the oracle")
        _first_diff(P.to_host(dres[g]), tool.rescale_ntt(ref, 2), f"c3 inner_product_relin_rescale_batched group {g} vs the oracle")
    del ctx, rlk, d1, dv, dres, dks
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# G: refusals
# ------------------------------------------------------------------------------------------------------------------------------
def _refused(fn, needle, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert needle in str(e.value), f"message {str(e.value)!r} does not name {needle!r}"


def test_refusals_leave_everything_untouched(gpu):
    import torch
    name = "hyb12_a2"
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 2, 3
    ct = 2 * ql * n
    rng = rng_for(9700)
    rlk = P.PhantomRelinKey.from_numpy(_keys(rng, primes, n, ql // size_p), gpu)
    d1 = P.to_device(_operands(rng, primes[:ql], batch, terms, n), gpu)
    d2 = P.to_device(_operands(rng, primes[:ql], batch, terms, n), gpu)
    keep1, keep2 = d1.clone(), d2.clone()
    r01, r2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    dres, dks = _poisoned((batch, 2, ql - 1, n), gpu), _poisoned((batch, 2, ql, n), gpu)
    dense = (ct, terms * ct, ct, terms * ct)
    f = ctx.tensor_prod_2x2_sum_batched
    # null buffers
    for args in ((None, d2, r01, r2), (d1, None, r01, r2), (d1, d2, None, r2), (d1, d2, r01, None)):
        _refused(f, "null", *args, ql, terms, batch, strides=dense)
    # no terms, limb counts outside the table
    _refused(f, "terms", d1, d2, r01, r2, ql, 0, batch, strides=dense)
    _refused(f, "coeff_mod_size out of range", d1, d2, r01, r2, 0, terms, batch, strides=dense)
    _refused(f, "coeff_mod_size out of range", d1, d2, r01, r2, len(primes) + 1, terms, batch, strides=dense)
    # odd strides, one at a time
    for i in range(4):
        odd = list(dense)
        odd[i] += 1
        _refused(f, "even", d1, d2, r01, r2, ql, terms, batch, strides=tuple(odd))
    # terms that overlap
    _refused(f, "term stride", d1, d2, r01, r2, ql, terms, batch, strides=(ct - 2, terms * ct, ct, terms * ct))
    _refused(f, "term stride", d1, d2, r01, r2, ql, terms, batch, strides=(ct, terms * ct, 0, terms * ct))
    # outputs on top of an operand ciphertext: the first of operand 1, the last of operand 2
    _refused(f, "overlap", d1, d2, d1.view(-1)[:batch * ct].view(batch, 2, ql, n), r2, ql, terms, batch)
    last = d2.view(-1)[d2.numel() - batch * ql * n:].view(batch, ql, n)
    _refused(f, "overlap", d1, d2, r01, last, ql, terms, batch)
    # the whole operations: their own refusals and the shared ones
    g, h = ctx.inner_product_relin_rescale_batched, ctx.inner_product_relin_batched
    _refused(g, "overlap", ql, d1, d2, terms, batch, rlk.public_keys_ptr, d1.view(-1)[:batch * 2 * (ql - 1) * n].view(batch, 2, ql - 1, n))
    _refused(h, "overlap", ql, d1, d2, terms, batch, rlk.public_keys_ptr, O.CKKS, d2.view(-1)[:batch * ct].view(batch, 2, ql, n))
    _refused(h, "bfv", ql, d1, d2, terms, batch, rlk.public_keys_ptr, O.BFV, dks)
    _refused(h, "plain modulus", ql, d1, d2, terms, batch, rlk.public_keys_ptr, O.BGV, dks)
    _refused(g, "terms", ql, d1, d2, 0, batch, rlk.public_keys_ptr, dres)
    _refused(h, "terms", ql, d1, d2, 0, batch, rlk.public_keys_ptr, O.CKKS, dks)
    _refused(g, "even", ql, d1, d2, terms, batch, rlk.public_keys_ptr, dres, strides=(ct, terms * ct + 1, ct, terms * ct))
    _refused(h, "term stride", ql, d1, d2, terms, batch, rlk.public_keys_ptr, O.CKKS, dks, strides=(ct, terms * ct, ct - 2, terms * ct))
    _refused(g, "size_Ql out of range", len(primes), d1, d2, terms, batch, rlk.public_keys_ptr, dres, strides=dense)
    _refused(g, "last remaining modulus", 1, d1, d2, terms, batch, rlk.public_keys_ptr, dres, strides=dense)
    _refused(g, "null", ql, d1, d2, terms, batch, None, dres)
    _refused(h, "null", ql, d1, d2, terms, batch, rlk.public_keys_ptr, O.CKKS, None)
    # an empty batch does nothing
    f(d1, d2, r01, r2, ql, terms, 0, strides=dense)
    g(ql, d1, d2, terms, 0, rlk.public_keys_ptr, dres, strides=dense)
    h(ql, d1, d2, terms, 0, rlk.public_keys_ptr, O.CKKS, dks, strides=dense)
    torch.cuda.synchronize()
    for out in (r01, r2, dres, dks):
        assert bool((out == POISON).all()), "a refused (or empty) call wrote to its output"
    assert torch.equal(d1, keep1) and torch.equal(d2, keep2), "a refused call wrote to an operand"
    # and the same arguments without the defect go through, leaving the operands as they were
    f(d1, d2, r01, r2, ql, terms, batch, strides=dense)
    g(ql, d1, d2, terms, batch, rlk.public_keys_ptr, dres)
    h(ql, d1, d2, terms, batch, rlk.public_keys_ptr, O.CKKS, dks)
    torch.cuda.synchronize()
    for out in (r01, r2, dres, dks):
        assert not bool((out == POISON).any())
    assert torch.equal(d1, keep1) and torch.equal(d2, keep2), "a successful call wrote to an operand"
    del ctx, rlk
    _release()


def _refused_with(fn, text, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == text, f"refused with {str(e.value)!r}, not with {text!r}"


def test_every_refusal_and_their_order(gpu):
    """The refusals of the four entries that test_refusals_leave_everything_untouched does not reach, the whole message compared, and
    for several defects in one call the one that is reported: the term count, the batch, odd strides, alignment of the operands,
    overlapping terms, and only then the output (its alignment, then what it lies on).  Nothing is launched."""
    import torch
    name = "hyb12_a2"
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    _, bgv, *_ = _setup(name, gpu, plain_t=BGV_T)
    n, batch, terms = 1 << log_n, 2, 3
    ct = 2 * ql * n
    rng = rng_for(9750)
    keys = P.PhantomRelinKey.from_numpy(_keys(rng, primes, n, ql // size_p), gpu)
    kp = keys.public_keys_ptr
    d1 = P.to_device(_operands(rng, primes[:ql], batch, terms, n, blocks=False), gpu)
    d2 = P.to_device(_operands(rng, primes[:ql], batch, terms, n, blocks=False), gpu)
    keep1, keep2 = d1.clone(), d2.clone()
    r2 = _poisoned((batch, ql, n), gpu)
    dense = (ct, terms * ct, ct, terms * ct)
    even, aligned = "strides must be even (16-byte loads)", "buffers must be 16-byte aligned"
    crowded = "term stride below 2 * L * N: the terms of an operand overlap"
    entries = {   # call(op1, op2, terms, batch, strides, out), the output and how the overlap refusal names it
        "sum": (lambda a, b, t, B, st, out: ctx.tensor_prod_2x2_sum_batched(a, b, out, r2, ql, t, B, strides=st),
                _poisoned((batch, 2, ql, n), gpu), "res01"),
        "rescale": (lambda a, b, t, B, st, out: ctx.inner_product_relin_rescale_batched(ql, a, b, t, B, kp, out, strides=st),
                    _poisoned((batch, 2, ql - 1, n), gpu), "dst"),
        "relin": (lambda a, b, t, B, st, out: ctx.inner_product_relin_batched(ql, a, b, t, B, kp, O.CKKS, out, strides=st),
                  _poisoned((batch, 2, ql, n), gpu), "dst"),
        "mod_switch": (lambda a, b, t, B, st, out: bgv.inner_product_relin_mod_switch_batched(ql, a, b, t, B, kp, out, strides=st),
                       _poisoned((batch, 2, ql - 1, n), gpu), "dst"),
    }
    off1, off2 = d1.view(-1)[1:], d2.view(-1)[1:]                     # 8 bytes past a 16-byte boundary
    for call, out, out_name in entries.values():
        off_out = out.view(-1)[1:]
        _refused_with(call, "terms out of range", d1, d2, 1 << 32, batch, dense, out)
        _refused_with(call, "batch out of range", d1, d2, terms, 65536, dense, out)
        _refused_with(call, aligned, off1, d2, terms, batch, dense, out)
        _refused_with(call, aligned, d1, off2, terms, batch, dense, out)
        _refused_with(call, aligned, d1, d2, terms, batch, dense, off_out)
        _refused_with(call, crowded, d1, d2, terms, batch, (ct - 2, terms * ct, ct, terms * ct), out)
        _refused_with(call, crowded, d1, d2, terms, batch, (ct, terms * ct, 0, terms * ct), out)
        _refused_with(call, out_name + " must not overlap an operand ciphertext", d1, d2, terms, batch, dense,
                      d2.view(-1)[d2.numel() - out.numel():])
        # every stride and alignment defect at once, then with the winner taken away each time
        _refused_with(call, even, off1, off2, terms, batch, (ct - 1, terms * ct + 1, 1, 3), off_out)
        _refused_with(call, aligned, off1, off2, terms, batch, (ct - 2, terms * ct, 0, 2), off_out)
        _refused_with(call, crowded, d1, d2, terms, batch, (ct - 2, terms * ct, 0, 2), off_out)
        _refused_with(call, aligned, d1, d2, terms, batch, dense, d1.view(-1)[1:1 + out.numel()])   # misaligned AND on operand 1
        # the term count and the batch come before the layout
        _refused_with(call, "terms must be at least 1", off1, d2, 0, 65536, (ct + 1, terms * ct, ct, terms * ct), out)
        _refused_with(call, "terms out of range", off1, d2, 1 << 32, 65536, (ct + 1, terms * ct, ct, terms * ct), out)
        _refused_with(call, "batch out of range", off1, d2, terms, 65536, (ct + 1, terms * ct, ct, terms * ct), out)
    # res2 of the summed tensor product: misaligned, and on top of operand 1
    f, res01 = ctx.tensor_prod_2x2_sum_batched, entries["sum"][1]
    _refused_with(f, aligned, d1, d2, res01, r2.view(-1)[1:], ql, terms, batch, strides=dense)
    _refused_with(f, "res2 must not overlap an operand ciphertext", d1, d2, res01, d1.view(-1)[ct:ct + batch * ql * n], ql, terms, batch, strides=dense)
    # what the whole operations check themselves, before any of the above
    g, h = ctx.inner_product_relin_rescale_batched, ctx.inner_product_relin_batched
    dres, dks = entries["rescale"][1], entries["relin"][1]
    _refused_with(h, "unsupported scheme", ql, d1, d2, terms, batch, kp, 99, dks)
    _refused_with(h, "size_Ql out of range", 0, d1, d2, terms, batch, kp, O.CKKS, dks, strides=dense)
    _refused_with(h, "size_Ql out of range", len(primes), d1, d2, terms, batch, kp, O.CKKS, dks, strides=dense)
    _refused_with(g, "size_Ql out of range", 0, d1, d2, terms, batch, kp, dres, strides=dense)
    _refused_with(g, "cannot rescale the last remaining modulus", 1, off1, d2, 0, batch, kp, dres, strides=(1, 1, 1, 1))
    _refused_with(bgv.inner_product_relin_mod_switch_batched, "cannot switch down the last remaining modulus", 1, off1, d2, 0, batch, kp,
                  entries["mod_switch"][1], strides=(1, 1, 1, 1))
    _refused_with(ctx.inner_product_relin_mod_switch_batched, "bgv needs a plain modulus (pha_context_set_plain_modulus)", ql, off1, d2, 0,
                  batch, kp, entries["mod_switch"][1], strides=(1, 1, 1, 1))
    _refused_with(h, "bgv needs a plain modulus (pha_context_set_plain_modulus)", ql, off1, d2, 0, batch, kp, O.BGV, dks, strides=(1, 1, 1, 1))
    log_n2, primes2, size_p2 = primes_of("c2_ntt14")
    assert size_p2 == 0
    nop = P.PhantomContext(log_n2, list(primes2), 0, device=gpu)
    _refused_with(nop.inner_product_relin_rescale_batched, "context has no special modulus", 4, d1, d2, 0, batch, kp, dres, strides=(1, 1, 1, 1))
    _refused_with(nop.inner_product_relin_batched, "context has no special modulus", 4, d1, d2, 0, batch, kp, O.CKKS, dks, strides=(1, 1, 1, 1))
    torch.cuda.synchronize()
    for _, out, _ in entries.values():
        assert bool((out == POISON).all()), "a refused call wrote to its output"
    assert bool((r2 == POISON).all()) and torch.equal(d1, keep1) and torch.equal(d2, keep2), "a refused call wrote to a buffer"
    del ctx, bgv, nop, keys
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# H: strict mode
# ------------------------------------------------------------------------------------------------------------------------------
def test_strict_mode_names_the_operand(gpu):
    import torch
    name = "hyb12_a2"
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 3, 4
    ct = 2 * ql * n
    rng = rng_for(9800)
    rlk = P.PhantomRelinKey.from_numpy(_keys(rng, primes, n, ql // size_p), gpu)
    d1 = P.to_device(_operands(rng, primes[:ql], batch, terms, n), gpu)
    d2 = P.to_device(_operands(rng, primes[:ql], batch, terms, n), gpu)
    dv = d2[0].contiguous()                                            # a shared operand 2
    # the same operands as views with gaps (the strided branch of the check)
    ts, bs = ct + 2 * n, terms * (ct + 2 * n) + 6
    big = []
    for src in (d1, d2):
        b = torch.zeros((batch * bs,), dtype=torch.int64, device=gpu)
        for g in range(batch):
            for k in range(terms):
                b[g * bs + k * ts:g * bs + k * ts + ct] = src[g, k].reshape(-1)
        big.append(b)
    r01, r2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
    dres, dks = _poisoned((batch, 2, ql - 1, n), gpu), _poisoned((batch, 2, ql, n), gpu)
    g_bad, k_bad, poly, limb, idx = 2, 3, 1, 4, 777                    # the last term of the last group
    was = P.set_strict(True)
    try:
        ctx.tensor_prod_2x2_sum_batched(d1, d2, r01, r2, ql, terms, batch)                 # canonical operands pass
        ctx.tensor_prod_2x2_sum_batched(big[0], big[1], r01, r2, ql, terms, batch, strides=(ts, bs, ts, bs))
        ctx.inner_product_relin_rescale_batched(ql, d1, dv, terms, batch, rlk.public_keys_ptr, dres)
        r01.fill_(POISON), r2.fill_(POISON), dres.fill_(POISON)
        for which, (dense, view) in enumerate(((d1, big[0]), (d2, big[1]))):
            named = f"tensor_prod_2x2_sum operand{which + 1}"
            good = int(dense[g_bad, k_bad, poly, limb, idx])
            at = g_bad * bs + k_bad * ts + (poly * ql + limb) * n + idx
            dense[g_bad, k_bad, poly, limb, idx] = int(primes[limb])   # q itself: the smallest non-canonical word
            view[at] = int(primes[limb])
            _refused(ctx.tensor_prod_2x2_sum_batched, named, d1, d2, r01, r2, ql, terms, batch)
            _refused(ctx.tensor_prod_2x2_sum_batched, named, big[0], big[1], r01, r2, ql, terms, batch, strides=(ts, bs, ts, bs))
            _refused(ctx.inner_product_relin_rescale_batched, named, ql, d1, d2, terms, batch, rlk.public_keys_ptr, dres)
            _refused(ctx.inner_product_relin_batched, named, ql, d1, d2, terms, batch, rlk.public_keys_ptr, O.CKKS, dks)
            torch.cuda.synchronize()
            for out in (r01, r2, dres, dks):
                assert bool((out == POISON).all()), "a call refused in strict mode wrote to its output"
            P.set_strict(False)                                        # accepted with strict mode off
            ctx.tensor_prod_2x2_sum_batched(d1, d2, r01, r2, ql, terms, batch)
            torch.cuda.synchronize()
            assert not bool((r01 == POISON).any())
            r01.fill_(POISON), r2.fill_(POISON)
            P.set_strict(True)
            dense[g_bad, k_bad, poly, limb, idx] = good
            view[at] = good
        # a bad word in a shared operand 2 is found although only one copy of it exists
        dv[k_bad, poly, limb, idx] = int(primes[limb])
        _refused(ctx.tensor_prod_2x2_sum_batched, "tensor_prod_2x2_sum operand2", d1, dv, r01, r2, ql, terms, batch)
    finally:
        P.set_strict(was)
    del ctx, rlk
    _release()
