"""The three sum kernels on a chain with one limb of every width at which they change their behaviour (util.CONFIGS["ladder12"]:
50, 49, 48, 47, 46, 45, 44, 42, 41, 51, 55, 59, 60, 60 bits of data, two 61-bit special primes), word for word against the oracle.

The kernels pick a flush period per limb from the bit length of its modulus:
  tensor_sum_kernel (pha_poly.hip)   FP64 limbs 2 / 4 / 8 / 17 / 35 / 71 / 143 terms at 50 .. 44 bits, integer limbs 16 / 64 / 256 at
                                     61 / 60 / 59 bits;
  plain_sum_kernel (pha_plain_sum.h) FP64 limbs 5 / 11 / 24 / 50 / 101 / 203 terms at 50 .. 45 bits, integer limbs 64 / 256 at 61 / 60.
The named sets of the other files cross 2, 71 and 16 (tensor) and 5, 101, 203 and 64 (plain) of these; an accumulator that flushes one
term late at any other width would go unnoticed there.  Here batch 1 runs at EVERY term count (1 .. 150, 1 .. 210), so no copy of the
kernels' formulas is needed and no period can be missed; batch 3 runs at T, T + 1 and 2 T + 1 of every period T <= 75.

Inputs as in test_gpu_inner_product.py / test_gpu_plain_sum.py: uniform residues and, in every term of every operand at the same
coefficient positions, blocks of q - 1, (q - 1) / 2, (q + 1) / 2 and 0, so the extreme products line up across the terms; the two
sweeps add a block of floor(sqrt(q / 2)) (_plant_root_blocks).  One run of
terms is uploaded once; a term count is a slice of it, and group g of a batch reads terms g .. g + K - 1 of it (batch stride = one
term).  Outputs are poisoned before every call, operands compared with their upload after the last one, failures name the limb and
its bit length (util.first_diff_limb).

1. pha_tensor_prod_2x2_sum_batched over every row of the table (the 61-bit primes are the special primes);
2. pha_multiply_plain_sum_batched over every row, with and without acc;
3. pha_bfv_lift_plain_batched + pha_bfv_multiply_plain_sum_batched and pha_bfv_plain_inner_product_batched over the data limbs, plain
   moduli 65537 and 2^20, terms 1, 2, 5, 6, 11, 12, 24, 25, 50, 51, with and without acc, slab and chunk 0 and 1, against the loop of
   bfv_multiply_plain and add that test_gpu_bfv_plain_sum.test_sum_against_oracle compares with (util.oracle_bfv_plain_sum).
"""
import math

import numpy as np
import pytest

from test_gpu_inner_product import _oracle_sum as _tensor_oracle_sum
from test_gpu_plain_sum import _oracle_sum as _plain_oracle_sum, _poisoned, _release, _setup, _uniform, _with_acc
from util import first_diff_limb, oracle_bfv_plain_sum, oracle_ctx, rng_for

pytestmark = pytest.mark.gpu

NAME = "ladder12"
TENSOR_MAX, PLAIN_MAX = 150, 210
# the flush periods of at most 75 terms that the ladder's limbs have (module docstring), and the batch-3 counts around them
TENSOR_PERIODS = [2, 4, 8, 16, 17, 35, 64, 71]
PLAIN_PERIODS = [5, 11, 24, 50, 64]
BFV_TERMS = [1, 2, 5, 6, 11, 12, 24, 25, 50, 51]
BLOCK = 64                            # coefficients per planted block, as in the other files


def _straddle(periods):
    return sorted({c for t in periods for c in (t, t + 1, 2 * t + 1)})


def _plant_root_blocks(x, primes):
    """x [..., limb, N]: next to the four blocks of the other files, at both ends of every polynomial, a block of floor(sqrt(q / 2)).  Its
    square is just below q / 2, the largest centred residue, with the same sign in every term: the products of the other blocks are
    1 or about q / 4 modulo q, this one makes an FP64 accumulator grow twice as fast."""
    n = x.shape[-1]
    for j, q in enumerate(primes):
        for at in (4 * BLOCK, n - 5 * BLOCK):
            x[..., j, at:at + BLOCK] = math.isqrt(int(q) // 2)
    return x


def test_tensor_sum_at_every_term_count(gpu):
    import torch
    P, ctx, log_n, primes, size_p, _ = _setup(NAME, gpu)
    n, ql = 1 << log_n, len(primes)
    ct = 2 * ql * n
    oc = oracle_ctx(NAME)
    rng = rng_for(12000)
    op1, op2 = (_plant_root_blocks(_uniform(rng, primes, (TENSOR_MAX, 2), n), primes) for _ in range(2))
    b3 = _straddle(TENSOR_PERIODS)
    ref = [_tensor_oracle_sum(oc, op1, op2, ql, upto=set(range(1, TENSOR_MAX + 1)))]
    ref += [_tensor_oracle_sum(oc, op1[g:g + max(b3)], op2[g:g + max(b3)], ql, upto=set(b3)) for g in (1, 2)]
    d1, d2 = P.to_device(op1, gpu), P.to_device(op2, gpu)
    keep1, keep2 = d1.clone(), d2.clone()
    for terms in range(1, TENSOR_MAX + 1):
        for batch in (1, 3) if terms in b3 else (1,):
            r01, r2 = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, ql, n), gpu)
            ctx.tensor_prod_2x2_sum_batched(d1, d2, r01, r2, ql, terms, batch, strides=(ct, ct, ct, ct))
            g01, g2 = P.to_host(r01), P.to_host(r2)
            for g in range(batch):
                first_diff_limb(g01[g], ref[g][terms][:2], f"tensor sum terms={terms} batch={batch} group {g} (c0, c1)", primes)
                first_diff_limb(g2[g], ref[g][terms][2], f"tensor sum terms={terms} batch={batch} group {g} c2", primes)
    assert torch.equal(d1, keep1) and torch.equal(d2, keep2), "the summed tensor product wrote to an operand"
    del ctx, d1, d2, keep1, keep2
    _release()


def test_plain_sum_at_every_term_count(gpu):
    import torch
    P, ctx, log_n, primes, size_p, _ = _setup(NAME, gpu)
    n, ql = 1 << log_n, len(primes)
    ln = ql * n
    oc = oracle_ctx(NAME)
    rng = rng_for(12100)
    plain, ct = _plant_root_blocks(_uniform(rng, primes, (PLAIN_MAX,), n), primes), _plant_root_blocks(_uniform(rng, primes, (PLAIN_MAX, 2), n), primes)
    acc = _uniform(rng, primes, (3, 2), n)
    b3 = _straddle(PLAIN_PERIODS)
    ref = [_plain_oracle_sum(oc, plain, ct, ql, upto=set(range(1, PLAIN_MAX + 1)))]
    ref += [_plain_oracle_sum(oc, plain[g:g + max(b3)], ct[g:g + max(b3)], ql, upto=set(b3)) for g in (1, 2)]
    dp, dc, da = P.to_device(plain, gpu), P.to_device(ct, gpu), P.to_device(acc, gpu)
    keep = [x.clone() for x in (dp, dc, da)]
    for terms in range(1, PLAIN_MAX + 1):
        for batch in (1, 3) if terms in b3 else (1,):
            for with_acc in (False, True):
                res = _poisoned((batch, 2, ql, n), gpu)
                ctx.multiply_plain_sum_batched(dp, dc, da if with_acc else None, res, ql, terms, batch, strides=(ln, ln, 2 * ln, 2 * ln, 2 * ln))
                got = P.to_host(res)
                for g in range(batch):
                    want = _with_acc(oc, ref[g][terms], acc[g], ql) if with_acc else ref[g][terms]
                    first_diff_limb(got[g], want, f"plain sum terms={terms} batch={batch} acc={with_acc} group {g}", primes)
    assert all(torch.equal(a, b) for a, b in zip((dp, dc, da), keep)), "the sum wrote to an operand"
    del ctx, dp, dc, da, keep
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# 3: the BFV sums over the ladder's data limbs
# ------------------------------------------------------------------------------------------------------------------------------
def _plains(rng, lead, n, t):
    """[*lead][N] uniform below t, blocks of 0, (t - 1) / 2, (t + 1) / 2 and t - 1 at both ends (the two sides of the lift's threshold)"""
    m = rng.integers(0, t, tuple(lead) + (n,), dtype=np.uint64)
    for at in (0, n - 4 * BLOCK):
        for i, v in enumerate((0, (t - 1) // 2, (t + 1) // 2, t - 1)):
            m[..., at + i * BLOCK:at + (i + 1) * BLOCK] = v
    return m


@pytest.mark.parametrize("t", [65537, 1 << 20])
def test_bfv_sums_on_the_ladder(t, gpu):
    import torch
    P, ctx, log_n, primes, size_p, ql = _setup(NAME, gpu, plain_t=t)
    n, batch, kmax = 1 << log_n, 3, max(BFV_TERMS)
    pl = [int(q) for q in primes[:ql]]
    oc = oracle_ctx(NAME)
    rng = rng_for(12200 + (t & 1))
    m, ct, acc = _plains(rng, (batch, kmax), n, t), _uniform(rng, pl, (batch, kmax, 2), n), _uniform(rng, pl, (batch, 2), n)
    ref = [oracle_bfv_plain_sum(oc, m[g], ct[g], ql, t, upto=set(BFV_TERMS)) for g in range(batch)]      # never modified
    dm, dc, da = P.to_device(m, gpu), P.to_device(ct, gpu), P.to_device(acc, gpu)
    dp = _poisoned((batch, kmax, ql, n), gpu)
    ctx.bfv_lift_plain_batched(ql, dm, batch * kmax, dp)
    keep = [x.clone() for x in (dm, dc, da, dp)]
    lw, cw = ql * n, 2 * ql * n
    for terms in BFV_TERMS:
        for with_acc in (False, True):
            want = [_with_acc(oc, ref[g][terms], acc[g], ql) if with_acc else ref[g][terms] for g in range(batch)]
            for slab in (0, 1):
                for chunk in (0, 1):
                    for fn, plain, pw in ((ctx.bfv_multiply_plain_sum_batched, dp, lw), (ctx.bfv_plain_inner_product_batched, dm, n)):
                        res = _poisoned((batch, 2, ql, n), gpu)
                        fn(ql, plain, dc, da if with_acc else None, res, terms, batch, strides=(pw, kmax * pw, cw, kmax * cw, cw),
                           chunk=chunk, slab=slab)
                        got = P.to_host(res)
                        for g in range(batch):
                            first_diff_limb(got[g], want[g], f"{fn.__name__} t={t} terms={terms} acc={with_acc} slab={slab} chunk={chunk} "
                                                             f"group {g}", pl)
    assert all(torch.equal(a, b) for a, b in zip((dm, dc, da, dp), keep)), "a bfv sum wrote to an operand"
    del ctx, dm, dc, da, dp, keep
    _release()
