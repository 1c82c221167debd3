"""GPU parity of the BFV plaintext-weighted sums: pha_bfv_lift_plain_batched (the centred lift as the load of the forward transform),
pha_bfv_multiply_plain_sum_batched (one forward transform per term, one inverse per sum, acc added in the inverse's final store) and
pha_bfv_plain_inner_product_batched (the same on raw plaintexts).  Bit-exact throughout, every output word compared, every output
buffer poisoned before the call so that an unwritten word fails; t = 65537.

A. the lift against the oracle (abs_plain + nwt_forward) and against the device's two calls: counts 1, 3, 7, 8, 9 (the batched
   transform's plan switch is at 8), plaintexts uniform below t with blocks of 0, (t - 1) / 2, (t + 1) / 2, t - 1 at both ends,
   dense and with gaps between plaintexts and between outputs;
B. the sum against the oracle's loop of bfv_multiply_plain and add (acc added last): terms 1, 2, 3, 8, 33, batch 1 and 3, with and
   without acc, ciphertext blocks of q - 1, (q +- 1) / 2, 0; operands unchanged; terms == 1 without acc = pha_bfv_multiply_plain;
C. every slab in {1, 2, 5, 0} x chunk in {1, 2, 0} gives the bits of the first (terms 5, batch 3);
D. addressing: shared ct, shared plain (stride 0 through the defaults and through explicit strides), views with gaps at even offsets,
   each against the dense call, which is compared with the oracle;
E. the raw-plaintext entry against lift + sum on the device and group by group against the oracle, one plaintext row shared;
F. c4_bfv15 (N = 2^15, 30 limbs), 4 terms, 2 groups sharing ct: the batch against the device loop, first and last group against
   the oracle;
G. refusals; H. strict mode; I. the raw-plaintext entry captured into a graph on a side stream and replayed on three input sets.
"""
import functools
import gc
import math

import numpy as np
import pytest

from oracle import polymath_ext as X
from util import oracle_ctx, primes_of, rng_for

pytestmark = pytest.mark.gpu

T = 65537
POISON = -0x2152411021524111          # 0xDEADBEEFDEADBEEF as int64
BLOCK = 64
SETS = ["c1_bfv4096", "hyb12_a2", "p61_a2"]
TERMS = [1, 2, 3, 8, 33]
MAX_TERMS = 33


def _setup(name, gpu, plain_t=T):
    import phantom_fhe_amd as P
    log_n, primes, size_p = primes_of(name)
    ctx = P.PhantomContext(log_n, list(primes), size_p, device=gpu)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    ql = len(primes) - size_p
    return P, ctx, 1 << log_n, [int(q) for q in primes[:ql]], ql


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _poisoned(shape, gpu):
    import torch
    return torch.full(shape, POISON, dtype=torch.int64, device=gpu)


def _plains(rng, lead, n):
    """[*lead][N] uniform below t, blocks of 0, (t - 1) / 2, (t + 1) / 2 and t - 1 at both ends."""
    m = rng.integers(0, T, tuple(lead) + (n,), dtype=np.uint64)
    for at in (0, n - 4 * BLOCK):
        for i, v in enumerate((0, (T - 1) // 2, (T + 1) // 2, T - 1)):
            m[..., at + i * BLOCK:at + (i + 1) * BLOCK] = v
    return m


def _cts(rng, primes, lead, n):
    """[*lead][L][N] uniform, blocks of q - 1, (q - 1) / 2, (q + 1) / 2 and 0 at both ends of every limb."""
    out = np.empty(tuple(lead) + (len(primes), n), dtype=np.uint64)
    for j, q in enumerate(primes):
        out[..., j, :] = rng.integers(0, q, tuple(lead) + (n,), dtype=np.uint64)
        for at in (0, n - 4 * BLOCK):
            for i, v in enumerate((q - 1, (q - 1) // 2, (q + 1) // 2, 0)):
                out[..., j, at + i * BLOCK:at + (i + 1) * BLOCK] = v
    return out


def _oracle_lift(oc, m, primes):
    ql = len(primes)
    return oc.nwt_forward(X.abs_plain(m, (T + 1) >> 1, [q - T for q in primes]).reshape(ql, -1), ql, 0)


def _oracle_sum(oc, m, ct, ql, acc=None):
    """the loop of bfv_multiply_plain and add over the terms of one group (m [K][N], ct [K][2][L][N]), acc added last"""
    s = None
    for k in range(m.shape[0]):
        prod = oc.bfv_multiply_plain(ct[k], m[k], T)
        s = prod if s is None else np.stack([oc.add(s[p], prod[p], ql) for p in range(2)])
    if acc is not None:
        s = np.stack([oc.add(acc[p], s[p], ql) for p in range(2)])
    return s


def _first_diff(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    idx = tuple(int(v) for v in np.argwhere(got != ref)[0])
    msg = f"{what}: {int(np.count_nonzero(got != ref))} words differ, first at {idx}: got {int(got[idx])}, want {int(ref[idx])}"
    print(msg)
    raise AssertionError(msg)


def _lifted(P, ctx, ql, n, m, gpu):
    """device tensor [*lead][L][N]: the plaintexts of m [*lead][N] through entry 1"""
    lead = m.shape[:-1]
    count = int(np.prod(lead))
    out = _poisoned(tuple(lead) + (ql, n), gpu)
    ctx.bfv_lift_plain_batched(ql, P.to_device(m, gpu), count, out)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# A: the lift
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_lift_against_oracle_and_two_calls(name, gpu):
    import torch
    P, ctx, n, primes, ql = _setup(name, gpu)
    oc = oracle_ctx(name)
    ln = ql * n
    m = _plains(rng_for(11000 + SETS.index(name)), (9,), n)
    ref = np.stack([_oracle_lift(oc, m[i], primes) for i in range(9)])
    dm = P.to_device(m, gpu)
    inc = P.to_device(np.array([q - T for q in primes], dtype=np.uint64), gpu)
    two = _poisoned((9, ql, n), gpu)
    for i in range(9):
        ctx.abs_plain_rns_poly(dm[i], (T + 1) >> 1, inc, two[i], ql)
        ctx.nwt_2d_radix8_forward_inplace(two[i], ql, 0)
    _first_diff(P.to_host(two), ref, f"{name}: the two-call composition vs the oracle")
    for count in (1, 3, 7, 8, 9):
        out = _poisoned((count, ql, n), gpu)
        ctx.bfv_lift_plain_batched(ql, dm, count, out)
        _first_diff(P.to_host(out), ref[:count], f"{name} count={count} dense")
        assert torch.equal(out, two[:count])
        # gaps: plaintext i at 6 + i * (N + 10), output i at 2 N + i * (L N + 2 N + 4)
        ps, os_ = n + 10, ln + 2 * n + 4
        big_in, big_out = _poisoned((6 + count * ps,), gpu), _poisoned((2 * n + count * os_,), gpu)
        for i in range(count):
            big_in[6 + i * ps:6 + i * ps + n] = dm[i]
        keep = big_in.clone()
        ctx.bfv_lift_plain_batched(ql, big_in[6:], count, big_out[2 * n:], strides=(ps, os_))
        got = big_out[2 * n:].view(count, os_)
        assert torch.equal(got[:, :ln].reshape(count, ql, n), two[:count]), f"{name} count={count} with gaps"
        assert bool((got[:, ln:] == POISON).all()) and bool((big_out[:2 * n] == POISON).all()), "the lift wrote between its outputs"
        assert torch.equal(big_in, keep)
    assert np.array_equal(P.to_host(dm), m), "the lift wrote to the plaintexts"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B: the sum against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(name):
    """3 groups of 33 terms, an acc per group, and the oracle's running sums after every tested term count (never modified)"""
    log_n, primes, size_p = primes_of(name)
    n, ql = 1 << log_n, len(primes) - size_p
    pl = [int(q) for q in primes[:ql]]
    rng = rng_for(11100 + SETS.index(name))
    m, ct, acc = _plains(rng, (3, MAX_TERMS), n), _cts(rng, pl, (3, MAX_TERMS, 2), n), _cts(rng, pl, (3, 2), n)
    oc = oracle_ctx(name)
    ref = []
    for g in range(3):
        s, part = None, {}
        for k in range(MAX_TERMS):
            prod = oc.bfv_multiply_plain(ct[g, k], m[g, k], T)
            s = prod if s is None else np.stack([oc.add(s[p], prod[p], ql) for p in range(2)])
            if k + 1 in TERMS:
                part[k + 1] = s
        ref.append(part)
    return m, ct, acc, ref


@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("name", SETS)
def test_sum_against_oracle(name, terms, batch, with_acc, gpu):
    import torch
    P, ctx, n, primes, ql = _setup(name, gpu)
    oc = oracle_ctx(name)
    m, ct, acc, ref = _pool(name)
    dp = _lifted(P, ctx, ql, n, np.ascontiguousarray(m[:batch, :terms]), gpu)
    dc = P.to_device(np.ascontiguousarray(ct[:batch, :terms]), gpu)
    da = P.to_device(np.ascontiguousarray(acc[:batch]), gpu) if with_acc else None
    ops = [dp, dc] + ([da] if with_acc else [])
    keep = [x.clone() for x in ops]
    res = _poisoned((batch, 2, ql, n), gpu)
    ctx.bfv_multiply_plain_sum_batched(ql, dp, dc, da, res, terms, batch)
    got = P.to_host(res)
    for g in range(batch):
        want = ref[g][terms]
        if with_acc:
            want = np.stack([oc.add(acc[g, p], want[p], ql) for p in range(2)])
        _first_diff(got[g], want, f"{name} terms={terms} batch={batch} acc={with_acc} group {g}")
    assert all(torch.equal(a, b) for a, b in zip(ops, keep)), "the sum wrote to an operand"
    if terms == 1 and not with_acc:
        dm = P.to_device(np.ascontiguousarray(m[:batch, 0]), gpu)
        loop = dc[:, 0].clone()
        for g in range(batch):
            ctx.bfv_multiply_plain(ql, loop[g], 2, dm[g])
        assert torch.equal(res, loop), f"{name}: terms == 1 differs from pha_bfv_multiply_plain"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C: slab and chunk invariance
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_every_slab_and_chunk_gives_the_same_bits(name, gpu):
    import torch
    P, ctx, n, primes, ql = _setup(name, gpu)
    batch, terms = 3, 5
    m, ct, acc, _ = _pool(name)
    dm = P.to_device(np.ascontiguousarray(m[:batch, :terms]), gpu)
    dp = _lifted(P, ctx, ql, n, np.ascontiguousarray(m[:batch, :terms]), gpu)
    dc = P.to_device(np.ascontiguousarray(ct[:batch, :terms]), gpu)
    da = P.to_device(np.ascontiguousarray(acc[:batch]), gpu)
    oc = oracle_ctx(name)
    first = None
    for slab in (1, 2, 5, 0):
        for chunk in (1, 2, 0):
            for fn, plain in ((ctx.bfv_multiply_plain_sum_batched, dp), (ctx.bfv_plain_inner_product_batched, dm)):
                res = _poisoned((batch, 2, ql, n), gpu)
                fn(ql, plain, dc, da, res, terms, batch, chunk=chunk, slab=slab)
                if first is None:
                    first = res
                    for g in range(batch):
                        _first_diff(P.to_host(res[g]), _oracle_sum(oc, m[g, :terms], ct[g, :terms], ql, acc[g]), f"{name} group {g}")
                assert torch.equal(res, first), f"{name}: slab={slab} chunk={chunk} {fn.__name__} differs from the first result"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: addressing
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hyb12_a2", "p61_a2"])
def test_shared_operands_and_views_with_gaps(name, gpu):
    import torch
    P, ctx, n, primes, ql = _setup(name, gpu)
    batch, terms = 3, 5
    ln = ql * n
    oc = oracle_ctx(name)
    m, ct, acc, _ = _pool(name)
    m, ct, acc = m[:batch, :terms], ct[:batch, :terms], acc[:batch]
    dp = _lifted(P, ctx, ql, n, np.ascontiguousarray(m), gpu)
    dc, da = P.to_device(np.ascontiguousarray(ct), gpu), P.to_device(np.ascontiguousarray(acc), gpu)
    f = ctx.bfv_multiply_plain_sum_batched
    dense = (ln, terms * ln, 2 * ln, terms * 2 * ln, 2 * ln)
    # the dense call against the oracle
    want_d = _poisoned((batch, 2, ql, n), gpu)
    f(ql, dp, dc, da, want_d, terms, batch, strides=dense)
    for g in range(batch):
        _first_diff(P.to_host(want_d[g]), _oracle_sum(oc, m[g], ct[g], ql, acc[g]), f"{name} dense, group {g}")
    # shared ct: replicated (dense) -> oracle, then batch stride 0 two ways, with more than one chunk too
    vec = dc[0].contiguous()
    want = _poisoned((batch, 2, ql, n), gpu)
    f(ql, dp, vec[None].expand(batch, terms, 2, ql, n).contiguous(), da, want, terms, batch)
    for g in range(batch):
        _first_diff(P.to_host(want[g]), _oracle_sum(oc, m[g], ct[0], ql, acc[g]), f"{name} replicated ct, group {g}")
    for strides, chunk in ((None, 0), ((ln, terms * ln, 2 * ln, 0, 2 * ln), 0), (None, 2)):
        res = _poisoned((batch, 2, ql, n), gpu)
        f(ql, dp, vec, da, res, terms, batch, strides=strides, chunk=chunk, slab=2)
        assert torch.equal(res, want), f"{name}: shared ct (strides={strides}, chunk={chunk}) differs"
    # shared plain
    row = dp[1].contiguous()
    want_p = _poisoned((batch, 2, ql, n), gpu)
    f(ql, row[None].expand(batch, terms, ql, n).contiguous(), dc, None, want_p, terms, batch)
    for g in range(batch):
        _first_diff(P.to_host(want_p[g]), _oracle_sum(oc, m[1], ct[g], ql), f"{name} replicated plain, group {g}")
    for strides in (None, (ln, 0, 2 * ln, terms * 2 * ln, 2 * ln)):
        res = _poisoned((batch, 2, ql, n), gpu)
        f(ql, row, dc, None, res, terms, batch, strides=strides)
        assert torch.equal(res, want_p), f"{name}: shared plain (strides={strides}) differs"
    # views with gaps, a different geometry for each operand (the ct terms are not adjacent: one transform launch per term)
    views = []
    for src, words, off, gap_t, gap_b in ((dp, ln, 6, 2 * n + 10, 14), (dc, 2 * ln, 2 * n, 4, 2 * ln + 2), (da[:, None], 2 * ln, 10, 0, 6 * n + 2)):
        k_count = src.shape[1]
        ts = words + gap_t
        bs = k_count * ts + gap_b
        big = _poisoned((off + batch * bs + 8,), gpu)
        for g in range(batch):
            for k in range(k_count):
                at = off + g * bs + k * ts
                big[at:at + words] = src[g, k].reshape(-1)
        views.append((big, big[off:], ts, bs))
    (bigp, vp_, tsp, bsp), (bigc, vc, tsc, bsc), (biga, va, _, bsa) = views
    keep = [b.clone() for b in (bigp, bigc, biga)]
    for slab in (0, 2):
        res = _poisoned((batch, 2, ql, n), gpu)
        f(ql, vp_, vc, va, res, terms, batch, strides=(tsp, bsp, tsc, bsc, bsa), slab=slab)
        assert torch.equal(res, want_d), f"{name}: operands with gaps differ from the dense call (slab={slab})"
    assert all(torch.equal(a, b) for a, b in zip((bigp, bigc, biga), keep))
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# E: the raw-plaintext entry
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_raw_plaintext_entry(name, gpu):
    import torch
    P, ctx, n, primes, ql = _setup(name, gpu)
    batch, terms = 3, 5
    ln = ql * n
    oc = oracle_ctx(name)
    m, ct, acc, _ = _pool(name)
    m, ct, acc = np.ascontiguousarray(m[:batch, :terms]), np.ascontiguousarray(ct[:batch, :terms]), np.ascontiguousarray(acc[:batch])
    dm, dc, da = P.to_device(m, gpu), P.to_device(ct, gpu), P.to_device(acc, gpu)
    keep = [x.clone() for x in (dm, dc, da)]
    for with_acc in (False, True):
        a = da if with_acc else None
        want = _poisoned((batch, 2, ql, n), gpu)
        ctx.bfv_multiply_plain_sum_batched(ql, _lifted(P, ctx, ql, n, m, gpu), dc, a, want, terms, batch)
        res = _poisoned((batch, 2, ql, n), gpu)
        ctx.bfv_plain_inner_product_batched(ql, dm, dc, a, res, terms, batch)
        assert torch.equal(res, want), f"{name} acc={with_acc}: the raw entry differs from lift + sum"
        for g in range(batch):
            _first_diff(P.to_host(res[g]), _oracle_sum(oc, m[g], ct[g], ql, acc[g] if with_acc else None), f"{name} acc={with_acc} group {g}")
    # one plaintext row shared between the groups (through the default and through explicit strides, gaps between its terms)
    row = dm[2].contiguous()
    want = _poisoned((batch, 2, ql, n), gpu)
    ctx.bfv_multiply_plain_sum_batched(ql, _lifted(P, ctx, ql, n, m[2], gpu), dc, da, want, terms, batch)
    for g in range(batch):
        _first_diff(P.to_host(want[g]), _oracle_sum(oc, m[2], ct[g], ql, acc[g]), f"{name} shared row, group {g}")
    res = _poisoned((batch, 2, ql, n), gpu)
    ctx.bfv_plain_inner_product_batched(ql, row, dc, da, res, terms, batch, chunk=2, slab=2)
    assert torch.equal(res, want), f"{name}: shared raw plaintext row differs"
    gap = _poisoned((terms * (n + 6),), gpu)
    for k in range(terms):
        gap[k * (n + 6):k * (n + 6) + n] = row[k]
    res = _poisoned((batch, 2, ql, n), gpu)
    ctx.bfv_plain_inner_product_batched(ql, gap, dc, da, res, terms, batch, strides=(n + 6, 0, 2 * ln, terms * 2 * ln, 2 * ln))
    assert torch.equal(res, want), f"{name}: shared raw plaintext row with gaps differs"
    assert all(torch.equal(a, b) for a, b in zip((dm, dc, da), keep)), "the raw entry wrote to an operand"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# F: the large shape
# ------------------------------------------------------------------------------------------------------------------------------
def test_c4_bfv15(gpu):
    """N = 2^15, 30 limbs: 4 terms, 2 groups sharing ct.  The batch against the device loop of pha_bfv_multiply_plain + add; the first
    and the last group against the oracle."""
    import torch
    name = "c4_bfv15"
    P, ctx, n, primes, ql = _setup(name, gpu)
    batch, terms = 2, 4
    oc = oracle_ctx(name)
    rng = rng_for(11500)
    m, ct, acc = _plains(rng, (batch, terms), n), _cts(rng, primes, (terms, 2), n), _cts(rng, primes, (batch, 2), n)
    dm, dc, da = P.to_device(m, gpu), P.to_device(ct, gpu), P.to_device(acc, gpu)
    keep = [x.clone() for x in (dm, dc, da)]
    res = _poisoned((batch, 2, ql, n), gpu)
    ctx.bfv_plain_inner_product_batched(ql, dm, dc, da, res, terms, batch)
    res2 = _poisoned((batch, 2, ql, n), gpu)
    ctx.bfv_multiply_plain_sum_batched(ql, _lifted(P, ctx, ql, n, m, gpu), dc, da, res2, terms, batch, slab=3)
    assert all(torch.equal(a, b) for a, b in zip((dm, dc, da), keep)), "the sum wrote to an operand"
    loop = da.clone()
    for g in range(batch):
        for k in range(terms):
            prod = dc[k].clone()
            ctx.bfv_multiply_plain(ql, prod, 2, dm[g, k])
            for p in range(2):
                ctx.add_rns_poly(loop[g, p], prod[p], loop[g, p], ql)
    if not torch.equal(res, loop):
        _first_diff(P.to_host(res), P.to_host(loop), "c4 raw entry vs the device loop")
    assert torch.equal(res2, loop), "c4 NTT-form entry vs the device loop"
    for g in (0, batch - 1):
        _first_diff(P.to_host(res[g]), _oracle_sum(oc, m[g], ct, ql, acc[g]), f"c4 group {g} vs the oracle")
    del ctx
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
    import phantom_fhe_amd as P
    name = "hyb12_a2"
    _, ctx, n, primes, ql = _setup(name, gpu)
    batch, terms = 2, 3
    ln = ql * n
    rng = rng_for(11600)
    m = _plains(rng, (batch, terms), n)
    dm = P.to_device(m, gpu)
    dp = _lifted(P, ctx, ql, n, m, gpu)
    dc = P.to_device(_cts(rng, primes, (batch, terms, 2), n), gpu)
    da = P.to_device(_cts(rng, primes, (batch, 2), n), gpu)
    keep = [x.clone() for x in (dm, dp, dc, da)]
    res, lifted = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch * terms, ql, n), gpu)
    dense = (ln, terms * ln, 2 * ln, terms * 2 * ln, 2 * ln)
    dense_raw = (n, terms * n, 2 * ln, terms * 2 * ln, 2 * ln)
    lift, f, h = ctx.bfv_lift_plain_batched, ctx.bfv_multiply_plain_sum_batched, ctx.bfv_plain_inner_product_batched
    cases = ((f, dp, dense), (h, dm, dense_raw))
    count = batch * terms
    # null required pointers (acc may be null)
    _refused(lift, "null", ql, None, count, lifted)
    _refused(lift, "null", ql, dm, count, None)
    for fn, pl, st in cases:
        for args in ((None, dc, da, res), (pl, None, da, res), (pl, dc, da, None)):
            _refused(fn, "null", ql, *args, terms, batch, strides=st)
        # no terms; levels outside 1..|Q|
        _refused(fn, "terms", ql, pl, dc, da, res, 0, batch, strides=st)
        for bad_ql in (0, ql + 1):
            _refused(fn, "RNSBase is invalid", bad_ql, pl, dc, da, res, terms, batch, strides=st)
        # odd strides, one at a time
        for i in range(5):
            odd = list(st)
            odd[i] += 1
            _refused(fn, "even", ql, pl, dc, da, res, terms, batch, strides=tuple(odd))
        # terms that overlap
        _refused(fn, "plain term stride", ql, pl, dc, da, res, terms, batch, strides=(st[0] - 2,) + st[1:])
        _refused(fn, "ct term stride", ql, pl, dc, da, res, terms, batch, strides=st[:2] + (2 * ln - 2,) + st[3:])
        # forbidden overlaps: res on the last ciphertext, on acc itself, on acc shifted by one polynomial
        flat_c = dc.view(-1)
        _refused(fn, "overlap", ql, pl, dc, da, flat_c[flat_c.numel() - batch * 2 * ln:].view(batch, 2, ql, n), terms, batch)
        _refused(fn, "overlap acc", ql, pl, dc, da, da, terms, batch)
        wide = torch.zeros((batch * 2 * ln + ln,), dtype=torch.int64, device=gpu)
        _refused(fn, "overlap acc", ql, pl, dc, wide, wide[ln:].view(batch, 2, ql, n), terms, batch)
        assert not bool(wide.any())
    _refused(f, "plaintext", ql, dp, dc, da, dp.view(-1)[:batch * 2 * ln].view(batch, 2, ql, n), terms, batch)
    both = torch.zeros((batch * 2 * ln + batch * terms * n,), dtype=torch.int64, device=gpu)
    _refused(h, "plaintext", ql, both[batch * 2 * ln - 2:], dc, da, both[:batch * 2 * ln].view(batch, 2, ql, n), terms, batch, strides=dense_raw)
    for bad_ql in (0, ql + 1):
        _refused(lift, "RNSBase is invalid", bad_ql, dm, count, lifted)
    _refused(lift, "even", ql, dm, count, lifted, strides=(n + 1, ln))
    _refused(lift, "even", ql, dm, count, lifted, strides=(n, ln + 1))
    _refused(lift, "out stride", ql, dm, count, lifted, strides=(n, ln - 2))
    io = torch.zeros((count * ln + count * n,), dtype=torch.int64, device=gpu)   # the first plaintext starts on out's last two words
    _refused(lift, "overlap", ql, io[count * ln - 2:], count, io[:count * ln].view(count, ql, n))
    _refused(lift, "overlap", ql, io[ln - 2:], 1, io[:ln].view(1, ql, n))
    # no plain modulus; a plain modulus that is not below every prime of the level (c1_bfv4096 has 36-bit primes)
    _, bare, _, _, _ = _setup(name, gpu, plain_t=None)
    _refused(bare.bfv_lift_plain_batched, "plain modulus", ql, dm, count, lifted)
    _refused(bare.bfv_multiply_plain_sum_batched, "plain modulus", ql, dp, dc, da, res, terms, batch)
    _refused(bare.bfv_plain_inner_product_batched, "plain modulus", ql, dm, dc, da, res, terms, batch)
    all_primes = [int(q) for q in primes_of(name)[1]]
    big_t = min(primes) + 2                                        # above the smallest prime of the level, coprime to the chain
    while any(math.gcd(big_t, q) != 1 for q in all_primes):
        big_t += 2
    bare.set_plain_modulus(big_t)
    _refused(bare.bfv_lift_plain_batched, "t below every q_i", ql, dm, count, lifted)
    _refused(bare.bfv_multiply_plain_sum_batched, "t below every q_i", ql, dp, dc, da, res, terms, batch)
    _refused(bare.bfv_plain_inner_product_batched, "t below every q_i", ql, dm, dc, da, res, terms, batch)
    # nothing to do
    lift(ql, dm, 0, lifted)
    f(ql, dp, dc, da, res, terms, 0, strides=dense)
    h(ql, dm, dc, da, res, terms, 0, strides=dense_raw)
    torch.cuda.synchronize()
    for out in (res, lifted):
        assert bool((out == POISON).all()), "a refused (or empty) call wrote to its output"
    assert all(torch.equal(a, b) for a, b in zip((dm, dp, dc, da), keep)), "a refused call wrote to an operand"
    assert not bool(both.any()) and not bool(io.any())
    # the same arguments without the defect go through
    lift(ql, dm, count, lifted)
    assert torch.equal(lifted.view(batch, terms, ql, n), dp)
    f(ql, dp, dc, da, res, terms, batch, strides=dense)
    res2 = _poisoned((batch, 2, ql, n), gpu)
    h(ql, dm, dc, da, res2, terms, batch, strides=dense_raw)
    torch.cuda.synchronize()
    assert not bool((res == POISON).any()) and torch.equal(res, res2)
    assert all(torch.equal(a, b) for a, b in zip((dm, dp, dc, da), keep)), "a successful call wrote to an operand"
    del ctx, bare
    _release()


def _refused_with(fn, text, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == text, f"refused with {str(e.value)!r}, not with {text!r}"


def test_every_refusal_and_their_order(gpu):
    """The refusals of the three entries that test_refusals_leave_everything_untouched does not reach, the whole message compared,
    and for several defects in one call the one that is reported: the level, the term count, odd strides, alignment (of res too),
    overlapping terms of plain, of ct, and then what res lies on (plain, ct, acc).  These two entries bound neither the batch nor a
    limb count of their own.  Nothing is launched."""
    import torch
    import phantom_fhe_amd as P
    name = "hyb12_a2"
    _, ctx, n, primes, ql = _setup(name, gpu)
    batch, terms = 2, 3
    ln = ql * n
    rng = rng_for(11650)
    m = _plains(rng, (batch, terms), n)
    dm = P.to_device(m, gpu)
    dp = _lifted(P, ctx, ql, n, m, gpu)
    dc = P.to_device(_cts(rng, primes, (batch, terms, 2), n), gpu)
    da = P.to_device(_cts(rng, primes, (batch, 2), n), gpu)
    keep = [x.clone() for x in (dm, dp, dc, da)]
    res, lifted = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch * terms, ql, n), gpu)
    even, aligned = "strides must be even (16-byte loads)", "buffers must be 16-byte aligned"
    crowded_c = "ct term stride below 2 * L * N: the terms of ct overlap"
    offc, offa, off_res, words = dc.view(-1)[1:], da.view(-1)[1:], res.view(-1)[1:], res.numel()
    cases = ((ctx.bfv_multiply_plain_sum_batched, dp, ln, "plain term stride below L * N: the terms of plain overlap"),
             (ctx.bfv_plain_inner_product_batched, dm, n, "plain term stride below N: the terms of plain overlap"))
    for fn, pl, pn, crowded_p in cases:
        st = (pn, terms * pn, 2 * ln, terms * 2 * ln, 2 * ln)
        offp = pl.view(-1)[1:]                                     # 8 bytes past a 16-byte boundary
        _refused_with(fn, "terms out of range", ql, pl, dc, da, res, 1 << 32, batch, strides=st)
        for args in ((offp, dc, da, res), (pl, offc, da, res), (pl, dc, offa, res), (pl, dc, da, off_res), (pl, dc, None, off_res)):
            _refused_with(fn, aligned, ql, *args, terms, batch, strides=st)
        _refused_with(fn, crowded_p, ql, pl, dc, da, res, terms, batch, strides=(pn - 2,) + st[1:])
        _refused_with(fn, crowded_c, ql, pl, dc, da, res, terms, batch, strides=st[:2] + (2 * ln - 2,) + st[3:])
        _refused_with(fn, even, ql, pl, dc, None, res, terms, batch, strides=st[:4] + (2 * ln + 1,))   # acc's stride although there is no acc
        _refused_with(fn, "res must not overlap an operand ciphertext", ql, pl, dc, da, dc.view(-1)[dc.numel() - words:], terms, batch, strides=st)
        _refused_with(fn, "res must not overlap acc", ql, pl, dc, da, da, terms, batch, strides=st)
        # every stride and alignment defect at once, then with the winner taken away each time
        _refused_with(fn, even, ql, offp, offc, offa, off_res, terms, batch, strides=(pn - 1, 1, 2 * ln - 1, 3, 5))
        _refused_with(fn, aligned, ql, offp, offc, offa, off_res, terms, batch, strides=(pn - 2, 0, 2 * ln - 2, 2, 4))
        _refused_with(fn, aligned, ql, pl, dc, da, off_res, terms, batch, strides=(pn - 2, 0, 2 * ln - 2, 2, 4))   # res counts with the operands
        _refused_with(fn, crowded_p, ql, pl, dc, da, res, terms, batch, strides=(pn - 2, 0, 2 * ln - 2, 2, 4))
        _refused_with(fn, crowded_c, ql, pl, dc, da, res, terms, batch, strides=(pn, 0, 2 * ln - 2, 2, 4))
        # the level and the term count come before the layout; no batch is too large to be looked at
        _refused_with(fn, "RNSBase is invalid", 0, offp, dc, da, res, 0, batch, strides=(1, 1, 1, 1, 1))
        _refused_with(fn, "terms must be at least 1", ql, offp, dc, da, res, 0, 65536, strides=(pn + 1,) + st[1:])
        _refused_with(fn, "terms out of range", ql, offp, dc, da, res, 1 << 32, 65536, strides=(pn + 1,) + st[1:])
        _refused_with(fn, even, ql, offp, dc, da, res, terms, 65536, strides=(pn + 1,) + st[1:])
    f, h = cases[0][0], cases[1][0]
    _refused_with(f, "res must not overlap a plaintext operand", ql, dp, dc, da, dp.view(-1)[:words], terms, batch)
    both = torch.zeros((words + batch * terms * n,), dtype=torch.int64, device=gpu)
    _refused_with(h, "res must not overlap a plaintext operand", ql, both[words - 2:], dc, da, both[:words], terms, batch,
                  strides=(n, terms * n, 2 * ln, terms * 2 * ln, 2 * ln))
    # the lift: alignment, and the order parity, alignment, out stride, overlap
    lift, count = ctx.bfv_lift_plain_batched, batch * terms
    offm, off_lifted = dm.view(-1)[1:], lifted.view(-1)[1:]
    _refused_with(lift, aligned, ql, offm, count, lifted, strides=(n, ln))
    _refused_with(lift, aligned, ql, dm, count, off_lifted, strides=(n, ln))
    _refused_with(lift, "out stride below L * N: the lifted plaintexts overlap", ql, dm, count, lifted, strides=(n, ln - 2))
    _refused_with(lift, "out must not overlap a plaintext operand", ql, dm, count, dm.view(-1)[:2], strides=(n, ln))
    _refused_with(lift, even, ql, offm, count, off_lifted, strides=(n + 1, ln - 1))
    _refused_with(lift, aligned, ql, offm, count, off_lifted, strides=(n, ln - 2))
    _refused_with(lift, "out stride below L * N: the lifted plaintexts overlap", ql, dm, count, dm.view(-1)[:2], strides=(n, ln - 2))
    _refused_with(lift, "RNSBase is invalid", 0, offm, count, off_lifted, strides=(n + 1, ln - 1))
    torch.cuda.synchronize()
    assert bool((res == POISON).all()) and bool((lifted == POISON).all()), "a refused call wrote to its output"
    assert all(torch.equal(a, b) for a, b in zip((dm, dp, dc, da), keep)) and not bool(both.any()), "a refused call wrote to an operand"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# H: strict mode
# ------------------------------------------------------------------------------------------------------------------------------
def test_strict_mode_names_the_operand(gpu):
    import torch
    import phantom_fhe_amd as P
    name = "hyb12_a2"
    _, ctx, n, primes, ql = _setup(name, gpu)
    batch, terms = 3, 4
    rng = rng_for(11700)
    m = _plains(rng, (batch, terms), n)
    dm = P.to_device(m, gpu)
    dp = _lifted(P, ctx, ql, n, m, gpu)
    dc = P.to_device(_cts(rng, primes, (batch, terms, 2), n), gpu)
    da = P.to_device(_cts(rng, primes, (batch, 2), n), gpu)
    res, lifted = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch * terms, ql, n), gpu)
    lift, f, h = ctx.bfv_lift_plain_batched, ctx.bfv_multiply_plain_sum_batched, ctx.bfv_plain_inner_product_batched
    g_bad, limb, idx = 2, 4, 777
    q = primes[limb]
    was = P.set_strict(True)
    try:
        f(ql, dp, dc, da, res, terms, batch)                       # sound operands pass
        h(ql, dm, dc, da, res, terms, batch)
        lift(ql, dm, batch * terms, lifted)
        res.fill_(POISON), lifted.fill_(POISON)
        spots = [(dp, (g_bad, terms - 1, limb, idx), q, ((f, dp, "bfv_multiply_plain_sum plain"),)),
                 (dm, (g_bad, terms - 1, idx), T, ((h, dm, "bfv_plain_inner_product plain"),)),
                 (dc, (g_bad, terms - 1, 1, limb, idx), q, ((f, dp, "bfv_multiply_plain_sum ct"), (h, dm, "bfv_plain_inner_product ct"))),
                 (da, (g_bad, 1, limb, idx), q, ((f, dp, "bfv_multiply_plain_sum acc"), (h, dm, "bfv_plain_inner_product acc")))]
        for buf, where, bad, calls in spots:
            good = int(buf[where])
            buf[where] = bad                                       # the modulus itself: the smallest unsound word
            for fn, pl, named in calls:
                _refused(fn, named, ql, pl, dc, da, res, terms, batch)
            if buf is dm:
                _refused(lift, "bfv_lift_plain plain", ql, dm, batch * terms, lifted)
            torch.cuda.synchronize()
            assert bool((res == POISON).all()) and bool((lifted == POISON).all()), "a call refused in strict mode wrote to its output"
            P.set_strict(False)                                    # accepted with strict mode off
            for fn, pl, _ in calls:
                fn(ql, pl, dc, da, res, terms, batch)
                torch.cuda.synchronize()
                assert not bool((res == POISON).any())
                res.fill_(POISON)
            P.set_strict(True)
            buf[where] = good
        # a bad word in a shared operand is found although only one copy of it exists
        row = dm[0].clone()
        row[1, idx] = T
        _refused(h, "bfv_plain_inner_product plain", ql, row, dc, da, res, terms, batch)
        dv = dc[0].clone()
        dv[terms - 1, 1, limb, idx] = q
        _refused(f, "bfv_multiply_plain_sum ct", ql, dp, dv, da, res, terms, batch)
    finally:
        P.set_strict(was)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# I: graph capture
# ------------------------------------------------------------------------------------------------------------------------------
def test_raw_entry_replays_from_a_graph(gpu):
    import torch
    name = "hyb12_a2"
    P, ctx, n, primes, ql = _setup(name, gpu)
    batch, terms = 3, 5
    r = rng_for(11800)
    ins = [(P.to_device(_plains(r, (batch, terms), n), gpu), P.to_device(_cts(r, primes, (batch, terms, 2), n), gpu),
            P.to_device(_cts(r, primes, (batch, 2), n), gpu)) for _ in range(3)]
    want = []
    for dm, dc, da in ins:
        out = _poisoned((batch, 2, ql, n), gpu)
        ctx.bfv_plain_inner_product_batched(ql, dm, dc, da, out, terms, batch, chunk=2, slab=2)
        want.append(out)
    dm, dc, da = (x.clone() for x in ins[0])
    out = _poisoned((batch, 2, ql, n), gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctx.bfv_plain_inner_product_batched(ql, dm, dc, da, out, terms, batch, chunk=2, slab=2)    # warm-up on the capture stream
    side.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            ctx.bfv_plain_inner_product_batched(ql, dm, dc, da, out, terms, batch, chunk=2, slab=2)
    for i in (1, 2, 0):
        dm.copy_(ins[i][0])
        dc.copy_(ins[i][1])
        da.copy_(ins[i][2])
        out.fill_(POISON)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[i]), i
    del ctx, gr
    _release()
