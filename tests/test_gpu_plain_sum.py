"""GPU parity of the plaintext-weighted sum (pha_multiply_plain_sum_batched) and of the whole operation built on it
(pha_plain_inner_product_rescale_batched).  Bit-exact throughout against the oracle's multiply, add, rescale_ntt and
mod_t_divide_q_last_ntt; every output word compared, every output buffer poisoned before the call so that an unwritten word fails.

A. the kernel against the oracle (multiply per term and polynomial, summed with add, acc added last): hyb12_a2, p61_a2, c2_ckks14,
   wide_p20 over every row of the prime table (special primes included: that is where p61_a2 has its 61-bit primes); terms 1, 2, 3,
   31, 32, 33, 64, 65, 100 and, for every FP64 limb of the set (bit length b <= 50), its own flush interval T = floor((56 * 2^(52 - b)
   - 40) / 35) and T - 1, T + 1: 4, 5, 6 at p61_a2 (50 bits), 101, 102, 202, 203, 204 at wide_p20 (46 and 45 bits), 6551, 6552, 6553 at
   hyb12_a2 and c2_ckks14 (40 bits).  Batch 1 and 3, with and without acc.  In every term of every operand, at the same coefficient
   positions, blocks of q - 1, (q - 1) / 2, (q + 1) / 2 and 0, so that the largest products and the largest centred values line up
   across all terms.  Up to 100 terms the operands are dense [batch][terms]...; the longer sums read one long run of terms through
   strides, group g taking terms g .. g + K - 1 of it (6555 dense terms per group would be 70 GB at c2_ckks14), generated on the
   device and streamed back term by term for the oracle;
B. one term, no acc: the words of pha_multiply_rns_poly per polynomial;
C. res == acc (accumulate in place) against the out-of-place call;
D. addressing: shared ct, shared plain (batch stride 0, through the dense default and through explicit strides), views with gaps
   between terms and groups at even word offsets -- each against the contiguous call (itself compared with the oracle);
E. the whole operation: hyb13_a3, hyb14_a4, c2_ckks14 as ckks and hyb12_a2 as bgv (t = 65537), batch 5: chunk 1, 3 and 0 against
   the two-call composition on the device, and every group against the oracle;
F. c3_ckks16, 45 limbs, 8 terms, 2 groups sharing ct: the whole batch against the device composition, the first and the last group
   against the oracle;
G. refusals (status -1, the message, poisoned outputs untouched), bfv and size_Ql == 1 for the rescale entry, batch == 0;
H. strict mode: one word >= its modulus in plain, ct or acc is refused with that operand named;
I. the rescale entry captured into a graph and replayed.
"""
import functools
import gc

import numpy as np
import pytest

from oracle import oracle as O
from util import oracle_ctx, primes_of, rng_for

pytestmark = pytest.mark.gpu

BGV_T = 65537
POISON = -0x2152411021524111          # 0xDEADBEEFDEADBEEF as int64
TERMS = [1, 2, 3, 31, 32, 33, 64, 65, 100]
DENSE_MAX = 100                       # longer sums go through the sliding-window layout
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


def _plant_blocks(x, primes):
    """x [..., limb, N] (numpy or torch): blocks of q - 1, (q - 1) / 2, (q + 1) / 2 and 0 at the start and at the end of every polynomial."""
    n = x.shape[-1]
    for j, q in enumerate(primes):
        q = int(q)
        for at in (0, n - 4 * BLOCK):
            for i, v in enumerate((q - 1, (q - 1) // 2, (q + 1) // 2, 0)):
                x[..., j, at + i * BLOCK:at + (i + 1) * BLOCK] = v
    return x


def _uniform(rng, primes, lead, n):
    """[*lead][L][N], uniform, with the special blocks planted."""
    out = np.empty(tuple(lead) + (len(primes), n), dtype=np.uint64)
    for j, q in enumerate(primes):
        out[..., j, :] = rng.integers(0, int(q), tuple(lead) + (n,), dtype=np.uint64)
    return _plant_blocks(out, primes)


def _gpu_uniform(primes, lead, n, gpu, gen):
    import torch
    out = torch.empty(tuple(lead) + (len(primes), n), dtype=torch.int64, device=gpu)
    for j, q in enumerate(primes):
        out[..., j, :] = torch.randint(0, int(q), tuple(lead) + (n,), dtype=torch.int64, device=gpu, generator=gen)
    return out


def _oracle_sum(oc, plain, ct, limbs, acc=None, upto=None):
    """sum over k of plain[k] (.) ct[k][p] for both polynomials with the oracle's multiply and add, then + acc; upto: the sums
    after those term counts instead (without acc)."""
    s, partial = None, {}
    for k in range(plain.shape[0]):
        prod = [oc.multiply(plain[k], ct[k][p], limbs) for p in range(2)]
        s = prod if s is None else [oc.add(s[p], prod[p], limbs) for p in range(2)]
        if upto and k + 1 in upto:
            partial[k + 1] = np.stack(s)
    if upto:
        return partial
    if acc is not None:
        s = [oc.add(acc[p], s[p], limbs) for p in range(2)]
    return np.stack(s)


def _with_acc(oc, s, acc, limbs):
    return np.stack([oc.add(acc[p], s[p], limbs) for p in range(2)])


def _first_diff(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    idx = tuple(int(v) for v in np.argwhere(got != ref)[0])
    msg = f"{what}: {int(np.count_nonzero(got != ref))} words differ, first at {idx}: got {int(got[idx])}, want {int(ref[idx])}"
    print(msg)
    raise AssertionError(msg)


def _per_fp(bits):
    return min((56 * (1 << (52 - bits)) - 40) // 35, 1 << 16)


def _flush_terms(name):
    """T - 1, T, T + 1 for every FP64 limb (bit length <= 50) of the set."""
    out = set()
    for q in primes_of(name)[1]:
        if int(q).bit_length() <= 50:
            t = _per_fp(int(q).bit_length())
            out |= {t - 1, t, t + 1}
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# A: the kernel against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
A_CONFIGS = ["hyb12_a2", "p61_a2", "c2_ckks14", "wide_p20"]
A_DENSE = [(name, t) for name in A_CONFIGS for t in sorted(set(TERMS) | {v for v in _flush_terms(name) if v <= DENSE_MAX})]
A_LONG = [(name, tuple(sorted(v for v in _flush_terms(name) if v > DENSE_MAX))) for name in A_CONFIGS
          if any(v > DENSE_MAX for v in _flush_terms(name))]


def test_the_flush_intervals_of_the_sets_are_covered():
    assert _flush_terms("p61_a2") == {4, 5, 6}
    assert _flush_terms("wide_p20") == {100, 101, 102, 202, 203, 204}
    assert _flush_terms("hyb12_a2") == _flush_terms("c2_ckks14") == {6551, 6552, 6553}
    covered = {(name, t) for name, t in A_DENSE} | {(name, t) for name, ts in A_LONG for t in ts}
    for name in A_CONFIGS:
        for t in set(TERMS) | _flush_terms(name):
            assert (name, t) in covered


@functools.lru_cache(maxsize=1)
def _pool(name):
    """Inputs for 3 groups of 100 terms, an acc per group, and the oracle's partial sums after every dense term count."""
    log_n, primes, size_p = primes_of(name)
    n, ql = 1 << log_n, len(primes)      # every row of the prime table: the 61-bit primes of p61_a2 are its special primes
    rng = rng_for(9900 + A_CONFIGS.index(name))
    plain, ct, acc = _uniform(rng, primes, (3, DENSE_MAX), n), _uniform(rng, primes, (3, DENSE_MAX, 2), n), _uniform(rng, primes, (3, 2), n)
    oc = oracle_ctx(name)
    counts = {t for nm, t in A_DENSE if nm == name}
    ref = [_oracle_sum(oc, plain[g], ct[g], ql, upto=counts) for g in range(3)]
    return plain, ct, acc, ref


@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name,terms", A_DENSE)
def test_sum_kernel_against_oracle(name, terms, batch, with_acc, gpu):
    import torch
    P, ctx, log_n, primes, size_p, _ = _setup(name, gpu)
    n, ql = 1 << log_n, len(primes)
    plain, ct, acc, ref = _pool(name)
    oc = oracle_ctx(name)
    dp, dc = P.to_device(plain[:batch, :terms], gpu), P.to_device(ct[:batch, :terms], gpu)
    da = P.to_device(acc[:batch], gpu) if with_acc else None
    keep = [x.clone() for x in (dp, dc)] + ([da.clone()] if with_acc else [])
    res = _poisoned((batch, 2, ql, n), gpu)
    ctx.multiply_plain_sum_batched(dp, dc, da, res, ql, terms, batch)
    got = P.to_host(res)
    for g in range(batch):
        want = _with_acc(oc, ref[g][terms], acc[g], ql) if with_acc else ref[g][terms]
        _first_diff(got[g], want, f"{name} terms={terms} batch={batch} acc={with_acc} group {g}")
    assert all(torch.equal(a, b) for a, b in zip([dp, dc] + ([da] if with_acc else []), keep)), "the sum wrote to an operand"
    del ctx, dp, dc, da, res, keep
    _release()


@pytest.mark.parametrize("name,counts", A_LONG)
def test_sum_kernel_at_long_flush_intervals(name, counts, gpu):
    """Sums longer than 100 terms (T - 1, T, T + 1 of the set's FP64 limbs): one run of max(counts) + 2 terms on the device, group g
    reading terms g .. g + K - 1 of it through the strides (batch stride = one term).  The oracle sees every term once, streamed
    back from the device, and keeps one running sum per group."""
    import torch
    P, ctx, log_n, primes, size_p, _ = _setup(name, gpu)
    n, ql = 1 << log_n, len(primes)
    ln = ql * n
    oc = oracle_ctx(name)
    run = max(counts) + 2
    gen = torch.Generator(device=gpu)
    gen.manual_seed(9950 + A_CONFIGS.index(name))
    dp = _plant_blocks(_gpu_uniform(primes, (run,), n, gpu, gen), primes)
    dc = _plant_blocks(_gpu_uniform(primes, (run, 2), n, gpu, gen), primes)
    acc = _uniform(rng_for(9960 + A_CONFIGS.index(name)), primes, (3, 2), n)
    da = P.to_device(acc, gpu)
    # running sums of the three windows; ref[g][K] = sum of terms g .. g + K - 1
    sums, ref = [None] * 3, [dict() for _ in range(3)]
    for k in range(run):
        pk, ck = P.to_host(dp[k]), P.to_host(dc[k])
        prod = [oc.multiply(pk, ck[p], ql) for p in range(2)]
        for g in range(3):
            if k < g:
                continue
            sums[g] = prod if sums[g] is None else [oc.add(sums[g][p], prod[p], ql) for p in range(2)]
            if k - g + 1 in counts:
                ref[g][k - g + 1] = np.stack(sums[g])
    for terms in counts:
        for batch in (1, 3):
            for with_acc in (False, True):
                res = _poisoned((batch, 2, ql, n), gpu)
                ctx.multiply_plain_sum_batched(dp, dc, da if with_acc else None, res, ql, terms, batch, strides=(ln, ln, 2 * ln, 2 * ln, 2 * ln))
                got = P.to_host(res)
                for g in range(batch):
                    want = _with_acc(oc, ref[g][terms], acc[g], ql) if with_acc else ref[g][terms]
                    _first_diff(got[g], want, f"{name} terms={terms} batch={batch} acc={with_acc} group {g} (window layout)")
    del ctx, dp, dc, da, res
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B: one term without acc is the per-polynomial multiply
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A_CONFIGS)
def test_one_term_equals_multiply_rns_poly(name, gpu):
    import torch
    P, ctx, log_n, primes, size_p, _ = _setup(name, gpu)
    n, batch, ql = 1 << log_n, 3, len(primes)
    rng = rng_for(10000 + A_CONFIGS.index(name))
    dp, dc = P.to_device(_uniform(rng, primes, (batch, 1), n), gpu), P.to_device(_uniform(rng, primes, (batch, 1, 2), n), gpu)
    res, want = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, 2, ql, n), gpu)
    ctx.multiply_plain_sum_batched(dp, dc, None, res, ql, 1, batch)
    for g in range(batch):
        for p in range(2):
            ctx.multiply_rns_poly(dp[g, 0], dc[g, 0, p], want[g, p], ql)
    assert torch.equal(res, want), f"{name}: terms == 1 differs from pha_multiply_rns_poly"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C: accumulate in place
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hyb12_a2", "p61_a2"])
def test_accumulate_in_place(name, gpu):
    import torch
    P, ctx, log_n, primes, size_p, _ = _setup(name, gpu)
    n, batch, terms, ql = 1 << log_n, 3, 7, len(primes)
    rng = rng_for(10100 + A_CONFIGS.index(name))
    plain, ct, acc = _uniform(rng, primes, (batch, terms), n), _uniform(rng, primes, (batch, terms, 2), n), _uniform(rng, primes, (batch, 2), n)
    dp, dc, da = P.to_device(plain, gpu), P.to_device(ct, gpu), P.to_device(acc, gpu)
    want = _poisoned((batch, 2, ql, n), gpu)
    ctx.multiply_plain_sum_batched(dp, dc, da, want, ql, terms, batch)
    oc = oracle_ctx(name)
    for g in range(batch):
        _first_diff(P.to_host(want[g]), _oracle_sum(oc, plain[g], ct[g], ql, acc=acc[g]), f"{name} out of place, group {g}")
    ctx.multiply_plain_sum_batched(dp, dc, da, da, ql, terms, batch)
    assert torch.equal(da, want), f"{name}: res == acc differs from the out-of-place result"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: addressing
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hyb12_a2", "p61_a2"])
def test_shared_operands_and_views_with_gaps(name, gpu):
    import torch
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 3, 5
    pl = primes[:ql]
    ln = ql * n
    rng = rng_for(10200 + A_CONFIGS.index(name))
    oc = oracle_ctx(name)
    plain, ct, acc = _uniform(rng, pl, (batch, terms), n), _uniform(rng, pl, (batch, terms, 2), n), _uniform(rng, pl, (batch, 2), n)
    dp, dc, da = P.to_device(plain, gpu), P.to_device(ct, gpu), P.to_device(acc, gpu)
    dense = (ln, terms * ln, 2 * ln, terms * 2 * ln, 2 * ln)
    # shared ct (rows of a matrix against one vector): replicated -> oracle, then batch stride 0 two ways
    vec = dc[0].contiguous()
    want = _poisoned((batch, 2, ql, n), gpu)
    ctx.multiply_plain_sum_batched(dp, vec[None].expand(batch, terms, 2, ql, n).contiguous(), da, want, ql, terms, batch)
    for g in range(batch):
        _first_diff(P.to_host(want[g]), _oracle_sum(oc, plain[g], ct[0], ql, acc=acc[g]), f"{name} replicated ct, group {g}")
    for strides in (None, (ln, terms * ln, 2 * ln, 0, 2 * ln)):
        res = _poisoned((batch, 2, ql, n), gpu)
        ctx.multiply_plain_sum_batched(dp, vec, da, res, ql, terms, batch, strides=strides)
        assert torch.equal(res, want), f"{name}: shared ct (strides={strides}) differs"
    # shared plain (one layer applied to a batch of inputs)
    row = dp[1].contiguous()
    want_p = _poisoned((batch, 2, ql, n), gpu)
    ctx.multiply_plain_sum_batched(row[None].expand(batch, terms, ql, n).contiguous(), dc, None, want_p, ql, terms, batch)
    for g in range(batch):
        _first_diff(P.to_host(want_p[g]), _oracle_sum(oc, plain[1], ct[g], ql), f"{name} replicated plain, group {g}")
    for strides in (None, (ln, 0, 2 * ln, terms * 2 * ln, 2 * ln)):
        res = _poisoned((batch, 2, ql, n), gpu)
        ctx.multiply_plain_sum_batched(row, dc, None, res, ql, terms, batch, strides=strides)
        assert torch.equal(res, want_p), f"{name}: shared plain (strides={strides}) differs"
    # views with gaps: operand (g, k) at off + g * bs + k * ts of a poisoned buffer, a different geometry for each operand
    want_d = _poisoned((batch, 2, ql, n), gpu)
    ctx.multiply_plain_sum_batched(dp, dc, da, want_d, ql, terms, batch, strides=dense)
    for g in range(batch):
        _first_diff(P.to_host(want_d[g]), _oracle_sum(oc, plain[g], ct[g], ql, acc=acc[g]), f"{name} dense, group {g}")
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
    res = _poisoned((batch, 2, ql, n), gpu)
    ctx.multiply_plain_sum_batched(vp_, vc, va, res, ql, terms, batch, strides=(tsp, bsp, tsc, bsc, bsa))
    assert torch.equal(res, want_d), f"{name}: operands with gaps differ from the dense call"
    assert all(torch.equal(a, b) for a, b in zip((bigp, bigc, biga), keep))
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# E: the whole operation against the two-call composition on the device and against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
E_CASES = [("hyb13_a3", O.CKKS), ("hyb14_a4", O.CKKS), ("c2_ckks14", O.CKKS), ("hyb12_a2", O.BGV)]


def _level_drop(ctx, scheme, ql, src, polys, dst):
    if scheme == O.CKKS:
        ctx.divide_and_round_q_last_ntt(ql, src, polys, dst)
    else:
        ctx.mod_t_and_divide_q_last_ntt(ql, src, polys, dst)


@pytest.mark.parametrize("name,scheme", E_CASES)
def test_whole_operation(name, scheme, gpu):
    import torch
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu, BGV_T if scheme == O.BGV else None)
    n, batch, terms = 1 << log_n, 5, 4
    pl = primes[:ql]
    rng = rng_for(10300 + len(name) + scheme)
    oc = oracle_ctx(name)
    tool = O.Tool(oc, ql)
    if scheme == O.BGV:
        tool.set_plain_modulus(BGV_T)
    plain, ct, acc = _uniform(rng, pl, (batch, terms), n), _uniform(rng, pl, (batch, terms, 2), n), _uniform(rng, pl, (batch, 2), n)
    dp, dc, da = P.to_device(plain, gpu), P.to_device(ct, gpu), P.to_device(acc, gpu)
    keep = [x.clone() for x in (dp, dc, da)]
    for with_acc in (False, True):
        a = da if with_acc else None
        s = _poisoned((batch, 2, ql, n), gpu)
        ctx.multiply_plain_sum_batched(dp, dc, a, s, ql, terms, batch)
        want = _poisoned((batch, 2, ql - 1, n), gpu)
        _level_drop(ctx, scheme, ql, s, 2 * batch, want)
        for chunk in (1, 3, 0):
            dst = _poisoned((batch, 2, ql - 1, n), gpu)
            ctx.plain_inner_product_rescale_batched(ql, dp, dc, a, terms, batch, scheme, dst, chunk=chunk)
            if not torch.equal(dst, want):
                _first_diff(P.to_host(dst), P.to_host(want), f"{name} scheme={scheme} acc={with_acc} chunk={chunk} vs the composition")
        got = P.to_host(want)
        for g in range(batch):
            ref = _oracle_sum(oc, plain[g], ct[g], ql, acc=acc[g] if with_acc else None)
            ref = tool.rescale_ntt(ref, 2) if scheme == O.CKKS else tool.mod_t_divide_q_last_ntt(ref, 2)
            _first_diff(got[g], ref, f"{name} scheme={scheme} acc={with_acc} group {g} vs the oracle")
    assert all(torch.equal(a, b) for a, b in zip((dp, dc, da), keep)), "the whole operation wrote to an operand"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# F: the large shape
# ------------------------------------------------------------------------------------------------------------------------------
def test_whole_operation_c3(gpu):
    """c3_ckks16, 45 limbs: 8 terms, 2 groups sharing ct (two rows of a matrix against one vector).  The whole batch against the
    device composition; the first and the last group against the oracle."""
    import torch
    name, scheme = "c3_ckks16", O.CKKS
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 2, 8
    pl = primes[:ql]
    oc = oracle_ctx(name)
    tool = O.Tool(oc, ql)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(10400)
    dp = _gpu_uniform(pl, (batch, terms), n, gpu, gen)
    dv = _gpu_uniform(pl, (terms, 2), n, gpu, gen)
    keep = dp.clone(), dv.clone()
    dst = _poisoned((batch, 2, ql - 1, n), gpu)
    ctx.plain_inner_product_rescale_batched(ql, dp, dv, None, terms, batch, scheme, dst)
    assert torch.equal(dp, keep[0]) and torch.equal(dv, keep[1]), "the whole operation wrote to an operand"
    s = _poisoned((batch, 2, ql, n), gpu)
    ctx.multiply_plain_sum_batched(dp, dv, None, s, ql, terms, batch)
    sums = P.to_host(s)
    want = _poisoned((batch, 2, ql - 1, n), gpu)
    ctx.divide_and_round_q_last_ntt(ql, s, 2 * batch, want)
    if not torch.equal(dst, want):
        _first_diff(P.to_host(dst), P.to_host(want), "c3 plain_inner_product_rescale_batched vs the device composition")
    vec = P.to_host(dv)
    for g in (0, batch - 1):
        ref = _oracle_sum(oc, P.to_host(dp[g]), vec, ql)
        _first_diff(sums[g], ref, f"c3 multiply_plain_sum_batched group {g} vs the oracle")
        _first_diff(P.to_host(dst[g]), tool.rescale_ntt(ref, 2), f"c3 plain_inner_product_rescale_batched group {g} vs the oracle")
    del ctx, dp, dv, dst, s, want
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
    pl = primes[:ql]
    ln = ql * n
    rng = rng_for(10500)
    dp = P.to_device(_uniform(rng, pl, (batch, terms), n), gpu)
    dc = P.to_device(_uniform(rng, pl, (batch, terms, 2), n), gpu)
    da = P.to_device(_uniform(rng, pl, (batch, 2), n), gpu)
    keep = [x.clone() for x in (dp, dc, da)]
    res, dst = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, 2, ql - 1, n), gpu)
    dense = (ln, terms * ln, 2 * ln, terms * 2 * ln, 2 * ln)
    f, g = ctx.multiply_plain_sum_batched, ctx.plain_inner_product_rescale_batched
    # null required pointers (acc may be null)
    for args in ((None, dc, da, res), (dp, None, da, res), (dp, dc, da, None)):
        _refused(f, "null", *args, ql, terms, batch, strides=dense)
    _refused(g, "null", ql, None, dc, da, terms, batch, O.CKKS, dst, strides=dense)
    _refused(g, "null", ql, dp, None, da, terms, batch, O.CKKS, dst, strides=dense)
    _refused(g, "null", ql, dp, dc, da, terms, batch, O.CKKS, None, strides=dense)
    # no terms, limb counts outside the table
    _refused(f, "terms", dp, dc, da, res, ql, 0, batch, strides=dense)
    _refused(g, "terms", ql, dp, dc, da, 0, batch, O.CKKS, dst, strides=dense)
    _refused(f, "coeff_mod_size out of range", dp, dc, da, res, 0, terms, batch, strides=dense)
    _refused(f, "coeff_mod_size out of range", dp, dc, da, res, len(primes) + 1, terms, batch, strides=dense)
    _refused(g, "size_Ql out of range", len(primes), dp, dc, da, terms, batch, O.CKKS, dst, strides=dense)
    _refused(g, "size_Ql out of range", 0, dp, dc, da, terms, batch, O.CKKS, dst, strides=dense)
    # odd strides, one at a time
    for i in range(5):
        odd = list(dense)
        odd[i] += 1
        _refused(f, "even", dp, dc, da, res, ql, terms, batch, strides=tuple(odd))
        _refused(g, "even", ql, dp, dc, da, terms, batch, O.CKKS, dst, strides=tuple(odd))
    # terms that overlap
    _refused(f, "plain term stride", dp, dc, da, res, ql, terms, batch, strides=(ln - 2, terms * ln, 2 * ln, terms * 2 * ln, 2 * ln))
    _refused(f, "ct term stride", dp, dc, da, res, ql, terms, batch, strides=(ln, terms * ln, 2 * ln - 2, terms * 2 * ln, 2 * ln))
    _refused(g, "plain term stride", ql, dp, dc, da, terms, batch, O.CKKS, dst, strides=(0, terms * ln, 2 * ln, terms * 2 * ln, 2 * ln))
    _refused(g, "ct term stride", ql, dp, dc, da, terms, batch, O.CKKS, dst, strides=(ln, terms * ln, ln, terms * 2 * ln, 2 * ln))
    # forbidden overlaps: res on a plaintext, on the last ciphertext, on acc shifted by one polynomial, on acc with another stride
    flat_c = dc.view(-1)
    _refused(f, "overlap", dp, dc, da, dp.view(-1)[:batch * 2 * ln].view(batch, 2, ql, n), ql, terms, batch)
    _refused(f, "overlap", dp, dc, da, flat_c[flat_c.numel() - batch * 2 * ln:].view(batch, 2, ql, n), ql, terms, batch)
    wide = torch.zeros((batch * 2 * ln + ln,), dtype=torch.int64, device=gpu)
    _refused(f, "overlap", dp, dc, wide, wide[ln:].view(batch, 2, ql, n), ql, terms, batch)
    big_acc = torch.zeros((batch * 4 * ln,), dtype=torch.int64, device=gpu)
    _refused(f, "overlap", dp, dc, big_acc, big_acc[:batch * 2 * ln].view(batch, 2, ql, n), ql, terms, batch,
             strides=(ln, terms * ln, 2 * ln, terms * 2 * ln, 4 * ln))
    _refused(g, "overlap", ql, dp, dc, da, terms, batch, O.CKKS, dc.view(-1)[:batch * 2 * (ql - 1) * n].view(batch, 2, ql - 1, n))
    _refused(g, "overlap", ql, dp, dc, da, terms, batch, O.CKKS, da.view(-1)[:batch * 2 * (ql - 1) * n].view(batch, 2, ql - 1, n))
    _refused(g, "overlap", ql, dp, dc, da, terms, batch, O.CKKS, dp.view(-1)[:batch * 2 * (ql - 1) * n].view(batch, 2, ql - 1, n))
    # the rescale entry's own refusals
    _refused(g, "bfv", ql, dp, dc, da, terms, batch, O.BFV, dst)
    _refused(g, "NTT-form product", ql, dp, dc, da, terms, batch, O.BFV, dst)
    _refused(g, "last remaining modulus", 1, dp, dc, da, terms, batch, O.CKKS, dst, strides=dense)
    _refused(g, "plain modulus", ql, dp, dc, da, terms, batch, O.BGV, dst)
    # an empty batch does nothing
    f(dp, dc, da, res, ql, terms, 0, strides=dense)
    g(ql, dp, dc, da, terms, 0, O.CKKS, dst, strides=dense)
    torch.cuda.synchronize()
    for out in (res, dst):
        assert bool((out == POISON).all()), "a refused (or empty) call wrote to its output"
    assert all(torch.equal(a, b) for a, b in zip((dp, dc, da), keep)), "a refused call wrote to an operand"
    assert not bool(wide.any()) and not bool(big_acc.any())
    # and the same arguments without the defect go through, leaving the operands as they were
    f(dp, dc, da, res, ql, terms, batch, strides=dense)
    g(ql, dp, dc, da, terms, batch, O.CKKS, dst)
    torch.cuda.synchronize()
    for out in (res, dst):
        assert not bool((out == POISON).any())
    assert all(torch.equal(a, b) for a, b in zip((dp, dc, da), keep)), "a successful call wrote to an operand"
    del ctx
    _release()


def _refused_with(fn, text, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == text, f"refused with {str(e.value)!r}, not with {text!r}"


def test_every_refusal_and_their_order(gpu):
    """The refusals of the two entries that test_refusals_leave_everything_untouched does not reach, the whole message compared, and
    for several defects in one call the one that is reported: the term count, the batch, odd strides, alignment of the operands,
    overlapping terms of plain, of ct, and only then the output (its alignment, then plain, ct, acc).  Nothing is launched."""
    import torch
    name = "hyb12_a2"
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 2, 3
    pl = primes[:ql]
    ln = ql * n
    rng = rng_for(10550)
    dp = P.to_device(_uniform(rng, pl, (batch, terms), n), gpu)
    dc = P.to_device(_uniform(rng, pl, (batch, terms, 2), n), gpu)
    da = P.to_device(_uniform(rng, pl, (batch, 2), n), gpu)
    keep = [x.clone() for x in (dp, dc, da)]
    dense = (ln, terms * ln, 2 * ln, terms * 2 * ln, 2 * ln)
    even, aligned = "strides must be even (16-byte loads)", "buffers must be 16-byte aligned"
    crowded_p, crowded_c = "plain term stride below L * N: the terms of plain overlap", "ct term stride below 2 * L * N: the terms of ct overlap"
    on_acc = " must not overlap acc (other than res == acc with a stride of 2 * L * N)"
    entries = (   # call(plain, ct, acc, terms, batch, strides, out), the output, its name in a refusal
        (lambda p, c, a, t, B, st, out: ctx.multiply_plain_sum_batched(p, c, a, out, ql, t, B, strides=st), _poisoned((batch, 2, ql, n), gpu), "res"),
        (lambda p, c, a, t, B, st, out: ctx.plain_inner_product_rescale_batched(ql, p, c, a, t, B, O.CKKS, out, strides=st),
         _poisoned((batch, 2, ql - 1, n), gpu), "dst"),
    )
    offp, offc, offa = dp.view(-1)[1:], dc.view(-1)[1:], da.view(-1)[1:]   # 8 bytes past a 16-byte boundary
    for call, out, out_name in entries:
        off_out, words = out.view(-1)[1:], out.numel()
        _refused_with(call, "terms out of range", dp, dc, da, 1 << 32, batch, dense, out)
        _refused_with(call, "batch out of range", dp, dc, da, terms, 65536, dense, out)
        for args in ((offp, dc, da), (dp, offc, da), (dp, dc, offa)):
            _refused_with(call, aligned, *args, terms, batch, dense, out)
        _refused_with(call, aligned, dp, dc, da, terms, batch, dense, off_out)
        _refused_with(call, aligned, dp, dc, None, terms, batch, dense, off_out)
        _refused_with(call, crowded_p, dp, dc, da, terms, batch, (ln - 2,) + dense[1:], out)
        _refused_with(call, crowded_c, dp, dc, da, terms, batch, dense[:2] + (2 * ln - 2,) + dense[3:], out)
        _refused_with(call, even, dp, dc, None, terms, batch, dense[:4] + (2 * ln + 1,), out)    # acc's stride although there is no acc
        _refused_with(call, out_name + " must not overlap a plaintext operand", dp, dc, da, terms, batch, dense, dp.view(-1)[:words])
        _refused_with(call, out_name + " must not overlap an operand ciphertext", dp, dc, da, terms, batch, dense, dc.view(-1)[dc.numel() - words:])
        _refused_with(call, out_name + on_acc, dp, dc, da, terms, batch, dense, da.view(-1)[2 * n:2 * n + words])
        # every stride and alignment defect at once, then with the winner taken away each time
        _refused_with(call, even, offp, offc, offa, terms, batch, (ln - 1, 1, 2 * ln - 1, 3, 5), off_out)
        _refused_with(call, aligned, offp, offc, offa, terms, batch, (ln - 2, 0, 2 * ln - 2, 2, 4), off_out)
        _refused_with(call, crowded_p, dp, dc, da, terms, batch, (ln - 2, 0, 2 * ln - 2, 2, 4), off_out)
        _refused_with(call, crowded_c, dp, dc, da, terms, batch, (ln, 0, 2 * ln - 2, 2, 4), off_out)
        _refused_with(call, aligned, dp, dc, da, terms, batch, dense, dp.view(-1)[1:1 + words])   # misaligned AND on a plaintext
        # the term count and the batch come before the layout
        _refused_with(call, "terms must be at least 1", offp, dc, da, 0, 65536, (ln + 1,) + dense[1:], out)
        _refused_with(call, "terms out of range", offp, dc, da, 1 << 32, 65536, (ln + 1,) + dense[1:], out)
        _refused_with(call, "batch out of range", offp, dc, da, terms, 65536, (ln + 1,) + dense[1:], out)
    f, g = ctx.multiply_plain_sum_batched, ctx.plain_inner_product_rescale_batched
    res, dst = entries[0][1], entries[1][1]
    # res == acc is the sum entry's alone, and only in acc's own layout; the plaintext and the ciphertext are looked at first
    big_acc = torch.zeros((batch * 4 * ln,), dtype=torch.int64, device=gpu)
    _refused_with(f, "res" + on_acc, dp, dc, big_acc, big_acc[:batch * 2 * ln], ql, terms, batch, strides=dense[:4] + (4 * ln,))
    _refused_with(g, "dst" + on_acc, ql, dp, dc, da, terms, batch, O.CKKS, da.view(-1)[:dst.numel()], strides=dense)
    _refused_with(f, "res must not overlap a plaintext operand", dp, dc, dp.view(-1)[:batch * 2 * ln], dp.view(-1)[:batch * 2 * ln], ql, terms,
                  batch, strides=dense)
    # the limb count sits between the term count and the batch; the rescale entry's own checks come before everything shared
    _refused_with(f, "coeff_mod_size out of range", offp, dc, da, res, 0, terms, 65536, strides=(ln + 1,) + dense[1:])
    _refused_with(f, "terms out of range", offp, dc, da, res, 0, 1 << 32, 65536, strides=(ln + 1,) + dense[1:])
    _refused_with(g, "unsupported scheme", ql, dp, dc, da, terms, batch, 99, dst)
    _refused_with(g, "cannot rescale the last remaining modulus", 1, offp, dc, da, 0, 65536, O.CKKS, dst, strides=(1, 1, 1, 1, 1))
    _refused_with(g, "bgv needs a plain modulus (pha_context_set_plain_modulus)", ql, offp, dc, da, 0, 65536, O.BGV, dst, strides=(1, 1, 1, 1, 1))
    _refused_with(g, "size_Ql out of range", 0, offp, dc, da, 0, 65536, O.BGV, dst, strides=(1, 1, 1, 1, 1))
    torch.cuda.synchronize()
    assert bool((res == POISON).all()) and bool((dst == POISON).all()), "a refused call wrote to its output"
    assert all(torch.equal(a, b) for a, b in zip((dp, dc, da), keep)) and not bool(big_acc.any()), "a refused call wrote to an operand"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# H: strict mode
# ------------------------------------------------------------------------------------------------------------------------------
def test_strict_mode_names_the_operand(gpu):
    import torch
    name = "hyb12_a2"
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 3, 4
    pl = primes[:ql]
    ln = ql * n
    rng = rng_for(10600)
    dp = P.to_device(_uniform(rng, pl, (batch, terms), n), gpu)
    dc = P.to_device(_uniform(rng, pl, (batch, terms, 2), n), gpu)
    da = P.to_device(_uniform(rng, pl, (batch, 2), n), gpu)
    # the same operands as views with gaps (the strided branches of the check)
    geo = {"plain": (dp, ln, ln + 2 * n, terms * (ln + 2 * n) + 6), "ct": (dc, 2 * ln, 2 * ln + 4, terms * (2 * ln + 4) + 2 * n),
           "acc": (da[:, None], 2 * ln, 2 * ln, 2 * ln + 10)}
    big = {}
    for key, (src, words, ts, bs) in geo.items():
        b = torch.zeros((batch * bs,), dtype=torch.int64, device=gpu)
        for g in range(batch):
            for k in range(src.shape[1]):
                b[g * bs + k * ts:g * bs + k * ts + words] = src[g, k].reshape(-1)
        big[key] = b
    gapped = (geo["plain"][2], geo["plain"][3], geo["ct"][2], geo["ct"][3], geo["acc"][3])
    res, dst = _poisoned((batch, 2, ql, n), gpu), _poisoned((batch, 2, ql - 1, n), gpu)
    f, h = ctx.multiply_plain_sum_batched, ctx.plain_inner_product_rescale_batched
    g_bad, limb, idx = 2, 4, 777                                   # the last group; the last term / second polynomial where there is one
    was = P.set_strict(True)
    try:
        f(dp, dc, da, res, ql, terms, batch)                       # canonical operands pass
        f(big["plain"], big["ct"], big["acc"], res, ql, terms, batch, strides=gapped)
        h(ql, dp, dc[0].contiguous(), da, terms, batch, O.CKKS, dst)
        res.fill_(POISON), dst.fill_(POISON)
        spots = {"plain": ((g_bad, terms - 1, limb, idx), (terms - 1, 0)), "ct": ((g_bad, terms - 1, 1, limb, idx), (terms - 1, 1)),
                 "acc": ((g_bad, 1, limb, idx), (0, 1))}
        for key, (where, (k, poly)) in spots.items():
            named = f"multiply_plain_sum {key}"
            dense = {"plain": dp, "ct": dc, "acc": da}[key]
            _, _, ts, bs = geo[key]
            at = g_bad * bs + k * ts + (poly * ql + limb) * n + idx
            good = int(dense[where])
            assert int(big[key][at]) == good
            dense[where] = int(primes[limb])                       # q itself: the smallest non-canonical word
            big[key][at] = int(primes[limb])
            _refused(f, named, dp, dc, da, res, ql, terms, batch)
            _refused(f, named, big["plain"], big["ct"], big["acc"], res, ql, terms, batch, strides=gapped)
            _refused(h, named, ql, dp, dc, da, terms, batch, O.CKKS, dst)
            torch.cuda.synchronize()
            for out in (res, dst):
                assert bool((out == POISON).all()), "a call refused in strict mode wrote to its output"
            P.set_strict(False)                                    # accepted with strict mode off
            f(dp, dc, da, res, ql, terms, batch)
            torch.cuda.synchronize()
            assert not bool((res == POISON).any())
            res.fill_(POISON)
            P.set_strict(True)
            dense[where] = good
            big[key][at] = good
        # a bad word in a shared operand is found although only one copy of it exists
        dv = dc[0].contiguous()
        dv[terms - 1, 1, limb, idx] = int(primes[limb])
        _refused(f, "multiply_plain_sum ct", dp, dv, da, res, ql, terms, batch)
        row = dp[0].contiguous()
        row[1, limb, idx] = int(primes[limb])
        _refused(f, "multiply_plain_sum plain", row, dc, da, res, ql, terms, batch)
    finally:
        P.set_strict(was)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# I: graph capture
# ------------------------------------------------------------------------------------------------------------------------------
def test_rescale_entry_replays_from_a_graph(gpu):
    import torch
    name = "hyb13_a3"
    P, ctx, log_n, primes, size_p, ql = _setup(name, gpu)
    n, batch, terms = 1 << log_n, 5, 4
    pl = primes[:ql]
    r = rng_for(10700)
    ins = [(P.to_device(_uniform(r, pl, (batch, terms), n), gpu), P.to_device(_uniform(r, pl, (batch, terms, 2), n), gpu),
            P.to_device(_uniform(r, pl, (batch, 2), n), gpu)) for _ in range(3)]
    want = []
    for dp, dc, da in ins:
        out = _poisoned((batch, 2, ql - 1, n), gpu)
        ctx.plain_inner_product_rescale_batched(ql, dp, dc, da, terms, batch, O.CKKS, out, chunk=2)
        want.append(out)
    dp, dc, da = (x.clone() for x in ins[0])
    out = _poisoned((batch, 2, ql - 1, n), gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctx.plain_inner_product_rescale_batched(ql, dp, dc, da, terms, batch, O.CKKS, out, chunk=2)    # warm-up on the capture stream
    side.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            ctx.plain_inner_product_rescale_batched(ql, dp, dc, da, terms, batch, O.CKKS, out, chunk=2)
    for i in (1, 2, 0):
        dp.copy_(ins[i][0])
        dc.copy_(ins[i][1])
        da.copy_(ins[i][2])
        out.fill_(POISON)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[i]), i
    del ctx, gr
    _release()
