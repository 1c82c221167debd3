"""The batched BFV multiplies (pha_bfv_multiply_{behz,hps,hps_overq}_batched), word for word:

A. small sets, every ciphertext of B = 1, 2, 3, 5 against the CPU oracle (extreme residues in every ciphertext but the first);
B. the config-4 shape: B = 8 against the single-pair entry (on the device) and the oracle (first and last), B = 64 with the default
   chunk against the single-pair entry;
C. chunk = 1, 3, 7, 0 give the same bits for B = 7;
D. squaring (the same tensor on both sides) against the oracle, incl. the hps_overq shortcut;
E. levels dropped (hps_overq_leveled) against the oracle;
F. bfv_multiply_hps_batched -> relinearize_rotate_batched against the single calls and the oracle;
G. refusals, const inputs, single and batched entries sharing one context;
H. strict mode.

The oracle multiplies at the full config-4 level are the slow part: six of them (group B), two more at level 15 (group E)."""
import gc

import numpy as np
import pytest

from oracle import oracle as O
from util import oracle_ctx, primes_of, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

_DIMS = ("ciphertext", "polynomial", "limb", "index")
VARIANTS = ("behz", "hps", "overq")


def _setup(name, plain_t, gpu):
    import phantom_fhe_amd as P
    log_n, primes, size_p = primes_of(name)
    ctx = P.PhantomContext(log_n, list(primes), size_p, device=gpu)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    return P, oracle_ctx(name), ctx, 1 << log_n, primes, size_p, len(primes) - size_p


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _check(got, ref, what, lead=()):
    """Bit-exact comparison; on a mismatch names the first differing (ciphertext, polynomial, limb, index)."""
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    sub = tuple(int(v) for v in np.argwhere(got != ref)[0])
    idx = tuple(int(v) for v in lead) + sub
    at = ", ".join(f"{k} {v}" for k, v in zip(_DIMS[len(_DIMS) - len(idx):], idx))
    msg = f"{what}: {int(np.count_nonzero(got != ref))} words differ, first at {at}: got {int(got[sub])}, want {int(ref[sub])}"
    print(msg)
    raise AssertionError(msg)


def _check_dev(P, got, ref, what):
    """The same for two device tensors [B][3][Q][N]; only a mismatch brings them to the host."""
    import torch
    if torch.equal(got, ref):
        return
    for b in range(got.shape[0]):
        if not torch.equal(got[b], ref[b]):
            _check(P.to_host(got[b]), P.to_host(ref[b]), what, lead=(b,))


def _pairs(r, primes, size_q, n, batch):
    """ct1, ct2 [B][2][Q][N], uniform; every ciphertext but the first carries q - 1 in its first 32 coefficients and 0 in the next 32
    of ct2 (where the single-pair BFV tests place them), the last one also in ct1."""
    q = primes[:size_q]
    ct1 = np.stack([np.stack([uniform_poly(r, q, n) for _ in range(2)]) for _ in range(batch)])
    ct2 = np.stack([np.stack([uniform_poly(r, q, n) for _ in range(2)]) for _ in range(batch)])
    top = np.array(q, dtype=np.uint64)[None, :, None] - 1
    for b in range(1, batch):
        ct2[b, :, :, :32] = top
        ct2[b, :, :, 32:64] = 0
    if batch > 1:
        ct1[batch - 1, :, :, :32] = 0
        ct1[batch - 1, :, :, 32:64] = top
    return ct1, ct2


def _oracle(variant, oc, plain_t, ql=None):
    if variant == "behz":
        return O.Behz(oc, plain_t)
    if variant == "hps":
        return O.Hps(oc, plain_t)
    return O.HpsOverQ(oc, plain_t, ql) if ql else O.HpsOverQ(oc, plain_t)


def _batched(ctx, variant, d1, d2, dst, size_q, ql=None, chunk=0):
    if variant == "behz":
        ctx.bfv_multiply_behz_batched(d1, d2, dst, chunk)
    elif variant == "hps":
        ctx.bfv_multiply_hps_batched(d1, d2, dst, chunk)
    else:
        ctx.bfv_multiply_hps_overq_batched(ql or size_q, d1, d2, dst, chunk)


def _single(ctx, variant, a, b, dst, size_q, ql=None):
    if variant == "behz":
        ctx.bfv_multiply_behz(a, b, dst)
    elif variant == "hps":
        ctx.bfv_multiply_hps(a, b, dst)
    elif ql and ql != size_q:
        ctx.bfv_multiply_hps_overq_leveled(ql, a, b, dst)
    else:
        ctx.bfv_multiply_hps_overq(a, b, dst)


def _singles(ctx, variant, d1, d2, size_q, ql=None, square=False):
    import torch
    one = torch.zeros((d1.shape[0], 3) + tuple(d1.shape[2:]), dtype=d1.dtype, device=d1.device)
    for b in range(d1.shape[0]):
        _single(ctx, variant, d1[b], d1[b] if square else d2[b], one[b], size_q, ql)
    return one


def _zeros3(P, batch, size_q, n, gpu):
    import torch
    return torch.full((batch, 3, size_q, n), -0x2152411021524111, dtype=torch.int64, device=gpu)     # poisoned: every word must be written


# ------------------------------------------------------------------------------------------------------------------------------
# A: small sets against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
SMALL = [("behz", "c1_bfv4096", 65537), ("behz", "hyb12_a2", 1032193), ("behz", "hyb13_a3", 786433),
         ("hps", "c1_bfv4096", 65537), ("hps", "bfv13_50", 65537), ("hps", "bfv13_50", 1032193),
         ("overq", "c1_bfv4096", 65537), ("overq", "bfv13_50", 65537), ("overq", "hyb12_a2", 1032193)]


@pytest.mark.parametrize("variant,name,plain_t", SMALL)
def test_small_sets_against_the_oracle(variant, name, plain_t, gpu):
    P, oc, ctx, n, primes, size_p, size_q = _setup(name, plain_t, gpu)
    orc = _oracle(variant, oc, plain_t)
    r = rng_for(9100 + size_q)
    for batch in (1, 2, 3, 5):
        ct1, ct2 = _pairs(r, primes, size_q, n, batch)
        d1, d2 = P.to_device(ct1, gpu), P.to_device(ct2, gpu)
        dst = _zeros3(P, batch, size_q, n, gpu)
        _batched(ctx, variant, d1, d2, dst, size_q)
        got = P.to_host(dst)
        for b in range(batch):
            _check(got[b], orc.multiply(ct1[b], ct2[b]), f"{variant} {name} t={plain_t} B={batch}", lead=(b,))
        assert np.array_equal(P.to_host(d1), ct1) and np.array_equal(P.to_host(d2), ct2), "the inputs were written to"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B: the config-4 shape
# ------------------------------------------------------------------------------------------------------------------------------
C4, C4_T = "c4_bfv15", 1032193


@pytest.mark.parametrize("variant", VARIANTS)
def test_config4_b8_against_single_entry_and_oracle(variant, gpu):
    P, oc, ctx, n, primes, size_p, size_q = _setup(C4, C4_T, gpu)
    batch = 8
    r = rng_for(9200)
    ct1, ct2 = _pairs(r, primes, size_q, n, batch)
    d1, d2 = P.to_device(ct1, gpu), P.to_device(ct2, gpu)
    dst = _zeros3(P, batch, size_q, n, gpu)
    _batched(ctx, variant, d1, d2, dst, size_q)
    _check_dev(P, dst, _singles(ctx, variant, d1, d2, size_q), f"{variant} c4 B=8 vs 8 single calls")
    orc = _oracle(variant, oc, C4_T)
    for b in (0, batch - 1):
        _check(P.to_host(dst[b]), orc.multiply(ct1[b], ct2[b]), f"{variant} c4 B=8 vs oracle", lead=(b,))
    assert np.array_equal(P.to_host(d1), ct1) and np.array_equal(P.to_host(d2), ct2), "the inputs were written to"
    del ctx, d1, d2, dst
    _release()


@pytest.mark.parametrize("variant", ["hps", "overq"])
def test_config4_b64_default_chunk_against_single_entry(variant, gpu):
    """64 pairs with the default chunk: several sets of launches over one scratch arena; every ciphertext against its single call."""
    import torch
    P, oc, ctx, n, primes, size_p, size_q = _setup(C4, C4_T, gpu)
    batch = 64
    g = torch.Generator(device=gpu)
    g.manual_seed(0x5EED9300)
    d1 = torch.empty((batch, 2, size_q, n), dtype=torch.int64, device=gpu)
    d2 = torch.empty_like(d1)
    for i in range(size_q):
        for d in (d1, d2):
            d[:, :, i] = torch.randint(0, int(primes[i]), (batch, 2, n), dtype=torch.int64, device=gpu, generator=g)
        d2[1:, :, i, :32] = int(primes[i]) - 1
        d2[1:, :, i, 32:64] = 0
    keep1, keep2 = d1.clone(), d2.clone()
    dst = _zeros3(P, batch, size_q, n, gpu)
    _batched(ctx, variant, d1, d2, dst, size_q)
    _check_dev(P, dst, _singles(ctx, variant, d1, d2, size_q), f"{variant} c4 B=64 vs 64 single calls")
    assert torch.equal(d1, keep1) and torch.equal(d2, keep2), "the inputs were written to"
    del ctx, d1, d2, dst, keep1, keep2
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C: chunking
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_any_chunk_gives_the_same_bits(variant, gpu):
    import torch
    name, plain_t, batch = "bfv13_50", 1032193, 7
    P, oc, ctx, n, primes, size_p, size_q = _setup(name, plain_t, gpu)
    ct1, ct2 = _pairs(rng_for(9300), primes, size_q, n, batch)
    d1, d2 = P.to_device(ct1, gpu), P.to_device(ct2, gpu)
    ref = _singles(ctx, variant, d1, d2, size_q)
    for chunk in (1, 3, 7, 0):
        dst = _zeros3(P, batch, size_q, n, gpu)
        _batched(ctx, variant, d1, d2, dst, size_q, chunk=chunk)
        _check_dev(P, dst, ref, f"{variant} {name} B=7 chunk={chunk} vs single calls")
    orc = _oracle(variant, oc, plain_t)
    got = P.to_host(dst)
    for b in range(batch):
        _check(got[b], orc.multiply(ct1[b], ct2[b]), f"{variant} {name} B=7 vs oracle", lead=(b,))
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: squaring
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,name,plain_t", [("behz", "hyb12_a2", 1032193), ("hps", "bfv13_50", 65537),
                                                  ("overq", "bfv13_50", 65537), ("overq", "hyb12_a2", 1032193)])
def test_same_tensor_on_both_sides_squares(variant, name, plain_t, gpu):
    """ct1 is ct2: the squaring path for the whole batch; over-Q keeps the reference's shortcut (multiply(ct, ct) of the oracle's
    HpsOverQ takes it too, and differs from the product of two separate copies)."""
    P, oc, ctx, n, primes, size_p, size_q = _setup(name, plain_t, gpu)
    batch = 3
    _, ct = _pairs(rng_for(9400), primes, size_q, n, batch)
    d = P.to_device(ct, gpu)
    dst = _zeros3(P, batch, size_q, n, gpu)
    _batched(ctx, variant, d, d, dst, size_q)
    orc = _oracle(variant, oc, plain_t)
    got = P.to_host(dst)
    for b in range(batch):
        x = ct[b]               # one object on both sides: the oracle squares on `ct2 is ct1`
        _check(got[b], orc.multiply(x, x), f"{variant} {name} square B={batch}", lead=(b,))
    _check_dev(P, dst, _singles(ctx, variant, d, d, size_q, square=True), f"{variant} {name} square vs single calls")
    assert np.array_equal(P.to_host(d), ct)
    if variant == "overq":      # two separate copies are a product, not the shortcut
        d_copy = d.clone()
        _batched(ctx, variant, d, d_copy, dst, size_q)
        got = P.to_host(dst)
        for b in range(batch):
            _check(got[b], orc.multiply(ct[b], ct[b].copy()), f"{variant} {name} product of two copies", lead=(b,))
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# E: levels dropped
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,plain_t,ql", [("bfv13_50", 65537, 3), ("bfv13_50", 65537, 2), (C4, C4_T, 15)])
def test_leveled_against_the_oracle(name, plain_t, ql, gpu):
    P, oc, ctx, n, primes, size_p, size_q = _setup(name, plain_t, gpu)
    batch = 4
    ct1, ct2 = _pairs(rng_for(9500 + ql), primes, size_q, n, batch)
    d1, d2 = P.to_device(ct1, gpu), P.to_device(ct2, gpu)
    dst = _zeros3(P, batch, size_q, n, gpu)
    ctx.bfv_multiply_hps_overq_batched(ql, d1, d2, dst)
    hq = O.HpsOverQ(oc, plain_t, ql)
    against_oracle = (0, batch - 1) if name == C4 else range(batch)
    for b in against_oracle:
        _check(P.to_host(dst[b]), hq.multiply(ct1[b], ct2[b]), f"leveled {name} ql={ql} vs oracle", lead=(b,))
    _check_dev(P, dst, _singles(ctx, "overq", d1, d2, size_q, ql), f"leveled {name} ql={ql} vs single calls")
    # squaring with levels dropped
    ctx.bfv_multiply_hps_overq_batched(ql, d2, d2, dst)
    _check_dev(P, dst, _singles(ctx, "overq", d2, d2, size_q, ql, square=True), f"leveled {name} ql={ql} square vs single calls")
    if name != C4:
        for b in range(batch):
            x = ct2[b]
            _check(P.to_host(dst[b]), hq.multiply(x, x), f"leveled {name} ql={ql} square vs oracle", lead=(b,))
    assert np.array_equal(P.to_host(d1), ct1) and np.array_equal(P.to_host(d2), ct2)
    del ctx, d1, d2, dst
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# F: multiply -> relinearize + rotate
# ------------------------------------------------------------------------------------------------------------------------------
def _keys(rng, primes, n, dnum):
    return np.stack([np.stack([uniform_poly(rng, primes, n), uniform_poly(rng, primes, n)]) for _ in range(dnum)])


def test_chain_into_relinearize_rotate(gpu):
    import torch
    name, plain_t, batch, elt = "hyb12_a2", 1032193, 4, 5
    P, oc, ctx, n, primes, size_p, size_q = _setup(name, plain_t, gpu)
    ql = size_q
    r = rng_for(9600)
    dnum = size_q // size_p
    evk, gk = _keys(r, primes, n, dnum), _keys(r, primes, n, dnum)
    rlk, glk = P.PhantomRelinKey.from_numpy(evk, gpu), P.PhantomRelinKey.from_numpy(gk, gpu)
    ct1, ct2 = _pairs(r, primes, size_q, n, batch)
    d1, d2 = P.to_device(ct1, gpu), P.to_device(ct2, gpu)
    ct3 = _zeros3(P, batch, size_q, n, gpu)
    ctx.bfv_multiply_hps_batched(d1, d2, ct3)
    out = torch.empty((batch, 2, ql, n), dtype=torch.int64, device=gpu)
    ctx.relinearize_rotate_batched(ql, ct3, batch, rlk.public_keys_ptr, glk.public_keys_ptr, elt, O.BFV, out)      # no reshaping in between
    # the single calls, one ciphertext at a time
    for b in range(batch):
        one3 = torch.empty((3, size_q, n), dtype=torch.int64, device=gpu)
        ctx.bfv_multiply_hps(d1[b], d2[b], one3)
        ct = one3[:2].clone()
        ctx.keyswitch_inplace(ql, ct, one3[2], rlk.public_keys_ptr, O.BFV)
        rot, g1 = torch.empty((1, 2, ql, n), dtype=torch.int64, device=gpu), torch.empty((1, ql, n), dtype=torch.int64, device=gpu)
        ctx.apply_galois_for_keyswitch(ct[None], rot, g1, elt, ql, 1, False)
        ctx.keyswitch_inplace(ql, rot[0], g1[0], glk.public_keys_ptr, O.BFV)
        _check(P.to_host(out[b]), P.to_host(rot[0]), "multiply -> relinearize_rotate vs the single calls", lead=(b,))
    # the oracle, ciphertext 1 (extreme residues)
    tool = O.Tool(oc, ql)
    b = 1
    prod = O.Hps(oc, plain_t).multiply(ct1[b], ct2[b])
    x = tool.keyswitch_inplace(prod[:2], prod[2], [evk[i] for i in range(tool.beta)], O.BFV)
    g = [oc.apply_galois_coeff(x[p], elt, ql) for p in range(2)]
    ref = tool.keyswitch_inplace(np.stack([g[0], np.zeros_like(g[0])]), g[1], [gk[i] for i in range(tool.beta)], O.BFV)
    _check(P.to_host(out[b]), ref, "multiply -> relinearize_rotate vs the oracle", lead=(b,))
    del ctx, rlk, glk
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# G: edges
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_shared_context(gpu):
    import torch
    name, plain_t, batch = "bfv13_50", 65537, 3
    P, oc, ctx, n, primes, size_p, size_q = _setup(name, 0, gpu)
    ct1, ct2 = _pairs(rng_for(9700), primes, size_q, n, batch)
    d1, d2 = P.to_device(ct1, gpu), P.to_device(ct2, gpu)
    dst = _zeros3(P, batch, size_q, n, gpu)
    poison = dst.clone()

    def refused(fn, *a):
        with pytest.raises(ValueError) as e:
            fn(*a)
        assert str(e.value).strip(), "a refusal carries a message"
        return str(e.value)

    # no plain modulus set
    for variant in VARIANTS:
        assert "plain modulus" in refused(_batched, ctx, variant, d1, d2, dst, size_q)
    ctx.set_plain_modulus(plain_t)
    # size_Ql out of range
    for ql in (0, size_q + 1):
        assert "RNSBase" in refused(ctx.bfv_multiply_hps_overq_batched, ql, d1, d2, dst)
    # null pointers
    for variant in VARIANTS:
        assert "null" in refused(_batched, ctx, variant, None, d2, dst, size_q)
        assert "null" in refused(_batched, ctx, variant, d1, None, dst, size_q)
        assert "null" in refused(_batched, ctx, variant, d1, d2, None, size_q)
    # shapes (the Python layer)
    refused(ctx.bfv_multiply_hps_batched, d1, d2[:2], dst)
    refused(ctx.bfv_multiply_hps_batched, d1, d2, dst[:2])
    refused(ctx.bfv_multiply_behz_batched, d1[0], d2[0], dst[0])
    # dst overlapping an input: one buffer holding [ct | dst] with dst starting inside ct's last ciphertext
    words = 2 * size_q * n
    buf = torch.zeros(batch * words + batch * 3 * size_q * n, dtype=torch.int64, device=gpu)
    inp = buf[:batch * words].view(batch, 2, size_q, n)
    inp.copy_(d1)
    over = buf[(batch - 1) * words:(batch - 1) * words + batch * 3 * size_q * n].view(batch, 3, size_q, n)
    for variant in VARIANTS:
        assert "overlap" in refused(_batched, ctx, variant, inp, d2, over, size_q)
        assert "overlap" in refused(_batched, ctx, variant, d1, inp, over, size_q)
    torch.cuda.synchronize()
    assert torch.equal(inp, d1), "a refused call wrote something"
    assert torch.equal(dst, poison), "a refused call wrote something"
    # batch == 0 does nothing: through the Python layer (empty tensors) and through the C entry with live pointers
    for variant in VARIANTS:
        _batched(ctx, variant, d1[:0], d2[:0], dst[:0], size_q)
    stream = torch.cuda.current_stream().cuda_stream
    a, b, c = d1.data_ptr(), d2.data_ptr(), dst.data_ptr()
    assert ctx._L.pha_bfv_multiply_behz_batched(ctx._h, a, b, c, 0, 0, stream) == 0
    assert ctx._L.pha_bfv_multiply_hps_batched(ctx._h, a, b, c, 0, 0, stream) == 0
    assert ctx._L.pha_bfv_multiply_hps_overq_batched(ctx._h, size_q, a, b, c, 0, 0, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, poison)
    # single entries and batched entries on one context, in both orders (the auxiliary table rows are shared, and grow with each
    # variant's first use)
    one = torch.empty((3, size_q, n), dtype=torch.int64, device=gpu)
    ctx.bfv_multiply_hps(d1[0], d2[0], one)                               # single first: builds base R
    _check(P.to_host(one), O.Hps(oc, plain_t).multiply(ct1[0], ct2[0]), "single hps before any batched call")
    for variant in ("overq", "behz", "hps"):                              # batched first for Rl (shared rows) and Bsk (new rows)
        _batched(ctx, variant, d1, d2, dst, size_q)
        orc = _oracle(variant, oc, plain_t)
        got = P.to_host(dst)
        for b in range(batch):
            _check(got[b], orc.multiply(ct1[b], ct2[b]), f"{variant} batched on the shared context", lead=(b,))
        _single(ctx, variant, d1[1], d2[1], one, size_q)
        _check(P.to_host(one), got[1], f"single {variant} after the batched call")
    ctx.bfv_multiply_hps_batched(d1, d2, dst)                             # and hps again after Bsk's rows were appended
    _check_dev(P, dst, _singles(ctx, "hps", d1, d2, size_q), "hps batched after the table rows grew")
    assert np.array_equal(P.to_host(d1), ct1) and np.array_equal(P.to_host(d2), ct2), "the inputs were written to"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# H: strict mode
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_strict_mode_names_the_operand(variant, gpu):
    name, plain_t, batch = "bfv13_50", 65537, 5
    P, oc, ctx, n, primes, size_p, size_q = _setup(name, plain_t, gpu)
    ct1, ct2 = _pairs(rng_for(9800), primes, size_q, n, batch)
    bad2 = ct2.copy()
    bad2[3, 1, size_q - 1, n - 1] = np.uint64(primes[size_q - 1])         # one word == q in ciphertext 3 of 5
    bad1 = ct1.copy()
    bad1[3, 0, 0, 7] = np.uint64(primes[0]) + np.uint64(5)
    d1, d2, db1, db2 = (P.to_device(x, gpu) for x in (ct1, ct2, bad1, bad2))
    dst = _zeros3(P, batch, size_q, n, gpu)
    prev = P.set_strict(True)
    try:
        with pytest.raises(ValueError) as e:
            _batched(ctx, variant, d1, db2, dst, size_q)
        assert "PHA_STRICT" in str(e.value) and "ct2" in str(e.value) and "1 word" in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:
            _batched(ctx, variant, db1, d2, dst, size_q)
        assert "PHA_STRICT" in str(e.value) and "ct1" in str(e.value), str(e.value)
        _batched(ctx, variant, d1, d2, dst, size_q)                       # canonical operands pass
        P.set_strict(False)
        _batched(ctx, variant, d1, db2, dst, size_q)                      # strict off: the call computes
        good = P.to_host(dst)
        for b in (0, 1, 2, 4):                                            # the other ciphertexts do not see ciphertext 3's word
            _check(good[b], _oracle(variant, oc, plain_t).multiply(ct1[b], ct2[b]), f"{variant} strict off", lead=(b,))
    finally:
        P.set_strict(prev)
    del ctx
    _release()
