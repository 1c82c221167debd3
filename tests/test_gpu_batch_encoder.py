"""The BFV / BGV batch encoder on the device (csrc/pha_batch.hip), word for word against tests/batch_restatement.py (which
tests/test_batch_restatement.py pins on the definition of batching).

A. every degree 2^12 .. 2^17 (each has its own tile split: one pass up to 2^14, two passes with 8, 16, 32 rows in the strided pass
   above), counts 1 and 3, the smallest batching prime of the degree and a 59-bit one: encode, both decode forms, the plain transforms,
   the index map, and the fused entries against the composition of the plain transforms and indexing;
B. the width ladder at 2^12 and 2^16.  The kernels have ONE arithmetic form (the integer Harvey butterflies) for every t, so there is
   no switch to straddle; the ladder walks 16, 17, 20, 33, 50, 51 and 59 bits all the same.  At 2^16 no batching prime of 16 or 17
   bits exists (t = 1 mod 2^17 needs 18 bits): those two steps take the smallest batching prime of the degree instead;
C. message shapes: values_size 0, 1, N/2, N - 1, N; padded strides on both sides; a shared message; words with bit 63 set; poisoned
   outputs with the words between strided outputs untouched; both forms of encode and of decode (reached through the hooks of
   phantom_amd_bench.h), and the library's own rule on each side of its switch;
D. semantics on the device: encode -> encrypt -> decrypt -> decode returns the messages (bgv and bfv, t = 65537, the sets
   tests/test_gpu_encrypt.py decrypts exactly); slot-wise product; row rotation and row swap; one K = 3 plaintext-weighted sum;
E. refusals, count == 0, strict mode, graph capture."""
import gc

import numpy as np
import pytest

import batch_restatement as R
from ckks_semantics import Scheme
from encrypt_restatement import Restatement
from oracle import oracle as O
from util import crt_compose, oracle_bfv_plain_sum, rng_for

pytestmark = pytest.mark.gpu

POISON = -0x2152411021524111
POISON_U = np.uint64(POISON & (2 ** 64 - 1))
T = 65537
NOISE = 21


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _ctx(gpu, log_n, t=0, primes=None, size_p=1):
    import phantom_fhe_amd as P
    primes = [int(p) for p in P.coeff_modulus_create(1 << log_n, [60, 60])] if primes is None else [int(p) for p in primes]
    ctx = P.PhantomContext(log_n, primes, size_p, device=gpu)
    if t:
        ctx.set_plain_modulus(t)
    return P, ctx


def _poisoned(shape, gpu):
    import torch
    return torch.full(shape, POISON, dtype=torch.int64, device=gpu)


def _signed(x, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(gpu)


def _messages(seed, count, n, t):
    return rng_for(seed).integers(0, t, (count, n), dtype=np.uint64)


def _encode_all_forms(P, enc, values, size, gpu, rows, count, strides=None, width=None):
    """plaintext buffers ([rows][width], poisoned first) of both encode forms (the permutation kernel, the gather in the first load)
    and of the library's own rule."""
    out = []
    try:
        for mode in (0, 1, -1):
            P.set_batch_encode_path(mode)
            dst = _poisoned((rows, enc.slot_count if width is None else width), gpu)
            enc.encode_batched(values, size, dst, count=count, strides=strides)
            out.append(dst)
    finally:
        P.set_batch_encode_path(-1)
    return out


def _decode_both_forms(P, enc, plain, gpu, count, n):
    """values of both decode forms (the gather kernel, the scatter in the last store) and of the library's own rule."""
    out = []
    try:
        for mode in (0, 1, -1):
            P.set_batch_decode_path(mode)
            dst = _poisoned((count, n), gpu)
            enc.decode_batched(plain, dst, count=count)
            out.append(P.to_host(dst))
    finally:
        P.set_batch_decode_path(-1)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# A: degrees and counts
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(12, 18))
def test_every_degree_counts_one_and_three(log_n, gpu):
    import torch
    n = 1 << log_n
    for t in (R.smallest_batching_prime(log_n), R.batching_prime(log_n, 59)):
        b = R.batch(log_n, t)
        P, ctx = _ctx(gpu, log_n, t)
        enc = P.BatchEncoder(ctx)
        assert enc.slot_count == n
        imap = enc.index_map()
        assert np.array_equal(imap, R.index_map(log_n))
        v = _messages(7000 + log_n, 3, n, t)
        want = np.stack([b.encode(v[k]) for k in range(3)])
        d_v = P.to_device(v, gpu)
        for count in (1, 3):
            for form, dst in zip(("permutation kernel", "gather", "rule"), _encode_all_forms(P, enc, d_v, n, gpu, 3, count)):
                got = P.to_host(dst)
                assert np.array_equal(got[:count], want[:count]), f"encode ({form}) N = 2^{log_n} t = {t} count {count}"
                assert np.all(got[count:] == POISON_U)
            for form, back in zip(("gather kernel", "scatter", "rule"), _decode_both_forms(P, enc, dst, gpu, count, n)):
                assert np.array_equal(back, v[:count]), f"decode ({form}) N = 2^{log_n} t = {t} count {count}"
        # the plain transforms: the reference's launchers over gpu_plain_tables()
        fwd, bwd = d_v.clone(), d_v.clone()
        enc.plain_nwt_forward_inplace_batched(fwd)
        enc.plain_nwt_backward_inplace_batched(bwd)
        assert np.array_equal(P.to_host(fwd), np.stack([b.nwt_forward(v[k]) for k in range(3)]))
        assert np.array_equal(P.to_host(bwd), np.stack([b.nwt_backward(v[k]) for k in range(3)]))
        # the fused entries against the composition: an index permutation as a launch of its own plus the plain entry
        d_map = torch.from_numpy(imap.astype(np.int64)).to(gpu)
        buf = torch.zeros((3, n), dtype=torch.int64, device=gpu)
        buf[:, d_map] = d_v
        enc.plain_nwt_backward_inplace_batched(buf)
        assert np.array_equal(P.to_host(buf), want)
        ntt = P.to_device(want, gpu)
        enc.plain_nwt_forward_inplace_batched(ntt)
        assert np.array_equal(P.to_host(ntt[:, d_map].contiguous()), v)
        del enc, ctx
        _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B: the width ladder
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", sorted(R.LADDER))
@pytest.mark.parametrize("log_n", [12, 16])
def test_width_ladder(log_n, bits, gpu):
    n = 1 << log_n
    t = R.smallest_batching_prime(log_n) if log_n == 16 and bits < 18 else R.batching_prime(log_n, bits)
    assert O.is_prime(t) and (t - 1) % (2 * n) == 0
    b = R.batch(log_n, t)
    P, ctx = _ctx(gpu, log_n, t)
    enc = P.BatchEncoder(ctx)
    v = _messages(7100 + bits, 2, n, t)
    v[0, :4] = [0, 1, t - 1, t // 2]
    size = n - 5
    dst = _poisoned((2, n), gpu)
    enc.encode_batched(P.to_device(v, gpu), size, dst)
    got = P.to_host(dst)
    assert np.array_equal(got, np.stack([b.encode(v[k, :size]) for k in range(2)])), f"encode t = {t} ({bits} bits)"
    assert int(got.max()) < t
    padded = v.copy()
    padded[:, size:] = 0
    for form, back in zip(("gather kernel", "scatter", "rule"), _decode_both_forms(P, enc, dst, gpu, 2, n)):
        assert np.array_equal(back, padded), f"decode ({form}) t = {t} ({bits} bits)"
    del enc, ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C: message shapes
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [12, 15])
def test_message_shapes(log_n, gpu):
    n, t = 1 << log_n, T
    b = R.batch(log_n, t)
    P, ctx = _ctx(gpu, log_n, t)
    enc = P.BatchEncoder(ctx)
    count, vpad, dpad = 3, 7, 11
    small = rng_for(7200 + log_n).integers(-(t - 1), t, (count, n))      # negative words: bit 63 set, the sign rule
    small[0, :3] = [-1, -(t - 1), t - 1]
    want_v = np.mod(small, t).astype(np.uint64)
    vs, ds = n + vpad, n + dpad
    d_v = _poisoned((count * vs,), gpu)
    for k in range(count):
        d_v[k * vs:k * vs + n] = _signed(small[k], gpu)
    for size in (0, 1, n // 2, n - 1, n):
        want = np.stack([b.encode(want_v[k, :size]) for k in range(count)])
        for form, dst in zip(("permutation kernel", "gather", "rule"),
                             _encode_all_forms(P, enc, d_v, size, gpu, count, count, strides=(vs, ds), width=ds)):
            got = P.to_host(dst)
            assert np.array_equal(got[:, :n], want), f"encode ({form}) values_size {size}"
            assert np.all(got[:, n:] == POISON_U), "the words between strided plaintexts were written to"
            assert int(got[:, :n].max()) < t
        assert np.array_equal(got[:, :n], np.stack([b.encode(small[k, :size]) for k in range(count)]))   # the restatement's own sign rule
        # decode into a padded buffer, both forms
        padded = want_v.copy()
        padded[:, size:] = 0
        try:
            for mode in (0, 1):
                P.set_batch_decode_path(mode)
                out = _poisoned((count * vs,), gpu)
                enc.decode_batched(dst, out, count=count, strides=(ds, vs))
                back = P.to_host(out).reshape(count, vs)
                assert np.array_equal(back[:, :n], padded), f"decode form {mode} values_size {size}"
                assert np.all(back[:, n:] == POISON_U), "the words between strided messages were written to"
        finally:
            P.set_batch_decode_path(-1)
    assert np.all(P.to_host(d_v).reshape(count, vs)[:, n:] == POISON_U) and np.array_equal(P.to_host(d_v).reshape(count, vs)[:, :n].view(np.int64), small)
    # values_stride == 0 shares one message
    dst = _poisoned((count, n), gpu)
    enc.encode_batched(d_v, n, dst, count=count, strides=(0, n))
    assert np.array_equal(P.to_host(dst), np.stack([b.encode(want_v[0])] * count))
    # values_size == 0 without a message
    dst = _poisoned((2, n), gpu)
    enc.encode_batched(None, 0, dst)
    assert not P.to_host(dst).any()
    del enc, ctx
    _release()


def test_both_sides_of_the_dispatch_rules(gpu):
    """The library's own rule on each side of its switch at N = 2^15 (two passes): from 2^20 words per call on (count 32) encode
    takes the permutation kernel and decode the gather kernel.  One message shared by the batch (encode: values_stride 0), so one
    reference serves every row; the sentinel row behind the batch stays untouched."""
    log_n, n, t = 15, 1 << 15, T
    b = R.batch(log_n, t)
    P, ctx = _ctx(gpu, log_n, t)
    enc = P.BatchEncoder(ctx)
    v = _messages(7250, 1, n, t)
    want = b.encode(v[0])
    d_v = P.to_device(v, gpu)
    for count in (31, 32):
        dst = _poisoned((count + 1, n), gpu)
        enc.encode_batched(d_v, n, dst, count=count, strides=(0, n))
        got = P.to_host(dst)
        assert np.all(got[:count] == want[None, :]), f"encode count {count}"
        assert np.all(got[count] == POISON_U)
    for count in (31, 32):
        out = _poisoned((count + 1, n), gpu)
        enc.decode_batched(dst[:count], out, count=count)
        back = P.to_host(out)
        assert np.all(back[:count] == v[0][None, :]), f"decode count {count}"
        assert np.all(back[count] == POISON_U)
    del enc, ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: semantics on the device
# ------------------------------------------------------------------------------------------------------------------------------
def _kind(P, scheme):
    return {O.BGV: P.scheme_type.bgv, O.BFV: P.scheme_type.bfv}[scheme]


@pytest.mark.parametrize("scheme,name,level", [(O.BGV, "hyb12_a2", 6), (O.BGV, "hyb12_a2", 2), (O.BFV, "c1_bfv4096", 2), (O.BFV, "bfv13_50", 4)],
                         ids=["bgv6", "bgv2", "bfv-c1", "bfv13"])
def test_encode_encrypt_decrypt_decode_returns_the_messages(scheme, name, level, gpu):
    from phantom_fhe_amd import workloads as W
    sch = Scheme(name, seed=27)
    assert (T - 1) % (2 * sch.n) == 0
    P, ctx = _ctx(gpu, sch.log_n, T, primes=sch.primes, size_p=sch.size_p)
    enc = P.BatchEncoder(ctx)
    batch, n = 5, sch.n
    rng = rng_for(7300 + level)
    a = np.stack([np.stack([rng.integers(0, int(sch.primes[r]), n, dtype=np.uint64) for r in range(level)]) for _ in range(batch)])
    e = rng.integers(-NOISE, NOISE + 1, (batch, n))
    msgs = rng.integers(-(T - 1), T, (batch, n - 9))                     # short, with negative words
    d_sk = P.to_device(sch.sk_ntt, gpu)
    cts = W.batch_encode_encrypt(ctx, enc, _signed(msgs, gpu), level, d_sk, (P.to_device(a, gpu), _signed(e, gpu)), _kind(P, scheme))
    assert tuple(cts.shape) == (batch, 2, level, n)
    got = P.to_host(W.batch_decrypt_decode(ctx, enc, cts, level, ctx.secret_key_powers(d_sk, 1), _kind(P, scheme)))
    want = np.zeros((batch, n), dtype=np.uint64)
    want[:, :n - 9] = np.mod(msgs, T)
    assert np.array_equal(got, want), f"{name} level {level}: the round trip does not return the messages in every slot"
    del enc, ctx
    _release()


def test_slotwise_product_rotation_and_swap(gpu):
    import torch
    log_n, n, t = 12, 4096, T
    P, ctx = _ctx(gpu, log_n, t)
    enc = P.BatchEncoder(ctx)
    v = _messages(7400, 2, n, t)
    plain = _poisoned((2, n), gpu)
    enc.encode_batched(P.to_device(v, gpu), n, plain)
    # slot-wise product: forward transforms, a torch product modulo t (below 2^34: exact in int64), the inverse transform
    ntt = plain.clone()
    enc.plain_nwt_forward_inplace_batched(ntt)
    prod = torch.remainder(ntt[0] * ntt[1], t).contiguous()
    enc.plain_nwt_backward_inplace_batched(prod)
    out = _poisoned((n,), gpu)
    enc.decode_batched(prod, out)
    assert np.array_equal(P.to_host(out), (v[0] * v[1]) % np.uint64(t))
    # the Galois automorphisms on a plaintext: a context whose first limb IS t negates modulo t
    other = int(P.coeff_modulus_create(n, [60])[0])
    _, gctx = _ctx(gpu, log_n, 0, primes=[t, other], size_p=1)
    rows = v[0].reshape(2, n // 2)
    for elt, want in [(pow(5, s, 2 * n), np.roll(rows, -s, axis=1)) for s in (1, 3, n // 2 - 1)] + [(2 * n - 1, rows[::-1])]:
        rot = _poisoned((n,), gpu)
        gctx.apply_galois(plain[0], rot, elt, 1, 0)
        out = _poisoned((n,), gpu)
        enc.decode_batched(rot, out)
        assert np.array_equal(P.to_host(out).reshape(2, n // 2), want), f"galois element {elt}"
    del enc, ctx, gctx
    _release()


def test_weighted_sum_of_three_through_the_bfv_inner_product(gpu):
    """res = sum_k w_k * ct_k (pha_bfv_plain_inner_product_batched) on encoder-made weights decrypts to sum_k w_k o a_k mod t slot by
    slot.  The oracle composition of the same case (the restated encryptions, the oracle's multiply_plain and add) is decrypted
    exactly on the CPU first, so the case is known to be inside the noise budget."""
    name, level, K = "c1_bfv4096", 2, 3
    sch = Scheme(name, seed=27)
    n = sch.n
    b = R.batch(sch.log_n, T)
    rng = rng_for(7500)
    w, msg = _messages(7501, K, n, T), _messages(7502, K, n, T)
    a = np.stack([np.stack([rng.integers(0, int(sch.primes[r]), n, dtype=np.uint64) for r in range(level)]) for _ in range(K)])
    e = rng.integers(-NOISE, NOISE + 1, (K, n))
    want = np.zeros(n, dtype=np.uint64)
    for k in range(K):
        want = (want + w[k] * msg[k]) % np.uint64(T)
    # the CPU composition decrypts exactly
    w_plain = np.stack([b.encode(w[k]) for k in range(K)])
    m_plain = np.stack([b.encode(msg[k]) for k in range(K)])
    r = Restatement(sch.oc, O.BFV, T)
    cpu_cts = np.stack([r.symmetric(sch.sk_ntt, a[k], e[k], m_plain[k], level) for k in range(K)])
    cpu_sum = oracle_bfv_plain_sum(sch.oc, w_plain, cpu_cts, level, T)
    oc, q = sch.oc, [int(p) for p in sch.primes[:level]]
    big_q = q[0] * q[1]
    c1s = oc.nwt_backward(oc.multiply(oc.nwt_forward(cpu_sum[1], level, 0), sch.sk_ntt[:level], level), level)
    phase = oc.add(cpu_sum[0], c1s, level)
    cpu_plain = np.array([((crt_compose([phase[l, j] for l in range(level)], q)[0] * T + big_q // 2) // big_q) % T for j in range(n)],
                         dtype=np.uint64)
    assert np.array_equal(b.decode(cpu_plain), want), "the oracle composition of this case does not decrypt exactly"
    # the device pipeline
    from phantom_fhe_amd import workloads as W
    P, ctx = _ctx(gpu, sch.log_n, T, primes=sch.primes, size_p=sch.size_p)
    enc = P.BatchEncoder(ctx)
    d_sk = P.to_device(sch.sk_ntt, gpu)
    cts = W.batch_encode_encrypt(ctx, enc, P.to_device(msg, gpu), level, d_sk, (P.to_device(a, gpu), _signed(e, gpu)), P.scheme_type.bfv)
    d_w = _poisoned((K, n), gpu)
    enc.encode_batched(P.to_device(w, gpu), n, d_w)
    assert np.array_equal(P.to_host(d_w), w_plain)
    res = _poisoned((1, 2, level, n), gpu)
    ctx.bfv_plain_inner_product_batched(level, d_w, cts, None, res, K, 1)
    got = P.to_host(W.batch_decrypt_decode(ctx, enc, res, level, ctx.secret_key_powers(d_sk, 1), P.scheme_type.bfv))[0]
    assert np.array_equal(got, want)
    del enc, ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# E: refusals and modes
# ------------------------------------------------------------------------------------------------------------------------------
def _refused(exc, text, fn, *args, **kw):
    with pytest.raises(exc) as err:
        fn(*args, **kw)
    assert text in str(err.value), str(err.value)


def test_refusals_and_empty_batch(gpu):
    log_n, n = 12, 4096
    P, bare = _ctx(gpu, log_n)
    _refused(ValueError, "plain modulus", P.BatchEncoder, bare)
    for bad_t in (65536, 65521, 8193):                 # a power of two; a prime that is not 1 mod 2N; a composite (3 * 2731) that is
        bare.set_plain_modulus(bad_t)
        _refused(ValueError, "encryption parameters are not valid for batching", P.BatchEncoder, bare)
    P, ctx = _ctx(gpu, log_n, T)
    enc = P.BatchEncoder(ctx)
    v, dst = P.to_device(_messages(7600, 2, n + 8, T), gpu), _poisoned((2, n), gpu)
    _refused(ArithmeticError, "values_matrix size is too large", enc.encode_batched, v, n + 1, dst)
    _refused(ValueError, "dst stride below N", enc.encode_batched, v, n, dst, count=2, strides=(n, n - 1))
    _refused(ValueError, "values stride below values_size", enc.encode_batched, v, n, dst, count=2, strides=(n - 1, n))
    _refused(ValueError, "null device pointer", enc.encode_batched, v, n, None, count=1)
    _refused(ValueError, "overlaps", enc.decode_batched, dst, dst, count=1)
    _refused(ValueError, "count out of range", enc.encode_batched, v, n, dst, count=65536, strides=(0, n))
    # count == 0 is a no-op
    enc.encode_batched(v, n, dst, count=0)
    enc.decode_batched(dst, dst, count=0)
    enc.plain_nwt_forward_inplace_batched(dst, count=0)
    enc.plain_nwt_backward_inplace_batched(dst, count=0)
    assert np.all(P.to_host(dst) == POISON_U), "a refused or empty call wrote to dst"
    # a changed plain modulus: every later call refuses; putting it back revives the encoder
    ctx.set_plain_modulus(40961)
    for call in (lambda: enc.encode_batched(v, n, dst), lambda: enc.decode_batched(v, dst), lambda: enc.plain_nwt_forward_inplace_batched(dst),
                 lambda: enc.plain_nwt_backward_inplace_batched(dst)):
        _refused(ValueError, "plain modulus has changed", call)
    assert np.all(P.to_host(dst) == POISON_U)
    ctx.set_plain_modulus(T)
    enc.encode_batched(v, n, dst, count=2, strides=(n + 8, n))
    assert int(P.to_host(dst).max()) < T
    del enc, ctx, bare
    _release()


def test_strict_mode_names_the_operand(gpu):
    log_n, n = 12, 4096
    P, ctx = _ctx(gpu, log_n, T)
    enc = P.BatchEncoder(ctx)
    v = _messages(7700, 2, n, T)
    good, dst = P.to_device(v, gpu), _poisoned((2, n), gpu)
    bad = v.copy()
    bad[1, 5], bad[0, 9] = T, 2 ** 64 - T - 1            # t itself; a negative word whose magnitude is above t
    neg = v.copy()
    neg[0, 3] = 2 ** 64 - 1                              # -1: inside the precondition
    was = P.set_strict(True)
    try:
        enc.encode_batched(P.to_device(neg, gpu), n, dst)
        _refused(ValueError, "PHA_STRICT: batch_encode values holds 2 word(s)", enc.encode_batched, P.to_device(bad, gpu), n, dst)
        out = _poisoned((2, n), gpu)
        _refused(ValueError, "PHA_STRICT: batch_decode plain holds 2 word(s)", enc.decode_batched, P.to_device(bad, gpu), out)
        assert np.all(P.to_host(out) == POISON_U)
        _refused(ValueError, "PHA_STRICT: plain_nwt_forward plain holds 2 word(s)", enc.plain_nwt_forward_inplace_batched, P.to_device(bad, gpu))
        _refused(ValueError, "PHA_STRICT: plain_nwt_backward plain holds 2 word(s)", enc.plain_nwt_backward_inplace_batched, P.to_device(bad, gpu))
        enc.decode_batched(good, out)                    # canonical operands pass
    finally:
        P.set_strict(was)
    del enc, ctx
    _release()


def test_encode_and_decode_replay_from_a_graph(gpu):
    import torch
    log_n, n, t, count = 15, 1 << 15, T, 3               # two passes: the scratch arena is in play
    b = R.batch(log_n, t)
    P, ctx = _ctx(gpu, log_n, t)
    enc = P.BatchEncoder(ctx)
    v = _messages(7800, 2 * count, n, t)
    d_v, plain, back = P.to_device(v[:count], gpu), _poisoned((count, n), gpu), _poisoned((count, n), gpu)
    stream = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(stream):                      # warm-up on the capture stream: the arena grows, the kernels load
        enc.encode_batched(d_v, n, plain)
        enc.decode_batched(plain, back)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        enc.encode_batched(d_v, n, plain)
        enc.decode_batched(plain, back)
    d_v.copy_(P.to_device(v[count:], gpu))
    plain.fill_(POISON)
    back.fill_(POISON)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(P.to_host(plain), np.stack([b.encode(v[count + k]) for k in range(count)]))
    assert np.array_equal(P.to_host(back), v[count:])
    del graph, enc, ctx
    _release()
