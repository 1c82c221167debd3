"""Decryption on the GPU (pha_secret_key_powers, pha_decrypt_phase_batched, pha_bgv_decrypt_batched, pha_bfv_decrypt_batched and the
two DRNSTool launchers):

A. the secret-key powers and the ckks / bgv phase, word for word against the oracle (oc.add / oc.multiply, the composition of
   Scheme.decrypt): hyb12_a2 (a 60-bit and five 40-bit limbs: both arithmetic forms) at levels 6, 3, 1, cipher_size 2, 3, 4, batch
   1, 5 (one full group and a tail of one), 9, a padded ct stride, dst == ct once; ladder12 at level 14, batch 3;
B. bgv, word for word against oracle phase -> nwt_backward -> exact_convert_array -> the inverse factor mod t in Python, with
   factors [1, 3, t - 1, 1, 2] and chunk 1, 2, 0; genuine encryptions decrypt to m in every coefficient; a non-invertible factor;
C. bfv: genuine size-2 encryptions and their BEHZ / HPS products of size 3 decrypt to m resp. m1 m2 in ALL N coefficients, batch 1,
   5, 9, every chunk the same words; ciphertexts (x, 0) with uniform x against the exact Python value (the margin and cap of
   tests/test_emu_decrypt.py); encryptions of zero give zeros, never t; the single-polynomial launchers give the batched words;
D. refusals, batch == 0, strict mode;
E. workloads.decrypt_decode_batch equals decode_batched of the oracle's phase bit for bit."""
import gc
from math import prod

import numpy as np
import pytest

from ckks_semantics import Scheme
from oracle import oracle as O
from util import rng_for, uniform_poly

pytestmark = pytest.mark.gpu

POISON = -0x2152411021524111
T = 65537


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _ctx(sch, gpu, plain_t=0):
    import phantom_fhe_amd as P
    ctx = P.PhantomContext(sch.log_n, list(sch.primes), sch.size_p, device=gpu)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    return P, ctx


def _poisoned(shape, gpu):
    import torch
    return torch.full(shape, POISON, dtype=torch.int64, device=gpu)


def _check(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    at = tuple(int(v) for v in np.argwhere(got != ref)[0])
    msg = f"{what}: {int(np.count_nonzero(got != ref))} words differ, first at {at}: got {int(got[at])}, want {int(ref[at])}"
    print(msg)
    raise AssertionError(msg)


def _powers(sch, count, level):
    """s, s^2, ... [count][level][N] from the oracle."""
    s = sch.sk_ntt[:level]
    out = [s]
    for _ in range(count - 1):
        out.append(sch.oc.multiply(out[-1], s, level))
    return out


def _phase(sch, ct, level, with_c0=True):
    """c0 + sum_i c_i s^i of ct [k][level][N] (NTT form), from the oracle; the composition of Scheme.decrypt for any size."""
    oc = sch.oc
    pw = _powers(sch, len(ct) - 1, level)
    out = np.ascontiguousarray(ct[0]) if with_c0 else np.zeros_like(ct[0])
    for i in range(1, len(ct)):
        out = oc.add(out, oc.multiply(ct[i], pw[i - 1], level), level)
    return out


def _uniform_cts(rng, sch, batch, k, level):
    return np.stack([np.stack([uniform_poly(rng, sch.primes[:level], sch.n) for _ in range(k)]) for _ in range(batch)])


# ------------------------------------------------------------------------------------------------------------------------------
# A: powers and phase
# ------------------------------------------------------------------------------------------------------------------------------
def test_secret_key_powers_equal_the_oracle(gpu):
    sch = Scheme("hyb12_a2", seed=11)
    P, ctx = _ctx(sch, gpu)
    d_sk = P.to_device(sch.sk_ntt, gpu)
    got = P.to_host(ctx.secret_key_powers(d_sk, 3))
    want = np.stack(_powers(sch, 3, sch.size_qp))
    _check(got, want, "secret_key_powers")
    assert np.array_equal(P.to_host(d_sk), sch.sk_ntt)
    one = P.to_host(ctx.secret_key_powers(d_sk, 1))
    _check(one, want[:1], "secret_key_powers max_power 1")
    del ctx
    _release()


@pytest.mark.parametrize("level", [6, 3, 1])
def test_phase_word_for_word_hyb12(level, gpu):
    import torch
    sch = Scheme("hyb12_a2", seed=11)
    P, ctx = _ctx(sch, gpu)
    n, ln = sch.n, level * sch.n
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 3)
    rng = rng_for(9400 + level)
    cts = _uniform_cts(rng, sch, 9, 4, level)
    for k in (2, 3, 4):
        ref = np.stack([_phase(sch, cts[b, :k], level) for b in range(9)])
        for batch in (1, 5, 9):
            ct = np.ascontiguousarray(cts[:batch, :k])
            d_ct = P.to_device(ct, gpu)
            dst = _poisoned((batch, level, n), gpu)
            ctx.decrypt_phase_batched(level, d_ct, sk, dst)
            _check(P.to_host(dst), ref[:batch], f"phase level {level} k {k} B {batch}")
            assert np.array_equal(P.to_host(d_ct), ct), "the ciphertexts were written to"
        # a padded ct stride and a padded dst stride (16 words each); the padding stays untouched
        batch, cs, ds = 5, k * ln + 16, ln + 16
        buf = _poisoned((batch * cs,), gpu)
        for b in range(batch):
            buf[b * cs:b * cs + k * ln] = P.to_device(cts[b, :k], gpu).reshape(-1)
        out = _poisoned((batch * ds,), gpu)
        ctx.decrypt_phase_batched(level, buf, sk, out, cipher_size=k, batch=batch, strides=(cs, ds))
        got = P.to_host(out).reshape(batch, ds)
        _check(got[:, :ln].reshape(batch, level, n), ref[:batch], f"phase level {level} k {k} padded strides")
        assert np.all(got[:, ln:] == np.uint64(POISON & (2 ** 64 - 1))), "the padding between results was written to"
    # dst == ct: result b takes c0 (b)'s place, the other polynomials stay
    k, batch = 3, 5
    ct = np.ascontiguousarray(cts[:batch, :k])
    d_ct = P.to_device(ct, gpu)
    ctx.decrypt_phase_batched(level, d_ct, sk, d_ct, strides=(k * ln, k * ln))
    got = P.to_host(d_ct)
    _check(got[:, 0], np.stack([_phase(sch, ct[b], level) for b in range(batch)]), f"phase level {level} in place")
    assert np.array_equal(got[:, 1:], ct[:, 1:])
    del ctx
    _release()


def test_phase_word_for_word_ladder12(gpu):
    sch = Scheme("ladder12", seed=12)
    P, ctx = _ctx(sch, gpu)
    level, batch = 14, 3
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 3)
    cts = _uniform_cts(rng_for(9410), sch, batch, 4, level)
    top = np.array(sch.primes[:level], dtype=np.uint64)[:, None] - 1
    cts[1, :, :, :64] = top                  # q - 1 against the key's words, and zeros
    cts[2, :, :, 64:128] = 0
    for k in (2, 3, 4):
        ct = np.ascontiguousarray(cts[:, :k])
        dst = _poisoned((batch, level, sch.n), gpu)
        ctx.decrypt_phase_batched(level, P.to_device(ct, gpu), sk, dst)
        ref = np.stack([_phase(sch, ct[b], level) for b in range(batch)])
        from util import first_diff_limb
        first_diff_limb(P.to_host(dst), ref, f"phase ladder12 k {k}", sch.primes)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B: bgv
# ------------------------------------------------------------------------------------------------------------------------------
def _bgv_ref(sch, ct, level, t, factor):
    coeff = sch.oc.nwt_backward(_phase(sch, ct, level), level)
    out = O.exact_convert_array(sch.primes[:level], t, coeff, sch.n)
    if factor != 1:
        inv = pow(int(factor), -1, t)
        out = np.array([int(v) * inv % t for v in out], dtype=np.uint64)
    return out


@pytest.mark.parametrize("level", [6, 2])
def test_bgv_word_for_word(level, gpu):
    sch = Scheme("hyb12_a2", seed=13)
    P, ctx = _ctx(sch, gpu, T)
    batch, factors = 5, [1, 3, T - 1, 1, 2]
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    for k in (2, 3):
        cts = _uniform_cts(rng_for(9420 + 10 * level + k), sch, batch, k, level)
        d_ct = P.to_device(cts, gpu)
        ref = np.stack([_bgv_ref(sch, cts[b], level, T, factors[b]) for b in range(batch)])
        for chunk in (1, 2, 0):
            dst = _poisoned((batch, sch.n), gpu)
            ctx.bgv_decrypt_batched(level, d_ct, sk, dst, correction_factors=factors, chunk=chunk)
            _check(P.to_host(dst), ref, f"bgv level {level} k {k} chunk {chunk}")
        dst = _poisoned((batch, sch.n), gpu)
        ctx.bgv_decrypt_batched(level, d_ct, sk, dst)         # no factors: all 1
        _check(P.to_host(dst), np.stack([_bgv_ref(sch, cts[b], level, T, 1) for b in range(batch)]), f"bgv level {level} k {k} no factors")
        assert np.array_equal(P.to_host(d_ct), cts), "the ciphertexts were written to"
    del ctx
    _release()


def test_bgv_genuine_encryptions_and_factor_refusal(gpu):
    sch = Scheme("hyb12_a2", seed=13)
    P, ctx = _ctx(sch, gpu, T)
    oc, level, batch, factors = sch.oc, 6, 5, [1, 3, T - 1, 1, 2]
    q = sch.primes[:level]
    rng = rng_for(9440)
    m = rng.integers(0, T, (batch, sch.n))
    cts = []
    for b in range(batch):      # c0 + c1 s = f m + t e: the decryption multiplies by f^-1
        small = (m[b] * factors[b]) % T + T * rng.integers(-3, 4, sch.n)
        c1 = sch._uniform(rng, q)
        c0 = oc.sub(sch._ntt(sch._residues(small, q), level), oc.multiply(c1, sch.sk_ntt[:level], level), level)
        cts.append(np.stack([c0, c1]))
    d_ct = P.to_device(np.stack(cts), gpu)
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 1)
    dst = _poisoned((batch, sch.n), gpu)
    ctx.bgv_decrypt_batched(level, d_ct, sk, dst, correction_factors=factors)
    _check(P.to_host(dst), m.astype(np.uint64), "bgv genuine encryptions")
    # a factor that is not invertible mod t: status -2, nothing written
    ctx.set_plain_modulus(65536 * 3)                         # composite: 3 and every even factor are not invertible
    dst = _poisoned((batch, sch.n), gpu)
    with pytest.raises(ArithmeticError) as e:
        ctx.bgv_decrypt_batched(level, d_ct, sk, dst, correction_factors=[1, 1, 1, 1, 6])
    assert "invalid correction factor" in str(e.value)
    assert bool((dst == POISON).all()), "something was launched before the refusal"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C: bfv
# ------------------------------------------------------------------------------------------------------------------------------
class Bfv:
    """Genuine encryptions (as BfvConfig4.encrypt) at any level: c0 + c1 s = floor(Q_l / t) m + e over q_0 .. q_{level-1}."""

    def __init__(self, name, level, t, seed=7):
        self.sch, self.level, self.t = Scheme(name, seed=seed), level, t
        self.q = [int(p) for p in self.sch.primes[:level]]
        self.big_q = prod(self.q)

    def encrypt(self, m, tag):
        sch, oc, L = self.sch, self.sch.oc, self.level
        rng = sch._rng("bfv.enc", tag)
        a = sch._uniform(rng, self.q)
        e = rng.integers(-3, 4, sch.n)
        delta = self.big_q // self.t
        dm = np.stack([np.array([(delta % p * int(v) + int(ev)) % p for v, ev in zip(m, e)], dtype=np.uint64) for p in self.q])
        a_s = oc.nwt_backward(oc.multiply(oc.nwt_forward(a, L, 0), sch.sk_ntt[:L], L), L)
        return np.stack([oc.sub(dm, a_s, L), a])

    def product(self, a, b):
        """(m_a m_b) mod (X^N + 1, t): the negacyclic schoolbook product in exact int64 (|sums| < N t^2 < 2^47)."""
        n = self.sch.n
        a, b = a.astype(np.int64), b.astype(np.int64)
        out = np.zeros(n, dtype=np.int64)
        for i in range(n):
            out[i:] += a[i] * b[:n - i]
            out[:i] -= a[i] * b[n - i:]
        return np.mod(out, self.t).astype(np.uint64)


def _bfv_all_chunks(ctx, P, level, d_ct, sk, batch, n, gpu, what, want):
    first = None
    for chunk in (0, 1, 2):
        dst = _poisoned((batch, n), gpu)
        ctx.bfv_decrypt_batched(level, d_ct, sk, dst, chunk=chunk)
        got = P.to_host(dst)
        _check(got, want, f"{what} chunk {chunk}")
        first = got if first is None else first
        assert np.array_equal(got, first)


@pytest.mark.parametrize("name,level", [("c1_bfv4096", 2), ("bfv13_50", 4), ("bfv13_50", 2)])
def test_bfv_genuine_encryptions_every_coefficient(name, level, gpu):
    kit = Bfv(name, level, T)
    sch = kit.sch
    P, ctx = _ctx(sch, gpu, T)
    n = sch.n
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    m = sch._rng("bfv.m").integers(0, T, (9, n))
    cts = np.stack([kit.encrypt(m[b], b) for b in range(9)])
    d_all = P.to_device(cts, gpu)
    for batch in (1, 5, 9):
        d_ct = d_all[:batch].contiguous()
        _bfv_all_chunks(ctx, P, level, d_ct, sk, batch, n, gpu, f"bfv {name} level {level} size 2 B {batch}", m[:batch].astype(np.uint64))
    assert np.array_equal(P.to_host(d_all), cts), "the ciphertexts were written to"
    if level == sch.size_q:     # the size-3 products of the existing entries, at the top level
        import torch
        d_rot = torch.roll(d_all, -1, 0).contiguous()
        want = np.stack([kit.product(m[b], m[(b + 1) % 9]) for b in range(9)])
        multiplies = [ctx.bfv_multiply_behz_batched, ctx.bfv_multiply_hps_batched] if name == "c1_bfv4096" else [ctx.bfv_multiply_hps_batched]
        for mul in multiplies:
            d3 = _poisoned((9, 3, level, n), gpu)
            mul(d_all, d_rot, d3, 0)
            for batch in (1, 5, 9):
                _bfv_all_chunks(ctx, P, level, d3[:batch].contiguous(), sk, batch, n, gpu,
                                f"bfv {name} {mul.__name__} size 3 B {batch}", want[:batch])
    del ctx
    _release()


def test_bfv_scale_round_against_exact_values_ladder12(gpu):
    """Ciphertexts (x, 0): the phase is x itself.  ladder12 at level 14 (limbs of 41 .. 60 bits, the 30-bit split), t = 65537."""
    sch = Scheme("ladder12", seed=12)
    P, ctx = _ctx(sch, gpu, T)
    level, batch, n = 14, 2, sch.n
    q = [int(p) for p in sch.primes[:level]]
    Q = prod(q)
    x = np.stack([uniform_poly(rng_for(9450 + b), q, n) for b in range(batch)])
    cts = np.zeros((batch, 2, level, n), dtype=np.uint64)
    cts[:, 0] = x
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 1)
    dst = _poisoned((batch, n), gpu)
    ctx.bfv_decrypt_batched(level, P.to_device(cts, gpu), sk, dst)
    got = P.to_host(dst)
    assert int(got.max()) < T
    w = [(Q // p) * pow(Q // p, -1, p) for p in q]
    for b in range(batch):
        cols = [[int(v) for v in x[b, i]] for i in range(level)]
        excluded, bad = 0, []
        for j in range(n):
            v = sum(c[j] * wi for c, wi in zip(cols, w)) % Q
            r = T * v % Q
            if abs(2 * r - Q) * (1 << 14) < 2 * level * Q:         # |frac(t x / Q) - 1/2| < L * 2^-14
                excluded += 1
                continue
            want = (2 * T * v + Q) // (2 * Q) % T
            if int(got[b, j]) != want:
                bad.append((j, int(got[b, j]), want))
        print(f"ciphertext {b}: {excluded} of {n} coefficients excluded")
        assert excluded * 100 <= n, f"{excluded} of {n} coefficients inside the margin: more than 1 %"
        assert not bad, f"{len(bad)} coefficients differ outside the margin, first (index, got, want): {bad[:3]}"
    # the DRNSTool launcher on one polynomial gives the batched entry's words
    one = _poisoned((n,), gpu)
    ctx.hps_decrypt_scale_and_round(level, one, P.to_device(x[1], gpu))
    _check(P.to_host(one), got[1], "hps_decrypt_scale_and_round")
    del ctx
    _release()


def test_bfv_zero_decrypts_to_zero_never_t(gpu):
    kit = Bfv("c1_bfv4096", 2, T)
    sch = kit.sch
    P, ctx = _ctx(sch, gpu, T)
    batch, n = 3, sch.n
    cts = np.stack([kit.encrypt(np.zeros(n, dtype=np.int64), 100 + b) for b in range(batch)])   # noise of both signs
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 1)
    dst = _poisoned((batch, n), gpu)
    ctx.bfv_decrypt_batched(2, P.to_device(cts, gpu), sk, dst)
    got = P.to_host(dst)
    assert not np.any(got == T), "a word equal to t was written"
    assert not np.any(got), "an encryption of zero decrypted to a non-zero word"
    del ctx
    _release()


def test_decrypt_mod_t_gives_the_batched_words(gpu):
    sch = Scheme("hyb12_a2", seed=13)
    P, ctx = _ctx(sch, gpu, T)
    level, n = 6, sch.n
    x = uniform_poly(rng_for(9460), sch.primes[:level], n)             # coefficient form
    cts = np.zeros((1, 2, level, n), dtype=np.uint64)
    cts[0, 0] = sch.oc.nwt_forward(x, level, 0)                        # the phase of (NTT(x), 0) is x
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 1)
    dst = _poisoned((1, n), gpu)
    ctx.bgv_decrypt_batched(level, P.to_device(cts, gpu), sk, dst)
    one = _poisoned((n,), gpu)
    ctx.decrypt_mod_t(level, one, P.to_device(x, gpu))
    _check(P.to_host(one), P.to_host(dst)[0], "decrypt_mod_t")
    _check(P.to_host(one), O.exact_convert_array(sch.primes[:level], T, x, n), "decrypt_mod_t against the oracle")
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: refusals, batch == 0, strict mode
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_batch(gpu):
    import torch
    sch = Scheme("hyb12_a2", seed=13)
    P, ctx = _ctx(sch, gpu, T)
    _, bare = _ctx(sch, gpu)                                              # no plain modulus
    level, k, batch, n = 3, 3, 2, sch.n
    ln = level * n
    ct = P.to_device(_uniform_cts(rng_for(9470), sch, batch, k, level), gpu)
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    big = _poisoned((batch * k * ln + 64,), gpu)

    def entries(c=ctx):
        """(name, call(ct, sk, dst, **kw), words of one result)"""
        return [("phase", lambda a, s, d, **kw: c.decrypt_phase_batched(level, a, s, d, **kw), ln),
                ("bgv", lambda a, s, d, **kw: c.bgv_decrypt_batched(level, a, s, d, **kw), n),
                ("bfv", lambda a, s, d, **kw: c.bfv_decrypt_batched(level, a, s, d, **kw), n)]

    def refused(call, text, *args, **kw):
        with pytest.raises(ValueError) as e:
            call(*args, **kw)
        assert text in str(e.value), str(e.value)

    for name, call, words in entries():
        dst = _poisoned((batch, words), gpu)
        shape = dict(cipher_size=k, batch=batch, n_powers=2)
        refused(call, "null", None, sk, dst, **shape)
        refused(call, "null", ct, None, dst, **shape)
        refused(call, "null", ct, sk, None, **shape)
        refused(call, "cipher_size", ct, sk, dst, cipher_size=1, batch=batch, n_powers=2)
        refused(call, "fewer powers", ct, sk, dst, cipher_size=k, batch=batch, n_powers=1)
        refused(call, "ct stride", ct, sk, dst, strides=(k * ln - 2, words))
        refused(call, "dst stride", ct, sk, dst, strides=(k * ln, words - 2))
        refused(call, "even", ct, sk, dst, strides=(k * ln + 1, words))
        refused(call, "even", ct, sk, dst, strides=(k * ln, words + 1))
        refused(call, "aligned", big[1:1 + batch * k * ln], sk, dst, **shape)
        refused(call, "aligned", ct, sk, big[1:1 + batch * words], **shape)
        refused(call, "overlap sk_powers", ct, sk, sk.reshape(-1)[:batch * words], **shape)
        refused(call, "overlap ct", ct, sk, ct.reshape(-1)[2 * n:2 * n + batch * words], **shape)
        assert bool((dst == POISON).all()), f"{name}: a refused call wrote to dst"
        call(ct, sk, dst, cipher_size=k, batch=0, n_powers=2)              # batch == 0 does nothing
        assert bool((dst == POISON).all()), f"{name}: batch == 0 wrote to dst"
    # size_Ql out of range
    dst = _poisoned((batch, ln), gpu)
    for bad_level in (0, sch.size_q + 1):
        with pytest.raises(ValueError) as e:
            ctx.decrypt_phase_batched(bad_level, ct, sk, dst, cipher_size=k, batch=batch, strides=(k * ln, ln))
        assert "RNSBase is invalid" in str(e.value)
    # dst == ct is the phase entry's alone (and needs the ciphertexts' own stride)
    with pytest.raises(ValueError) as e:
        ctx.decrypt_phase_batched(level, ct, sk, ct, strides=(k * ln, ln))
    assert "overlap ct" in str(e.value)
    for name, call, words in entries()[1:]:
        refused(call, "overlap ct", ct, sk, ct, strides=(k * ln, k * ln))
    # no plain modulus: the bgv / bfv entries and the two launchers
    for name, call, words in entries(bare)[1:]:
        refused(call, "plain modulus", ct, sk, _poisoned((batch, words), gpu))
    one = _poisoned((n,), gpu)
    for fn in (bare.hps_decrypt_scale_and_round, bare.decrypt_mod_t):
        with pytest.raises(ValueError) as e:
            fn(level, one, ct[0, 0])
        assert "plain modulus" in str(e.value)
    with pytest.raises(ValueError):
        ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 0, out=torch.empty((1, sch.size_qp, n), dtype=torch.int64, device=gpu))
    torch.cuda.synchronize()
    del ctx, bare
    _release()


def test_strict_mode_names_the_operand(gpu):
    sch = Scheme("hyb12_a2", seed=13)
    P, ctx = _ctx(sch, gpu, T)
    level, k, batch, n = 3, 3, 5, sch.n
    cts = _uniform_cts(rng_for(9480), sch, batch, k, level)
    bad = cts.copy()
    bad[3, 2, level - 1, n - 1] = np.uint64(sch.primes[level - 1])        # one word == q in ciphertext 3 of 5
    d_ct, d_bad = P.to_device(cts, gpu), P.to_device(bad, gpu)
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 2)
    bad_sk = sk.clone()
    bad_sk[1, 0, 5] = int(sch.primes[0]) + 1
    calls = [("decrypt_phase", lambda a, s: ctx.decrypt_phase_batched(level, a, s, _poisoned((batch, level, n), gpu))),
             ("bgv_decrypt", lambda a, s: ctx.bgv_decrypt_batched(level, a, s, _poisoned((batch, n), gpu))),
             ("bfv_decrypt", lambda a, s: ctx.bfv_decrypt_batched(level, a, s, _poisoned((batch, n), gpu)))]
    prev = P.set_strict(True)
    try:
        for entry, call in calls:
            with pytest.raises(ValueError) as e:
                call(d_bad, sk)
            assert "PHA_STRICT" in str(e.value) and entry + " ct" in str(e.value) and "1 word" in str(e.value), str(e.value)
            with pytest.raises(ValueError) as e:
                call(d_ct, bad_sk)
            assert "PHA_STRICT" in str(e.value) and entry + " sk_powers" in str(e.value), str(e.value)
            call(d_ct, sk)                                                 # canonical operands pass
        P.set_strict(False)
        calls[0][1](d_bad, sk)                                             # strict off: the call computes
    finally:
        P.set_strict(prev)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# E: decrypt -> decode on the device
# ------------------------------------------------------------------------------------------------------------------------------
def test_decrypt_decode_batch_equals_decode_of_the_oracle_phase(gpu):
    import torch
    from phantom_fhe_amd import workloads as W
    sch = Scheme("hyb12_a2", seed=11)
    P, ctx = _ctx(sch, gpu)
    enc = ctx.ckks_encoder()
    level, batch, scale = 3, 5, 2.0 ** 40
    cts = _uniform_cts(rng_for(9490), sch, batch, 2, level)
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 1)
    got = W.decrypt_decode_batch(ctx, enc, P.to_device(cts, gpu), level, scale, sk)
    phase = np.stack([sch.decrypt(cts[b], level) for b in range(batch)])
    want = torch.empty((batch, enc.slot_count), dtype=torch.complex128, device=gpu)
    enc.decode_batched(level, P.to_device(phase, gpu), scale, want)
    assert got.shape == want.shape
    assert torch.equal(torch.view_as_real(got).view(torch.int64), torch.view_as_real(want).view(torch.int64)), "bits differ"
    assert bool(torch.isfinite(torch.view_as_real(got)).all())
    del enc, ctx
    _release()
