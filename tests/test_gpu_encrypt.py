"""Encryption on the GPU (pha_encrypt_zero_symmetric_batched, pha_public_key_generate, pha_encrypt_symmetric_batched,
pha_encrypt_asymmetric_batched), word for word against tests/encrypt_restatement.py (the reference's sequences as oracle steps):

A. symmetric, ckks and bgv (t = 65537): hyb12_a2 at levels 6, 3, 1 with count 1, 5, 9, a padded ct and e stride, one shared plaintext
   (the one-pass plan, both arithmetic back ends); hyb13_a3 level 9 count 2 (18 limb-polynomials: two passes at 2^13, prologue and
   epilogue in different kernels) and count 8 (72: the one-workgroup plan of 2^13, both in one kernel; the zero encryption with the
   special rows at that size too); hyb14_a4 level 8 count 3; c3_ckks16 level 2 count 2; hyb17_a2 level 4 count 1; ladder12 level 14 count 3 (every width);
   the zero encryption with and without the special rows, in NTT and in coefficient form;
B. the public key against the restatement on hyb12_a2 and ladder12, equal to the zero encryption at the key level;
C. asymmetric, ckks and bgv: hyb12_a2 at levels 6 and 3, hyb13_a3 at 9, hyb14_a4 at 8, count 1, 5, 9, chunk 1, 2, 0 the same words;
   wide_p20 at the top level (a 20-prime special base through the mod-down);
D. bfv on c1_bfv4096 and bfv13_50, symmetric and asymmetric, count 1, 5, every chunk the same;
E. round trips on the device: encode_encrypt_batch -> decrypt_decode_batch returns the messages (symmetric and public-key), a
   GPU-encrypted pair through tensor product, key switch + rescale, decrypt, decode; bgv / bfv decrypt to m in all N coefficients;
F. refusals with nothing launched, count == 0, strict mode.
Outputs are poisoned first; the inputs other than c1 and the padding between strided results are checked untouched."""
import gc

import numpy as np
import pytest

import ckks_semantics as S
from ckks_semantics import Scheme
from encrypt_restatement import Restatement
from oracle import oracle as O
from util import first_diff_limb, rng_for

pytestmark = pytest.mark.gpu

POISON = -0x2152411021524111
POISON_U = np.uint64(POISON & (2 ** 64 - 1))
T = 65537
NOISE = 21
EXTREMES = [0, 1, -1, NOISE, -NOISE, 1 << 16, -(1 << 16)]


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


def _signed(x, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(gpu)


def _kind(P, scheme):
    return {O.CKKS: P.scheme_type.ckks, O.BGV: P.scheme_type.bgv, O.BFV: P.scheme_type.bfv}[scheme]


def _noise(rng, shape, n, wide=True):
    """Signed samples in the reference's range; the first words of every polynomial walk the extremes of the accepted range."""
    e = rng.integers(-NOISE, NOISE + 1, tuple(shape) + (n,))
    if wide:
        e[..., :len(EXTREMES)] = EXTREMES
    return e


def _uniform(rng, sch, rows):
    return np.stack([rng.integers(0, int(sch.primes[r]), sch.n, dtype=np.uint64) for r in rows])


def _plain(rng, sch, scheme, level, count):
    """ckks: NTT-form words [count][level][N] (any canonical words are a plaintext); bgv / bfv: [count][N] below t."""
    if scheme == O.CKKS:
        return np.stack([_uniform(rng, sch, range(level)) for _ in range(count)])
    return rng.integers(0, T, (count, sch.n)).astype(np.uint64)


def _restatement(sch, scheme):
    return Restatement(sch.oc, scheme, 0 if scheme == O.CKKS else T)


class SymCase:
    """count symmetric encryptions at one level: the inputs and the restated ciphertexts."""

    def __init__(self, sch, scheme, level, count, seed, shared_plain=False):
        rng = rng_for(seed)
        self.sch, self.scheme, self.level, self.count = sch, scheme, level, count
        self.a = np.stack([_uniform(rng, sch, range(level)) for _ in range(count)])
        self.e = _noise(rng, (count,), sch.n)
        self.plain = _plain(rng, sch, scheme, level, 1 if shared_plain else count)
        self.shared = shared_plain
        r = _restatement(sch, scheme)
        self.ref = np.stack([r.symmetric(sch.sk_ntt, self.a[b], self.e[b], self.plain[0 if shared_plain else b], level) for b in range(count)])

    def run(self, P, ctx, gpu, count=None, pad=0):
        """Encrypt the first `count` on the device (ct and e strides padded by `pad` words) and compare everything."""
        sch, level, n = self.sch, self.level, self.sch.n
        B = self.count if count is None else count
        ln = level * n
        cs, es = 2 * ln + pad, n + pad
        pw = self.plain.shape[1] * (n if self.scheme == O.CKKS else 1)
        ct = _poisoned((B * cs,), gpu)
        e = _poisoned((B * es,), gpu)
        for b in range(B):
            ct[b * cs + ln:b * cs + 2 * ln] = P.to_device(self.a[b], gpu).reshape(-1)
            e[b * es:b * es + n] = _signed(self.e[b], gpu)
        d_plain = P.to_device(self.plain[:1 if self.shared else B], gpu)
        d_sk = P.to_device(sch.sk_ntt, gpu)
        ctx.encrypt_symmetric_batched(level, d_sk, e, d_plain, ct, _kind(P, self.scheme), count=B,
                                      strides=(es, 0 if self.shared else pw, cs))
        got = P.to_host(ct).reshape(B, cs)
        what = f"{sch.name} scheme {self.scheme} level {level} count {B} pad {pad}"
        first_diff_limb(got[:, :2 * ln].reshape(B, 2, level, n), self.ref[:B], "symmetric " + what, sch.primes)
        assert np.all(got[:, 2 * ln:] == POISON_U), "the padding between ciphertexts was written to"
        e_back = P.to_host(e).reshape(B, es)
        assert np.array_equal(e_back[:, :n].view(np.int64), self.e[:B]) and np.all(e_back[:, n:] == POISON_U), "the samples were written to"
        assert np.array_equal(P.to_host(d_plain), self.plain[:1 if self.shared else B]), "the plaintexts were written to"
        assert np.array_equal(P.to_host(d_sk), sch.sk_ntt), "the key was written to"


# ------------------------------------------------------------------------------------------------------------------------------
# A: symmetric
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [O.CKKS, O.BGV], ids=["ckks", "bgv"])
@pytest.mark.parametrize("level", [6, 3, 1])
def test_symmetric_word_for_word_hyb12(level, scheme, gpu):
    sch = Scheme("hyb12_a2", seed=21)
    P, ctx = _ctx(sch, gpu, T if scheme != O.CKKS else 0)
    case = SymCase(sch, scheme, level, 9, 9600 + 10 * level + scheme)
    for count in (1, 5, 9):
        case.run(P, ctx, gpu, count)
    case.run(P, ctx, gpu, 5, pad=16)
    SymCase(sch, scheme, level, 5, 9650 + 10 * level + scheme, shared_plain=True).run(P, ctx, gpu)
    del ctx
    _release()


@pytest.mark.parametrize("scheme", [O.CKKS, O.BGV], ids=["ckks", "bgv"])
@pytest.mark.parametrize("name,level,count", [("hyb13_a3", 9, 2), ("hyb13_a3", 9, 8), ("hyb14_a4", 8, 3), ("c3_ckks16", 2, 2), ("hyb17_a2", 4, 1),
                                              ("ladder12", 14, 3)])
def test_symmetric_word_for_word_other_sets(name, level, count, scheme, gpu):
    """Which plan a launch takes (resolve_plan): N = 4096 always the one-workgroup transform; N = 8192 the one-workgroup transform from
    64 limb-polynomials per launch and two passes below.  hyb13_a3 at level 9: count 2 is 18 limb-polynomials -- two passes, the sample
    lift and the epilogue in different kernels; count 8 is 72 -- the one-workgroup N = 8192 kernel with PRO_SMALL and
    EPI_FWD_NEG_MULADD in one.  The other sets (N >= 2^14) always take two passes."""
    sch = Scheme(name, seed=22)
    P, ctx = _ctx(sch, gpu, T if scheme != O.CKKS else 0)
    SymCase(sch, scheme, level, count, 9700 + sch.log_n + scheme).run(P, ctx, gpu)
    del ctx
    _release()


@pytest.mark.parametrize("special", [False, True], ids=["data", "special"])
def test_zero_encryption_word_for_word(special, gpu):
    _zero_case("hyb12_a2", 3, 3, special, ((O.CKKS, True), (O.BGV, True), (O.BFV, False)), 9750, gpu)


def test_zero_encryption_one_workgroup_8192_with_special(gpu):
    """hyb13_a3, level 9, count 8, with the special rows: the data rows are one launch of 72 limb-polynomials (the one-workgroup
    N = 8192 kernel, sample lift and negated mul-add in one), the 3 special rows one of 24 (two passes) -- both plans in one call."""
    _zero_case("hyb13_a3", 9, 8, True, ((O.CKKS, True), (O.BGV, True)), 9760, gpu)


def _zero_case(name, level, count, special, forms, seed, gpu):
    sch = Scheme(name, seed=23)
    n = sch.n
    rows = sch.rows(level, special)
    rn = len(rows) * n
    for scheme, ntt_form in forms:
        P, ctx = _ctx(sch, gpu, T if scheme != O.CKKS else 0)
        rng = rng_for(seed + scheme + int(special))
        a = np.stack([_uniform(rng, sch, rows) for _ in range(count)])
        e = _noise(rng, (count,), n)
        r = _restatement(sch, scheme)
        ref = np.stack([r.zero_symmetric(sch.sk_ntt, a[b], e[b], level, special, ntt_form) for b in range(count)])
        ct = _poisoned((count, 2, len(rows), n), gpu)
        ct[:, 1] = P.to_device(a, gpu)
        d_e = _signed(e, gpu)
        ctx.encrypt_zero_symmetric_batched(level, P.to_device(sch.sk_ntt, gpu), d_e, ct, _kind(P, scheme), with_special=special,
                                           ntt_form=ntt_form)
        first_diff_limb(P.to_host(ct), ref, f"zero encryption scheme {scheme} special {special}", [sch.primes[i] for i in rows])
        assert np.array_equal(P.to_host(d_e).view(np.int64), e)
        assert rn == ref[0, 0].size
        del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B: the public key
# ------------------------------------------------------------------------------------------------------------------------------
def _public_key(P, ctx, sch, scheme, seed, gpu):
    """(pk on the device, pk from the restatement, the key's noise)."""
    rng = rng_for(seed)
    a = _uniform(rng, sch, range(sch.size_qp))
    e = _noise(rng, (), sch.n, wide=False)
    ref = _restatement(sch, scheme).public_key(sch.sk_ntt, a, e)
    pk = _poisoned((2, sch.size_qp, sch.n), gpu)
    pk[1] = P.to_device(a, gpu)
    ctx.public_key_generate(P.to_device(sch.sk_ntt, gpu), _signed(e, gpu), pk, _kind(P, scheme))
    return pk, ref, a, e


@pytest.mark.parametrize("scheme", [O.CKKS, O.BGV], ids=["ckks", "bgv"])
@pytest.mark.parametrize("name", ["hyb12_a2", "ladder12"])
def test_public_key_word_for_word(name, scheme, gpu):
    sch = Scheme(name, seed=24)
    P, ctx = _ctx(sch, gpu, T if scheme != O.CKKS else 0)
    pk, ref, a, e = _public_key(P, ctx, sch, scheme, 9800 + scheme, gpu)
    first_diff_limb(P.to_host(pk), ref, f"public key {name} scheme {scheme}", sch.primes)
    ct = _poisoned((1, 2, sch.size_qp, sch.n), gpu)
    ct[0, 1] = P.to_device(a, gpu)
    ctx.encrypt_zero_symmetric_batched(sch.size_q, P.to_device(sch.sk_ntt, gpu), _signed(e[None], gpu), ct, _kind(P, scheme), with_special=True)
    assert np.array_equal(P.to_host(ct[0]), P.to_host(pk)), "the public key is the zero encryption at the key level"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C, D: asymmetric
# ------------------------------------------------------------------------------------------------------------------------------
def _asymmetric(name, level, scheme, counts, chunks, seed, gpu, pad=0):
    sch = Scheme(name, seed=25)
    P, ctx = _ctx(sch, gpu, T if scheme != O.CKKS else 0)
    n, ln, total = sch.n, level * sch.n, max(counts)
    pk, pk_ref, _, _ = _public_key(P, ctx, sch, scheme, seed, gpu)
    first_diff_limb(P.to_host(pk), pk_ref, f"public key {name}", sch.primes)
    rng = rng_for(seed + 1)
    u = rng.integers(-1, 2, (total, n))
    e = _noise(rng, (total, 2), n)
    plain = _plain(rng, sch, scheme, level, total)
    r = _restatement(sch, scheme)
    ref = np.stack([r.asymmetric(pk_ref, u[b], e[b], plain[b], level) for b in range(total)])
    d_u, d_e, d_plain = _signed(u, gpu), _signed(e, gpu), P.to_device(plain, gpu)
    pw = plain[0].size
    for count in counts:
        for chunk in chunks:
            cs = 2 * ln + pad
            ct = _poisoned((count * cs,), gpu)
            ctx.encrypt_asymmetric_batched(level, pk, d_u, d_e, d_plain, ct, _kind(P, scheme), count=count, strides=(n, 2 * n, pw, cs),
                                           chunk=chunk)
            got = P.to_host(ct).reshape(count, cs)
            first_diff_limb(got[:, :2 * ln].reshape(count, 2, level, n), ref[:count],
                            f"asymmetric {name} scheme {scheme} level {level} count {count} chunk {chunk} pad {pad}", sch.primes)
            assert np.all(got[:, 2 * ln:] == POISON_U), "the padding between ciphertexts was written to"
    assert np.array_equal(P.to_host(pk), pk_ref), "the public key was written to"
    assert np.array_equal(P.to_host(d_u).view(np.int64), u) and np.array_equal(P.to_host(d_e).view(np.int64), e), "the samples were written to"
    assert np.array_equal(P.to_host(d_plain), plain), "the plaintexts were written to"
    del ctx
    _release()


@pytest.mark.parametrize("scheme", [O.CKKS, O.BGV], ids=["ckks", "bgv"])
@pytest.mark.parametrize("name,level", [("hyb12_a2", 6), ("hyb12_a2", 3), ("hyb13_a3", 9), ("hyb14_a4", 8)])
def test_asymmetric_word_for_word(name, level, scheme, gpu):
    _asymmetric(name, level, scheme, (1, 5, 9), (1, 2, 0), 9900 + 10 * level + scheme, gpu)


@pytest.mark.parametrize("scheme", [O.CKKS, O.BGV], ids=["ckks", "bgv"])
def test_asymmetric_padded_stride(scheme, gpu):
    _asymmetric("hyb12_a2", 3, scheme, (5,), (2,), 9950 + scheme, gpu, pad=16)


def test_asymmetric_wide_special_base(gpu):
    _asymmetric("wide_p20", 24, O.CKKS, (1,), (0,), 9960, gpu)


@pytest.mark.parametrize("name,level", [("c1_bfv4096", 2), ("c1_bfv4096", 1), ("bfv13_50", 4), ("bfv13_50", 2)])
def test_bfv_word_for_word(name, level, gpu):
    sch = Scheme(name, seed=26)
    P, ctx = _ctx(sch, gpu, T)
    case = SymCase(sch, O.BFV, level, 5, 9970 + level + sch.log_n)
    for count in (1, 5):
        case.run(P, ctx, gpu, count)
    case.run(P, ctx, gpu, 5, pad=16)
    del ctx
    _release()
    _asymmetric(name, level, O.BFV, (1, 5), (1, 2, 0), 9980 + level + sch.log_n, gpu)


# ------------------------------------------------------------------------------------------------------------------------------
# E: round trips on the device
# ------------------------------------------------------------------------------------------------------------------------------
def _roundtrip_inputs(sch, level, batch, seed):
    rng = rng_for(seed)
    a = np.stack([_uniform(rng, sch, range(level)) for _ in range(batch)])
    return a, _noise(rng, (batch,), sch.n, wide=False), rng.integers(-1, 2, (batch, sch.n)), _noise(rng, (batch, 2), sch.n, wide=False)


@pytest.mark.parametrize("public", [False, True], ids=["symmetric", "public"])
def test_ckks_encode_encrypt_decrypt_decode_returns_the_messages(public, gpu):
    import torch
    from phantom_fhe_amd import workloads as W
    sch = S.scheme("hyb12_a2")
    P, ctx = _ctx(sch, gpu)
    enc = ctx.ckks_encoder()
    level, batch, scale = 3, 5, 2.0 ** 40
    z = S.messages(31, batch, sch.slots)
    a, e1, u, e2 = _roundtrip_inputs(sch, level, batch, 9990)
    r = _restatement(sch, O.CKKS)
    codec = S.cpu_codec("hyb12_a2")
    pts = codec.encode(z, level, scale)
    if public:
        pk, pk_ref, _, _ = _public_key(P, ctx, sch, O.CKKS, 9991, gpu)
        cpu_cts = [r.asymmetric(pk_ref, u[b], e2[b], pts[b], level) for b in range(batch)]
        key, samples = pk, (_signed(u, gpu), _signed(e2, gpu))
    else:
        cpu_cts = [r.symmetric(sch.sk_ntt, a[b], e1[b], pts[b], level) for b in range(batch)]
        key, samples = P.to_device(sch.sk_ntt, gpu), (P.to_device(a, gpu), _signed(e1, gpu))
    cpu_err = S.max_err(codec.decode(np.stack([sch.decrypt(ct, level) for ct in cpu_cts]), level, scale), z)
    cts = W.encode_encrypt_batch(ctx, enc, torch.from_numpy(z).to(gpu), level, scale, key, samples, public=public)
    assert tuple(cts.shape) == (batch, 2, level, sch.n)
    sk = ctx.secret_key_powers(P.to_device(sch.sk_ntt, gpu), 1)
    got = W.decrypt_decode_batch(ctx, enc, cts, level, scale, sk).cpu().numpy()
    gpu_err = S.max_err(got, z)
    print(f"round trip public={public}: cpu_err {cpu_err:.3e} gpu_err {gpu_err:.3e} bound {S.bound(cpu_err):.3e}")
    assert cpu_err < S.CPU_CAP
    assert gpu_err <= S.bound(cpu_err)
    assert S.max_err(got, np.conj(z)) > S.FAR
    del enc, ctx
    _release()


def test_ckks_gpu_encrypted_pair_through_keyswitch_rescale(gpu):
    import torch
    from phantom_fhe_amd import workloads as W
    sch = S.scheme("hyb12_a2")
    P, ctx = _ctx(sch, gpu)
    enc = ctx.ckks_encoder()
    level, scale = 4, 2.0 ** 40
    z = S.messages(32, 2, sch.slots)
    a, e1, _, _ = _roundtrip_inputs(sch, level, 2, 9992)
    codec, r = S.cpu_codec("hyb12_a2"), _restatement(sch, O.CKKS)
    pts = codec.encode(z, level, scale)
    cpu_cts = [r.symmetric(sch.sk_ntt, a[b], e1[b], pts[b], level) for b in range(2)]
    out_scale = scale * scale / float(sch.primes[level - 1])
    cpu_prod = S.Reference(sch, codec).multiply_many([cpu_cts[0]], [cpu_cts[1]], level)[0]
    cpu_err = S.max_err(codec.decode(sch.decrypt(cpu_prod, level - 1)[None], level - 1, out_scale)[0], z[0] * z[1])
    # the device pipeline: encode, encrypt, tensor product, key switch + rescale, decrypt, decode
    d_sk = P.to_device(sch.sk_ntt, gpu)
    cts = W.encode_encrypt_batch(ctx, enc, torch.from_numpy(z).to(gpu), level, scale, d_sk, (P.to_device(a, gpu), _signed(e1, gpu)))
    new_key, ka, ke = sch.relin_randomness()
    rlk = ctx.generate_one_kswitch_key(d_sk, P.to_device(new_key, gpu), P.to_device(ka, gpu), P.to_device(ke, gpu), P.scheme_type.ckks)
    t3, dst = _poisoned((3, level, sch.n), gpu), _poisoned((1, 2, level - 1, sch.n), gpu)
    ctx.tensor_prod_2x2_rns_poly(cts[0], cts[1], t3, level)
    ctx.keyswitch_rescale(level, t3[:2], t3[2], rlk.public_keys_ptr, dst[0])
    got = W.decrypt_decode_batch(ctx, enc, dst, level - 1, out_scale, ctx.secret_key_powers(d_sk, 1)).cpu().numpy()[0]
    gpu_err = S.max_err(got, z[0] * z[1])
    print(f"product: cpu_err {cpu_err:.3e} gpu_err {gpu_err:.3e} bound {S.bound(cpu_err):.3e}")
    assert cpu_err < S.CPU_CAP
    assert gpu_err <= S.bound(cpu_err)
    assert S.nearest_wrong(got, S.product_wrongs(z[0], z[1])) > S.FAR
    del enc, ctx
    _release()


@pytest.mark.parametrize("scheme,name,level", [(O.BGV, "hyb12_a2", 6), (O.BGV, "hyb12_a2", 2), (O.BFV, "c1_bfv4096", 2), (O.BFV, "bfv13_50", 4)],
                         ids=["bgv6", "bgv2", "bfv-c1", "bfv13"])
def test_bgv_and_bfv_decrypt_to_m_on_the_device(scheme, name, level, gpu):
    sch = Scheme(name, seed=27)
    P, ctx = _ctx(sch, gpu, T)
    batch, n = 5, sch.n
    a, e1, u, e2 = _roundtrip_inputs(sch, level, batch, 9995)
    m = rng_for(9996).integers(0, T, (batch, n)).astype(np.uint64)
    d_sk, d_m, kind = P.to_device(sch.sk_ntt, gpu), P.to_device(m, gpu), _kind(P, scheme)
    sym = _poisoned((batch, 2, level, n), gpu)
    sym[:, 1] = P.to_device(a, gpu)
    ctx.encrypt_symmetric_batched(level, d_sk, _signed(e1, gpu), d_m, sym, kind)
    pk, _, _, _ = _public_key(P, ctx, sch, scheme, 9997, gpu)
    asym = _poisoned((batch, 2, level, n), gpu)
    ctx.encrypt_asymmetric_batched(level, pk, _signed(u, gpu), _signed(e2, gpu), d_m, asym, kind)
    sk = ctx.secret_key_powers(d_sk, 1)
    for what, cts in (("symmetric", sym), ("public-key", asym)):
        dst = _poisoned((batch, n), gpu)
        if scheme == O.BGV:
            ctx.bgv_decrypt_batched(level, cts, sk, dst)
        else:
            ctx.bfv_decrypt_batched(level, cts, sk, dst)
        assert np.array_equal(P.to_host(dst), m), f"{what} {name} level {level}: the decryption is not m in every coefficient"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# F: refusals, count == 0, strict mode
# ------------------------------------------------------------------------------------------------------------------------------
def _calls(ctx, P, level, scheme):
    """(entry name, call(key, samples..., plain, ct, **kw)) with uniform keyword handling: count, ct_stride, e_stride."""
    kind = _kind(P, scheme)

    def count_of(ct, count):   # the methods read the count off a [count][2][L][N] buffer; a null or flat ct names it (2: the test's batch)
        return count if count is not None else int(ct.shape[0]) if ct is not None and ct.dim() == 4 else 2

    def zero(sk, pk, u, e1, e2, plain, ct, count=None, cs=None, es=None, ps=None):
        ctx.encrypt_zero_symmetric_batched(level, sk, e1, ct, kind, count=count_of(ct, count),
                                           strides=None if cs is None and es is None else (es or ctx.n, cs or 2 * level * ctx.n))

    def sym(sk, pk, u, e1, e2, plain, ct, count=None, cs=None, es=None, ps=None):
        pw = level * ctx.n if scheme == O.CKKS else ctx.n
        strides = None if cs is None and es is None and ps is None else (es or ctx.n, pw if ps is None else ps, cs or 2 * level * ctx.n)
        ctx.encrypt_symmetric_batched(level, sk, e1, plain, ct, kind, count=count_of(ct, count), strides=strides)

    def asym(sk, pk, u, e1, e2, plain, ct, count=None, cs=None, es=None, ps=None):
        pw = level * ctx.n if scheme == O.CKKS else ctx.n
        strides = None if cs is None and es is None and ps is None else (ctx.n, es or 2 * ctx.n, pw if ps is None else ps, cs or 2 * level * ctx.n)
        ctx.encrypt_asymmetric_batched(level, pk, u, e2, plain, ct, kind, count=count_of(ct, count), strides=strides)

    return [("encrypt_zero_symmetric", zero), ("encrypt_symmetric", sym), ("encrypt_asymmetric", asym)]


def test_refusals_and_empty_batch(gpu):
    import torch
    sch = Scheme("hyb12_a2", seed=28)
    P, ctx = _ctx(sch, gpu, T)
    _, bare = _ctx(sch, gpu)                                              # no plain modulus
    level, batch, n = 3, 2, sch.n
    ln = level * n
    rng = rng_for(9998)
    d_sk = P.to_device(sch.sk_ntt, gpu)
    pk = P.to_device(np.stack([_uniform(rng, sch, range(sch.size_qp)) for _ in range(2)]), gpu)
    u, e1, e2 = _signed(rng.integers(-1, 2, (batch, n)), gpu), _signed(_noise(rng, (batch,), n), gpu), _signed(_noise(rng, (batch, 2), n), gpu)
    plain = P.to_device(_plain(rng, sch, O.CKKS, level, batch), gpu)
    big = _poisoned((batch * 2 * ln + 64,), gpu)

    def refused(call, text, *args, **kw):
        with pytest.raises(ValueError) as err:
            call(*args, **kw)
        assert text in str(err.value), str(err.value)

    for name, call in _calls(ctx, P, level, O.CKKS):
        ct = _poisoned((batch, 2, level, n), gpu)
        ok = [d_sk, pk, u, e1, e2, plain, ct]
        uses = {"encrypt_zero_symmetric": (0, 3, 6), "encrypt_symmetric": (0, 3, 5, 6), "encrypt_asymmetric": (1, 2, 4, 5, 6)}[name]
        for i in uses:                                                     # a null pointer in every place
            refused(call, "null", *[None if j == i else v for j, v in enumerate(ok)])
        refused(call, "ct stride", *ok, cs=2 * ln - 2)
        refused(call, "e stride", *ok, es=(2 * n if name == "encrypt_asymmetric" else n) - 2)
        refused(call, "even", *ok, cs=2 * ln + 1)
        refused(call, "even", *ok, es=2 * n + 1)
        if name != "encrypt_zero_symmetric":
            refused(call, "plain stride", *ok, ps=ln - 2)
            refused(call, "overlap plain", d_sk, pk, u, e1, e2, ct.reshape(-1)[:batch * ln], ct)
        refused(call, "aligned", d_sk, pk, u, e1, e2, plain, big[1:1 + batch * 2 * ln], count=batch)
        key_overlap = "overlap pk" if name == "encrypt_asymmetric" else "overlap sk_ntt"
        refused(call, key_overlap, d_sk, pk, u, e1, e2, plain, (pk if name == "encrypt_asymmetric" else d_sk).reshape(-1)[:batch * 2 * ln], count=batch)
        refused(call, "count out of range", *ok, count=65536)
        assert bool((ct == POISON).all()), f"{name}: a refused call wrote to ct"
        call(*ok, count=0)                                                 # count == 0 does nothing
        assert bool((ct == POISON).all()), f"{name}: count == 0 wrote to ct"
    # size_Ql out of range
    ct = _poisoned((batch, 2, level, n), gpu)
    for bad_level in (0, sch.size_q + 1):
        for name, call in _calls(ctx, P, bad_level, O.CKKS):
            refused(call, "RNSBase is invalid", d_sk, pk, u, e1, e2, plain, ct, count=batch, cs=2 * ln)
    # an unknown scheme; bgv / bfv without a plain modulus
    with pytest.raises(ValueError):
        ctx.encrypt_symmetric_batched(level, d_sk, e1, plain, ct, 7)
    raw = P.to_device(_plain(rng, sch, O.BGV, level, batch), gpu)
    for scheme in (O.BGV, O.BFV):
        for name, call in _calls(bare, P, level, scheme):
            refused(call, "plain modulus", d_sk, pk, u, e1, e2, raw, ct)
    with pytest.raises(ValueError) as err:
        bare.public_key_generate(d_sk, e1, _poisoned((2, sch.size_qp, n), gpu), P.scheme_type.bgv)
    assert "plain modulus" in str(err.value)
    assert bool((ct == POISON).all())
    # the special rows on a context that has none
    import phantom_fhe_amd as PP
    flat = PP.PhantomContext(sch.log_n, list(sch.primes[:sch.size_q]), 0, device=gpu)
    with pytest.raises(ValueError) as err:
        flat.encrypt_zero_symmetric_batched(level, d_sk, e1, ct, P.scheme_type.ckks, with_special=True)
    assert "special modulus" in str(err.value)
    torch.cuda.synchronize()
    del ctx, bare, flat
    _release()


def test_small_primes_are_refused(gpu):
    """A sample of magnitude 2^16 needs every prime used above it: a context with a 17-bit prime (below 2^17) among the rows is refused."""
    import phantom_fhe_amd as P
    n = 4096
    primes = [int(p) for p in O.coeff_modulus_create(n, [40, 17, 40])]
    ctx = P.PhantomContext(12, primes, 1, device=gpu)
    ct = _poisoned((1, 2, 2, n), gpu)
    sk, e = _poisoned((3, n), gpu), _signed(np.zeros((1, n)), gpu)
    with pytest.raises(ValueError) as err:
        ctx.encrypt_zero_symmetric_batched(2, sk, e, ct, P.scheme_type.ckks)
    assert "2^17" in str(err.value)
    assert bool((ct == POISON).all())
    one = _poisoned((1, 2, 1, n), gpu)
    one[0, 1] = 0
    sk[:] = 0
    ctx.encrypt_zero_symmetric_batched(1, sk, e, one, P.scheme_type.ckks)     # the first row alone is wide enough
    assert bool((one == 0).all())
    del ctx
    _release()


def test_strict_mode_names_the_operand(gpu):
    sch = Scheme("hyb12_a2", seed=29)
    P, ctx = _ctx(sch, gpu, T)
    level, batch, n = 3, 5, sch.n
    rng = rng_for(9999)
    d_sk = P.to_device(sch.sk_ntt, gpu)
    pk, _, _, _ = _public_key(P, ctx, sch, O.CKKS, 10000, gpu)
    a = np.stack([_uniform(rng, sch, range(level)) for _ in range(batch)])
    u, e1, e2 = _signed(rng.integers(-1, 2, (batch, n)), gpu), _signed(_noise(rng, (batch,), n), gpu), _signed(_noise(rng, (batch, 2), n), gpu)
    plain = P.to_device(_plain(rng, sch, O.CKKS, level, batch), gpu)
    raw = P.to_device(_plain(rng, sch, O.BGV, level, batch), gpu)

    def fresh():
        ct = _poisoned((batch, 2, level, n), gpu)
        ct[:, 1] = P.to_device(a, gpu)
        return ct

    def bad_word(t, at, value):
        out = t.clone()
        out[at] = value
        return out

    q_last = int(sch.primes[level - 1])
    bad_sk, bad_pk = bad_word(d_sk, (level - 1, 5), q_last), bad_word(pk, (1, sch.size_q, 7), int(sch.primes[sch.size_q]) + 1)
    bad_e1, bad_e2, bad_u = bad_word(e1, (3, n - 1), (1 << 16) + 1), bad_word(e2, (3, 1, 0), -(1 << 16) - 1), bad_word(u, (4, 9), 1 << 40)
    bad_plain, bad_raw = bad_word(plain, (2, level - 1, 3), q_last), bad_word(raw, (2, 3), T)
    ckks, bgv = P.scheme_type.ckks, P.scheme_type.bgv
    prev = P.set_strict(True)
    try:
        def refused(text, call):
            with pytest.raises(ValueError) as err:
                call()
            assert "PHA_STRICT" in str(err.value) and text in str(err.value) and "1 word" in str(err.value), str(err.value)

        refused("encrypt_zero_symmetric sk", lambda: ctx.encrypt_zero_symmetric_batched(level, bad_sk, e1, fresh(), ckks))
        refused("encrypt_zero_symmetric samples", lambda: ctx.encrypt_zero_symmetric_batched(level, d_sk, bad_e1, fresh(), ckks))
        refused("encrypt_zero_symmetric a", lambda: ctx.encrypt_zero_symmetric_batched(level, d_sk, e1, bad_word(fresh(), (3, 1, 0, 0), int(sch.primes[0])), ckks))
        refused("encrypt_symmetric sk", lambda: ctx.encrypt_symmetric_batched(level, bad_sk, e1, plain, fresh(), ckks))
        refused("encrypt_symmetric a", lambda: ctx.encrypt_symmetric_batched(level, d_sk, e1, plain, bad_word(fresh(), (0, 1, 2, 1), -1), ckks))
        refused("encrypt_symmetric plain", lambda: ctx.encrypt_symmetric_batched(level, d_sk, e1, bad_plain, fresh(), ckks))
        refused("encrypt_symmetric plain", lambda: ctx.encrypt_symmetric_batched(level, d_sk, e1, bad_raw, fresh(), bgv))
        refused("encrypt_symmetric samples", lambda: ctx.encrypt_symmetric_batched(level, d_sk, bad_e1, plain, fresh(), ckks))
        refused("encrypt_asymmetric pk", lambda: ctx.encrypt_asymmetric_batched(level, bad_pk, u, e2, plain, fresh(), ckks))
        refused("encrypt_asymmetric plain", lambda: ctx.encrypt_asymmetric_batched(level, pk, u, e2, bad_plain, fresh(), ckks))
        refused("encrypt_asymmetric samples", lambda: ctx.encrypt_asymmetric_batched(level, pk, bad_u, e2, plain, fresh(), ckks))
        refused("encrypt_asymmetric samples", lambda: ctx.encrypt_asymmetric_batched(level, pk, u, bad_e2, plain, fresh(), ckks))
        refused("encrypt_zero_symmetric sk", lambda: ctx.public_key_generate(bad_sk, e1, pk.clone(), ckks))
        # canonical operands and samples of exactly +-2^16 pass
        ctx.encrypt_symmetric_batched(level, d_sk, e1, plain, fresh(), ckks)
        ctx.encrypt_asymmetric_batched(level, pk, u, e2, plain, fresh(), ckks)
        P.set_strict(False)
        ctx.encrypt_symmetric_batched(level, d_sk, bad_e1, plain, fresh(), ckks)    # strict off: the call computes
    finally:
        P.set_strict(prev)
    del ctx
    _release()
