"""What the library's entries do to a CKKS message, layer by layer: the C ABI through ctypes, the compositions in workloads, and
host/phantom.h through pyPhantom.  The cases, inputs, seeds, expected values and wrong answers are those of
tests/test_ckks_semantics.py (tests/ckks_semantics.py); here the GPU encodes (CKKSEncoder.encode_batched), generates the keys
(generate_one_kswitch_key, from the same randomness the oracle's keys take), runs the operation into poisoned buffers and decodes
(decode_batched); encryption and decryption stay on the CPU through the helper, independent of the code under test.

Bounds: every case runs the helper's oracle pipeline on the same inputs and asserts gpu_err <= 16 * cpu_err, capped at 2^-12
(ckks_semantics.bound); every rotation, product and matrix-vector case is farther than 0.1 from every plausible wrong answer (opposite
direction, conjugate, unrotated, transpose, BSGS weights without the roll-back, ...).  Measured values: profiles/ckks_semantics.md.

a. rotations (apply_galois_for_keyswitch + keyswitch_inplace)      f. workloads.diag_matvec / diag_matvec_batch + encode_diagonals
b. products (unfused, keyswitch_rescale, its batched form, square)  g. workloads.diag_matvec_bsgs / _batch / _blocks + bsgs_diagonals
c. inner_product_relin_rescale_batched                              h. relinearize_rotate_batch (config 4) in CKKS
d. plain_inner_product_rescale_batched on real encryptions          i. config 4 in BFV: exact
e. hoisting / hoisting_batched                                      j. pyPhantom: rotate (direct, negative, 0, NAF), hoisting, ..."""
import functools
import gc

import numpy as np
import pytest

import ckks_semantics as S
from util import CONFIGS

pytestmark = pytest.mark.gpu

NAME, SCALE = "hyb12_a2", 2.0 ** 40


class Device:
    """The library at one parameter set: context, encoder, keys generated on the device, numpy ciphertexts in and out."""

    def __init__(self, name, scheme=None):
        import torch
        import phantom_fhe_amd as P
        self.P, self.torch = P, torch
        self.sch = sch = S.scheme(name) if scheme is None else scheme
        self.gpu = torch.device("cuda:0")
        self.ctx = P.PhantomContext(sch.log_n, list(sch.primes), sch.size_p, device=self.gpu)
        self.kind = P.scheme_type.ckks
        self.codec = None
        if scheme is None:
            self.codec = S.GpuCodec(sch, P, self.ctx, self.ctx.ckks_encoder(), self.gpu)
        self._keys = {}

    def dev(self, x):
        return self.P.to_device(np.ascontiguousarray(x), self.gpu)

    def host(self, t):
        return self.P.to_host(t)

    def poison(self, *shape):
        return self.torch.full(shape, S.GpuCodec.POISON, dtype=self.torch.int64, device=self.gpu)

    def key(self, elt=None):
        """The key of Galois element elt (None: relinearisation) made by generate_one_kswitch_key."""
        if elt not in self._keys:
            new_key, a, e = self.sch.relin_randomness() if elt is None else self.sch.galois_randomness(elt)
            self._keys[elt] = self.ctx.generate_one_kswitch_key(self.dev(self.sch.sk_ntt), self.dev(new_key), self.dev(a), self.dev(e), self.kind)
        return self._keys[elt]

    def keys(self, elts):
        return [None if e == 1 else self.key(e) for e in elts]

    def rescale(self, d_ct, level):
        out = self.poison(2, level - 1, self.sch.n)
        self.ctx.divide_and_round_q_last_ntt(level, d_ct.contiguous(), 2, out)
        return self.host(out)

    # -- a ---------------------------------------------------------------------------------------------------------------------------
    def rotate(self, ct, level, elt):
        n = self.sch.n
        rot, g1 = self.poison(1, 2, level, n), self.poison(1, level, n)
        self.ctx.apply_galois_for_keyswitch(self.dev(ct[None]), rot, g1, elt, level, 1, True)
        self.ctx.keyswitch_inplace(level, rot[0], g1[0], self.key(elt).public_keys_ptr, self.kind)
        return self.host(rot[0])

    # -- b ---------------------------------------------------------------------------------------------------------------------------
    def _tensor(self, x, y, level):
        t3 = self.poison(3, level, self.sch.n)
        if y is x:
            self.ctx.tensor_square_2x2_rns_poly(self.dev(x), t3, level)
        else:
            self.ctx.tensor_prod_2x2_rns_poly(self.dev(x), self.dev(y), t3, level)
        return t3

    def multiply_unfused(self, a, b, level):
        out = []
        for x, y in zip(a, b):
            t3 = self._tensor(x, y, level)
            self.ctx.keyswitch_inplace(level, t3[:2], t3[2], self.key().public_keys_ptr, self.kind)
            out.append(self.rescale(t3[:2], level))
        return out

    def multiply_fused(self, a, b, level):
        out = []
        for x, y in zip(a, b):
            t3, dst = self._tensor(x, y, level), self.poison(2, level - 1, self.sch.n)
            self.ctx.keyswitch_rescale(level, t3[:2], t3[2], self.key().public_keys_ptr, dst)
            out.append(self.host(dst))
        return out

    def multiply_batched(self, a, b, level):
        t3 = self.torch.stack([self._tensor(x, y, level) for x, y in zip(a, b)])
        dst = self.poison(len(a), 2, level - 1, self.sch.n)
        self.ctx.keyswitch_rescale_batched(level, t3[:, :2].contiguous(), t3[:, 2].contiguous(), len(a), self.key().public_keys_ptr, dst)
        return list(self.host(dst))

    # -- c, d ------------------------------------------------------------------------------------------------------------------------
    def inner(self, a, b, level):
        op1 = self.dev(np.stack([np.stack(row) for row in a]))
        op2 = self.dev(np.stack([np.stack(row) for row in b]) if isinstance(b[0], list) else np.stack(b))
        dst = self.poison(len(a), 2, level - 1, self.sch.n)
        self.ctx.inner_product_relin_rescale_batched(level, op1, op2, len(a[0]), len(a), self.key().public_keys_ptr, dst)
        return list(self.host(dst))

    def plain_sum(self, plain, ct, acc, level):
        dst = self.poison(len(ct), 2, level - 1, self.sch.n)
        self.ctx.plain_inner_product_rescale_batched(level, self.dev(np.stack(plain)), self.dev(np.stack([np.stack(row) for row in ct])),
                                                     None if acc is None else self.dev(np.stack(acc)), len(ct[0]), len(ct), self.kind, dst)
        return list(self.host(dst))

    # -- e ---------------------------------------------------------------------------------------------------------------------------
    def hoist_single(self, cts, level, elts):
        out = []
        for ct in cts:
            d = self.dev(ct)
            self.ctx.hoisting(level, d, elts, [self.key(e) for e in elts], self.kind)
            out.append(self.host(d))
        return out

    def hoist_batched(self, cts, level, elts):
        out = self.poison(len(cts), 2, level, self.sch.n)
        self.ctx.hoisting_batched(level, self.dev(np.stack(cts)), elts, [self.key(e) for e in elts], self.kind, out=out)
        return list(self.host(out))

    # -- f ---------------------------------------------------------------------------------------------------------------------------
    def matvec_single(self, cts, level, m, elts, scale):
        from phantom_fhe_amd import workloads as W
        diags = list(W.encode_diagonals(self.codec.enc, level, m, scale))
        return [self.rescale(W.diag_matvec(self.ctx, level, self.dev(ct), elts, self.keys(elts), diags, self.kind), level) for ct in cts]

    def matvec_batched(self, cts, level, m, elts, scale):
        from phantom_fhe_amd import workloads as W
        diags = list(W.encode_diagonals(self.codec.enc, level, m, scale))
        out = W.diag_matvec_batch(self.ctx, level, self.dev(np.stack(cts)), elts, self.keys(elts), diags, self.kind)
        return [self.rescale(out[b], level) for b in range(len(cts))]

    # -- g ---------------------------------------------------------------------------------------------------------------------------
    def _weights(self, values, level, scale):
        flat = self.codec.encode_device(np.stack([w for row in values for w in row]), level, scale, with_special=True)
        nb = len(values[0])
        return [[flat[i * nb + j] for j in range(nb)] for i in range(len(values))]

    def bsgs_single(self, cts, level, baby, giant, values, scale):
        from phantom_fhe_amd import workloads as W
        ws = self._weights(values, level, scale)
        return [self.rescale(W.diag_matvec_bsgs(self.ctx, level, self.dev(ct), baby, self.keys(baby), giant, self.keys(giant), ws, self.kind),
                             level) for ct in cts]

    def bsgs_batched(self, cts, level, baby, giant, values, scale):
        from phantom_fhe_amd import workloads as W
        out = W.diag_matvec_bsgs_batch(self.ctx, level, self.dev(np.stack(cts)), baby, self.keys(baby), giant, self.keys(giant),
                                       self._weights(values, level, scale), self.kind)
        return [self.rescale(out[b], level) for b in range(len(cts))]

    def bsgs_blocks(self, ct, level, baby, giant, blocks, scale):
        from phantom_fhe_amd import workloads as W
        out = W.diag_matvec_bsgs_blocks(self.ctx, level, self.dev(ct), baby, self.keys(baby), giant, self.keys(giant),
                                        [self._weights(values, level, scale) for values in blocks], self.kind)
        return [self.rescale(out[r], level) for r in range(len(blocks))]

    # -- h ---------------------------------------------------------------------------------------------------------------------------
    def relin_rotate_many(self, ct3s, level, elt):
        from phantom_fhe_amd import workloads as W
        return list(self.host(W.relinearize_rotate_batch(self.ctx, level, self.dev(np.stack(ct3s)), self.key(), self.key(elt), elt, self.kind)))


@functools.lru_cache(maxsize=1)
def _setup(name):
    return Device(name)


def _release():
    import torch
    _setup.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _cpu(case, name, *args):
    """The oracle pipeline of one case (the baseline of its bound); computed once per distinct case."""
    sch, codec = S.scheme(name), S.cpu_codec(name)
    ref = S.Reference(sch, codec)
    fn = {"rotation": ref.rotate, "products": ref.multiply_many, "inner_product": ref.inner, "plain_sum": ref.plain_sum,
          "hoisting": ref.hoist_many, "matvec": ref.matvec_many, "bsgs": ref.bsgs_many, "bsgs_blocks": ref.bsgs_blocks,
          "config4": ref.relin_rotate_many}[case]
    return getattr(S, "case_" + case)(sch, codec, fn, *args)


def _check(gpu_res, cpu_res):
    """gpu_err <= 16 * cpu_err (capped at 2^-12), cpu_err < 2^-16, and farther than 0.1 from every wrong answer."""
    both = list(zip(gpu_res, cpu_res)) if isinstance(gpu_res, list) else [(gpu_res, cpu_res)]
    for g, c in both:
        assert g.label == c.label and np.array_equal(g.want, c.want)
        print(f"{g.label}: gpu error {g.err:.3e}, cpu error {c.err:.3e}, ratio {g.err / c.err:.2f}, nearest wrong answer "
              f"{'-' if g.wrong is None else round(g.wrong, 3)}")
        assert c.err < S.CPU_CAP, g.label
        assert g.err <= S.bound(c.err), g.label
        assert g.wrong is None or g.wrong > S.FAR, g.label


def _run(dev, case, fn, *args):
    _check(getattr(S, "case_" + case)(dev.sch, dev.codec, fn, *args), _cpu(case, dev.sch.name, *args))


# ---- a -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [6, 3])
def test_rotations_and_conjugation(gpu, level):
    dev = _setup(NAME)
    for step in (1, 3, dev.sch.slots - 1, dev.sch.slots // 2, None):
        _run(dev, "rotation", dev.rotate, level, SCALE, step)
    _release()


@pytest.mark.parametrize("name,level,scale", [("hyb13_a3", 7, 2.0 ** 50),       # short last digit
                                              ("c2_ckks14", 8, 2.0 ** 40),      # alpha 1, beta 8: unfused mod-up and inner product
                                              ("hyb14_a2", 8, 2.0 ** 50)])      # beta 4 under the fused mod-up + inner product
def test_rotations_at_other_sets(gpu, name, level, scale):
    dev = _setup(name)
    for step in (1, 3):
        _run(dev, "rotation", dev.rotate, level, scale, step)
    _release()


# ---- b -----------------------------------------------------------------------------------------------------------------------------
def test_products(gpu):
    dev = _setup(NAME)
    _run(dev, "products", dev.multiply_unfused, 6, SCALE, 1)
    _run(dev, "products", dev.multiply_fused, 6, SCALE, 1)
    _run(dev, "products", dev.multiply_batched, 6, SCALE, 3)
    _run(dev, "products", dev.multiply_unfused, 6, SCALE, 1, True)
    _release()


# ---- c -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_encrypted_inner_products(gpu, shared):
    dev = _setup(NAME)
    _run(dev, "inner_product", dev.inner, 6, SCALE, 5, 2, shared)
    _release()


# ---- d -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_acc", [False, True])
def test_plain_weighted_sums_of_real_encryptions(gpu, with_acc):
    dev = _setup(NAME)
    _run(dev, "plain_sum", dev.plain_sum, 6, SCALE, 4, 2, with_acc)
    _release()


# ---- e -----------------------------------------------------------------------------------------------------------------------------
def test_hoisting(gpu):
    dev = _setup(NAME)
    _run(dev, "hoisting", dev.hoist_single, 6, SCALE, (1, 2, 5), 1)
    _run(dev, "hoisting", dev.hoist_batched, 6, SCALE, (1, 2, 5), 2)
    _release()


# ---- f -----------------------------------------------------------------------------------------------------------------------------
def test_diag_matvec_multiplies_by_the_matrix(gpu):
    dev = _setup(NAME)
    _run(dev, "matvec", dev.matvec_single, 5, SCALE, 8, 1)
    _run(dev, "matvec", dev.matvec_single, 5, SCALE, 16, 1)
    _run(dev, "matvec", dev.matvec_batched, 5, SCALE, 8, 3)
    _release()


# ---- g -----------------------------------------------------------------------------------------------------------------------------
def test_bsgs_matvec_with_the_documented_preparation(gpu):
    dev = _setup(NAME)
    _run(dev, "bsgs", dev.bsgs_single, 5, SCALE, 4, 2, 1)
    _run(dev, "bsgs", dev.bsgs_single, 5, SCALE, 4, 4, 1)
    _run(dev, "bsgs", dev.bsgs_batched, 5, SCALE, 4, 2, 2)
    _run(dev, "bsgs_blocks", dev.bsgs_blocks, 5, SCALE, 4, 2, 2)
    _release()


# ---- h -----------------------------------------------------------------------------------------------------------------------------
def test_config4_relinearize_rotate_in_ckks(gpu):
    dev = _setup(NAME)
    _run(dev, "config4", dev.relin_rotate_many, 6, SCALE, 3)
    _release()


# ---- i -----------------------------------------------------------------------------------------------------------------------------
def test_config4_in_bfv_decrypts_to_the_rotated_product(gpu):
    """c1_bfv4096, t = 65537: bfv_multiply_behz -> relinearize_rotate_batch with generated keys decrypts to (m1 m2)(X^elt) and
    (m1^2)(X^elt) mod (X^N + 1, t), exactly, on every 53rd coefficient."""
    from phantom_fhe_amd import workloads as W
    c = S.BfvConfig4()
    dev = Device(c.NAME, scheme=c.sch)
    dev.kind = dev.P.scheme_type.bfv
    dev.ctx.set_plain_modulus(c.T)
    L, n = c.sch.size_q, c.sch.n
    pairs = [(0, 1), (0, 0)]
    d3 = dev.poison(len(pairs), 3, L, n)
    for b, (k1, k2) in enumerate(pairs):
        dev.ctx.bfv_multiply_behz(dev.dev(c.ct[k1]), dev.dev(c.ct[k2]), d3[b])
    out = dev.host(W.relinearize_rotate_batch(dev.ctx, L, d3, dev.key(), dev.key(c.ELT), c.ELT, dev.kind))
    for b, (k1, k2) in enumerate(pairs):
        assert c.decrypt(out[b]) == c.want(k1, k2), (k1, k2)
        assert np.array_equal(out[b], c.oracle(k1, k2)), (k1, k2)
    del dev
    _release()


# ---- j -----------------------------------------------------------------------------------------------------------------------------
class PyPhantomApi:
    """case_host_api's `api` through pyPhantom: ciphertexts, plaintexts and generated keys loaded from numpy."""

    def __init__(self, sch, scale):
        from phantom_fhe_amd import pyPhantom as ph
        self.ph, self.sch, self.scale = ph, sch, scale
        parms = ph.params(ph.scheme_type.ckks)
        parms.set_poly_modulus_degree(sch.n)
        parms.set_special_modulus_size(sch.size_p)
        parms.set_coeff_modulus(ph.create_coeff_modulus(sch.n, list(CONFIGS[sch.name][1])))
        self.ctx = ph.context(parms)
        self.rlk = self._generate(sch.relin_randomness())
        self.glk, self.glk_conj = ph.galois_key(), ph.galois_key()
        for step in S.HOST_KEY_STEPS:
            elt = ph.get_elt_from_step(step, sch.n)
            assert elt == S.elt_of_step(step, sch.n), step
            evk = self._generate(sch.galois_randomness(elt)).to_numpy()
            self.glk.load(self.ctx, elt, evk)
            self.glk_conj.load(self.ctx, elt, evk)
        conj = ph.get_elt_from_step(0, sch.n)
        assert conj == 2 * sch.n - 1
        self.glk_conj.load(self.ctx, conj, self._generate(sch.galois_randomness(conj)).to_numpy())

    def _generate(self, randomness):
        new_key, a, e = randomness
        key = self.ph.relin_key()
        key.generate(self.ctx, self.sch.sk_ntt, new_key, a, e)
        return key

    def _ct(self, h):
        ct = self.ph.ciphertext()
        ct.load(self.ctx, 1, np.ascontiguousarray(h))
        ct.set_scale(self.scale)
        return ct

    def _pt(self, h):
        pt = self.ph.plaintext()
        pt.load(np.ascontiguousarray(h), 1, self.scale)
        return pt

    @staticmethod
    def _out(ct):
        return ct.to_numpy(), ct.coeff_modulus_size(), ct.scale()

    def rotate(self, ct, step, with_conjugation_key):
        return self._out(self.ph.rotate(self.ctx, self._ct(ct), step, self.glk_conj if with_conjugation_key else self.glk))

    def hoisting(self, ct, steps):
        return self._out(self.ph.hoisting(self.ctx, self._ct(ct), self.glk, list(steps)))

    def multiply_relin_rescale(self, a, b):
        return self._out(self.ph.multiply_relin_rescale(self.ctx, self._ct(a), self._ct(b), self.rlk))

    def add(self, a, b):
        return self._out(self.ph.add(self.ctx, self._ct(a), self._ct(b)))

    def sub(self, a, b):
        return self._out(self.ph.sub(self.ctx, self._ct(a), self._ct(b)))

    def negate(self, a):
        return self._out(self.ph.negate(self.ctx, self._ct(a)))

    def add_plain(self, a, pt):
        return self._out(self.ph.add_plain(self.ctx, self._ct(a), self._pt(pt)))

    def multiply_plain(self, a, pt):
        return self._out(self.ph.multiply_plain(self.ctx, self._ct(a), self._pt(pt)))

    def mod_switch_to(self, a, chain_index):
        low = self.ph.mod_switch_to(self.ctx, self._ct(a), chain_index)
        assert low.chain_index() == chain_index
        return self._out(low)


def test_pyphantom_rotations_with_and_without_a_direct_key(gpu):
    """rotate by 1 and -1 (direct keys), 0 (conjugation), 3 and 5 (no key: NAF 4 - 1 and 4 + 1 through rotate_inplace's loop),
    hoisting, multiply_relin_rescale, add, sub, negate, add_plain, multiply_plain, mod_switch_to (message, scale, chain index)."""
    dev = _setup(NAME)
    sch = dev.sch
    api = PyPhantomApi(sch, SCALE)
    cpu = S.case_host_api(sch, S.cpu_codec(NAME), S.ReferenceHost(S.Reference(sch, S.cpu_codec(NAME)), SCALE), SCALE)
    _check(S.case_host_api(sch, dev.codec, api, SCALE), cpu)
    # without the key of element 2N - 1, step 0 has an empty NAF: the reference's rotate_internal leaves the ciphertext as it is
    h = S._enc(sch, dev.codec, S.messages(20, 1, sch.slots), sch.size_q, SCALE, "host")[0]
    assert np.array_equal(api.rotate(h, 0, False)[0], h)
    with pytest.raises(ValueError):
        api.rotate(h, 8, False)              # a power of two without a key: one NAF term, refused
    del api
    _release()
