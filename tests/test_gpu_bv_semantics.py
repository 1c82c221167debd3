"""What the library's entries do to a BGV or BFV message, layer by layer: the C ABI through ctypes, the compositions in workloads, and
host/phantom.h through pyPhantom.  The cases, inputs, seeds, expected slots and wrong answers are those of
tests/test_bv_semantics.py (tests/bv_semantics.py); here the GPU encodes (BatchEncoder), generates the keys (generate_one_kswitch_key
with the scheme's own scheme_type, from the same randomness the helper's keys take) and runs the operation into poisoned buffers.
Ciphertexts enter as the helper's numpy encryptions, so the CPU and the GPU pipeline see the same inputs.

Every result is checked twice: (i) the helper decrypts and decodes it on the CPU -- exact in ALL N slots, margin >= the margin of the
oracle pipeline of the same case - MARGIN_LOSS bits; (ii) workloads.batch_decrypt_decode on the device (with correction_factors under
BGV) returns the same slots, and under BGV with the factor left out it does not.  Measured margins: profiles/bv_semantics.md.

BGV (hyb12_a2, level 6 -> 5; rotation and product again at level 3 and at hyb14_a2):
a. rotations, row swap, a batch of 3        f. workloads.diag_matvec / diag_matvec_batch
b. products and the square, three forms     g. workloads.diag_matvec_bsgs / _batch / _blocks
c. inner_product_relin(_mod_switch)_batched h. relinearize_rotate_batch
d. plain_inner_product_rescale_batched      i. depth two: the factors multiply
e. hoisting / hoisting_batched              j. pyPhantom at scheme_type.bgv
BFV (coefficient form; c1_bfv4096 and bfv13_50):
a. rotations, row swap, hoisting            d. plaintext sum, add_plain, sub, multiply_plain
b. BEHZ multiplies, relinearize_rotate      e. pyPhantom at scheme_type.bfv
c. HPS, HPS-over-Q, leveled, fused, depth two; the same-pointer shortcut of HPS-over-Q"""
import functools
import gc

import numpy as np
import pytest

import bv_semantics as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HALF12 = 2048


class Device:
    """The library at one parameter set and scheme: context with the plain modulus, BatchEncoder, keys generated on the device, numpy
    ciphertexts in and out."""

    def __init__(self, name, kind):
        import torch
        import phantom_fhe_amd as P
        self.P, self.torch = P, torch
        self.sch = sch = S.scheme(name, kind)
        self.gpu = torch.device("cuda:0")
        self.ctx = P.PhantomContext(sch.log_n, list(sch.primes), sch.size_p, device=self.gpu)
        self.ctx.set_plain_modulus(S.T)
        self.kind = {O.BGV: P.scheme_type.bgv, O.BFV: P.scheme_type.bfv}[kind]
        self.ntt_form = kind == O.BGV
        self.enc = P.BatchEncoder(self.ctx)
        self.codec = S.GpuCodec(sch, P, self.enc, self.gpu)
        self.d_sk = self.dev(sch.sk_ntt)
        self.sk_powers = self.ctx.secret_key_powers(self.d_sk, 1)
        self._keys = {}

    def dev(self, x):
        return self.P.to_device(np.ascontiguousarray(x), self.gpu)

    def host(self, t):
        return self.P.to_host(t)

    def poison(self, *shape):
        return self.torch.full(shape, S.GpuCodec.POISON, dtype=self.torch.int64, device=self.gpu)

    def key(self, elt=None):
        """The key of Galois element elt (None: relinearisation) made by generate_one_kswitch_key with the scheme's scheme_type."""
        if elt not in self._keys:
            new_key, a, e = self.sch.relin_randomness() if elt is None else self.sch.galois_randomness(elt)
            self._keys[elt] = self.ctx.generate_one_kswitch_key(self.d_sk, self.dev(new_key), self.dev(a), self.dev(e), self.kind)
        return self._keys[elt]

    def keys(self, elts):
        return [None if e == 1 else self.key(e) for e in elts]

    def device_slots(self, cts, level, factor):
        """(ii): decrypt and decode on the device; factor None: correction_factors left out."""
        from phantom_fhe_amd import workloads as W
        d = self.dev(np.stack(cts))
        cf = None if factor is None or self.sch.kind == O.BFV else [factor] * len(cts)
        return self.host(W.batch_decrypt_decode(self.ctx, self.enc, d, level, self.sk_powers, self.kind, correction_factors=cf))

    # -- rotations (BGV a, BFV a) ------------------------------------------------------------------------------------------------------
    def rotate_single(self, cts, level, elt):
        out, n = [], self.sch.n
        for ct in cts:
            rot, g1 = self.poison(1, 2, level, n), self.poison(1, level, n)
            self.ctx.apply_galois_for_keyswitch(self.dev(ct[None]), rot, g1, elt, level, 1, self.ntt_form)
            self.ctx.keyswitch_inplace(level, rot[0], g1[0], self.key(elt).public_keys_ptr, self.kind)
            out.append(self.host(rot[0]))
        return out

    def rotate_batched(self, cts, level, elt):
        b, n = len(cts), self.sch.n
        rot, g1 = self.poison(b, 2, level, n), self.poison(b, level, n)
        self.ctx.apply_galois_for_keyswitch(self.dev(np.stack(cts)), rot, g1, elt, level, b, self.ntt_form)
        self.ctx.keyswitch_inplace_batched(level, rot, g1, b, self.key(elt).public_keys_ptr, self.kind)
        return list(self.host(rot))

    # -- BGV products (b, i) ----------------------------------------------------------------------------------------------------------
    def _tensor(self, x, y, level):
        t3 = self.poison(3, level, self.sch.n)
        if y is x:
            self.ctx.tensor_square_2x2_rns_poly(self.dev(x), t3, level)
        else:
            self.ctx.tensor_prod_2x2_rns_poly(self.dev(x), self.dev(y), t3, level)
        return t3

    def _switched(self, outs, level):
        return outs, level - 1, self.sch.switch_factor(level)

    def bgv_multiply_unfused(self, a, b, level):
        out = []
        for x, y in zip(a, b):
            t3, dst = self._tensor(x, y, level), self.poison(2, level - 1, self.sch.n)
            self.ctx.keyswitch_inplace(level, t3[:2], t3[2], self.key().public_keys_ptr, self.kind)
            self.ctx.mod_t_and_divide_q_last_ntt(level, t3[:2], 2, dst)
            out.append(self.host(dst))
        return self._switched(out, level)

    def bgv_multiply_fused(self, a, b, level):
        out = []
        for x, y in zip(a, b):
            t3, dst = self._tensor(x, y, level), self.poison(2, level - 1, self.sch.n)
            self.ctx.keyswitch_mod_switch(level, t3[:2], t3[2], self.key().public_keys_ptr, dst)
            out.append(self.host(dst))
        return self._switched(out, level)

    def bgv_multiply_batched(self, a, b, level):
        t3 = self.torch.stack([self._tensor(x, y, level) for x, y in zip(a, b)])
        dst = self.poison(len(a), 2, level - 1, self.sch.n)
        self.ctx.keyswitch_mod_switch_batched(level, t3[:, :2].contiguous(), t3[:, 2].contiguous(), len(a), self.key().public_keys_ptr, dst)
        return self._switched(list(self.host(dst)), level)

    def bgv_mod_switch(self, ct, level):
        dst = self.poison(2, level - 1, self.sch.n)
        self.ctx.mod_t_and_divide_q_last_ntt(level, self.dev(ct), 2, dst)
        return self.host(dst), level - 1, self.sch.switch_factor(level)

    # -- BGV sums (c, d) ----------------------------------------------------------------------------------------------------------------
    def _operands(self, a, b):
        op1 = self.dev(np.stack([np.stack(row) for row in a]))
        op2 = self.dev(np.stack([np.stack(row) for row in b]) if isinstance(b[0], list) else np.stack(b))
        return op1, op2

    def bgv_inner(self, a, b, level):
        op1, op2 = self._operands(a, b)
        dst = self.poison(len(a), 2, level, self.sch.n)
        self.ctx.inner_product_relin_batched(level, op1, op2, len(a[0]), len(a), self.key().public_keys_ptr, self.kind, dst)
        return list(self.host(dst)), level, 1

    def bgv_inner_switch(self, a, b, level):
        op1, op2 = self._operands(a, b)
        dst = self.poison(len(a), 2, level - 1, self.sch.n)
        self.ctx.inner_product_relin_mod_switch_batched(level, op1, op2, len(a[0]), len(a), self.key().public_keys_ptr, dst)
        return self._switched(list(self.host(dst)), level)

    def bgv_plain_sum(self, plain, ct, acc, level):
        """The weights as the header prescribes: BatchEncoder plaintexts through bgv_lift_plain, one [level][N] each."""
        groups, terms, n = len(ct), len(ct[0]), self.sch.n
        d_plain, lifted = self.dev(plain), self.poison(groups, terms, level, n)
        for g in range(groups):
            for k in range(terms):
                self.ctx.bgv_lift_plain(level, d_plain[g, k], lifted[g, k])
        dst = self.poison(groups, 2, level - 1, n)
        self.ctx.plain_inner_product_rescale_batched(level, lifted, self.dev(np.stack([np.stack(row) for row in ct])),
                                                     None if acc is None else self.dev(np.stack(acc)), terms, groups, self.kind, dst)
        return self._switched(list(self.host(dst)), level)

    # -- hoisting (BGV e, BFV a) ------------------------------------------------------------------------------------------------------
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

    # -- BGV matrix-vector products (f, g) ----------------------------------------------------------------------------------------------
    def lift_wide(self, plain, level):
        """Plaintexts [count][N] below t (on the host) -> device [count][level + |P|][N] in NTT form over [Q_l || P]: every residue is
        the word itself (t is below every prime), so each plaintext is copied to its level + |P| rows and transformed there in one
        call whose last |P| limbs take the special primes' tables."""
        ctx, sch = self.ctx, self.sch
        rows = level + sch.size_p
        out = self.dev(plain)[:, None, :].repeat(1, rows, 1).contiguous()
        assert tuple(out.shape) == (len(plain), rows, sch.n)
        for k in range(len(plain)):
            ctx.nwt_2d_radix8_forward_inplace_include_special_mod(out[k], rows, 0, sch.size_qp, sch.size_p)
        return out

    def matvec_single(self, cts, level, diags, elts):
        from phantom_fhe_amd import workloads as W
        ws = list(self.lift_wide(diags, level))
        return [self.host(W.diag_matvec(self.ctx, level, self.dev(ct), elts, self.keys(elts), ws, self.kind)) for ct in cts]

    def matvec_batched(self, cts, level, diags, elts):
        from phantom_fhe_amd import workloads as W
        ws = list(self.lift_wide(diags, level))
        return list(self.host(W.diag_matvec_batch(self.ctx, level, self.dev(np.stack(cts)), elts, self.keys(elts), ws, self.kind)))

    def _weights(self, values, level):
        nb = len(values[0])
        flat = self.lift_wide(np.stack([w for row in values for w in row]), level)
        return [[flat[i * nb + j] for j in range(nb)] for i in range(len(values))]

    def bsgs_single(self, cts, level, baby, giant, values):
        from phantom_fhe_amd import workloads as W
        ws = self._weights(values, level)
        return [self.host(W.diag_matvec_bsgs(self.ctx, level, self.dev(ct), baby, self.keys(baby), giant, self.keys(giant), ws, self.kind))
                for ct in cts]

    def bsgs_batched(self, cts, level, baby, giant, values):
        from phantom_fhe_amd import workloads as W
        return list(self.host(W.diag_matvec_bsgs_batch(self.ctx, level, self.dev(np.stack(cts)), baby, self.keys(baby), giant, self.keys(giant),
                                                       self._weights(values, level), self.kind)))

    def bsgs_blocks(self, ct, level, baby, giant, blocks):
        from phantom_fhe_amd import workloads as W
        return list(self.host(W.diag_matvec_bsgs_blocks(self.ctx, level, self.dev(ct), baby, self.keys(baby), giant, self.keys(giant),
                                                        [self._weights(values, level) for values in blocks], self.kind)))

    # -- relinearize + rotate (BGV h, BFV b) ----------------------------------------------------------------------------------------------
    def relin_rotate_many(self, a, b, level, elt):
        from phantom_fhe_amd import workloads as W
        if self.sch.kind == O.BGV:
            d3 = self.torch.stack([self._tensor(x, y, level) for x, y in zip(a, b)])
        else:
            d3 = self.poison(len(a), 3, level, self.sch.n)
            self.ctx.bfv_multiply_behz_batched(self.dev(np.stack(a)), self.dev(np.stack(b)), d3)
        return list(self.host(W.relinearize_rotate_batch(self.ctx, level, d3, self.key(), self.key(elt), elt, self.kind)))

    # -- BFV multiplies (b, c) ----------------------------------------------------------------------------------------------------------
    def bfv_multiply(self, entry, same_tensor_squares=False):
        """case_products' multiply_many: the single entry `entry`, then keyswitch_inplace.  Equal operands go in as two buffers holding
        equal words unless same_tensor_squares (BEHZ: the same tensor twice squares)."""
        def run(a, b, level):
            out = []
            for x, y in zip(a, b):
                d1 = self.dev(x)
                d2 = d1 if y is x and same_tensor_squares else self.dev(y)
                d3 = self.poison(3, level, self.sch.n)
                getattr(self.ctx, entry)(d1, d2, d3)
                self.ctx.keyswitch_inplace(level, d3[:2], d3[2], self.key().public_keys_ptr, self.kind)
                out.append(self.host(d3[:2]))
            return out, level, 1
        return run

    def bfv_multiply_batched(self, entry, size_ql=None):
        """The batched entry (with size_ql: bfv_multiply_hps_overq_batched at that level), then the key switch: batched at the top level,
        keyswitch_inplace_bfv_leveled per ciphertext with levels dropped."""
        def run(a, b, level):
            d1, d2 = self.dev(np.stack(a)), self.dev(np.stack(b))
            d3 = self.poison(len(a), 3, level, self.sch.n)
            getattr(self.ctx, entry)(*([] if size_ql is None else [size_ql]), d1, d2, d3)
            ct, c2 = d3[:, :2].contiguous(), d3[:, 2].contiguous()
            if size_ql is None or size_ql == level:
                self.ctx.keyswitch_inplace_batched(level, ct, c2, len(a), self.key().public_keys_ptr, self.kind)
            else:
                for k in range(len(a)):
                    self.ctx.keyswitch_inplace_bfv_leveled(size_ql, ct[k], c2[k], self.key().public_keys_ptr)
            return list(self.host(ct)), level, 1
        return run

    def bfv_multiply_leveled(self, size_ql, fused):
        def run(a, b, level):
            out = []
            for x, y in zip(a, b):
                d1, d2 = self.dev(x), self.dev(y)
                if fused:
                    dst = self.poison(2, level, self.sch.n)
                    self.ctx.bfv_mul_relin_hps_overq_leveled(size_ql, d1, d2, self.key().public_keys_ptr, dst)
                else:
                    d3 = self.poison(3, level, self.sch.n)
                    self.ctx.bfv_multiply_hps_overq_leveled(size_ql, d1, d2, d3)
                    self.ctx.keyswitch_inplace_bfv_leveled(size_ql, d3[:2], d3[2], self.key().public_keys_ptr)
                    dst = d3[:2]
                out.append(self.host(dst))
            return out, level, 1
        return run

    # -- BFV plaintext operations (d) ---------------------------------------------------------------------------------------------------
    def plain_sum(self, plain, ct, acc, level):
        groups, terms = len(ct), len(ct[0])
        res = self.poison(groups, 2, level, self.sch.n)
        self.ctx.bfv_plain_inner_product_batched(level, self.dev(plain), self.dev(np.stack([np.stack(row) for row in ct])),
                                                 self.dev(np.stack(acc)), res, terms, groups)
        return list(self.host(res))

    def add_plain(self, ct, plain, level, subtract):
        d = self.dev(ct)
        self.ctx.bfv_add_plain(level, d, self.dev(plain), subtract=subtract)
        return self.host(d)

    def multiply_plain(self, ct, plain, level):
        d = self.dev(ct)
        self.ctx.bfv_multiply_plain(level, d, 2, self.dev(plain))
        return self.host(d)


@functools.lru_cache(maxsize=1)
def _setup(name, kind):
    return Device(name, kind)


def _release():
    import torch
    _setup.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _check(dev, gpu_res, cpu_res):
    """(i) exact in all slots by the helper's decryption, margin >= the oracle pipeline's - MARGIN_LOSS; (ii) the device's own
    decryption returns the same slots, and under BGV without the correction factor it does not."""
    both = list(zip(gpu_res, cpu_res)) if isinstance(gpu_res, list) else [(gpu_res, cpu_res)]
    for g, c in both:
        assert g.label == c.label and np.array_equal(g.want, c.want)
        print(f"{dev.sch.name} {g.label}: gpu margin {g.margin:.1f} bits, cpu margin {c.margin:.1f} bits, factor {g.factor}")
        assert c.exact and c.margin >= S.MIN_MARGIN, g.label
        S.check(g, floor=c.margin - S.MARGIN_LOSS)
        assert np.array_equal(dev.device_slots(g.cts, g.level, g.factor), g.want), f"{g.label}: batch_decrypt_decode differs"
        if g.factor != 1:
            assert S.differ(dev.device_slots(g.cts, g.level, None), g.want) > 0.5, f"{g.label}: right without the correction factor"


def _run(dev, case, cpu_impls, fns, *args):
    fns = fns if isinstance(fns, tuple) else (fns,)
    res = getattr(S, "case_" + case)(dev.sch, dev.codec, *fns, *args)
    _check(dev, res, S.cpu(dev.sch.name, dev.sch.kind, case, cpu_impls, *args))


# ==== BGV =============================================================================================================================
@pytest.mark.parametrize("level", [6, 3])
def test_bgv_rotations_and_row_swap(gpu, level):
    dev = _setup(*S.BGV12)
    for step in (1, 3, HALF12 - 1, None) if level == 6 else (1,):
        _run(dev, "rotation", "rotate_many", dev.rotate_single, level, step)
    if level == 6:
        _run(dev, "rotation", "rotate_many", dev.rotate_batched, level, 1, 3)
    _release()


def test_bgv_rotation_and_product_at_2_to_the_14(gpu):
    dev = _setup(*S.BGV14)
    _run(dev, "rotation", "rotate_many", dev.rotate_single, 8, 1)
    _run(dev, "products", "bgv_multiply_many", dev.bgv_multiply_fused, 8, 1)
    _release()


def test_bgv_products_carry_q_last_inverse(gpu):
    """Decoded with q_last^-1 the product is exact; with factor 1, the factor squared or the factor un-inverted it is wrong
    (bv_semantics.check runs the three controls on every result whose factor is not 1)."""
    dev = _setup(*S.BGV12)
    _run(dev, "products", "bgv_multiply_many", dev.bgv_multiply_unfused, 6, 1)
    _run(dev, "products", "bgv_multiply_many", dev.bgv_multiply_fused, 6, 1)
    _run(dev, "products", "bgv_multiply_many", dev.bgv_multiply_batched, 6, 3)
    _run(dev, "products", "bgv_multiply_many", dev.bgv_multiply_unfused, 6, 1, True)
    _run(dev, "products", "bgv_multiply_many", dev.bgv_multiply_fused, 3, 1)
    _release()


def test_bgv_encrypted_inner_products(gpu):
    dev = _setup(*S.BGV12)
    _run(dev, "inner_product", "bgv_inner", dev.bgv_inner, 6, 3, 2, False)
    _run(dev, "inner_product", "bgv_inner_switch", dev.bgv_inner_switch, 6, 3, 2, False)
    _run(dev, "inner_product", "bgv_inner_switch", dev.bgv_inner_switch, 6, 3, 2, True)
    _release()


@pytest.mark.parametrize("with_acc", [False, True])
def test_bgv_plain_weighted_sums(gpu, with_acc):
    dev = _setup(*S.BGV12)
    _run(dev, "plain_sum", "bgv_plain_sum", dev.bgv_plain_sum, 6, 3, 2, with_acc)
    _release()


def test_bgv_hoisting(gpu):
    dev = _setup(*S.BGV12)
    _run(dev, "hoisting", "hoist_many", dev.hoist_single, 6, (1, 2, 5), 1)
    _run(dev, "hoisting", "hoist_many", dev.hoist_batched, 6, (1, 2, 5), 3)
    _release()


def test_bgv_diag_matvec_multiplies_by_the_matrix(gpu):
    dev = _setup(*S.BGV12)
    _run(dev, "matvec", "matvec_many", dev.matvec_single, 6, 8, 1)
    _run(dev, "matvec", "matvec_many", dev.matvec_batched, 6, 8, 2)
    _release()


def test_bgv_bsgs_matvec_with_the_documented_preparation(gpu):
    dev = _setup(*S.BGV12)
    _run(dev, "bsgs", "bsgs_many", dev.bsgs_single, 6, 4, 2, 1)
    _run(dev, "bsgs", "bsgs_many", dev.bsgs_batched, 6, 4, 2, 2)
    _run(dev, "bsgs_blocks", "bsgs_blocks", dev.bsgs_blocks, 6, 4, 2, 3)
    # the control: the diagonals as they are, without the roll-back by the giant step, give another vector
    res = S.case_bsgs(dev.sch, dev.codec, dev.bsgs_single, 6, 4, 2, 1, prepare=S.bsgs_diagonals_without_roll_back)
    assert S.differ(res.got, res.want) > 0.5 and np.array_equal(res.got, res.wrongs[-1])
    _release()


def test_bgv_relinearize_rotate(gpu):
    dev = _setup(*S.BGV12)
    _run(dev, "relin_rotate", "bgv_relin_rotate_many", dev.relin_rotate_many, 6, 3)
    _release()


def test_bgv_depth_two_multiplies_the_factors(gpu):
    dev = _setup(*S.BGV12)
    _run(dev, "depth_two", ("+", "bgv_multiply_many", "mod_switch"), (dev.bgv_multiply_fused, dev.bgv_mod_switch), 6)
    _release()


# ==== BFV =============================================================================================================================
def test_bfv_rotations_row_swap_and_hoisting(gpu):
    dev = _setup(*S.BFV12)
    for step in (1, 3, HALF12 - 1, None):
        _run(dev, "rotation", "rotate_many", dev.rotate_single, 2, step)
    _run(dev, "hoisting", "hoist_many", dev.hoist_single, 2, (1, 2, 5), 1)
    _run(dev, "hoisting", "hoist_many", dev.hoist_batched, 2, (1, 2, 5), 3)
    _release()


def test_bfv_behz_multiplies_and_relinearize_rotate(gpu):
    dev = _setup(*S.BFV12)
    behz = ("bfv_multiply_many", "behz")
    _run(dev, "products", behz, dev.bfv_multiply("bfv_multiply_behz"), 2, 1)
    _run(dev, "products", behz, dev.bfv_multiply("bfv_multiply_behz", same_tensor_squares=True), 2, 1, True)
    _run(dev, "products", behz, dev.bfv_multiply_batched("bfv_multiply_behz_batched"), 2, 3)
    _run(dev, "relin_rotate", "bfv_relin_rotate_many", dev.relin_rotate_many, 2, 3)
    _release()


def test_bfv_hps_multiplies(gpu):
    dev = _setup(*S.BFV13)
    hps, overq = ("bfv_multiply_many", "hps"), ("bfv_multiply_many", "overq")
    _run(dev, "products", hps, dev.bfv_multiply("bfv_multiply_hps"), 4, 1)
    _run(dev, "products", hps, dev.bfv_multiply_batched("bfv_multiply_hps_batched"), 4, 2)
    _run(dev, "products", overq, dev.bfv_multiply("bfv_multiply_hps_overq"), 4, 1)
    _run(dev, "products", overq, dev.bfv_multiply("bfv_multiply_hps_overq"), 4, 1, True)       # two buffers holding equal words
    _run(dev, "products", overq, dev.bfv_multiply_batched("bfv_multiply_hps_overq_batched", 4), 4, 2)
    _release()


def test_bfv_leveled_multiplies_and_depth_two(gpu):
    dev = _setup(*S.BFV13)
    _run(dev, "products", ("bfv_multiply_leveled", 3, False), dev.bfv_multiply_leveled(3, False), 4, 1)
    _run(dev, "products", ("bfv_multiply_leveled", 3, True), dev.bfv_multiply_leveled(3, True), 4, 1)
    _run(dev, "products", ("bfv_multiply_leveled", 3, False), dev.bfv_multiply_batched("bfv_multiply_hps_overq_batched", 3), 4, 2)
    _run(dev, "depth_two", ("+", ("bfv_multiply_many", "hps"), None), (dev.bfv_multiply("bfv_multiply_hps"), None), 4)
    _run(dev, "depth_two", ("+", ("bfv_multiply_many", "overq"), None), (dev.bfv_multiply("bfv_multiply_hps_overq"), None), 4)
    _release()


def test_bfv_hps_overq_same_pointer_keeps_the_shortcut(gpu):
    """pha_bfv_multiply_hps_overq with ct1 == ct2 as the SAME pointer keeps the reference's squaring shortcut, whose result is scaled by
    Q / Rl: relinearised, t phase / Q is nowhere near the integers (margin below one bit) and the slots are not m^2.  The oracle,
    given the same object twice, has the same words; no exactness is claimed for this call."""
    dev = _setup(*S.BFV13)
    sch, level = dev.sch, 4
    z = S.messages(12, 1, sch.n)
    a = S._enc(sch, dev.codec, z, level, "mul.a")[0]
    d1, d3 = dev.dev(a), dev.poison(3, level, sch.n)
    dev.ctx.bfv_multiply_hps_overq(d1, d1, d3)
    ref = S.Reference(sch)
    assert np.array_equal(dev.host(d3), ref.multiplier("overq").multiply(a, a)), "the oracle's same-object square has other words"
    dev.ctx.keyswitch_inplace(level, d3[:2], d3[2], dev.key().public_keys_ptr, dev.kind)
    got, margin = sch.decode_ct(dev.host(d3[:2]), level)
    print(f"same pointer: margin {margin:.2f} bits, {S.differ(got, z[0] * z[0] % S.TU):.3f} of the slots differ from m^2")
    assert margin < 1 and S.differ(got, z[0] * z[0] % S.TU) > 0.5
    _release()


def test_bfv_plaintext_operations(gpu):
    dev = _setup(*S.BFV12)
    _check(dev, S.case_bfv_plain_ops(dev.sch, dev.codec, dev, 2), S.cpu(dev.sch.name, dev.sch.kind, "bfv_plain_ops", "self", 2))
    _release()


def test_bfv_is_refused_where_the_entry_has_no_bfv_form(gpu):
    """Weighted hoisting and the NTT-form summed products are ckks / bgv only: under bfv the refusal is the behaviour."""
    dev = _setup(*S.BFV12)
    sch, level, n = dev.sch, 2, dev.sch.n
    ct = S._enc(sch, dev.codec, S.messages(50, 1, n), level, "refuse")[0]
    elts = [S.elt_of_step(1, n)]
    w = dev.poison(level + sch.size_p, n)
    d, keep = dev.dev(ct), dev.dev(ct)
    with pytest.raises(ValueError):
        dev.ctx.hoisting_weighted(level, d, elts, dev.keys(elts), [w], dev.kind)
    op = dev.dev(ct[None, None])
    dst = dev.poison(1, 2, level, n)
    with pytest.raises(ValueError):
        dev.ctx.inner_product_relin_batched(level, op, op, 1, 1, dev.key().public_keys_ptr, dev.kind, dst)
    with pytest.raises(ValueError):
        dev.ctx.plain_inner_product_rescale_batched(level, dev.poison(1, 1, level, n), op, None, 1, 1, dev.kind, dev.poison(1, 2, level - 1, n))
    dev.torch.cuda.synchronize()
    assert dev.torch.equal(d, keep) and bool((dst == S.GpuCodec.POISON).all()), "a refused call wrote"
    _release()


# ==== pyPhantom =======================================================================================================================
class PyPhantom:
    """A pyPhantom context at the scheme's parameters with keys generated from the helper's randomness."""

    def __init__(self, sch, mul_tech=None):
        from phantom_fhe_amd import pyPhantom as ph
        self.ph, self.sch = ph, sch
        self.kind = {O.BGV: ph.scheme_type.bgv, O.BFV: ph.scheme_type.bfv}[sch.kind]
        parms = ph.params(self.kind)
        parms.set_poly_modulus_degree(sch.n)
        parms.set_special_modulus_size(sch.size_p)
        parms.set_coeff_modulus([ph.modulus(int(p)) for p in sch.primes])
        parms.set_plain_modulus(ph.modulus(S.T))
        if mul_tech:
            parms.set_mul_tech(getattr(ph.mul_tech_type, mul_tech))
        self.ctx = ph.context(parms)
        self.rlk = self._generate(sch.relin_randomness())
        self.glk = ph.galois_key()
        for step in S.HOST_STEPS:
            elt = ph.get_elt_from_step(step, sch.n)
            assert elt == S.elt_of_step(step, sch.n), step
            self.glk.load(self.ctx, elt, self._generate(sch.galois_randomness(elt)).to_numpy())

    def _generate(self, randomness):
        new_key, a, e = randomness
        key = self.ph.relin_key()
        key.generate(self.ctx, self.sch.sk_ntt, new_key, a, e)
        return key

    def pt(self, plain):
        p = self.ph.plaintext()
        p.load(np.ascontiguousarray(plain, dtype=np.uint64)[None])
        return p


class PyPhantomBgv(PyPhantom):
    """case_host_bgv's `api`: (numpy, limbs, factor) in and out; the factor going out is what correction_factor() reports."""

    def _ct(self, x):
        h, limbs, factor = x
        ct = self.ph.ciphertext()
        ct.load(self.ctx, 1 + self.sch.size_q - limbs, np.ascontiguousarray(h))
        ct.set_correction_factor(int(factor))
        return ct

    @staticmethod
    def _out(ct):
        assert ct.is_ntt_form() and ct.size() == 2
        return ct.to_numpy(), ct.coeff_modulus_size(), ct.correction_factor()

    def multiply_relin_mod_switch(self, x, y):
        return self._out(self.ph.multiply_relin_mod_switch(self.ctx, self._ct(x), self._ct(y), self.rlk))

    def multiply_relinearize_switch(self, x, y):
        prod = self.ph.relinearize(self.ctx, self.ph.multiply(self.ctx, self._ct(x), self._ct(y)), self.rlk)
        return self._out(self.ph.mod_switch_to_next(self.ctx, prod))

    def mod_switch(self, x):
        return self._out(self.ph.mod_switch_to_next(self.ctx, self._ct(x)))

    def rotate(self, x, step):
        return self._out(self.ph.rotate(self.ctx, self._ct(x), step, self.glk))

    def hoisting(self, x, steps):
        return self._out(self.ph.hoisting(self.ctx, self._ct(x), self.glk, list(steps)))

    def add(self, x, y):
        return self._out(self.ph.add(self.ctx, self._ct(x), self._ct(y)))

    def sub(self, x, y):
        return self._out(self.ph.sub(self.ctx, self._ct(x), self._ct(y)))

    def add_many(self, xs):
        return self._out(self.ph.add_many(self.ctx, [self._ct(x) for x in xs]))

    def add_plain(self, x, plain):
        return self._out(self.ph.add_plain(self.ctx, self._ct(x), self.pt(plain)))

    def multiply_plain(self, x, plain):
        return self._out(self.ph.multiply_plain(self.ctx, self._ct(x), self.pt(plain)))


class PyPhantomBfv(PyPhantom):
    """case_host_bfv's `api`: numpy ciphertexts [2][Q][N] in coefficient form."""

    def _ct(self, h):
        ct = self.ph.ciphertext()
        ct.load(self.ctx, 1, np.ascontiguousarray(h))
        ct.set_ntt_form(False)
        return ct

    @staticmethod
    def _out(ct):
        assert not ct.is_ntt_form() and ct.size() == 2
        return ct.to_numpy()

    def multiply_and_relin(self, a, b):
        return self._out(self.ph.multiply_and_relin(self.ctx, self._ct(a), self._ct(b), self.rlk))

    def rotate(self, a, step):
        return self._out(self.ph.rotate(self.ctx, self._ct(a), step, self.glk))

    def add_plain(self, a, plain, subtract):
        return self._out((self.ph.sub_plain if subtract else self.ph.add_plain)(self.ctx, self._ct(a), self.pt(plain)))

    def multiply_plain(self, a, plain):
        return self._out(self.ph.multiply_plain(self.ctx, self._ct(a), self.pt(plain)))

    def add_many(self, cts):
        return self._out(self.ph.add_many(self.ctx, [self._ct(c) for c in cts]))


def test_pyphantom_bgv_reports_the_factor_that_decrypts(gpu):
    """host/phantom.h at scheme_type.bgv: after every operation correction_factor() is the factor under which the helper's decryption
    is exact -- the product of the factors in multiply, q_last^-1 more per switch (bgv_switched_correction_factor), the common factor
    of balance_correction_factors in add, sub and add_many of operands with different factors, add_plain scaled by the factor."""
    dev = _setup(*S.BGV12)
    api = PyPhantomBgv(dev.sch)
    _check(dev, S.case_host_bgv(dev.sch, dev.codec, api), S.cpu_host(*S.BGV12))
    del api
    _release()


@pytest.mark.parametrize("name,kind,tech", [S.BFV12 + ("behz",), S.BFV13 + ("hps",)])
def test_pyphantom_bfv(gpu, name, kind, tech):
    dev = _setup(name, kind)
    api = PyPhantomBfv(dev.sch, tech)
    _check(dev, S.case_host_bfv(dev.sch, dev.codec, api), S.cpu_host(name, kind, tech))
    del api
    _release()
