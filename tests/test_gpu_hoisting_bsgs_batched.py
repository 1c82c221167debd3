"""GPU parity of the batched baby-step / giant-step hoisted rotations (pha_hoisting_weighted_bsgs_batched): every ciphertext of every
batch word for word against B calls of the single-ciphertext entry, the first and the last one also against the oracle's
Tool.hoisting_weighted_bsgs; chunk invariance, in place, B = 1, extreme residues, refusals, strict mode, the workload wrapper,
N = 2^16 on both sides of the fused-conversion threshold.  Configuration names are those of tests/util.py; keys and weights are
uniform synthetic (the arithmetic is data-independent)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from util import oracle_ctx, primes_of, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

BGV_T = 65537
CANARY = 0x5A5A5A5A5A5A5A5A


class Setup:
    """Contexts of one (configuration, scheme, level) on both sides and the operands of one (baby, giant) split."""

    def __init__(self, name, scheme, ql, gpu):
        import phantom_fhe_amd as P
        self.P, self.gpu, self.scheme, self.ql = P, gpu, scheme, ql
        self.log_n, self.primes, self.size_p = primes_of(name)
        self.n = 1 << self.log_n
        self.size_q = len(self.primes) - self.size_p
        self.oc = oracle_ctx(name)
        self.ctx = P.PhantomContext(self.log_n, list(self.primes), self.size_p, device=gpu)
        self.tool = O.Tool(self.oc, ql)
        if scheme == O.BGV:
            self.ctx.set_plain_modulus(BGV_T)
            self.tool.set_plain_modulus(BGV_T)
        self.qlp_primes = [self.primes[i] for i in list(range(ql)) + [self.size_q + j for j in range(self.size_p)]]

    def host_key(self, rng, fill=None):
        """One Galois key [dnum][2][QP][N]; fill(q) -> a constant word per limb instead of uniform ones."""
        dnum = -(-self.size_q // self.size_p)
        if fill is None:
            return np.stack([np.stack([uniform_poly(rng, self.primes, self.n) for _ in range(2)]) for _ in range(dnum)])
        row = np.stack([np.full(self.n, fill(q), dtype=np.uint64) for q in self.primes])
        return np.stack([np.stack([row, row])] * dnum)

    def split(self, rng, nb, ng, ident, pool=None, null=None):
        """Elements, keys and weights of an nb x ng split; ident: element 1 leads both lists.  Keys cycle over `pool` distinct ones."""
        first = 0 if ident else 1
        self.baby = [int(pow(5, k, 2 * self.n)) for k in range(first, first + nb)]
        self.giant = [int(pow(5, nb * k, 2 * self.n)) for k in range(first, first + ng)]
        n_keys = sum(e != 1 for e in self.baby + self.giant)
        self.key_pool = [self.host_key(rng) for _ in range(n_keys if pool is None else min(pool, n_keys))]
        self.h_w = [[uniform_poly(rng, self.qlp_primes, self.n) for _ in self.baby] for _ in self.giant]
        if null is not None:
            self.h_w[null[0]][null[1]] = None
        self.upload()

    def upload(self):
        """Device and oracle forms of the key pool and the weights."""
        P = self.P
        dev = [P.PhantomRelinKey.from_numpy(k, self.gpu) for k in self.key_pool]
        it = iter(range(1 << 30))
        slots = [None if e == 1 else next(it) % len(dev) for e in self.baby + self.giant]
        nb = len(self.baby)
        self.d_bk = [None if z is None else dev[z] for z in slots[:nb]]
        self.d_gk = [None if z is None else dev[z] for z in slots[nb:]]
        okey = lambda z: None if z is None else [self.key_pool[z][d] for d in range(self.tool.beta)]
        self.o_bk, self.o_gk = [okey(z) for z in slots[:nb]], [okey(z) for z in slots[nb:]]
        self.d_w = [[None if w is None else P.to_device(w, self.gpu) for w in row] for row in self.h_w]

    def cts(self, rng, batch):
        return np.stack([np.stack([uniform_poly(rng, self.primes[:self.ql], self.n) for _ in range(2)]) for _ in range(batch)])

    def batched(self, d_ct, **kw):
        return self.ctx.hoisting_weighted_bsgs_batched(self.ql, d_ct, self.baby, self.d_bk, self.giant, self.d_gk, self.d_w, self.scheme, **kw)

    def singles(self, cts):
        """B calls of the single-ciphertext entry."""
        out = []
        for ct in cts:
            d = self.P.to_device(ct, self.gpu)
            self.ctx.hoisting_weighted_bsgs(self.ql, d, self.baby, self.d_bk, self.giant, self.d_gk, self.d_w, self.scheme)
            out.append(self.P.to_host(d))
        return np.stack(out)

    def oracle(self, ct):
        return self.tool.hoisting_weighted_bsgs(ct, self.baby, self.o_bk, self.giant, self.o_gk, self.h_w, self.scheme)


# ---- A. parity per ciphertext ----------------------------------------------------------------------------------------------------
CASES = [
    ("hyb12_a2", O.CKKS, 5, 4, 3, True, 5),          # beta = 3, short last digit; one full group of 4 + a tail of 1; a missing weight
    ("hyb12_a2", O.BGV, 6, 3, 2, True, 2),
    ("hyb12_a2", O.CKKS, 2, 3, 2, True, 3),          # beta = 1
    ("hyb13_a3", O.CKKS, 7, 4, 2, False, 3),         # no identity steps
    ("hyb13_a3", O.CKKS, 9, 2, 9, True, 3),          # G = 9: the NG ladder 8 + 1
    ("hyb13_b5", O.CKKS, 8, 3, 2, True, 3),          # beta = 4
    ("c1_bfv4096", O.CKKS, 2, 3, 2, True, 3),        # alpha = 1: the mod-up's per-ciphertext loop
    ("p61_a2", O.CKKS, 6, 20, 2, True, 2),           # 61-bit special primes
]


@pytest.mark.parametrize("name,scheme,ql,nb,ng,ident,batch", CASES)
def test_every_ciphertext_equals_the_single_entry_and_the_oracle(name, scheme, ql, nb, ng, ident, batch, gpu):
    s = Setup(name, scheme, ql, gpu)
    r = rng_for(6100 + 64 * ql + 8 * nb + ng)
    first_case = (name, scheme, ql, nb) == CASES[0][:4]
    s.split(r, nb, ng, ident, pool=3 if nb + ng > 8 else None, null=(ng - 1, nb - 1) if first_case else None)
    cts = s.cts(r, batch)
    d_ct = s.P.to_device(cts, gpu)
    got = s.P.to_host(s.batched(d_ct))
    assert np.array_equal(s.P.to_host(d_ct), cts), "ct is only read"
    ref = s.singles(cts)
    for b in range(batch):
        assert np.array_equal(got[b], ref[b]), f"ciphertext {b} of {batch} differs from pha_hoisting_weighted_bsgs"
    for b in (0, batch - 1):
        assert np.array_equal(got[b], s.oracle(cts[b])), f"ciphertext {b} of {batch} differs from the oracle"


# ---- B, C. chunk invariance, in place, B = 1 ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five(gpu):
    """The first case's shape with five ciphertexts and the single entry's results -- made once."""
    name, scheme, ql, nb, ng, ident, batch = CASES[0]
    s = Setup(name, scheme, ql, gpu)
    r = rng_for(6200)
    s.split(r, nb, ng, ident, null=(1, 2))
    cts = s.cts(r, batch)
    return s, cts, s.singles(cts)


def test_every_chunk_size_gives_the_same_words(five, gpu):
    s, cts, ref = five
    d_ct = s.P.to_device(cts, gpu)
    for chunk in (1, 2, 3, 4, 0):
        got = s.P.to_host(s.batched(d_ct, chunk=chunk))
        assert np.array_equal(got, ref), f"chunk = {chunk} differs from {len(cts)} calls of pha_hoisting_weighted_bsgs"
    assert np.array_equal(s.P.to_host(d_ct), cts), "ct is only read"


def test_in_place(five, gpu):
    s, cts, ref = five
    for chunk in (0, 2):
        d_ct = s.P.to_device(cts, gpu)
        assert s.batched(d_ct, out=d_ct, chunk=chunk) is d_ct
        assert np.array_equal(s.P.to_host(d_ct), ref), f"in place, chunk = {chunk}"


def test_a_batch_of_one(five, gpu):
    s, cts, ref = five
    one = s.P.to_device(cts[:1], gpu)
    assert np.array_equal(s.P.to_host(s.batched(one)), ref[:1]), "B = 1 differs from the single entry"
    s.batched(one, out=one)
    assert np.array_equal(s.P.to_host(one), ref[:1]), "B = 1 in place differs from the single entry"


# ---- D. extreme residues ---------------------------------------------------------------------------------------------------------
def test_extreme_residues(gpu):
    """Ciphertext words at q - 1, 0 and q - 1 - r inside one batch; one baby key, one giant key and one weight at q - 1 throughout."""
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    r = rng_for(6300)
    s.split(r, 3, 2, True)                             # keys: baby 5, baby 25, giant 125
    s.key_pool[1] = s.host_key(r, fill=lambda q: q - 1)
    s.key_pool[2] = s.host_key(r, fill=lambda q: q - 1)
    s.h_w[1][1] = np.stack([np.full(s.n, q - 1, dtype=np.uint64) for q in s.qlp_primes])
    s.upload()
    top = np.stack([np.full(s.n, q - 1, dtype=np.uint64) for q in s.primes[:s.ql]])
    near = np.stack([np.stack([np.uint64(q - 1) - r.integers(0, 1 << 16, s.n, dtype=np.uint64) for q in s.primes[:s.ql]]) for _ in range(2)])
    cts = np.stack([np.stack([top, top]), np.zeros((2, s.ql, s.n), dtype=np.uint64), near])
    got = s.P.to_host(s.batched(s.P.to_device(cts, gpu)))
    ref = s.singles(cts)
    for b in range(3):
        assert np.array_equal(got[b], ref[b]), f"ciphertext {b} differs from the single entry"
        assert np.array_equal(got[b], s.oracle(cts[b])), f"ciphertext {b} differs from the oracle"


# ---- E. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_and_ct_untouched(gpu):
    import torch
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    P, ql, ctx = s.P, s.ql, s.ctx
    r = rng_for(6400)
    s.split(r, 3, 2, True)
    cts = s.cts(r, 3)
    d_ct = P.to_device(cts, gpu)
    canary = np.full(cts.shape, CANARY, dtype=np.uint64)
    out = P.to_device(canary, gpu)

    def call(baby=s.baby, bk=s.d_bk, giant=s.giant, gk=s.d_gk, w=s.d_w, scheme=s.scheme, ct=d_ct, o=out, c=ctx, level=ql):
        return c.hoisting_weighted_bsgs_batched(level, ct, baby, bk, giant, gk, w, scheme, out=o)

    def untouched():
        torch.cuda.synchronize()
        assert np.array_equal(P.to_host(out), canary), "a refused call wrote to out"
        assert np.array_equal(P.to_host(d_ct), cts), "a refused call wrote to ct"

    with pytest.raises(ValueError):                                       # empty step lists
        call(baby=[], bk=[], w=[[], []])
    with pytest.raises(ValueError):
        call(giant=[], gk=[], w=[])
    untouched()
    with pytest.raises(ArithmeticError):                                  # a keyed element without its key (std::logic_error)
        call(bk=[None, s.d_bk[1], None])
    with pytest.raises(ArithmeticError):
        call(gk=[None, None])
    untouched()
    with pytest.raises(ValueError):                                       # an even Galois element
        call(baby=[1, 5, 4])
    with pytest.raises(ValueError):
        call(giant=[1, 6])
    untouched()
    with pytest.raises(ValueError):                                       # bfv
        call(scheme=O.BFV)
    untouched()
    # out overlapping ct by one polynomial (everything but the exact in-place form is refused)
    polys = np.concatenate([cts.reshape(6, ql, s.n), np.full((1, ql, s.n), CANARY, dtype=np.uint64)])
    buf = P.to_device(polys, gpu)
    ct_v, out_v = buf[:6].view(3, 2, ql, s.n), buf[1:].view(3, 2, ql, s.n)
    with pytest.raises(ValueError):
        call(ct=ct_v, o=out_v)
    torch.cuda.synchronize()
    assert np.array_equal(P.to_host(buf), polys), "a refused call wrote to the overlapping buffers"
    # batch == 0: OK, nothing happens (raw entry: real buffers, zero ciphertexts)
    from phantom_fhe_amd import lib as plib
    L = plib.load()
    stream = torch.cuda.current_stream().cuda_stream
    be, ge = (C.c_uint32 * 3)(*s.baby), (C.c_uint32 * 2)(*s.giant)
    bk = (C.c_void_p * 3)(*[None if k is None else k.public_keys_ptr.data_ptr() for k in s.d_bk])
    gk = (C.c_void_p * 2)(*[None if k is None else k.public_keys_ptr.data_ptr() for k in s.d_gk])
    ws = (C.c_void_p * 6)(*[w.data_ptr() for row in s.d_w for w in row])
    assert L.pha_hoisting_weighted_bsgs_batched(ctx._h, ql, d_ct.data_ptr(), 0, be, 3, bk, ge, 2, gk, ws, int(s.scheme), out.data_ptr(), 0,
                                                stream) == 0
    untouched()
    assert s.batched(d_ct[:0]).shape[0] == 0
    untouched()


def test_five_digits_are_refused(gpu):
    """beta = 5 (hyb13_b5, level 10): refused like the single entry, nothing written."""
    import torch
    s = Setup("hyb13_b5", O.CKKS, 10, gpu)
    assert s.tool.beta == 5
    r = rng_for(6450)
    s.split(r, 2, 2, True, pool=1)
    cts = s.cts(r, 2)
    d_ct = s.P.to_device(cts, gpu)
    canary = np.full(cts.shape, CANARY, dtype=np.uint64)
    out = s.P.to_device(canary, gpu)
    with pytest.raises(ValueError):
        s.batched(d_ct, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(s.P.to_host(out), canary) and np.array_equal(s.P.to_host(d_ct), cts)


# ---- F. strict mode --------------------------------------------------------------------------------------------------------------
def test_strict_mode_counts_every_ciphertext_of_the_batch(gpu):
    import torch
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    P = s.P
    r = rng_for(6500)
    s.split(r, 3, 2, True)
    cts = s.cts(r, 4)
    bad = cts.copy()
    bad[2, 1, 3, 17] = np.uint64(s.primes[3])          # ciphertext 3 of 4: one word equal to its modulus
    canary = np.full(cts.shape, CANARY, dtype=np.uint64)
    out = P.to_device(canary, gpu)
    d_bad, d_ok = P.to_device(bad, gpu), P.to_device(cts, gpu)
    before = P.set_strict(True)
    try:
        with pytest.raises(ValueError, match="PHA_STRICT"):
            s.batched(d_bad, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(P.to_host(out), canary), "a strict-mode refusal wrote to out"
        strict = P.to_host(s.batched(d_ok))            # canonical operands: computed as usual
    finally:
        P.set_strict(before)
    assert np.array_equal(strict, P.to_host(s.batched(d_ok)))


# ---- G. the workload -------------------------------------------------------------------------------------------------------------
def test_diag_matvec_bsgs_batch_equals_diag_matvec_bsgs_per_vector(gpu):
    from phantom_fhe_amd import workloads as W
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    r = rng_for(6600)
    s.split(r, 3, 2, True)
    d_cts = s.P.to_device(s.cts(r, 3), gpu)
    out = W.diag_matvec_bsgs_batch(s.ctx, s.ql, d_cts, s.baby, s.d_bk, s.giant, s.d_gk, s.d_w, s.scheme)
    assert tuple(out.shape) == tuple(d_cts.shape)
    for b in range(3):
        one = W.diag_matvec_bsgs(s.ctx, s.ql, d_cts[b], s.baby, s.d_bk, s.giant, s.d_gk, s.d_w, s.scheme)
        assert np.array_equal(s.P.to_host(out[b]), s.P.to_host(one)), f"vector {b}"


# ---- H. N = 2^16 on both sides of the fused-conversion threshold -----------------------------------------------------------------
@pytest.fixture(scope="module")
def n16(gpu):
    """hyb16_a12, level 24 (beta = 2), 2 x 2 steps with the identity first, four ciphertexts: inputs, the single entry's results
    and the oracle's for ciphertext 0 -- made once."""
    s = Setup("hyb16_a12", O.CKKS, 24, gpu)
    assert s.tool.beta == 2
    r = rng_for(6700)
    s.split(r, 2, 2, True)
    cts = s.cts(r, 4)
    return s, cts, s.singles(cts), s.oracle(cts[0])


@pytest.mark.parametrize("batch", [3, 4], ids=["below", "at"])
def test_n16_both_sides_of_the_fused_conversion_threshold(batch, n16, gpu):
    """One chunk of B ciphertexts: the baby mod-down has 2 G B = 12 polynomials at B = 3, below the 16 polynomials / 1024 workgroups
    from which the mod-down takes its conversion fused into the transform, and 16 at B = 4."""
    s, cts, singles, oracle0 = n16
    got = s.P.to_host(s.batched(s.P.to_device(cts[:batch], gpu), chunk=batch))
    assert np.array_equal(got[0], oracle0), "ciphertext 0 differs from the oracle"
    assert np.array_equal(got, singles[:batch]), "differs from single pha_hoisting_weighted_bsgs calls"


# ---- I. refusals of the single and the row-block entry --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single_refusals(gpu):
    """hyb12_a2, level 6, 3 x 2 steps with the identity first, one ciphertext -- made once."""
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    r = rng_for(6800)
    s.split(r, 3, 2, True)
    return s, s.cts(r, 1)[0]


@pytest.mark.parametrize("defect,exc", [("even", ValueError), ("beyond_2n", ValueError), ("missing_key", ArithmeticError)])
@pytest.mark.parametrize("side", ["baby", "giant"])
def test_single_entry_refusals_leave_ct_untouched(side, defect, exc, single_refusals, gpu):
    """pha_hoisting_weighted_bsgs with exactly one defect per call: the exception class, and ct keeps its words."""
    import torch
    s, ct = single_refusals
    baby, giant, bk, gk = list(s.baby), list(s.giant), list(s.d_bk), list(s.d_gk)
    elts, keys = (baby, bk) if side == "baby" else (giant, gk)
    if defect == "even":
        elts[-1] = 4
    elif defect == "beyond_2n":
        elts[-1] = 2 * s.n + 5
    else:
        keys[-1] = None
    d_ct = s.P.to_device(ct, gpu)
    with pytest.raises(exc):
        s.ctx.hoisting_weighted_bsgs(s.ql, d_ct, baby, bk, giant, gk, s.d_w, s.scheme)
    torch.cuda.synchronize()
    assert np.array_equal(s.P.to_host(d_ct), ct), "a refused call wrote to ct"


def test_single_entry_refuses_five_digits(gpu):
    """beta = 5 (hyb13_b5, level 10): pha_hoisting_weighted_bsgs refuses, ct keeps its words."""
    import torch
    s = Setup("hyb13_b5", O.CKKS, 10, gpu)
    assert s.tool.beta == 5
    r = rng_for(6850)
    s.split(r, 2, 2, True, pool=1)
    ct = s.cts(r, 1)[0]
    d_ct = s.P.to_device(ct, gpu)
    with pytest.raises(ValueError):
        s.ctx.hoisting_weighted_bsgs(s.ql, d_ct, s.baby, s.d_bk, s.giant, s.d_gk, s.d_w, s.scheme)
    torch.cuda.synchronize()
    assert np.array_equal(s.P.to_host(d_ct), ct), "a refused call wrote to ct"


def test_blocks_entry_refuses_out_overlapping_ct(single_refusals, gpu):
    """pha_hoisting_weighted_bsgs_blocks, one block whose out starts at ct's second polynomial: refused, nothing written."""
    import torch
    s, ct = single_refusals
    polys = np.concatenate([ct, np.full((1, s.ql, s.n), CANARY, dtype=np.uint64)])
    buf = s.P.to_device(polys, gpu)
    with pytest.raises(ValueError):
        s.ctx.hoisting_weighted_bsgs_blocks(s.ql, buf[:2], s.baby, s.d_bk, s.giant, s.d_gk, [s.d_w], buf[1:].view(1, 2, s.ql, s.n), s.scheme)
    torch.cuda.synchronize()
    assert np.array_equal(s.P.to_host(buf), polys), "a refused call wrote to the overlapping buffers"


# ---- J. one scratch claim per call ----------------------------------------------------------------------------------------------
def test_tail_of_one_on_a_fresh_and_on_a_warm_context(five, gpu):
    """Five ciphertexts at the default chunk (a group of four and a tail of one) as the FIRST hoisting call of a new context, whose
    scratch arena therefore grows inside this call, then the same call again on the warm context: both equal five single calls."""
    s, cts, ref = five
    fresh = s.P.PhantomContext(s.log_n, list(s.primes), s.size_p, device=gpu)
    d_ct = s.P.to_device(cts, gpu)
    for state in ("fresh", "warm"):
        got = fresh.hoisting_weighted_bsgs_batched(s.ql, d_ct, s.baby, s.d_bk, s.giant, s.d_gk, s.d_w, s.scheme)
        assert np.array_equal(s.P.to_host(got), ref), f"{state} context: differs from five calls of pha_hoisting_weighted_bsgs"
    assert np.array_equal(s.P.to_host(d_ct), cts), "ct is only read"


# ---- K. one row block ------------------------------------------------------------------------------------------------------------
def test_one_row_block_equals_the_single_entry_and_the_oracle(gpu):
    """pha_hoisting_weighted_bsgs_blocks at n_blocks = 1 with nine giant steps (the NG ladder runs 8 + 1): word for word
    pha_hoisting_weighted_bsgs on a copy, and the oracle."""
    s = Setup("hyb13_a3", O.CKKS, 9, gpu)
    r = rng_for(6900)
    s.split(r, 2, 9, True, pool=3)
    ct = s.cts(r, 1)[0]
    d_ct = s.P.to_device(ct, gpu)
    out = s.P.to_device(np.full((1,) + ct.shape, CANARY, dtype=np.uint64), gpu)
    s.ctx.hoisting_weighted_bsgs_blocks(s.ql, d_ct, s.baby, s.d_bk, s.giant, s.d_gk, [s.d_w], out, s.scheme)
    got = s.P.to_host(out)[0]
    assert np.array_equal(s.P.to_host(d_ct), ct), "ct is only read"
    assert np.array_equal(got, s.singles(ct[None])[0]), "differs from pha_hoisting_weighted_bsgs"
    assert np.array_equal(got, s.oracle(ct)), "differs from the oracle"
