"""GPU parity of the batched hoisted rotations (pha_hoisting_batched, pha_hoisting_weighted_batched): every ciphertext of every
batch against the oracle's Tool.hoisting / Tool.hoisting_weighted of that ciphertext alone, bit-exact, and word for word against
the single-ciphertext entries; chunk invariance, in place, extreme residues, refusals, strict mode, the workload wrapper.
Configuration names are those of tests/util.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from util import oracle_ctx, primes_of, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

BGV_T = 65537
CANARY = 0x5A5A5A5A5A5A5A5A


def _keys(rng, primes, n, size_q, size_p):
    """Uniform synthetic Galois keys [dnum][2][QP][N] (arithmetic is data-independent)."""
    dnum = -(-size_q // size_p)
    return np.stack([np.stack([uniform_poly(rng, primes, n), uniform_poly(rng, primes, n)]) for _ in range(dnum)])


class Setup:
    """Contexts of one (configuration, scheme, level) on both sides."""

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

    def keys(self, rng, count, pool=None):
        """(oracle form, device form) of `count` Galois keys, cycling over `pool` distinct ones."""
        pool = count if pool is None else min(pool, count)
        host = [_keys(rng, self.primes, self.n, self.size_q, self.size_p) for _ in range(pool)]
        dev = [self.P.PhantomRelinKey.from_numpy(k, self.gpu) for k in host]
        return ([[host[i % pool][d] for d in range(self.tool.beta)] for i in range(count)], [dev[i % pool] for i in range(count)], host)

    def weights(self, rng, count, pool=None):
        pool = count if pool is None else min(pool, count)
        host = [uniform_poly(rng, self.qlp_primes, self.n) for _ in range(pool)]
        dev = [self.P.to_device(w, self.gpu) for w in host]
        return [host[i % pool] for i in range(count)], [dev[i % pool] for i in range(count)]

    def cts(self, rng, batch):
        return np.stack([np.stack([uniform_poly(rng, self.primes[:self.ql], self.n) for _ in range(2)]) for _ in range(batch)])

    def singles(self, cts, elts, dev_keys, dev_w=None):
        """B calls of the single-ciphertext entry."""
        out = []
        for ct in cts:
            d = self.P.to_device(ct, self.gpu)
            if dev_w is None:
                self.ctx.hoisting(self.ql, d, elts, dev_keys, self.scheme)
            else:
                self.ctx.hoisting_weighted(self.ql, d, elts, dev_keys, dev_w, self.scheme)
            out.append(self.P.to_host(d))
        return np.stack(out)


def _elements(n, count):
    return [int(pow(5, i + 1, 2 * n)) for i in range(count)]


# ---- A. the plain form --------------------------------------------------------------------------------------------------------
PLAIN_CASES = [
    ("hyb12_a2", O.CKKS, 6, [5, 25, 125], 5),        # beta = 3; one full group of 4 + a tail of 1
    ("hyb12_a2", O.CKKS, 3, [5], 2),                 # beta = 2, one-limb last digit
    ("hyb12_a2", O.BFV, 6, [5, 8191], 3),            # coefficient-domain c0 path
    ("hyb12_a2", O.BGV, 6, [5, 25], 2),
    ("c1_bfv4096", O.CKKS, 2, [5, 25], 3),           # alpha = 1: the mod-up's per-ciphertext loop
    ("p61_a2", O.CKKS, 6, 22, 3),                    # 61-bit primes: 21 elements per launch, the 22nd in a second, accumulating launch
    ("hyb13_b5", O.CKKS, 10, [5, 25], 3),            # beta = 5: the run-time digit loop
]


@pytest.mark.parametrize("name,scheme,ql,elts,batch", PLAIN_CASES)
def test_plain_form_equals_the_oracle_per_ciphertext(name, scheme, ql, elts, batch, gpu):
    s = Setup(name, scheme, ql, gpu)
    if isinstance(elts, int):
        elts = _elements(s.n, elts)
    r = rng_for(9100 + ql + 16 * batch + len(elts))
    o_keys, d_keys, _ = s.keys(r, len(elts), pool=3)
    cts = s.cts(r, batch)
    out = s.ctx.hoisting_batched(ql, s.P.to_device(cts, gpu), elts, d_keys, scheme)
    got = s.P.to_host(out)
    for b in range(batch):
        assert np.array_equal(got[b], s.tool.hoisting(cts[b], elts, o_keys, scheme)), f"ciphertext {b} of {batch}"


# ---- B, C. chunk invariance, in place, B = 1 ------------------------------------------------------------------------------------
def test_every_chunk_size_gives_the_same_words(gpu):
    name, scheme, ql, elts, batch = PLAIN_CASES[0]
    s = Setup(name, scheme, ql, gpu)
    r = rng_for(9200)
    _, d_keys, _ = s.keys(r, len(elts))
    cts = s.cts(r, batch)
    d_ct = s.P.to_device(cts, gpu)
    ref = s.singles(cts, elts, d_keys)
    for chunk in (1, 2, 3, 4, 8):
        got = s.P.to_host(s.ctx.hoisting_batched(ql, d_ct, elts, d_keys, scheme, chunk=chunk))
        assert np.array_equal(got, ref), f"chunk = {chunk} differs from {batch} calls of pha_hoisting"
    assert np.array_equal(s.P.to_host(d_ct), cts), "ct is only read"


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_in_place_and_a_batch_of_one(weighted, gpu):
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    r = rng_for(9300 + int(weighted))
    rot = [5, 25, 125]
    elts = ([1] if weighted else []) + rot
    _, d_rot, _ = s.keys(r, len(rot))
    d_keys = ([None] if weighted else []) + d_rot
    d_w = s.weights(r, len(elts))[1] if weighted else None
    cts = s.cts(r, 5)

    def run(d_ct, **kw):
        if weighted:
            return s.ctx.hoisting_weighted_batched(s.ql, d_ct, elts, d_keys, d_w, s.scheme, **kw)
        return s.ctx.hoisting_batched(s.ql, d_ct, elts, d_keys, s.scheme, **kw)

    ref = s.singles(cts, elts, d_keys, d_w)
    assert np.array_equal(s.P.to_host(run(s.P.to_device(cts, gpu))), ref)
    for chunk in (0, 2):
        d_ct = s.P.to_device(cts, gpu)
        assert run(d_ct, out=d_ct, chunk=chunk) is d_ct
        assert np.array_equal(s.P.to_host(d_ct), ref), f"in place, chunk = {chunk}"
    one = s.P.to_device(cts[:1], gpu)
    assert np.array_equal(s.P.to_host(run(one)), ref[:1]), "B = 1 differs from the single entry"
    run(one, out=one)
    assert np.array_equal(s.P.to_host(one), ref[:1]), "B = 1 in place differs from the single entry"


# ---- D. the weighted form --------------------------------------------------------------------------------------------------------
WEIGHTED_CASES = [
    ("hyb12_a2", O.CKKS, 6, 3, 5),
    ("hyb12_a2", O.BGV, 5, 3, 2),
    ("hyb13_a3", O.CKKS, 7, 4, 3),
    ("hyb12_a2", O.CKKS, 2, 0, 2),                   # identity only: no key switch at all
    ("hyb12_a2", O.CKKS, 4, 127, 2),                 # the 63-element launch split and the 48-term fold of the c-kernel
]


@pytest.mark.parametrize("name,scheme,ql,n_rot,batch", WEIGHTED_CASES)
def test_weighted_form_equals_the_oracle_per_ciphertext(name, scheme, ql, n_rot, batch, gpu):
    s = Setup(name, scheme, ql, gpu)
    r = rng_for(9400 + n_rot)
    rot = _elements(s.n, n_rot)
    elts = [1] + rot
    many = n_rot > 8                                  # many diagonals: a few distinct keys and weights, reused
    o_rot, d_rot, _ = s.keys(r, n_rot, pool=3 if many else None) if n_rot else ([], [], None)
    h_w, d_w = s.weights(r, len(elts), pool=5 if many else None)
    cts = s.cts(r, batch)
    out = s.ctx.hoisting_weighted_batched(ql, s.P.to_device(cts, gpu), elts, [None] + d_rot, d_w, scheme)
    got = s.P.to_host(out)
    for b in range(batch):
        assert np.array_equal(got[b], s.tool.hoisting_weighted(cts[b], elts, [None] + o_rot, h_w, scheme)), f"ciphertext {b} of {batch}"


# ---- E. N = 2^16 on both sides of the fused-conversion thresholds ----------------------------------------------------------------
@pytest.fixture(scope="module")
def n16(gpu):
    """hyb16_a12, level 24 (beta = 2), two elements, eight ciphertexts: inputs, the single entry's results and the oracle's for the
    ciphertexts the two cases look at -- made once."""
    s = Setup("hyb16_a12", O.CKKS, 24, gpu)
    r = rng_for(9500)
    elts = [5, 25]
    o_keys, d_keys, _ = s.keys(r, 2)
    cts = s.cts(r, 8)
    oracle = {b: s.tool.hoisting(cts[b], elts, o_keys, s.scheme) for b in (0, 6, 7)}
    return s, elts, d_keys, cts, s.singles(cts, elts, d_keys), oracle


@pytest.mark.parametrize("batch", [7, 8], ids=["below", "at"])
def test_n16_both_sides_of_the_fused_conversion_thresholds(batch, n16, gpu):
    """B = 7 in one chunk: beta * B = 2 * B = 14 polynomials, below the 16 polynomials / 1024 workgroups from which the mod-up and
    the mod-down take their conversions fused into the transforms; B = 8: 16 of each (profiles/hoisting_batched.md)."""
    s, elts, d_keys, cts, singles, oracle = n16
    got = s.P.to_host(s.ctx.hoisting_batched(s.ql, s.P.to_device(cts[:batch], gpu), elts, d_keys, s.scheme, chunk=batch))
    for b in (0, batch - 1):
        assert np.array_equal(got[b], oracle[b]), f"ciphertext {b} differs from the oracle"
    assert np.array_equal(got, singles[:batch]), "differs from single pha_hoisting calls"


# ---- F. extreme residues ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_extreme_residues(weighted, gpu):
    """Ciphertext words at q - 1, 0 and q - 1 - r inside one batch; one key and one weight at q - 1 throughout."""
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    r = rng_for(9600 + int(weighted))
    rot = [5, 25, 125]
    elts = ([1] if weighted else []) + rot
    host_keys = [_keys(r, s.primes, s.n, s.size_q, s.size_p) for _ in rot]
    host_keys[1] = np.stack([np.stack([np.stack([np.full(s.n, q - 1, dtype=np.uint64) for q in s.primes])] * 2)] * host_keys[1].shape[0])
    o_rot = [[k[d] for d in range(s.tool.beta)] for k in host_keys]
    d_rot = [s.P.PhantomRelinKey.from_numpy(k, gpu) for k in host_keys]
    top = np.stack([np.full(s.n, q - 1, dtype=np.uint64) for q in s.primes[:s.ql]])
    near = np.stack([np.stack([np.uint64(q - 1) - r.integers(0, 1 << 16, s.n, dtype=np.uint64) for q in s.primes[:s.ql]]) for _ in range(2)])
    cts = np.stack([np.stack([top, top]), np.zeros((2, s.ql, s.n), dtype=np.uint64), near])
    if weighted:
        h_w = [uniform_poly(r, s.qlp_primes, s.n) for _ in elts]
        h_w[2] = np.stack([np.full(s.n, q - 1, dtype=np.uint64) for q in s.qlp_primes])
        d_w = [s.P.to_device(w, gpu) for w in h_w]
        got = s.P.to_host(s.ctx.hoisting_weighted_batched(s.ql, s.P.to_device(cts, gpu), elts, [None] + d_rot, d_w, s.scheme))
        want = [s.tool.hoisting_weighted(ct, elts, [None] + o_rot, h_w, s.scheme) for ct in cts]
    else:
        got = s.P.to_host(s.ctx.hoisting_batched(s.ql, s.P.to_device(cts, gpu), elts, d_rot, s.scheme))
        want = [s.tool.hoisting(ct, elts, o_rot, s.scheme) for ct in cts]
    for b in range(3):
        assert np.array_equal(got[b], want[b]), f"ciphertext {b}"


# ---- G. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched(gpu):
    import torch
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    P, ql, ctx = s.P, s.ql, s.ctx
    r = rng_for(9700)
    rot = [5, 25]
    _, d_rot, _ = s.keys(r, 2)
    d_w = s.weights(r, 3)[1]
    cts = s.cts(r, 3)
    d_ct = P.to_device(cts, gpu)
    canary = np.full(cts.shape, CANARY, dtype=np.uint64)
    out = P.to_device(canary, gpu)

    def untouched():
        torch.cuda.synchronize()
        assert np.array_equal(P.to_host(out), canary), "a refused call wrote to out"
        assert np.array_equal(P.to_host(d_ct), cts), "a refused call wrote to ct"

    with pytest.raises(ValueError):                                       # no elements
        ctx.hoisting_batched(ql, d_ct, [], [], s.scheme, out=out)
    with pytest.raises(ValueError):
        ctx.hoisting_weighted_batched(ql, d_ct, [], [], [], s.scheme, out=out)
    untouched()
    with pytest.raises(ArithmeticError):                                  # a keyed element without its key (std::logic_error)
        ctx.hoisting_batched(ql, d_ct, rot, [d_rot[0], None], s.scheme, out=out)
    with pytest.raises(ArithmeticError):
        ctx.hoisting_weighted_batched(ql, d_ct, [1] + rot, [None, d_rot[0], None], d_w, s.scheme, out=out)
    untouched()
    with pytest.raises(ValueError):                                       # a null weight
        ctx.hoisting_weighted_batched(ql, d_ct, [1] + rot, [None] + d_rot, [d_w[0], None, d_w[2]], s.scheme, out=out)
    untouched()
    with pytest.raises(ValueError):                                       # bfv to the weighted form
        ctx.hoisting_weighted_batched(ql, d_ct, [1] + rot, [None] + d_rot, d_w, O.BFV, out=out)
    untouched()
    with pytest.raises(ValueError):                                       # an even Galois element
        ctx.hoisting_batched(ql, d_ct, [5, 4], d_rot, s.scheme, out=out)
    with pytest.raises(ValueError):
        ctx.hoisting_weighted_batched(ql, d_ct, [1, 5, 4], [None] + d_rot, d_w, s.scheme, out=out)
    untouched()
    # out overlapping ct by one polynomial (everything but the exact in-place form is refused)
    polys = np.concatenate([cts.reshape(6, ql, s.n), np.full((1, ql, s.n), CANARY, dtype=np.uint64)])
    buf = P.to_device(polys, gpu)
    ct_v, out_v = buf[:6].view(3, 2, ql, s.n), buf[1:].view(3, 2, ql, s.n)
    with pytest.raises(ValueError):
        ctx.hoisting_batched(ql, ct_v, rot, d_rot, s.scheme, out=out_v)
    with pytest.raises(ValueError):
        ctx.hoisting_weighted_batched(ql, ct_v, [1] + rot, [None] + d_rot, d_w, s.scheme, out=out_v)
    torch.cuda.synchronize()
    assert np.array_equal(P.to_host(buf), polys), "a refused call wrote to the overlapping buffers"
    # batch == 0: OK, nothing happens (raw entries: real buffers, zero ciphertexts)
    from phantom_fhe_amd import lib as plib
    L = plib.load()
    stream = torch.cuda.current_stream().cuda_stream
    e2 = (C.c_uint32 * 2)(*rot)
    k2 = (C.c_void_p * 2)(*[k.public_keys_ptr.data_ptr() for k in d_rot])
    w2 = (C.c_void_p * 2)(*[w.data_ptr() for w in d_w[:2]])
    assert L.pha_hoisting_batched(ctx._h, ql, d_ct.data_ptr(), 0, e2, 2, k2, int(s.scheme), out.data_ptr(), 0, stream) == 0
    assert L.pha_hoisting_weighted_batched(ctx._h, ql, d_ct.data_ptr(), 0, e2, 2, k2, w2, int(s.scheme), out.data_ptr(), 0, stream) == 0
    untouched()
    empty = d_ct[:0]
    assert ctx.hoisting_batched(ql, empty, rot, d_rot, s.scheme).shape[0] == 0
    untouched()


# ---- H. strict mode --------------------------------------------------------------------------------------------------------------
def test_strict_mode_counts_every_ciphertext_of_the_batch(gpu):
    import torch
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    P = s.P
    r = rng_for(9800)
    rot = [5, 25]
    _, d_rot, _ = s.keys(r, 2)
    d_w = s.weights(r, 3)[1]
    cts = s.cts(r, 4)
    bad = cts.copy()
    bad[2, 1, 3, 17] = np.uint64(s.primes[3])          # ciphertext 3 of 4: one word equal to its modulus
    canary = np.full(cts.shape, CANARY, dtype=np.uint64)
    out = P.to_device(canary, gpu)
    d_bad, d_ok = P.to_device(bad, gpu), P.to_device(cts, gpu)
    before = P.set_strict(True)
    try:
        with pytest.raises(ValueError, match="PHA_STRICT"):
            s.ctx.hoisting_batched(s.ql, d_bad, rot, d_rot, s.scheme, out=out)
        with pytest.raises(ValueError, match="PHA_STRICT"):
            s.ctx.hoisting_weighted_batched(s.ql, d_bad, [1] + rot, [None] + d_rot, d_w, s.scheme, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(P.to_host(out), canary), "a strict-mode refusal wrote to out"
        strict = P.to_host(s.ctx.hoisting_batched(s.ql, d_ok, rot, d_rot, s.scheme))       # canonical operands: computed as usual
    finally:
        P.set_strict(before)
    assert np.array_equal(strict, P.to_host(s.ctx.hoisting_batched(s.ql, d_ok, rot, d_rot, s.scheme)))


# ---- I. the workload -------------------------------------------------------------------------------------------------------------
def test_diag_matvec_batch_equals_diag_matvec_per_vector(gpu):
    from phantom_fhe_amd import workloads as W
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    r = rng_for(9900)
    rot = [5, 25, 125]
    elts = [1] + rot
    _, d_rot, _ = s.keys(r, 3)
    d_w = s.weights(r, 4)[1]
    d_cts = s.P.to_device(s.cts(r, 3), gpu)
    out = W.diag_matvec_batch(s.ctx, s.ql, d_cts, elts, [None] + d_rot, d_w, s.scheme)
    assert tuple(out.shape) == tuple(d_cts.shape)
    for b in range(3):
        one = W.diag_matvec(s.ctx, s.ql, d_cts[b], elts, [None] + d_rot, d_w, s.scheme)
        assert np.array_equal(s.P.to_host(out[b]), s.P.to_host(one)), f"vector {b}"


# ---- J. refusals of the single entries ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def single_refusals(gpu):
    """hyb12_a2, level 6: one ciphertext, two rotation keys and three weights -- made once."""
    s = Setup("hyb12_a2", O.CKKS, 6, gpu)
    r = rng_for(9950)
    _, d_rot, _ = s.keys(r, 2)
    return s, d_rot, s.weights(r, 3)[1], s.cts(r, 1)[0]


SINGLE_REFUSALS = [
    ("plain", "even", ValueError), ("plain", "beyond_2n", ValueError), ("plain", "missing_key", ArithmeticError),
    ("weighted", "even", ValueError), ("weighted", "beyond_2n", ValueError), ("weighted", "missing_key", ArithmeticError),
    ("weighted", "null_weight", ValueError),
]


@pytest.mark.parametrize("form,defect,exc", SINGLE_REFUSALS, ids=[f"{f}-{d}" for f, d, _ in SINGLE_REFUSALS])
def test_single_entry_refusals_leave_ct_untouched(form, defect, exc, single_refusals, gpu):
    """pha_hoisting / pha_hoisting_weighted with exactly one defect per call: the exception class, and ct keeps its words."""
    import torch
    from phantom_fhe_amd import lib as plib
    s, d_rot, d_w, ct = single_refusals
    weighted = form == "weighted"
    elts = ([1] if weighted else []) + [5, 25]
    keys = ([None] if weighted else []) + list(d_rot)
    w = list(d_w)
    if defect == "even":
        elts[-1] = 4
    elif defect == "beyond_2n":
        elts[-1] = 2 * s.n + 5
    elif defect == "missing_key":
        keys[-1] = None
    else:
        w[1] = None
    d_ct = s.P.to_device(ct, gpu)
    with pytest.raises(exc):
        if weighted:
            s.ctx.hoisting_weighted(s.ql, d_ct, elts, keys, w, s.scheme)
        else:   # (the wrapper takes no None key: the raw entry with a null key table)
            e = (C.c_uint32 * 2)(*elts)
            k = (C.c_void_p * 2)(*[None if x is None else x.public_keys_ptr.data_ptr() for x in keys])
            plib.check(plib.load().pha_hoisting(s.ctx._h, s.ql, d_ct.data_ptr(), e, 2, k, int(s.scheme), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert np.array_equal(s.P.to_host(d_ct), ct), "a refused call wrote to ct"
