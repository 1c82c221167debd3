"""GPU parity on both sides of every plan switch of the NTT launchers, bit-exact against the CPU oracle.

`choose_plan` / `launch_zloop` (csrc/pha_ntt.hip) pick a code path by degree, limb count, batch size and prime width.  With
lp = limbs x batch and `tiles` = lp x N / 4096, as read from that code:

  * N = 2^13: two passes below lp 64, the one-launch plan from 64;
  * N = 2^14 / 2^15 / 2^16: plan 5 (four coefficients per thread) while lp x N / 256 <= 8192, i.e. lp <= 128 / 64 / 32;
  * above that plan 3 (table-driven last round) below 1024 tiles and plan 4 (last-round twiddles formed on the fly) from 1024
    tiles, i.e. from lp 256 / 128 / 32 at 2^14 / 2^15 / 2^17; N = 2^16 takes plan 10 (64 x 1024) instead of either;
  * batches of >= 8 polynomials with >= 8192 tiles take plan 3 in the polynomial-fastest block order;
  * on plans 3 / 4 / 10 a batch of >= 8 polynomials runs the contiguous pass in `ntt_zloop_kernel` when
    waves per polynomial x ceil(B / zper) >= 4096, the selection has <= 128 limbs and at least half of them are FP64 limbs.

Which kernel every case below launched is recorded in profiles/ntt_plan_switch_kernels.md.  A context's own chain holds at most
64 primes (the reference's COEFF_MOD_COUNT_MAX), but the plain entries select rows of the context's table set, and that set grows:
once the BEHZ tool of a 64-prime context is built, its |Bsk| = 65 auxiliary primes (61-bit, with tables) follow the chain, 129
consecutive rows in all.  The `wide` fixture builds such a context, which gives the selections of 65 .. 129 limbs below: single
polynomials past the 2^14 / 2^15 switches, lp 127 = 127 x 1, the full `limb[128]` map of the resident-twiddle kernel and its
`count > 128` decline, and plan 4 at N = 2^15 for the epilogue entries that take a plain limb range.

Inputs: chains that mix the back ends (util.MIXED_BITS: integer limbs in the middle and at the end), every polynomial of a batch
from its own seed, every second-of-four polynomial with all residues just below q, and in every polynomial three blocks
(q - 1 - r with r < 2^16, q - 1, 0) at its start, across coefficient 4096 (a boundary of every tile size) and at its end."""
import numpy as np
import pytest

from oracle import oracle as O
from util import chain_bits, chain_primes, primes_of, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

_BLK = 48


def plan_poly(seed, primes, n, near_q=False):
    """[len(primes)][n] residues from rng_for(seed): uniform (or all within 2^16 of q), plus the three edge blocks."""
    r = rng_for(seed)
    L = len(primes)
    q = np.array(primes, dtype=np.uint64)[:, None]
    if near_q:
        x = q - 1 - r.integers(0, 1 << 16, (L, n), dtype=np.uint64)
    else:
        x = uniform_poly(r, primes, n)
    for at in (0, 4096 - 3 * _BLK // 2, n - 3 * _BLK):
        x[:, at:at + _BLK] = q - 1 - r.integers(0, 1 << 16, (L, _BLK), dtype=np.uint64)
        x[:, at + _BLK:at + 2 * _BLK] = q - 1
        x[:, at + 2 * _BLK:at + 3 * _BLK] = 0
    return x


def plan_batch(seed, primes, n, batch):
    return np.stack([plan_poly(seed + z, primes, n, near_q=(z % 4 == 1)) for z in range(batch)])


def _pair(log_n, primes, size_p, gpu):
    import phantom_fhe_amd as P
    return O.Ctx(log_n, list(primes), size_p), P.PhantomContext(log_n, list(primes), size_p, device=gpu)


def _both_ways(oc, ctx, buf, gpu, batch=None, count=None, start=0, singles=False):
    """buf: [Z][Lb][n].  The launch covers limbs [start, start + count) (default: all Lb) of the first `batch` polynomials (default:
    all Z), poly_stride = Lb x n; Z = batch = 1 goes through the single-polynomial entries.  Forward values, the round trip, and the
    inverse's values on the input itself (not a forward image): every polynomial against the oracle, and every word outside the
    launch -- other limbs, guard limbs, polynomials after the batch -- must come back as it was.  singles: the batched results also
    word for word against one single-polynomial call per polynomial."""
    import phantom_fhe_amd as P
    Z, Lb, n = buf.shape
    batch = Z if batch is None else batch
    count = Lb if count is None else count
    sl = slice(start, start + count)
    single = Z == 1 and batch == 1

    def run(d, name):
        if single:
            getattr(ctx, f"nwt_2d_radix8_{name}_inplace")(d, count, start)
        else:
            getattr(ctx, f"nwt_2d_radix8_{name}_inplace_batched")(d, count, start, batch, Lb * n)

    def check(got, name, fn):
        for z in range(Z):
            want = buf[z].copy()
            if z < batch:
                want[sl] = fn(buf[z, sl], count, start)
            assert np.array_equal(got[z], want), (name, z)
        if singles:
            for z in range(batch):
                d1 = P.to_device(buf[z], gpu)
                getattr(ctx, f"nwt_2d_radix8_{name}_inplace")(d1, count, start)
                assert np.array_equal(P.to_host(d1), got[z]), (name, "single call", z)

    d = P.to_device(buf, gpu)
    run(d, "forward")
    check(P.to_host(d), "forward", oc.nwt_forward)
    run(d, "backward")
    assert np.array_equal(P.to_host(d), buf), "round trip"
    d = P.to_device(buf, gpu)
    run(d, "backward")
    check(P.to_host(d), "backward", oc.nwt_backward)


# A 64-prime chain of FP64-back-end primes (<= 50 bits: plain, light-forward and light-inverse sizes) at N = 2^log_n whose BEHZ tool
# is built: rows 64 .. 128 of the table set are the 65 primes of Bsk (61-bit: the integer back end).
_FP_BITS = [50, 48, 47, 46, 43, 42, 41, 40, 36, 30]


@pytest.fixture(scope="module")
def wide(request, gpu):
    """(log_n, the 129 primes of the rows, oracle context over them, GPU context); parametrised indirectly by log_n."""
    import phantom_fhe_amd as P
    log_n = request.param
    n = 1 << log_n
    chain = chain_primes(log_n, tuple(chain_bits(64, _FP_BITS)))
    ctx = P.PhantomContext(log_n, list(chain), 0, device=gpu)
    ctx.set_plain_modulus(65537)
    ctx.nwt_2d_radix8_forward_inplace_include_temp_mod(P.to_device(np.zeros((65, n), dtype=np.uint64), gpu), 65, 0, 66)   # builds the tool
    rows = [ctx.prime_info(i)["value"] for i in range(129)]
    assert rows[:64] == list(chain)
    assert all(q >> 60 == 1 and (q - 1) % (2 * n) == 0 and O.is_prime(q) for q in rows[64:]) and len(set(rows)) == 129
    return log_n, rows, O.Ctx(log_n, rows, 0), ctx


# ---- A: both sides of each threshold ----------------------------------------------------------------------------------------------
# (log_n, limbs, batch, what choose_plan gives); batches stay below 8 polynomials, so neither the resident-twiddle kernel nor the
# polynomial-fastest order takes part here
_A_CASES = [
    (13, 9, 7, "lp63-two-pass"), (13, 8, 8, "lp64-one-launch"),
    (14, 64, 2, "lp128-plan5"), (14, 43, 3, "lp129-plan3"), (14, 51, 5, "lp255-plan3"), (14, 64, 4, "lp256-plan4"),
    (15, 16, 4, "lp64-plan5"), (15, 13, 5, "lp65-plan3"), (15, 63, 2, "lp126-plan3"), (15, 32, 4, "lp128-plan4"),
    (16, 16, 2, "lp32-plan5"), (16, 11, 3, "lp33-plan10"),
    (17, 31, 1, "lp31-plan3"), (17, 16, 2, "lp32-plan4"),
    # one polynomial of many limbs: the same switches without the batched entry (64 limbs is the most a context takes)
    (14, 64, 1, "single-lp64-plan5"), (15, 64, 1, "single-lp64-plan5"), (16, 32, 1, "single-lp32-plan5"),
    (16, 33, 1, "single-lp33-plan10"), (17, 32, 1, "single-lp32-plan4"),
]


@pytest.mark.parametrize("log_n,limbs,batch,side", _A_CASES, ids=[f"2^{c[0]}-{c[1]}x{c[2]}-{c[3]}" for c in _A_CASES])
def test_a_threshold_sides(log_n, limbs, batch, side, gpu):
    n = 1 << log_n
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    oc, ctx = _pair(log_n, primes, 0, gpu)
    _both_ways(oc, ctx, plan_batch(1000 * log_n + limbs * batch, primes, n, batch), gpu)


# one polynomial of 65 .. 129 limbs (the chain's FP64 limbs, then integer limbs of Bsk): (log_n, count, start, what choose_plan gives)
_A_WIDE = [(14, 128, 0, "plan5"), (14, 129, 0, "plan3"), (15, 65, 30, "plan3"), (15, 127, 1, "plan3"), (15, 128, 1, "plan4")]


@pytest.mark.parametrize("wide,count,start,side", _A_WIDE, indirect=["wide"], ids=[f"2^{c[0]}-{c[1]}x1-{c[3]}" for c in _A_WIDE])
def test_a_single_polynomial_past_64_limbs(wide, count, start, side, gpu):
    log_n, rows, oc, ctx = wide
    _both_ways(oc, ctx, plan_batch(1500 * log_n + count, rows, 1 << log_n, 1), gpu, count=count, start=start)


# ---- B: ntt_zloop_kernel at each degree it is instantiated for ----------------------------------------------------------------------
# the smallest shapes that clear its minimum: (tiles per limb x limbs x wavefronts per tile) x ceil(B / zper) >= 4096 with zper = 4
_B_SHAPES = [(14, 16, 32), (14, 32, 16), (15, 32, 8), (16, 16, 8), (17, 8, 8)]


@pytest.mark.parametrize("log_n,limbs,batch", _B_SHAPES, ids=[f"2^{c[0]}-{c[1]}x{c[2]}" for c in _B_SHAPES])
def test_b_resident_twiddles_mixed_chain(log_n, limbs, batch, gpu):
    """Forward, then inverse, through the batched entries on the mixed chain: light and plain FP64 butterflies and several
    integer limbs (the head of the grid) in one launch; every polynomial against the oracle."""
    n = 1 << log_n
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    oc, ctx = _pair(log_n, primes, 0, gpu)
    _both_ways(oc, ctx, plan_batch(2000 * log_n + batch, primes, n, batch), gpu)


def test_b_batch_12_three_polynomials_per_workgroup(gpu):
    """B = 12 at N = 2^16 x 16 limbs: zper = 12 / 2 = 6, halved to 3 (2048 wavefronts per polynomial x 2 groups < 12288)."""
    log_n, limbs, batch = 16, 16, 12
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    oc, ctx = _pair(log_n, primes, 0, gpu)
    _both_ways(oc, ctx, plan_batch(2100, primes, 1 << log_n, batch), gpu)


def test_b_batch_17_short_last_group_and_the_polynomial_after(gpu):
    """B = 17 at N = 2^16 x 32 limbs: 4096 wavefronts per polynomial x 3 groups = 12288, so zper stays ceil(17 / 3) = 6 and the
    last group holds 5.  The buffer carries an eighteenth polynomial that the launch of 17 must not touch: a group that runs to
    z0 + zper instead of the batch's end transforms it."""
    log_n, limbs, batch = 16, 32, 17
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    oc, ctx = _pair(log_n, primes, 0, gpu)
    _both_ways(oc, ctx, plan_batch(2200, primes, 1 << log_n, batch + 1), gpu, batch=batch)


def test_b_limb_range_that_starts_at_an_integer_limb(gpu):
    """Limbs [3, 19) of a 20-limb chain at N = 2^16, B = 8: the first selected limb is a 60-bit one, two more integer limbs sit
    inside the range (selection-relative 8 and 12), and limbs 0..2 and 19 stay untouched."""
    log_n, limbs, batch = 16, 20, 8
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    assert primes[3] >> 59 and not primes[2] >> 50
    oc, ctx = _pair(log_n, primes, 0, gpu)
    _both_ways(oc, ctx, plan_batch(2300, primes, 1 << log_n, batch), gpu, count=16, start=3)


def test_b_poly_stride_with_a_guard_limb(gpu):
    """poly_stride = (L + 1) N: a poisoned limb between the polynomials comes back untouched, forward and inverse."""
    log_n, limbs, batch = 16, 16, 8
    n = 1 << log_n
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    oc, ctx = _pair(log_n, primes, 0, gpu)
    buf = np.full((batch, limbs + 1, n), 0xA5A5A5A5DEADBEEF, dtype=np.uint64)
    buf[:, :limbs] = plan_batch(2400, primes, n, batch)
    _both_ways(oc, ctx, buf, gpu, count=limbs)


_HALF_INT = (50, 60, 47, 55, 42, 60, 36, 55, 50, 60, 47, 55, 42, 60, 36, 55)          # 8 integer + 8 FP64 limbs: taken
_HALF_INT_PLUS_ONE = (50, 60, 47, 55, 42, 60, 36, 55, 50, 60, 47, 55, 42, 60, 60, 55)  # 9 + 7 (n_fp * 2 < count): declined


@pytest.mark.parametrize("bits", [_HALF_INT, _HALF_INT_PLUS_ONE], ids=["half-integer-taken", "half-plus-one-declined"])
def test_b_integer_limb_share(bits, gpu):
    """N = 2^16, 16 limbs x 8: with exactly half the limbs on the integer back end the resident-twiddle kernel still runs (half its
    grid is the plain pass); with one more it declines and every limb takes the plain pass of plan 10."""
    log_n, batch = 16, 8
    primes = chain_primes(log_n, bits)
    assert sum(1 for q in primes if q >> 50) == (8 if bits is _HALF_INT else 9)
    oc, ctx = _pair(log_n, primes, 0, gpu)
    _both_ways(oc, ctx, plan_batch(2500 + len([b for b in bits if b > 50]), primes, 1 << log_n, batch), gpu)


@pytest.mark.parametrize("wide", [14], indirect=True)
@pytest.mark.parametrize("count", [128, 129], ids=["128-limbs-map-full", "129-limbs-declined"])
def test_b_selections_of_128_and_129_limbs(wide, count, gpu):
    """N = 2^14, B = 8 (4096 wavefronts per polynomial x 2 groups): 128 selected limbs = 64 FP64 + 64 integer limbs fill the
    kernel's limb map and it runs (exactly half FP64); 129 are more than the map holds and every limb takes the plain pass of plan 4.
    Every polynomial against the oracle, and against single-polynomial calls (128 / 129 limb-polynomials: plan 5 / plan 3)."""
    log_n, rows, oc, ctx = wide
    _both_ways(oc, ctx, plan_batch(2600 + count, rows, 1 << log_n, 8), gpu, count=count, singles=True)


# ---- C: the polynomial-fastest block order without the resident-twiddle kernel --------------------------------------------------------
def test_c_polynomial_fastest_order_on_a_wide_prime_chain(gpu):
    """N = 2^17, 32 limbs x 8 = 8192 tiles (256 MiB): batch >= 8 and >= 8192 tiles give the polynomial-fastest block order on plan 3;
    28 of the 32 primes are 60-bit ones, so the resident-twiddle kernel declines.  Every polynomial against the oracle, forward and
    inverse, and word for word against eight single-polynomial calls (32 limb-polynomials each: plan 4, the plain block order)."""
    log_n, batch = 17, 8
    bits = ([60] * 7 + [50]) + ([60] * 7 + [47]) + ([60] * 7 + [42]) + ([60] * 7 + [30])
    primes = chain_primes(log_n, tuple(bits))
    oc, ctx = _pair(log_n, primes, 0, gpu)
    _both_ways(oc, ctx, plan_batch(3000, primes, 1 << log_n, batch), gpu, singles=True)


# ---- D: the epilogue entries on the two-pass plans ------------------------------------------------------------------------------------
# name: (log_n, primes, special primes).  Every selection of the two 40-prime shapes has >= 33 limbs.  Plan 4 at N = 2^15 needs
# >= 128 limbs in one polynomial: test_d_plain_range_epilogues_on_plan4_at_2_15 below, over the rows of the `wide` context.
_D_SHAPES = {
    "plan5-2^14": lambda: (14, primes_of("hyb14_a2")[1], 2),
    "plan3-2^17": lambda: (17, primes_of("hyb17_a2")[1], 2),
    "plan10-2^16": lambda: (16, chain_primes(16, tuple(chain_bits(36) + [60] * 4)), 4),
    "plan4-2^17": lambda: (17, chain_primes(17, tuple(chain_bits(36) + [60] * 4)), 4),
}


@pytest.fixture(scope="module", params=list(_D_SHAPES))
def shape(request, gpu):
    """(log_n, primes, size_p, oracle context, GPU context) of one shape; nothing here changes the context."""
    log_n, primes, size_p = _D_SHAPES[request.param]()
    return (log_n, primes, size_p) + _pair(log_n, primes, size_p, gpu)


def _scales(primes, seed):
    """Per-limb constants 1, q - 1, 3, random, 1, ... with their Shoup companions."""
    r = rng_for(seed)
    s = np.array([(1, q - 1, 3, int(r.integers(1, q)))[i % 4] for i, q in enumerate(primes)], dtype=np.uint64)
    sh = np.array([O.compute_shoup(int(v), int(q)) for v, q in zip(s, primes)], dtype=np.uint64)
    return s, sh


def _fuse_moddown(log_n, primes, L, oc, ctx, gpu):
    """ct = (cx - NTT(delta)) * PInv over limbs [0, L) into a third buffer, and with ct aliasing cx."""
    import phantom_fhe_amd as P
    n = 1 << log_n
    cx = plan_poly(4001, primes[:L], n)
    delta = plan_poly(4002, primes[:L], n, near_q=True)
    c, cs = _scales(primes[:L], 4003)
    ref = oc.multiply_scalar(oc.sub(cx, oc.nwt_forward(delta, L, 0), L, 0), c, L, 0)
    d_c, d_cs = P.to_device(c, gpu), P.to_device(cs, gpu)
    d_cx, d_ct = P.to_device(cx, gpu), P.to_device(np.zeros_like(cx), gpu)
    ctx.nwt_2d_radix8_forward_inplace_fuse_moddown(d_ct, d_cx, d_c, d_cs, P.to_device(delta, gpu), L, 0)
    assert np.array_equal(P.to_host(d_ct), ref)
    assert np.array_equal(P.to_host(d_cx), cx)
    ctx.nwt_2d_radix8_forward_inplace_fuse_moddown(d_cx, d_cx, d_c, d_cs, P.to_device(delta, gpu), L, 0)
    assert np.array_equal(P.to_host(d_cx), ref)


def _backward_trio(log_n, primes, L, oc, ctx, gpu):
    """backward (source untouched), backward_scale and backward_inplace_scale over limbs [0, L)."""
    import phantom_fhe_amd as P
    n = 1 << log_n
    x = plan_poly(4101, primes[:L], n)
    ref = oc.nwt_backward(x, L, 0)
    d_in, d_out = P.to_device(x, gpu), P.to_device(np.zeros_like(x), gpu)
    ctx.nwt_2d_radix8_backward(d_out, d_in, L, 0)
    assert np.array_equal(P.to_host(d_out), ref)
    assert np.array_equal(P.to_host(d_in), x)
    s, sh = _scales(primes[:L], 4102)
    scaled = oc.multiply_scalar(ref, s, L, 0)
    d_s, d_sh = P.to_device(s, gpu), P.to_device(sh, gpu)
    d_out = P.to_device(np.zeros_like(x), gpu)
    ctx.nwt_2d_radix8_backward_scale(d_out, d_in, L, 0, d_s, d_sh)
    assert np.array_equal(P.to_host(d_out), scaled)
    assert np.array_equal(P.to_host(d_in), x)
    ctx.nwt_2d_radix8_backward_inplace_scale(d_in, L, 0, d_s, d_sh)
    assert np.array_equal(P.to_host(d_in), scaled)


def test_d_forward_fuse_moddown(shape, gpu):
    log_n, primes, size_p, oc, ctx = shape
    _fuse_moddown(log_n, primes, len(primes) - size_p, oc, ctx, gpu)


def test_d_backward_out_of_place_and_scaled(shape, gpu):
    log_n, primes, size_p, oc, ctx = shape
    _backward_trio(log_n, primes, len(primes) - size_p, oc, ctx, gpu)


@pytest.mark.parametrize("wide", [15], indirect=True)
def test_d_plain_range_epilogues_on_plan4_at_2_15(wide, gpu):
    """128 limbs of one polynomial at N = 2^15 (1024 tiles: plan 4) through the epilogue entries that take a plain limb range:
    fuse_moddown, backward, backward_scale, backward_inplace_scale.  (The special_mod / temp_mod entries address the special primes
    and Bsk by their own rule and cannot select that many limbs.)"""
    log_n, rows, oc, ctx = wide
    _fuse_moddown(log_n, rows, 128, oc, ctx, gpu)
    _backward_trio(log_n, rows, 128, oc, ctx, gpu)


def test_d_special_mod_entries(shape, gpu):
    """[Ql || P] buffers one level down (the special primes' rows are not adjacent to the data limbs'): forward, forward with a
    skipped range, and the inverse over the whole buffer and over the special limbs alone (mod-down's call)."""
    import phantom_fhe_amd as P
    log_n, primes, size_p, oc, ctx = shape
    n, size_qp = 1 << log_n, len(primes)
    size_q = size_qp - size_p
    ql = size_q - 1
    idx = list(range(ql)) + [size_q + i for i in range(size_p)]
    x = plan_poly(4201, [primes[i] for i in idx], n)
    fwd = oc.nwt_forward_map(x, idx)
    d = P.to_device(x, gpu)
    ctx.nwt_2d_radix8_forward_inplace_include_special_mod(d, ql + size_p, 0, size_qp, size_p)
    assert np.array_equal(P.to_host(d), fwd)
    ctx.nwt_2d_radix8_backward_inplace_include_special_mod(d, ql + size_p, 0, size_qp, size_p)
    assert np.array_equal(P.to_host(d), x), "round trip"
    d = P.to_device(x, gpu)
    ctx.nwt_2d_radix8_forward_inplace_include_special_mod_exclude_range(d, ql + size_p, 0, size_qp, size_p, 1, 3)
    want = fwd.copy()
    want[1:3] = x[1:3]
    assert np.array_equal(P.to_host(d), want)
    d = P.to_device(x, gpu)
    ctx.nwt_2d_radix8_backward_inplace_include_special_mod(d, ql + size_p, 0, size_qp, size_p)
    inv = oc.nwt_backward_map(x, idx)
    assert np.array_equal(P.to_host(d), inv)
    d = P.to_device(x, gpu)
    ctx.nwt_2d_radix8_backward_inplace_include_special_mod(d, size_p, ql, size_qp, size_p)
    want = x.copy()
    want[ql:] = inv[ql:]
    assert np.array_equal(P.to_host(d), want)


def test_d_temp_mod_entries(shape, gpu):
    """include_temp_mod / include_temp_mod_scale over Bsk = B u {m_sk} of the shape's data limbs (plain modulus 65537)."""
    import phantom_fhe_amd as P
    log_n, primes, size_p = shape[:3]
    oc, ctx = _pair(log_n, primes, size_p, gpu)   # a context of its own: the plain modulus and the BEHZ rows change it
    n = 1 << log_n
    ctx.set_plain_modulus(65537)
    behz = O.Behz(oc, 65537)
    sk = behz.size_bsk
    ob = O.Ctx(log_n, behz.bsk, 0)
    x = plan_poly(4301, behz.bsk, n)
    d = P.to_device(x, gpu)
    ctx.nwt_2d_radix8_forward_inplace_include_temp_mod(d, sk, 0, sk + 1)
    assert np.array_equal(P.to_host(d), ob.nwt_forward(x, sk, 0))
    d = P.to_device(x, gpu)
    s, sh = _scales(behz.bsk, 4302)
    ctx.nwt_2d_radix8_backward_inplace_include_temp_mod_scale(d, sk, 0, sk + 1, P.to_device(s, gpu), P.to_device(sh, gpu))
    assert np.array_equal(P.to_host(d), ob.multiply_scalar(ob.nwt_backward(x, sk, 0), s, sk, 0))
