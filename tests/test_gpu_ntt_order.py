"""GPU parity of the batched NTT launch pair on both sides of the rule that gives its strided pass the reverse block order
(csrc/pha_ntt.hip: forward_impl / inverse_impl with PassOrder of csrc/pha_ntt_core.h), bit-exact against the CPU oracle.

The order engages exactly where the pair's contiguous pass is `ntt_zloop_kernel`: a batch of >= 8 polynomials with
waves per polynomial x ceil(B / zper) >= 4096, i.e. 128 x limbs x ceil(B / zper) at N = 2^16 and 32 x limbs x ceil(B / zper) at
N = 2^14 (plan 3 / 4 strided pass).  The smallest shapes on both sides, read off `plan_zloop` / `zloop_zper`:

  * N = 2^16: 8 x 16 limbs engages (zper 4, two groups: 4096; 64 MiB); 8 x 15 does not (3840); 7 x 32 does not (batch < 8);
  * N = 2^14: 8 x 64 limbs engages (4096); 8 x 63 does not (4032); 16 x 32 engages too (zper 4, four groups: 4096), which is the
    shape for a limb sub-range there (a context holds 64 primes).

Every case: forward values, backward values on the input itself, the round trip, and every word outside the launch -- other limbs,
guard limbs, the polynomial after the batch -- unchanged.  Inputs as in tests/test_gpu_ntt_plans.py: util.MIXED_BITS chains (integer
limbs in the middle and at the end of every 12), every polynomial from its own seed, every second-of-four polynomial just below q, edge
blocks at the start, across coefficient 4096 and at the end.  A block order that loses, repeats or misplaces a (limb, polynomial,
tile) leaves words untransformed or transforms words outside the launch, and either shows here."""
import numpy as np
import pytest

from oracle import oracle as O
from util import chain_bits, chain_primes, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

_BLK = 48


def order_poly(seed, primes, n, near_q=False):
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


def order_batch(seed, primes, n, batch):
    return np.stack([order_poly(seed + z, primes, n, near_q=(z % 4 == 1)) for z in range(batch)])


def _pair(log_n, primes, gpu):
    import phantom_fhe_amd as P
    return O.Ctx(log_n, list(primes), 0), P.PhantomContext(log_n, list(primes), 0, device=gpu)


def both_ways(oc, ctx, buf, gpu, batch=None, count=None, start=0, singles=False):
    """buf: [Z][Lb][n].  The launch covers limbs [start, start + count) of the first `batch` polynomials, poly_stride = Lb x n.
    singles: the batched results also word for word against one single-polynomial call per polynomial."""
    import phantom_fhe_amd as P
    Z, Lb, n = buf.shape
    batch = Z if batch is None else batch
    count = Lb if count is None else count
    sl = slice(start, start + count)

    def run(d, name):
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


# (log_n, limbs) of the smallest engaging launch of 8 polynomials
_ENGAGING = [(16, 16), (14, 64)]
_ENGAGING_IDS = ["2^16-16-limbs", "2^14-64-limbs"]


@pytest.mark.parametrize("log_n,limbs", _ENGAGING, ids=_ENGAGING_IDS)
def test_engages_8_polynomials_mixed_chain_against_single_calls(log_n, limbs, gpu):
    """The smallest engaging launch on the mixed chain (integer limbs in the middle and at the end: the tail of the strided pass's
    order), every polynomial against the oracle and word for word against single-polynomial calls (plain block order)."""
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    assert primes[3] >> 59 and primes[limbs - 1] >> 50 and not primes[0] >> 50
    oc, ctx = _pair(log_n, primes, gpu)
    both_ways(oc, ctx, order_batch(7000 + log_n, primes, 1 << log_n, 8), gpu, singles=True)


@pytest.mark.parametrize("log_n,limbs,batch", [(16, 15, 8), (16, 32, 7), (14, 63, 8)], ids=["2^16-8x15", "2^16-7x32", "2^14-8x63"])
def test_does_not_engage_one_step_below(log_n, limbs, batch, gpu):
    """One limb, or one polynomial, short of the rule: the plain grid of the strided pass, the same words."""
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    oc, ctx = _pair(log_n, primes, gpu)
    both_ways(oc, ctx, order_batch(7100 + limbs, primes, 1 << log_n, batch), gpu)


@pytest.mark.parametrize("batch", [9, 11])
@pytest.mark.parametrize("log_n,limbs", _ENGAGING, ids=_ENGAGING_IDS)
def test_ragged_batches(log_n, limbs, batch, gpu):
    """B = 9 and 11 (zper 3: the contiguous pass's last group holds fewer polynomials; the strided pass walks B polynomials per limb,
    descending), with one more polynomial behind the batch that no block may touch."""
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    oc, ctx = _pair(log_n, primes, gpu)
    both_ways(oc, ctx, order_batch(7200 + batch, primes, 1 << log_n, batch + 1), gpu, batch=batch)


@pytest.mark.parametrize("log_n,total,count,start,batch", [(16, 20, 16, 3, 8), (14, 40, 32, 3, 16)], ids=["2^16-16-of-20", "2^14-32-of-40"])
def test_limb_sub_range_with_guard_limbs(log_n, total, count, start, batch, gpu):
    """Limbs [3, 3 + count) of a longer chain: the first selected limb is a 60-bit one, more integer limbs sit inside the range, and
    the limbs before and after it stay untouched."""
    primes = chain_primes(log_n, tuple(chain_bits(total)))
    assert primes[start] >> 59 and not primes[start - 1] >> 50
    oc, ctx = _pair(log_n, primes, gpu)
    both_ways(oc, ctx, order_batch(7300 + log_n, primes, 1 << log_n, batch), gpu, count=count, start=start)


@pytest.mark.parametrize("log_n,limbs", _ENGAGING, ids=_ENGAGING_IDS)
def test_poly_stride_larger_than_the_selection(log_n, limbs, gpu):
    """poly_stride = (limbs + 1) N: a poisoned limb between the polynomials comes back untouched, forward and inverse."""
    n = 1 << log_n
    primes = chain_primes(log_n, tuple(chain_bits(limbs)))
    oc, ctx = _pair(log_n, primes, gpu)
    buf = np.full((8, limbs + 1, n), 0xA5A5A5A5DEADBEEF, dtype=np.uint64)
    buf[:, :limbs] = order_batch(7400 + log_n, primes, n, 8)
    both_ways(oc, ctx, buf, gpu, count=limbs)
