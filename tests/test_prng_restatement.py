"""tests/prng_restatement.py is what the seeded samplers are held to; this file pins the restatement itself -- no library, no GPU.

a. the quarter-round on (1, 0, 0, 0): worked out by hand from the rotation rule (b = rotl(1, 7) = 0x80; c = rotl(0x81, 9) = 0x10200;
   d = rotl(0x10280, 13) = 0x20500000; a = 1 ^ rotl(0x20510200, 18) = 0x08008145) -- the Salsa20 specification's first example
b. an all-zero input block gives an all-zero output (no constants: the core maps 0 to 0, and 0 + 0 = 0)
c. the scalar loop-by-loop transcription of the reference's thread programs agrees with the vectorised form, the one-block-per-limb
   recomputation of the ternary and noise kernels included
d. the residue form and the signed form agree limb by limb
e. on reject12 with STAT_SEED the redraw log shows, per limb: >= 100 redrawn words, a redraw at index 0 and one at index 7, a group
   that redraws at two different indexes, a word that needed two redraws in a row (conditions on the INPUTS of the GPU tests)
f. the ternary sample of STAT_SEED holds each of -1, 0, 1 in 25 .. 42 % of 4096 coefficients (86 / 256, 85 / 256, 85 / 256 expected)
g. the noise sample of STAT_SEED has mean within +-0.25 and variance within 10.5 +- 1.5 (42 fair bits times 1 / 4)"""
import numpy as np
import pytest

import prng_restatement as R
from util import primes_of


def test_quarter_round_by_hand():
    one, zero = np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32)
    assert [int(v[0]) for v in R.quarter_round(one, zero, zero, zero)] == [0x08008145, 0x00000080, 0x00010200, 0x20500000]
    assert [int(v[0]) for v in R.quarter_round(zero, zero, zero, zero)] == [0, 0, 0, 0]


def test_all_zero_input_gives_all_zero_output():
    assert not R.core(np.zeros((16, 3), dtype=np.uint32)).any()
    assert not R.block(np.zeros(64, dtype=np.uint8), [0]).any()
    assert R.scalar_block(np.zeros(64, dtype=np.uint8), 0) == bytes(64)
    assert R.block(np.zeros(64, dtype=np.uint8), [1]).any()              # the nonce is an input


def test_input_layout():
    seed = np.arange(64, dtype=np.uint8)
    x = R.input_words(seed, [0x1122334455667788])
    assert int(x[0, 0]) == 0x03020100 and int(x[7, 0]) == 0x1F1E1D1C
    assert int(x[8, 0]) == 0x55667788 and int(x[9, 0]) == 0x11223344
    assert int(x[10, 0]) == 0x23222120 and int(x[15, 0]) == 0x37363534
    other = seed.copy()
    other[56:] ^= 0xFF                                                   # bytes 56..63 are never read
    assert np.array_equal(R.block(seed, [5, 6]), R.block(other, [5, 6]))
    other[55] ^= 1
    assert not np.array_equal(R.block(seed, [5]), R.block(other, [5]))


@pytest.mark.parametrize("tag", [0, 1])
def test_scalar_block_equals_vectorised(tag):
    seed = R.seed_bytes(tag)
    nonces = [0, 1, 7, 4095, 1 << 16, (1 << 17) + 3, (1 << 32) - 1, 1 << 32, (1 << 40) + 12345, (1 << 64) - 1]
    got = R.block(seed, nonces)
    for k, nonce in enumerate(nonces):
        assert got[k].astype("<u4").tobytes() == R.scalar_block(seed, nonce), nonce
    w = R.block_words64(seed, nonces)
    assert int(w[3, 2]) == int.from_bytes(R.scalar_block(seed, 4095)[16:24], "little")


def test_scalar_samplers_equal_vectorised_with_per_limb_recomputation():
    n, primes = 64, [int(q) for q in primes_of("hyb12_a2")[1]][:3]
    for tag in (2, 3):
        seed = R.seed_bytes(tag)
        assert np.array_equal(R.scalar_ternary_poly(seed, primes, n), R.residues(R.ternary_signed(seed, n), primes))
        assert np.array_equal(R.scalar_error_poly(seed, primes, n), R.residues(R.error_signed(seed, n), primes))
        assert np.array_equal(R.scalar_uniform_poly(seed, primes, n), R.uniform(seed, primes, n))


def test_scalar_uniform_equals_vectorised_where_it_redraws():
    log_n, primes, _ = R.REJECT12
    n = 1 << log_n
    log = []
    want = R.uniform(R.STAT_SEED_ARRAY, primes, n, log)
    twice = [(y, j) for y, j, _, r in log if r >= 2][:6]
    multi = [k for k in {(y, j) for y, j, _, _ in log} if len({i for y, j, i, _ in log if (y, j) == k}) >= 2][:6]
    first = [(y, j) for y, j, _, _ in log][:20]
    tids = sorted({y * (n // 8) + j for y, j in twice + multi + first} | set(range(8)))
    got = R.scalar_uniform_poly(R.STAT_SEED_ARRAY, primes, n, tids).reshape(-1, 8)
    assert twice and multi
    for tid in tids:
        assert np.array_equal(got[tid], want.reshape(-1, 8)[tid]), tid


def test_residue_and_signed_forms_agree():
    primes = [int(q) for q in primes_of("ladder12")[1]]
    for fn in (R.ternary_signed, R.error_signed):
        v = fn(R.seed_bytes(4), 256)
        res = R.residues(v, primes)
        for y, q in enumerate(primes):
            assert np.all(res[y] < q)
            centred = np.where(res[y] > q // 2, res[y].astype(np.int64) - np.int64(q), res[y].astype(np.int64))
            assert np.array_equal(centred, v), q
    assert set(np.unique(R.ternary_signed(R.seed_bytes(4), 256))) <= {-1, 0, 1}
    assert np.max(np.abs(R.error_signed(R.seed_bytes(4), 4096))) <= 21


def test_acceptance_bound():
    for q in list(primes_of("ladder12")[1]) + list(R.REJECT12[1]):
        q = int(q)
        b = R.max_multiple(q)
        assert (b + 1) % q == 0 and b + 1 + q > 2 ** 64 - 1     # one below the largest multiple of q that fits 64 bits
        assert b == (2 ** 64 - 1) - ((2 ** 64 - 1) % q) - 1
    for q in R.REJECT12[1]:
        rejected = 1 - (R.max_multiple(q) + 1) / 2.0 ** 64
        assert 0.0587 < rejected < 0.0589, rejected


def test_redraw_log_of_the_fixed_seed_on_reject12():
    log_n, primes, size_p = R.REJECT12
    assert size_p == 1 and all(q % (2 << log_n) == 1 for q in primes)
    log = []
    out = R.uniform(R.STAT_SEED_ARRAY, primes, 1 << log_n, log)
    for y, q in enumerate(primes):
        assert np.all(out[y] < q)
        mine = [(j, i, r) for yy, j, i, r in log if yy == y]
        print(f"limb {y}: {len(mine)} redrawn words, {sum(1 for _, _, r in mine if r >= 2)} redrawn twice in a row or more")
        assert len(mine) >= 100
        assert any(i == 0 for _, i, _ in mine) and any(i == 7 for _, i, _ in mine)
        by_group = {}
        for j, i, _ in mine:
            by_group.setdefault(j, set()).add(i)
        assert any(len(s) >= 2 for s in by_group.values())
        assert any(r >= 2 for _, _, r in mine)


def test_ternary_shares_of_the_fixed_seed():
    v = R.ternary_signed(R.STAT_SEED_ARRAY, 4096)
    for value in (-1, 0, 1):
        share = np.count_nonzero(v == value) / 4096.0
        print(f"ternary {value}: {share:.4f}")
        assert 0.25 <= share <= 0.42


def test_noise_moments_of_the_fixed_seed():
    v = R.error_signed(R.STAT_SEED_ARRAY, 4096).astype(np.float64)
    print(f"noise mean {v.mean():.4f}, variance {v.var():.4f}")
    assert abs(v.mean()) <= 0.25
    assert abs(v.var() - 10.5) <= 1.5
