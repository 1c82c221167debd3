"""Shared helpers for the test-suite: parameter sets of BASELINE.json's configs and seeded inputs."""
import functools

import numpy as np

from oracle import oracle as O

# BFVDefault(4096) literal primes, src/host/globals.cu:71 (2 data primes + 1 special)
C1_PRIMES = [0xffffee001, 0xffffc4001, 0x1ffffe0001]

CONFIGS = {
    # name: (log_n, bit sizes of QP, special_modulus_size)
    "c1_bfv4096": (12, None, 1),
    "c2_ntt14": (14, [50] * 8, 0),                       # test/ntt_test.cu:78 (50-bit primes), 8 limbs
    "hyb12_a2": (12, [60, 40, 40, 40, 40, 40, 60, 60], 2),  # 6 data limbs, alpha 2 -> beta 3
    "hyb13_a3": (13, [60] + [50] * 8 + [60] * 3, 3),  # 9 data limbs (dnum 3); lower levels have a short last digit
    "c3_ckks16": (16, [60] + [50] * 44 + [60] * 15, 15),  # examples/3_ckks.cu:729-739
    "c4_bfv15": (15, [60] + [50] * 29 + [60] * 15, 15),   # benchmark/keyswitch_bench.cu:25-34
    "c2_ckks14": (14, [60] + [40] * 7 + [60], 1),         # benchmark/ckks_bench.cu:255 (8 data limbs + 1 special)
    "hyb14_a4": (14, [60] + [50] * 7 + [60] * 4, 4),      # 8 data limbs in 2 digits of 4
    "hyb14_a2": (14, [60] + [50] * 7 + [60] * 2, 2),      # beta = 4 at N = 2^14: the one shape whose fused key products take the full (not the light) FP64 form
    "hyb17_a2": (17, [60, 50, 50, 50, 60, 60], 2),        # N = 2^17: the 256 x 512 plan under the fused mod-up + inner product (4 data limbs, beta 2)
    "hyb16_a12": (16, [60] + [50] * 23 + [60] * 12, 12),  # N = 2^16 with alpha = 12 (beta = 2): the 16-input instantiation of the r05 fused mod-up conversion
    "wide_p33": (12, [36] * 6 + [37] * 33, 33),            # special base wider than the register-resident converters (alpha > 32)
    "wide_p20": (12, [45] * 24 + [46] * 20, 20),           # 17..32 special primes: the 30 / 31-bit split converter (two digits: 20 + 4 limbs)
    "p61_a2": (12, [50] * 6 + [61, 61], 2),               # 61-bit special primes: 30 / 31 cuts in mod-up, 31 / 30 in mod-down
    "p61_14_a2": (14, [50] * 6 + [61, 61], 2),            # the same at N = 2^14 (beta 3): no fused key switch + rescale (wide primes), but ONE ciphertext has the fused mod-up + inner product
    "bfv13_50": (13, [50] * 4 + [60, 60], 2),             # uniform data primes: what the HPS variant of BFV multiply needs
    # more than four key-switch digits with alpha > 1 (tests/test_gpu_batched_dispatch.py): the unfused mod-up + inner product of one
    # ciphertext, the per-ciphertext inner product loop of a batch, the mod-up that copies the digits' own limbs
    "hyb13_b5": (13, [60] + [50] * 9 + [60] * 2, 2),      # 10 data limbs: beta 5 at levels 10 and 9 (short last digit), 4 at level 8
    "hyb14_b6": (14, [60] + [50] * 11 + [60] * 2, 2),     # beta 6 at N = 2^14, a size whose fused mod-up + inner product stops at beta 4
    "hyb16_b5": (16, [60] + [50] * 44 + [60] * 9, 9),     # 45 data limbs in 5 digits of 9 at N = 2^16: the 16-input fused mod-up conversion with 9 live inputs; beta 5 at levels 45 and 37 (one-limb last digit), 4 at level 36
    # one limb of every width at which the sum kernels change their flush period (tests/test_gpu_sum_widths.py): FP64 limbs of
    # 50 .. 41 bits, integer limbs of 51 .. 61 bits, the 61-bit primes as the special base
    "ladder12": (12, [50, 49, 48, 47, 46, 45, 44, 42, 41, 51, 55, 59, 60, 60, 61, 61], 2),
}

# (config, live data limbs) -> number of key-switch digits, for the sets above
BETA_GT4_LEVELS = {
    "hyb13_b5": {10: 5, 9: 5, 8: 4, 1: 1},
    "hyb14_b6": {12: 6, 8: 4},
    "hyb16_b5": {45: 5, 37: 5, 36: 4},
}


# NTT plan-switch chains (tests/test_gpu_ntt_plans.py).  Both back ends side by side: primes of 51 bits and more run the integer
# butterflies, smaller ones the FP64 ones -- the plain ones at 48..50 bits, the light forward ones below 2^47, the light inverse
# ones below 2^42.  The order puts the integer limbs in the middle and at the end of every 12 limbs, never at the start.
MIXED_BITS = [50, 48, 47, 60, 46, 43, 42, 41, 40, 36, 30, 55]


def chain_bits(count, pattern=MIXED_BITS):
    """The first `count` prime sizes of `pattern` repeated."""
    return [pattern[i % len(pattern)] for i in range(count)]


@functools.lru_cache(maxsize=None)
def chain_primes(log_n, bits):
    """Distinct NTT primes of the sizes `bits` (a tuple) at N = 2^log_n, in that order."""
    return tuple(int(x) for x in O.coeff_modulus_create(1 << log_n, list(bits)))


@functools.lru_cache(maxsize=None)
def primes_of(name):
    log_n, bits, size_p = CONFIGS[name]
    if bits is None:
        return log_n, tuple(C1_PRIMES), size_p
    return log_n, tuple(int(x) for x in O.coeff_modulus_create(1 << log_n, list(bits))), size_p


@functools.lru_cache(maxsize=4)
def oracle_ctx(name):
    log_n, primes, size_p = primes_of(name)
    return O.Ctx(log_n, list(primes), size_p)


def uniform_poly(rng, primes, n):
    """[len(primes)][n] uniform residues, limb i in [0, primes[i])."""
    out = np.empty((len(primes), n), dtype=np.uint64)
    for i, q in enumerate(primes):
        out[i] = rng.integers(0, int(q), n, dtype=np.uint64)
    return out


def rng_for(config_id):
    return np.random.default_rng(0x5EED0000 + config_id)


def oracle_bfv_plain_sum(oc, m, ct, ql, t, acc=None, upto=None):
    """The oracle's loop of bfv_multiply_plain and add over the terms of one group (m [K][N] below t, ct [K][2][L][N] in coefficient
    form), acc added last -- what tests/test_gpu_bfv_plain_sum.py compares with at t = 65537, for any plain modulus; upto: the sums
    after those term counts instead (without acc)."""
    s, partial = None, {}
    for k in range(m.shape[0]):
        prod = oc.bfv_multiply_plain(ct[k], m[k], t)
        s = prod if s is None else np.stack([oc.add(s[p], prod[p], ql) for p in range(2)])
        if upto and k + 1 in upto:
            partial[k + 1] = s
    if upto:
        return partial
    if acc is not None:
        s = np.stack([oc.add(acc[p], s[p], ql) for p in range(2)])
    return s


def first_diff_limb(got, ref, what, primes):
    """Word-for-word comparison of [..., limb, N] arrays over `primes`; a failure names the limb, its bit length and the first
    differing word."""
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    bad = got != ref
    idx = tuple(int(v) for v in np.argwhere(bad)[0])
    limbs = sorted({int(j) for j in np.nonzero(bad.any(axis=-1))[-1]})
    q = int(primes[idx[-2]])
    msg = (f"{what}: {int(np.count_nonzero(bad))} words differ in limbs {[(j, int(primes[j]).bit_length()) for j in limbs]} (index, bits), "
           f"first at {idx} (limb {idx[-2]}, q = {q}, {q.bit_length()} bits): got {int(got[idx])}, want {int(ref[idx])}")
    print(msg)
    raise AssertionError(msg)


def brev(k, bits):
    return int(bin(k)[2:].zfill(bits)[::-1], 2) if bits else 0


def crt_compose(residues, primes):
    """Python big-int CRT: residues[i] mod primes[i] -> value in [0, prod)."""
    M = 1
    for p in primes:
        M *= int(p)
    x = 0
    for r, p in zip(residues, primes):
        p = int(p)
        Mi = M // p
        x += int(r) * Mi * pow(Mi, -1, p)
    return x % M, M
