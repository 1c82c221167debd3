"""The reference's seeded samplers (src/prng.cu) restated in numpy from their description, for the tests of csrc/pha_prng.h / .hip.

Two independent forms.  The VECTORISED one (block, ternary, noise, uniform) works on whole arrays of nonces and is what the tests
compare the library with.  The SCALAR one (scalar_*) transcribes the reference's thread programs loop by loop on Python integers,
including the one-block-per-limb recomputation of the ternary and noise kernels; tests/test_prng_restatement.py holds the two
against each other and pins both by hand-worked values.

The generator block: 16 32-bit words = seed bytes 0..31 (little endian), nonce low, nonce high, seed bytes 32..55; no constants, seed
bytes 56..63 never read; 10 double rounds of the Salsa20 quarter-round (rotations 7, 9, 13, 18; columns, then rows); plus the input.
"""
import numpy as np

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
COLUMNS = ((0, 4, 8, 12), (5, 9, 13, 1), (10, 14, 2, 6), (15, 3, 7, 11))
ROWS = ((0, 1, 2, 3), (5, 6, 7, 4), (10, 11, 8, 9), (15, 12, 13, 14))

# Parameter set reject12: N = 2^12, NTT primes just above 2^64 / 17 (each rejects 1 - 16 q / 2^64 = 5.88 % of the 64-bit words), the
# last one special.  Every other set of the suite sits just below a power of two and never redraws.
REJECT12 = (12, (0xf0f0f0f0f11a001, 0xf0f0f0f0f124001, 0xf0f0f0f0f132001), 1)
# the fixed seed of the redraw, ternary and noise statistics (chosen on the CPU: tests/test_prng_restatement.py states what it meets)
STAT_SEED = bytes((37 * i + 11) & 0xFF for i in range(64))
STAT_SEED_ARRAY = np.frombuffer(STAT_SEED, dtype=np.uint8)


def seed_bytes(tag):
    """A deterministic 64-byte test seed per integer tag (numpy uint8 [64])."""
    return np.random.default_rng([0x5A15A, int(tag)]).integers(0, 256, 64, dtype=np.uint8)


def _rotl(x, c):
    return (x << np.uint32(c)) | (x >> np.uint32(32 - c))


def quarter_round(a, b, c, d):
    """The Salsa20 quarter-round on uint32 arrays; returns the new (a, b, c, d)."""
    b = b ^ _rotl(a + d, 7)
    c = c ^ _rotl(b + a, 9)
    d = d ^ _rotl(c + b, 13)
    a = a ^ _rotl(d + c, 18)
    return a, b, c, d


def input_words(seed, nonces):
    """[16][len(nonces)] uint32 input words."""
    seed = np.asarray(seed, dtype=np.uint8)
    nonces = np.asarray(nonces, dtype=np.uint64)
    key = seed[:56].copy().view("<u4")
    x = np.empty((16, nonces.size), dtype=np.uint32)
    for i in range(8):
        x[i] = key[i]
    x[8] = (nonces & np.uint64(M32)).astype(np.uint32)
    x[9] = (nonces >> np.uint64(32)).astype(np.uint32)
    for i in range(6):
        x[10 + i] = key[8 + i]
    return x


def core(x):
    """The block function on [16][K] uint32 input words: the output words."""
    with np.errstate(over="ignore"):
        y = [x[i].copy() for i in range(16)]
        for _ in range(10):
            for group in (COLUMNS, ROWS):
                for i, j, k, l in group:
                    y[i], y[j], y[k], y[l] = quarter_round(y[i], y[j], y[k], y[l])
        return np.stack([y[i] + x[i] for i in range(16)])


def block(seed, nonces):
    """[len(nonces)][16] uint32 output words of the blocks (seed, nonce)."""
    return np.ascontiguousarray(core(input_words(seed, nonces)).T)


def block_words64(seed, nonces):
    """[len(nonces)][8] uint64: the 64 output bytes read as eight little-endian 64-bit words."""
    b = block(seed, nonces).astype(np.uint64)
    return b[:, 0::2] | (b[:, 1::2] << np.uint64(32))


def _popcount(x):
    x = np.ascontiguousarray(x, dtype=np.uint32)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).astype(np.int64)


def ternary_signed(seed, n):
    """[n] int64: coefficient i = byte 0 of the block of nonce i, % 3, - 1."""
    b = block(seed, np.arange(n, dtype=np.uint64))
    return (b[:, 0] & np.uint32(0xFF)).astype(np.int64) % 3 - 1


def error_signed(seed, n):
    """[n] int64: popcount(b0) + popcount(b1) + popcount(b2 & 0x1f) - popcount(b3) - popcount(b4) - popcount(b5 & 0x1f)."""
    b = block(seed, np.arange(n, dtype=np.uint64))
    by = np.ascontiguousarray(b[:, :2]).view(np.uint8).reshape(n, 8).astype(np.uint32)
    pc = lambda v: _popcount(v)   # noqa: E731
    return pc(by[:, 0]) + pc(by[:, 1]) + pc(by[:, 2] & 0x1F) - pc(by[:, 3]) - pc(by[:, 4]) - pc(by[:, 5] & 0x1F)


def residues(signed, primes):
    """[len(primes)][n] uint64: the signed values modulo every prime (-1 becomes q - 1)."""
    signed = np.asarray(signed, dtype=np.int64)          # |v| <= 21 and q < 2^62: numpy's % of a positive modulus is non-negative
    return np.stack([(signed % np.int64(int(q))).astype(np.uint64) for q in primes])


def max_multiple(q):
    return M64 - (M64 % int(q)) - 1


def uniform(seed, primes, n, log=None):
    """[len(primes)][n] uint64, the reference's sample_uniform_poly over the limbs `primes` (in this order: the nonce uses the limb's
    POSITION).  Vectorised over the groups: every round looks at word `index` of each group's newest block and redraws, for the
    groups whose word is above the bound, the block of nonce g + tries * n * len(primes).
    log: a list that receives (limb position, group j, index, redraws in a row at this index) for every redrawn word."""
    cms, groups = len(primes), n // 8
    out = np.empty((cms, n), dtype=np.uint64)
    g = np.arange(cms * groups, dtype=np.uint64)
    bound = np.repeat(np.array([max_multiple(q) for q in primes], dtype=np.uint64), groups)
    qs = np.repeat(np.array([int(q) for q in primes], dtype=np.uint64), groups)
    cur = block_words64(seed, g)
    tries = np.ones(g.size, dtype=np.uint64)
    step = np.uint64(n * cms)
    for index in range(8):
        in_a_row = np.zeros(g.size, dtype=np.int64)
        while True:
            bad = np.nonzero(cur[:, index] > bound)[0]
            if bad.size == 0:
                break
            cur[bad] = block_words64(seed, g[bad] + tries[bad] * step)
            tries[bad] += np.uint64(1)
            in_a_row[bad] += 1
        if log is not None:
            for k in np.nonzero(in_a_row)[0]:
                log.append((int(k) // groups, int(k) % groups, index, int(in_a_row[k])))
        out.reshape(cms * groups, 8)[:, index] = cur[:, index] % qs
    return out


def rows_of(primes, size_p, size_ql, with_special):
    """The primes of the encoder's row convention: [0, size_ql), then the special ones."""
    primes = [int(q) for q in primes]
    return primes[:size_ql] + (primes[len(primes) - size_p:] if with_special and size_p else [])


# ---- the scalar transcription of the reference's thread programs (Python integers, one thread at a time) ---------------------------
def scalar_block(seed, nonce):
    """salsa20_gpu(out, 64, nonce, key, 64): the 64 output bytes."""
    key = bytes(bytearray(np.asarray(seed, dtype=np.uint8)))
    load = lambda at: int.from_bytes(key[at:at + 4], "little")   # noqa: E731
    rot = lambda v, c: ((v << c) | (v >> (32 - c))) & M32        # noqa: E731
    j = [load(4 * i) for i in range(8)] + [nonce & M32, (nonce >> 32) & M32] + [load(32 + 4 * i) for i in range(6)]
    x = list(j)
    for _ in range(10):
        for a, b, c, d in COLUMNS + ROWS:
            x[b] ^= rot((x[a] + x[d]) & M32, 7)
            x[c] ^= rot((x[b] + x[a]) & M32, 9)
            x[d] ^= rot((x[c] + x[b]) & M32, 13)
            x[a] ^= rot((x[d] + x[c]) & M32, 18)
    return b"".join(((x[i] + j[i]) & M32).to_bytes(4, "little") for i in range(16))


def scalar_ternary_poly(seed, primes, n):
    """sample_ternary_poly: thread tid < n * cms recomputes the block of nonce tid % n for its own limb."""
    out = np.empty((len(primes), n), dtype=np.uint64)
    for tid in range(n * len(primes)):
        twr = tid // n
        r = scalar_block(seed, tid % n)[0] % 3
        out[twr, tid % n] = (r + (int(primes[twr]) if r == 0 else 0) - 1) & M64
    return out


def scalar_error_poly(seed, primes, n):
    """sample_error_poly: thread tid < n * cms recomputes the block of nonce tid % n for its own limb."""
    hw = lambda v: bin(v).count("1")   # noqa: E731
    out = np.empty((len(primes), n), dtype=np.uint64)
    for tid in range(n * len(primes)):
        twr = tid // n
        t = scalar_block(seed, tid % n)
        cbd = hw(t[0]) + hw(t[1]) + hw(t[2] & 0x1F) - hw(t[3]) - hw(t[4]) - hw(t[5] & 0x1F)
        out[twr, tid % n] = (cbd + (int(primes[twr]) if cbd < 0 else 0)) & M64
    return out


def scalar_uniform_poly(seed, primes, n, groups=None):
    """sample_uniform_poly: thread tid < (n / 8) * cms, starting at index = 0, tries = 0.  groups: only these thread ids (the rest
    of the output stays zero)."""
    cms = len(primes)
    out = np.zeros((cms, n), dtype=np.uint64)
    flat = out.reshape(-1)
    for tid in (range((n >> 3) * cms) if groups is None else groups):
        q = int(primes[tid // (n >> 3)])
        bound = M64 - (M64 % q) - 1
        index, tries = 0, 0
        tmp = scalar_block(seed, tid)
        tries += 1
        while index < 8:
            while int.from_bytes(tmp[8 * index:8 * index + 8], "little") > bound:
                tmp = scalar_block(seed, tid + tries * n * cms)
                tries += 1
            flat[tid * 8 + index] = int.from_bytes(tmp[8 * index:8 * index + 8], "little") % q
            index += 1
    return out
