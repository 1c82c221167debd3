// pha_prng.h -- the per-thread arithmetic of the seeded samplers (pha_prng.hip): host/device functions, so
// that tests/emu/emu_prng.cpp replays them on the CPU against the numpy restatement (tests/prng_restatement.py).
//
// Reference semantics (src/prng.cu, include/prng.cuh).  A seed is 64 bytes; one generator block is 64 bytes from (seed, nonce):
//   input words x[0..7] = seed bytes 0..31 (little endian), x[8], x[9] = the low and high half of the 64-bit nonce,
//   x[10..15] = seed bytes 32..55; NO constants, seed bytes 56..63 are never read;
//   10 double rounds of the Salsa20 quarter-round (rotations 7, 9, 13, 18; columns, then rows); output = result + input, word by word.
// This is the Salsa20 core on the reference's own input layout, not the Salsa20 stream cipher.
//   ternary  coefficient i: nonce i, v = (byte 0) % 3 - 1
//   noise    coefficient i: nonce i, v = popcount(b0) + popcount(b1) + popcount(b2 & 0x1f) - popcount(b3) - popcount(b4) - popcount(b5 & 0x1f)
//            (centred binomial over 21 + 21 bits, |v| <= 21).  Both need output words 0 and 1 only and do not depend on the limb.
//   uniform  group g = row position * (N / 8) + j owns words 8 j .. 8 j + 7 of its row: prng_uniform_group below.
// The 16 state words are named registers and the output block is only ever indexed by constants (the uniform rule unrolls its eight
// indexes), so nothing of a thread's state is addressed at run time: no scratch (the compiler's figures are in DESIGN.md 4.14).
#pragma once
#include "pha_arith.h"

namespace pha {

constexpr int kPrngSeedBytes = 64;        // a seed, of which bytes 0..55 are used
constexpr int kPrngGroupWords = 8;        // 64-bit words per generator block = coefficients per uniform group

struct PrngKey {                          // the 14 seed words: input words 0..7 and 10..15
    u32 k[14];
};
struct PrngBlock {
    u32 w[16];
    PHA_HD u64 word64(int i) const { return (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32); }
};

// little-endian words of the seed.  The device form reads aligned 32-bit words (the entries refuse a seed buffer that is not
// 16-byte aligned; the address is uniform over the workgroup); the host form composes bytes
PHA_HD PrngKey prng_load_key(const uint8_t *seed) {
    PrngKey key;
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 *s = reinterpret_cast<const u32 *>(seed);
#pragma unroll
    for (int i = 0; i < 14; i++) key.k[i] = s[i];
#else
    for (int i = 0; i < 14; i++)
        key.k[i] = (u32)seed[4 * i] | ((u32)seed[4 * i + 1] << 8) | ((u32)seed[4 * i + 2] << 16) | ((u32)seed[4 * i + 3] << 24);
#endif
    return key;
}

PHA_HD u32 prng_rotl(u32 x, int c) { return (x << c) | (x >> (32 - c)); }
// the Salsa20 quarter-round on (a, b, c, d)
#define PHA_PRNG_QR(a, b, c, d)      \
    b ^= prng_rotl(a + d, 7);        \
    c ^= prng_rotl(b + a, 9);        \
    d ^= prng_rotl(c + b, 13);       \
    a ^= prng_rotl(d + c, 18);
PHA_HD void prng_quarter_round(u32 &a, u32 &b, u32 &c, u32 &d) { PHA_PRNG_QR(a, b, c, d) }

PHA_HD PrngBlock prng_block(const PrngKey &key, u64 nonce) {
    const u32 j0 = key.k[0], j1 = key.k[1], j2 = key.k[2], j3 = key.k[3], j4 = key.k[4], j5 = key.k[5], j6 = key.k[6], j7 = key.k[7];
    const u32 j8 = (u32)nonce, j9 = (u32)(nonce >> 32);
    const u32 j10 = key.k[8], j11 = key.k[9], j12 = key.k[10], j13 = key.k[11], j14 = key.k[12], j15 = key.k[13];
    u32 x0 = j0, x1 = j1, x2 = j2, x3 = j3, x4 = j4, x5 = j5, x6 = j6, x7 = j7, x8 = j8, x9 = j9, x10 = j10, x11 = j11, x12 = j12,
        x13 = j13, x14 = j14, x15 = j15;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int r = 0; r < 10; r++) {
        PHA_PRNG_QR(x0, x4, x8, x12)      // columns
        PHA_PRNG_QR(x5, x9, x13, x1)
        PHA_PRNG_QR(x10, x14, x2, x6)
        PHA_PRNG_QR(x15, x3, x7, x11)
        PHA_PRNG_QR(x0, x1, x2, x3)       // rows
        PHA_PRNG_QR(x5, x6, x7, x4)
        PHA_PRNG_QR(x10, x11, x8, x9)
        PHA_PRNG_QR(x15, x12, x13, x14)
    }
    return PrngBlock{{x0 + j0, x1 + j1, x2 + j2, x3 + j3, x4 + j4, x5 + j5, x6 + j6, x7 + j7, x8 + j8, x9 + j9, x10 + j10, x11 + j11,
                      x12 + j12, x13 + j13, x14 + j14, x15 + j15}};
}

// the value rules, on output words 0 and 1; the results are signed
PHA_HD int prng_ternary_value(u32 w0) { return (int)((w0 & 0xffu) % 3u) - 1; }
PHA_HD int prng_error_value(u32 w0, u32 w1) {
    return __builtin_popcount(w0 & 0x001fffffu) - __builtin_popcount(w0 >> 24) - __builtin_popcount(w1 & 0x00001fffu);
}
// the two stored forms of a small signed value: the two's-complement word of the encryption entries, the canonical residue (|v| < q)
PHA_HD u64 prng_signed_word(int v) { return (u64)(int64_t)v; }
PHA_HD u64 prng_residue(int v, u64 q) { return v < 0 ? q - (u64)(-v) : (u64)v; }

// the largest accepted word: (2^64 - 1) - ((2^64 - 1) mod q) - 1.  barrett64 is exact for every 64-bit word and every q < 2^63 (its
// quotient estimate is the true one or one less, so the remainder is below 2 q before the conditional subtraction)
PHA_HD u64 prng_max_multiple(u64 q, u64 ratio1) {
    const u64 max_random = ~(u64)0;
    return max_random - barrett64(max_random, q, ratio1) - 1;
}

// One uniform group: eight words below q.  The thread draws the block of nonce g; for index 0..7 it takes word `index` of the
// CURRENT block, and while that word exceeds the bound it draws the block of nonce g + tries * redraw_step (tries = blocks drawn so
// far; redraw_step = N * rows) and looks at word `index` of the new one.  Words already stored stay; later indexes read the newest
// block.  Returns the number of blocks drawn.
PHA_HD u32 prng_uniform_group(const PrngKey &key, u64 g, u64 redraw_step, u64 q, u64 ratio1, u64 (&out)[kPrngGroupWords]) {
    const u64 bound = prng_max_multiple(q, ratio1);
    PrngBlock b = prng_block(key, g);
    u32 tries = 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int index = 0; index < kPrngGroupWords; index++) {
        u64 w = b.word64(index);
        while (w > bound) {
            b = prng_block(key, g + (u64)tries * redraw_step);
            tries++;
            w = b.word64(index);
        }
        out[index] = barrett64(w, q, ratio1);
    }
    return tries;
}

}  // namespace pha
