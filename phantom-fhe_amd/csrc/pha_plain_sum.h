// pha_plain_sum.h -- the per-thread program of plain_sum_kernel (pha_poly.hip): res = acc + sum over k of plain[k] (.) ct[k] for two
// adjacent coefficients of both polynomials of a ciphertext, the four sums held in registers.  Host/device functions like
// pha_arith.h, so that tests/emu/emu_plain_sum.cpp replays the very source the kernel runs (test-only; the product never executes
// it on the host).  The kernel supplies the loads (`Src::next`: one term's plaintext word pair and the two ciphertext word pairs,
// then advance); `Probe` sees every accumulator just before it is reduced (the kernel passes PlainSumNoProbe, which compiles to
// nothing).
//
// Terms per flush, per limb, from the bit length b of its modulus (q < 2^b, read from the modulus, not assumed).  The per-term
// magnitudes are those of a plaintext product, NOT the summed tensor product's: there is no (a0 + a1)(b0 + b1) term here, every
// product is of two canonical words.
//
// Integer limbs: 128-bit accumulators (mac128), one barrett128 per accumulator and flush -- it reduces ANY 128-bit value.  One
// product is at most (q - 1)^2.  An accumulator starts from acc's word or, after a flush, from the residue it restarts with: at
// most q - 1 either way (0 without acc).  After T terms it holds at most
//     (q - 1) + T (q - 1)^2  <  2^b + T (2^b - 1)^2  =  2^b + T 2^(2b) - T 2^(b + 1) + T,
// and with T = 2^(128 - 2b) that is 2^128 - (2^(129 - b) - 2^b - 2^(128 - 2b)) < 2^128 for every b <= 64 (2^b + 2^(128 - 2b) <
// 2^(129 - b): at b = 61, 2^61 + 2^6 < 2^68; at b = 64, 2^64 + 1 < 2^65).  T = 2^(128 - 2b), capped at kPlainSumMaxPer = 2^16:
//     64 terms per flush at 61 bits, 256 at 60 bits, and the cap at 50, 49 and 40 bits (2^28, 2^30 and 2^48 uncapped; limbs
//     that narrow take this path only where the FP64 tables are absent).
//
// FP64 limbs (fpinfo.ok: q < 2^50, b <= 50): a double cannot hold the unreduced product, so every product is reduced on the spot
// by fp_mulmod_light to an exact integer r == plain * ct (mod q) with |r| <= q (0.5 + 1.5 |Y| 2^-52) (pha_arith.h), |Y| < q <=
// 2^50: |r| <= 0.875 q.  What is deferred is the re-centring and the conversion to canonical words: the values are summed in
// doubles, exact while the magnitude stays below 2^53.  An accumulator starts from acc's word, below q, or after a flush
// (fp_reduce) from |x| <= q / 2 + 1 <= q; T terms later |x| <= q (1 + 0.875 T) < 2^b (1 + 0.875 T).  Keeping that at or below
// 1.4 * 2^52 < 2^52.5 -- inside fp_reduce's domain (|x| < 2^52.6) and exact in a double -- needs 1 + 0.875 T <= 1.4 * 2^(52 - b):
//     T = floor((56 * 2^(52 - b) - 40) / 35), capped at 2^16:   5 terms per flush at 50 bits, 11 at 49, 6552 at 40.
// (61 and 60 bits have no FP64 form.)  The last interval is not flushed: fp_to_canon reduces before it converts, and its input
// obeys the same bound.
#pragma once
#include "pha_arith.h"

namespace pha {

constexpr uint32_t kPlainSumMaxPer = 1u << 16;

PHA_HD int modulus_bits(u64 q) { return 64 - __builtin_clzll(q); }   // q < 2^bits (q != 0)

PHA_HD uint32_t plain_sum_per_int(int bits) {
    const int sh = 128 - 2 * bits;
    return sh <= 0 ? 1u : (sh >= 16 ? kPlainSumMaxPer : 1u << sh);
}
PHA_HD uint32_t plain_sum_per_fp(int bits) {   // bits <= 50
    const u64 t = ((56ull << (52 - bits)) - 40) / 35;
    return t < kPlainSumMaxPer ? (uint32_t)t : kPlainSumMaxPer;
}

struct PlainSumNoProbe {
    PHA_HD void i128(u64, u64) const {}
    PHA_HD void f64(double) const {}
};

// a0 / a1: acc's words for the two polynomials (zero without acc); r0 / r1: the canonical sums
template <class Src, class Probe>
PHA_HD void plain_sum_int(Src &src, uint32_t terms, const DModulus &m, u64x2 a0, u64x2 a1, u64x2 &r0, u64x2 &r1, Probe &probe) {
    const uint32_t per = plain_sum_per_int(modulus_bits(m.value));
    u64 l0x = a0.x, l0y = a0.y, l1x = a1.x, l1y = a1.y;
    u64 h0x = 0, h0y = 0, h1x = 0, h1y = 0;
    uint32_t t = 0;
    for (;;) {
        const uint32_t end = terms - t < per ? terms : t + per;
#pragma unroll 2
        for (; t < end; t++) {
            u64x2 w, c0, c1;
            src.next(w, c0, c1);
            mac128(w.x, c0.x, l0x, h0x);
            mac128(w.y, c0.y, l0y, h0y);
            mac128(w.x, c1.x, l1x, h1x);
            mac128(w.y, c1.y, l1y, h1y);
        }
        probe.i128(l0x, h0x); probe.i128(l0y, h0y); probe.i128(l1x, h1x); probe.i128(l1y, h1y);
        r0 = u64x2{barrett128(l0x, h0x, m), barrett128(l0y, h0y, m)};
        r1 = u64x2{barrett128(l1x, h1x, m), barrett128(l1y, h1y, m)};
        if (t >= terms) return;
        l0x = r0.x; l0y = r0.y; l1x = r1.x; l1y = r1.y;   // restart from the residues
        h0x = h0y = h1x = h1y = 0;
    }
}

template <class Src, class Probe>
PHA_HD void plain_sum_fp(Src &src, uint32_t terms, FpMod fm, int bits, u64x2 a0, u64x2 a1, u64x2 &r0, u64x2 &r1, Probe &probe) {
    const uint32_t per = plain_sum_per_fp(bits);
    double s0x = fp_from_canon(a0.x), s0y = fp_from_canon(a0.y), s1x = fp_from_canon(a1.x), s1y = fp_from_canon(a1.y);
    uint32_t t = 0;
    for (;;) {
        const uint32_t end = terms - t < per ? terms : t + per;
#pragma unroll 2
        for (; t < end; t++) {
            u64x2 w, c0, c1;
            src.next(w, c0, c1);
            const double wx = fp_from_canon(w.x), wy = fp_from_canon(w.y);
            s0x += fp_mulmod_light(fp_from_canon(c0.x), wx, fm);
            s0y += fp_mulmod_light(fp_from_canon(c0.y), wy, fm);
            s1x += fp_mulmod_light(fp_from_canon(c1.x), wx, fm);
            s1y += fp_mulmod_light(fp_from_canon(c1.y), wy, fm);
        }
        probe.f64(s0x); probe.f64(s0y); probe.f64(s1x); probe.f64(s1y);
        if (t >= terms) break;
        s0x = fp_reduce(s0x, fm); s0y = fp_reduce(s0y, fm);
        s1x = fp_reduce(s1x, fm); s1y = fp_reduce(s1y, fm);
    }
    r0 = u64x2{fp_to_canon(s0x, fm), fp_to_canon(s0y, fm)};
    r1 = u64x2{fp_to_canon(s1x, fm), fp_to_canon(s1y, fm)};
}

}  // namespace pha
