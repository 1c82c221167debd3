// pha_noise.h -- the per-thread programs of the noise kernels (pha_noise.hip): the exact infinity norm max_j min(v_j, Q - v_j) of an
// RNS polynomial, v_j in [0, Q) the CRT composition of coefficient j -- the reference's compose_array followed by
// poly_infinity_norm_coeffmod (PhantomSecretKey::invariant_noise_budget, src/secretkey.cu:752-840), without a big integer in the
// per-coefficient path.  Host/device functions like pha_decrypt.h, so that tests/emu/emu_noise.cpp replays the very source the
// kernels run (test-only; the product never executes it on the host).  Integer arithmetic only: no floating point, no atomics.
// `Col` is one coefficient's column of L words, col(i) a reference to word i (the kernel: LDS laid out [limb][thread]; the host: an
// array); the tables come from pha_rns_tables.h noise_tables / noise_level_tables.
//
// ---- mixed radix (Garner) -------------------------------------------------------------------------------------------------------
// v = a_0 + a_1 q_0 + a_2 q_0 q_1 + ... + a_{L-1} q_0 .. q_{L-2}, 0 <= a_i < q_i, is the unique such representation of v in [0, Q).
// Digit a_i depends on q_0 .. q_i only, so ONE table for the top level serves every level by prefix.  From the residues x_j:
//     for i = 0 .. L - 1:   a_i = x_i (now final);   for j > i:   x_j <- (x_j - a_i) q_i^-1 mod q_j
// -- the updates of one i are independent of each other (the column is swept L - 1 times, L (L - 1) / 2 modular multiply-subtracts).
// The limbs differ in width (41 .. 61 bits), so a_i can exceed q_j: the difference is formed as x_j + lift_j - a_i with lift_j =
// q_j ceil(2^61 / q_j), a multiple of q_j in [2^61, 2^61 + q_j): a_i < 2^61 <= lift_j keeps it non-negative, and with x_j < 2 q_j
// (the lazy range of shoup_lazy) it stays below 3 q_j + 2^61 < 2^63: an ordinary 64-bit word, which shoup_lazy takes as it is.
// A word is made canonical once, when it becomes a digit.
//
// ---- sign, magnitude, maximum ---------------------------------------------------------------------------------------------------
// Mixed-radix digit vectors of numbers below Q order like the numbers, most significant digit (a_{L-1}) first.  Q is odd, so
// min(v, Q - v) = v when v <= (Q - 1) / 2 and Q - v otherwise (the reference's threshold (Q + 1) / 2): v is compared with the digits
// `half` of (Q - 1) / 2.  Q - 1 has the digits q_i - 1 (the largest number of the system), so Q - 1 - v has the digits q_i - 1 - a_i
// with no borrow; Q - v adds 1, a carry that runs while a digit reaches q_i.  The comparisons run from the LEAST significant digit
// upward and let every later digit overrule: no data-dependent exit, the same sweep for every lane.
//
// ---- binary -----------------------------------------------------------------------------------------------------------------------
// Horner from the top digit over little-endian 64-bit words: acc <- acc q_i + a_i.  After the k top digits acc < q_{L-1} .. q_{L-k} <
// 2^(61 k) <= 2^(64 k): step k touches min(k, L) words and its last carry is 0.  Run once per polynomial, on the winner only.
#pragma once
#include "pha_arith.h"

namespace pha {

constexpr uint32_t kNoiseMaxLimbs = 64;   // as the bgv / bfv decrypt entries (pha_decrypt.h kDecryptMaxLimbs)

// x_j <- (x_j - a) q_i^-1 mod q_j, lazy: x in [0, 2 q_j) -> [0, 2 q_j); a < 2^61; inv = (q_i^-1 mod q_j, Shoup); lift: see above
PHA_HD u64 noise_garner_step(u64 x, u64 a, u64x2 inv, u64 q, u64 lift) { return shoup_lazy(x + lift - a, inv, q); }

// The column's canonical residues -> its mixed-radix digits, in place.  q(i): modulus i; inv(i, j), i < j: (q_i^-1 mod q_j, Shoup);
// lift(j).
template <class Col, class Q, class Inv, class Lift>
PHA_HD void noise_garner(Col &col, uint32_t L, Q q, Inv inv, Lift lift) {
    constexpr int U = 4;   // updates in flight: their loads (column word, table entries) are issued together, then the four chains run
    for (uint32_t i = 0; i < L; i++) {
        const u64 a = csub(col(i), q(i));
        col(i) = a;
        uint32_t j = i + 1;
        for (; j + U <= L; j += U) {
            u64 x[U], qj[U], lf[U];
            u64x2 w[U];
#pragma unroll
            for (int u = 0; u < U; u++) { x[u] = col(j + u); w[u] = inv(i, j + u); qj[u] = q(j + u); lf[u] = lift(j + u); }
#pragma unroll
            for (int u = 0; u < U; u++) x[u] = noise_garner_step(x[u], a, w[u], qj[u], lf[u]);
#pragma unroll
            for (int u = 0; u < U; u++) col(j + u) = x[u];
        }
        for (; j < L; j++) col(j) = noise_garner_step(col(j), a, inv(i, j), q(j), lift(j));
    }
}

// is the number with digits a(.) greater than the one with digits b(.)?
template <class A, class B>
PHA_HD bool noise_greater(A a, B b, uint32_t L) {
    bool gt = false;
    for (uint32_t i = 0; i < L; i++) {
        const u64 x = a(i), y = b(i);
        gt = x > y ? true : (x < y ? false : gt);
    }
    return gt;
}

// digits of v -> digits of min(v, Q - v), in place; returns whether v was above (Q - 1) / 2 (digits half(.))
template <class Col, class Q, class Half>
PHA_HD bool noise_magnitude(Col &col, uint32_t L, Q q, Half half) {
    const bool neg = noise_greater(col, half, L);
    if (neg) {
        u64 carry = 1;
        for (uint32_t i = 0; i < L; i++) {
            const u64 qi = q(i);
            u64 d = qi - 1 - col(i) + carry;   // at most q_i
            carry = d == qi;
            col(i) = carry ? 0 : d;
        }
    }
    return neg;
}

// mixed-radix digits a(.) -> the number as L little-endian words (acc [L])
template <class A, class Q>
PHA_HD void noise_horner(A a, uint32_t L, Q q, u64 *acc) {
    for (uint32_t w = 0; w < L; w++) acc[w] = 0;
    for (uint32_t k = 1; k <= L; k++) {
        const uint32_t i = L - k;
        const u64 qi = q(i);
        u64 carry = a(i);
        for (uint32_t w = 0; w < k; w++) {   // (k <= L)
            u64 lo, hi;
            mul128(acc[w], qi, lo, hi);      // hi <= 2^64 - 2: the carry below cannot wrap it
            lo += carry;
            hi += lo < carry;
            acc[w] = lo;
            carry = hi;
        }
    }
}

// significant bits of a word (0 for 0) and of L little-endian words: no shift by the word size
PHA_HD uint32_t noise_word_bits(u64 v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }
PHA_HD uint32_t noise_bits(const u64 *words, uint32_t L) {
    uint32_t bits = 0;
    for (uint32_t w = 0; w < L; w++)
        if (words[w]) bits = 64 * w + noise_word_bits(words[w]);
    return bits;
}

// invariant_noise_budget's last lines: max(0, bitcount(Q) - bitcount(norm) - 1)
PHA_HD int32_t noise_budget(int q_bits, uint32_t norm_bits) {
    const int d = q_bits - (int)norm_bits - 1;
    return d > 0 ? d : 0;
}

}  // namespace pha
