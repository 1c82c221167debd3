// pha_decrypt.h -- the per-thread programs of the decryption kernels (pha_decrypt.hip): the phase c0 + sum_i c_i (.) s^i of a group
// of ciphertexts, the BFV scale-and-round floor(t x / Q + 1/2) mod t, and the BGV tail (the exact conversion to t with the inverse
// correction factor in its store).  Host/device functions like pha_plain_sum.h, so that tests/emu/emu_decrypt.cpp replays the
// very source the kernels run (test-only; the product never executes it on the host).  The kernels supply the loads (`Src`);
// `Probe` sees every accumulator just before it is reduced (the kernels pass PlainSumNoProbe, which compiles to nothing).
//
// ---- phase ------------------------------------------------------------------------------------------------------------------
// One thread holds two adjacent coefficients of one limb of G <= kPhaseGroup ciphertexts of k polynomials: for i = 1 .. k - 1 it
// loads the words of s^i ONCE and multiplies them into the G running sums, so the secret key costs (k - 1) / G words per output
// word instead of k - 1 (derived from the loop below, not measured).  Every product is of two canonical words, and an accumulator
// starts from c0's word (at most q - 1; 0 when c0 is dropped): the magnitudes of a plaintext product, so the terms per flush are
// those derived in pha_plain_sum.h, read from the modulus' bit length b:
//   integer limbs: 128-bit accumulators, one barrett128 per output (it reduces ANY 128-bit value).  After T terms an accumulator
//     holds at most (q - 1) + T (q - 1)^2 < 2^128 for T = 2^(128 - 2b) (pha_plain_sum.h has the inequality): 64 terms at 61
//     bits, 256 at 60.  So k - 1 <= 64, i.e. every k <= 65, needs NO flush at 61 bits (k <= 257 at 60 bits); from k = 66 on
//     the sums are reduced every 64 terms and restart from their residues (at most q - 1 again).
//   FP64 limbs (q < 2^50): every product reduced on the spot by fp_mulmod_light to |r| <= 0.875 q, summed in doubles, re-centred
//     (fp_reduce) only every T = floor((56 * 2^(52 - b) - 40) / 35) terms, which keeps |x| <= q (1 + 0.875 T) <= 1.4 * 2^52 <
//     2^52.6: exact integers inside fp_reduce's domain.  5 terms at 50 bits (k <= 6 without a re-centring), 11 at 49, 6552 at 40.
//     The last interval is not flushed: fp_to_canon reduces before it converts.
// Every word written is canonical (barrett128 / fp_to_canon).
//
// ---- BFV scale-and-round (one form; the reference picks one of four by bit counts, src/rns.cu:1519-1689) -------------------------
// x in [0, Q) is given by its canonical residues x_i.  With y_i = [x_i qhat_i^-1]_{q_i}, x = sum_i y_i qhat_i - (an integer) Q, so
// t x / Q == sum_i y_i t / q_i == sum_i x_i t [qhat_i^-1]_{q_i} / q_i (mod t) -- the congruences drop integer multiples of t.  Every
// word is split at h = ceil(bits of the level's largest prime / 2) <= 31 into x_i = lo_i + hi_i 2^h, lo_i, hi_i < 2^h <= 2^31, and
//     t x / Q == sum_i lo_i A_i / q_i + hi_i B_i / q_i  (mod t),   A_i = t [qhat_i^-1]_{q_i},  B_i = t [qhat_i^-1 2^h]_{q_i},
// big integers below t q_i.  Per limb two integer tables (floor(A_i / q_i) mod t, floor(B_i / q_i) mod t) and two fraction tables
// (frac(A_i / q_i), frac(B_i / q_i) as doubles; pha_rns_tables.h decrypt_round_tables builds all four from 128-bit integers):
//     out = (sum_i lo_i intA_i + hi_i intB_i  +  llround(F)) mod t,     F = sum_i lo_i fracA_i + hi_i fracB_i  in [0, 2 L 2^31).
// The integer side is exact for every admitted t (t < 2^60): one product is below 2^31 * 2^60 = 2^91 -- no 64-bit word holds even
// one, so the sum lives in a 128-bit accumulator (mac128) whose HIGH word cannot overflow before 2^(128 - 91) = 2^37 products:
// the flush period is 2^37 terms, beyond the 2 L <= 2^33 terms of any limb count a 32-bit L can name, so the loop has no flush;
// llround(F) < 2^39 is added to the accumulator and ONE barrett128 gives the canonical word.
// Error of F as computed (fused multiply-adds in limb order, lo before hi), for L <= 64:
//   tables: each within 2^-52 of its true value (2^-64 from the 64-bit quotient, 2^-54 from its conversion), times a factor below
//     2^31: 2^-21 per term, 2 L terms: L 2^-20;
//   accumulation: the products lo * frac are exact inside the fma; each of the 2 L accumulates rounds a partial sum below
//     2 L 2^31 <= 2^38 once, i.e. by at most half an ulp of [2^37, 2^38) = 2^-16: L 2^-15;
//   total: L (2^-15 + 2^-20) < L 2^-14.95 <= L 2^-14, the margin the tests use: out differs from floor(t x / Q + 1/2) mod t only
//     where |frac(t x / Q) - 1/2| is below that.
// Deviation from the reference, deliberate: its kernels store llround of a value in [0, t), which can be t itself (a plaintext 0
// with slightly negative noise); here that word is 0 -- only canonical words are written, as with the encoder's -0.0.
//
// ---- BGV tail -------------------------------------------------------------------------------------------------------------------
// exact_convert_array (src/rns_bconv.cu:374-414; exact_convert_kernel in pha_behz.hip has the same arithmetic) to the ONE modulus t,
// then, unless the factor is 1, one multiply mod t by the inverse correction factor: the words of the two separate steps.
#pragma once
#include "pha_arith.h"
#include "pha_plain_sum.h"

namespace pha {

constexpr uint32_t kDecryptMaxLimbs = 64;   // the error bound of the fraction sum above is derived for L <= 64: larger levels are refused
constexpr int kPhaseGroup = 4;   // ciphertexts per thread: G accumulator pairs and one secret-key word pair live in registers

// Src: c(g, i) = the word pair of polynomial i < k of the group's ciphertext g < G (each read once); s(i) = that of s^i, i >= 1.
// K: the ciphertext size when it is a compile-time constant (2, 3: the loop unrolls and every load is in flight at once), 0: `k`.
template <int G, int K, class Src, class Probe>
PHA_HD void phase_int(Src &src, uint32_t k, bool with_c0, const DModulus &m, u64x2 *r, Probe &probe) {
    const uint32_t kk = K ? (uint32_t)K : k;
    const uint32_t per = plain_sum_per_int(modulus_bits(m.value));
    u64 lx[G], ly[G], hx[G], hy[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const u64x2 c = with_c0 ? src.c(g, 0) : u64x2{0, 0};
        lx[g] = c.x; ly[g] = c.y;
        hx[g] = hy[g] = 0;
    }
    uint32_t since = 0;
    for (uint32_t i = 1; i < kk; i++) {   // (a constant trip count with K: unrolled, every load in flight at once)
        if (since == per) {   // (never below k = 66 at 61 bits) restart from the residues
#pragma unroll
            for (int g = 0; g < G; g++) {
                probe.i128(lx[g], hx[g]); probe.i128(ly[g], hy[g]);
                lx[g] = barrett128(lx[g], hx[g], m); ly[g] = barrett128(ly[g], hy[g], m);
                hx[g] = hy[g] = 0;
            }
            since = 0;
        }
        const u64x2 s = src.s(i);
#pragma unroll
        for (int g = 0; g < G; g++) {
            const u64x2 c = src.c(g, i);
            mac128(c.x, s.x, lx[g], hx[g]);
            mac128(c.y, s.y, ly[g], hy[g]);
        }
        since++;
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        probe.i128(lx[g], hx[g]); probe.i128(ly[g], hy[g]);
        r[g] = u64x2{barrett128(lx[g], hx[g], m), barrett128(ly[g], hy[g], m)};
    }
}

template <int G, int K, class Src, class Probe>
PHA_HD void phase_fp(Src &src, uint32_t k, bool with_c0, FpMod fm, int bits, u64x2 *r, Probe &probe) {
    const uint32_t kk = K ? (uint32_t)K : k;
    const uint32_t per = plain_sum_per_fp(bits);
    double sx[G], sy[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const u64x2 c = with_c0 ? src.c(g, 0) : u64x2{0, 0};
        sx[g] = fp_from_canon(c.x); sy[g] = fp_from_canon(c.y);
    }
    uint32_t since = 0;
    for (uint32_t i = 1; i < kk; i++) {   // (a constant trip count with K: unrolled, every load in flight at once)
        if (since == per) {
#pragma unroll
            for (int g = 0; g < G; g++) {
                probe.f64(sx[g]); probe.f64(sy[g]);
                sx[g] = fp_reduce(sx[g], fm); sy[g] = fp_reduce(sy[g], fm);
            }
            since = 0;
        }
        const u64x2 s = src.s(i);
        const double wx = fp_from_canon(s.x), wy = fp_from_canon(s.y);
#pragma unroll
        for (int g = 0; g < G; g++) {
            const u64x2 c = src.c(g, i);
            sx[g] += fp_mulmod_light(fp_from_canon(c.x), wx, fm);
            sy[g] += fp_mulmod_light(fp_from_canon(c.y), wy, fm);
        }
        since++;
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        probe.f64(sx[g]); probe.f64(sy[g]);
        r[g] = u64x2{fp_to_canon(sx[g], fm), fp_to_canon(sy[g], fm)};
    }
}

// the split point of the scale-and-round: h = ceil(bits / 2) for the widest modulus of the level (bits <= 61: h <= 31)
PHA_HD int decrypt_split_bits(int max_modulus_bits) { return (max_modulus_bits + 1) / 2; }

// One coefficient.  src(i) = its canonical word in limb i < L; frac / itab [L][2]: the (lo, hi) fraction and integer tables; `f_out`
// (tests): the fraction sum as computed.
template <class Src>
PHA_HD u64 decrypt_scale_round(Src &src, uint32_t L, int h, const double *frac, const u64 *itab, const DModulus &t, double *f_out = nullptr) {
    const u64 mask = ((u64)1 << h) - 1;
    double f = 0.0;
    u64 lo = 0, hi = 0;
    for (uint32_t i = 0; i < L; i++) {
        const u64 x = src(i);
        const u32 xl = (u32)(x & mask), xh = (u32)(x >> h);   // both below 2^h <= 2^31
        f = __builtin_fma((double)xl, frac[2 * i], f);
        f = __builtin_fma((double)xh, frac[2 * i + 1], f);
        mac128(xl, itab[2 * i], lo, hi);
        mac128(xh, itab[2 * i + 1], lo, hi);
    }
    if (f_out) *f_out = f;
    const u64 k = (u64)__builtin_round(f);   // llround: f >= 0, below 2^39
    lo += k;
    hi += lo < k;
    return barrett128(lo, hi, t);
}

// One coefficient of the BGV tail.  hat_inv [L]: qhat_i^-1 mod q_i (+ Shoup); mat [L]: qhat_i mod t; q [L]: the primes; q_mod_t: Q mod t;
// factor: the inverse correction factor mod t (1: nothing is multiplied).  v is a sum of IEEE divisions in limb order.
template <class Src>
PHA_HD u64 decrypt_mod_t_convert(Src &src, uint32_t L, const u64x2 *hat_inv, const u64 *mat, const u64 *q, u64 q_mod_t, const DModulus &t,
                                 u64 factor) {
    u64 lo = 0, hi = 0;
    double v = 0.0;
    for (uint32_t i = 0; i < L; i++) {
        const u64 qi = q[i];
        const u64 yi = shoup(src(i), hat_inv[i], qi);
        mac128(yi, mat[i], lo, hi);
        v += (double)yi / (double)qi;
    }
    const u64 inner = barrett128(lo, hi, t);
    const u64 rounded = (u64)__builtin_round(v);
    const u64 out = sub_mod(inner, mul_mod(rounded, q_mod_t, t), t.value);
    return factor == 1 ? out : mul_mod(out, factor, t);
}

}  // namespace pha
