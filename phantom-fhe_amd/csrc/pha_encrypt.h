// pha_encrypt.h -- the per-thread arithmetic of the encryption entries (pha_encrypt.hip): host/device
// functions, so that tests/emu/emu_encrypt.cpp replays them on the CPU against Python integers.
//
// Reference semantics (src/secretkey.cu:11-192, 232-295, 382-395, 463-531), with k = t for bgv and k = 1 otherwise:
//   encrypt_zero_symmetric, NTT form          (c0, c1) = (-(a (.) s + NTT(k e)), a)
//   encrypt_zero_asymmetric, NTT form         c_j = pk_j (.) NTT(u) + NTT(k e_j)
// A sampled polynomial (the noise e, the ternary u) is ONE polynomial of small signed integers shared by every limb; the reference
// expands it to [L][N] residues (sample_error_poly / sample_ternary_poly write v mod q_i per limb), multiplies by t under bgv
// (multiply_scalar_rns_poly) and transforms that.  Here the sample stays [N] signed words and the expansion is the LOAD of the forward
// transform's first pass (PRO_SMALL, pha_ntt_core.h); the product with the key and the sum are the STORE of its last pass
// (EPI_FWD_MULADD / EPI_FWD_NEG_MULADD).  Every stored word is the canonical residue, so the words equal the reference's sequence of
// launches whatever the order of the modular operations inside.
//
// PRO_SMALL: a word w is the two's complement of a signed v with |v| <= kSmallSampleMax = 2^16 (the reference's samplers give
//   |v| <= 21).  Every prime used is above 2^17 (the entries refuse a context that has a smaller one among the rows used), so
//   |v| < q and [v] mod q is v or q + v: small_lift.  With a factor k (bgv: k = t) the limb receives kq = k mod q and the word
//   becomes [kq |v|] mod q by Barrett's 128-bit reduction (the product is below 2^16 q < 2^77), negated for v < 0: small_lift_scaled.
//   Either way the result is the canonical residue in [0, q): what the pass's first round expects from a global load on both back
//   ends (the FP64 back end converts canonical words below 2^50 itself, PassProgram::fp_after_global_load).
//
// The epilogues, on x = the transform's value of this coefficient, a and b = canonical words of the two factors, p = the optional
// NTT-form plaintext word (canonical):
//   EPI_FWD_MULADD       out = [a b + x] mod q                       (asymmetric: a = pk_j, b = NTT(u))
//   EPI_FWD_NEG_MULADD   out = [-(a b + x) + p] mod q                (symmetric: a = c1's own word, b = the key's)
// Integer back end: x arrives canonical (the caller reduces the lazy value below 8 q as EPI_FWD_CANON does); a b + x < q^2 + q fits
//   128 bits and is reduced once (barrett128), as multiply_and_add_negate_rns_poly does.
// FP64 back end (q < 2^50): x arrives as the last round's lazy double, an exact integer with |x| < 8 q < 2^53 (the bound EPI_INV_SCALE
//   states for the same hand-over; PassProgram::fp_sched keeps the registers below 7.5 q).  Then, every value an exact integer:
//     t = fp_reduce(x)                                   |t| <= q / 2 + 2   (the quotient estimate x fl(1/q) is within 2^-49 of x / q for
//                                                         |x| < 8 q, so it rounds the other way only that close to a half-integer)
//     m = fp_mulmod_light(fp_from_canon(a), fp_from_canon(b))    0 <= a, b < q < 2^50: |m| <= q (0.5 + 1.5 a 2^-52) < 0.875 q
//     s = m + t                                          |s| < 1.375 q + 2                            (kMulAddSumBound)
//     r = s, or -s + p with 0 <= p < q                    |r| < 2.375 q + 2 < 2^51.3                    (kMulAddOutBound)
//   and fp_to_canon reduces anything below 2^52.6 to [0, q).  The probe hooks below let the CPU replay record the magnitudes.
#pragma once
#include "pha_arith.h"

namespace pha {

constexpr u64 kSmallSampleMax = (u64)1 << 16;        // |v| of a sampled word
constexpr int kSmallMinPrimeBits = 18;               // every prime used is at least 2^17 (bit length >= 18), so |v| < q
// the FP64 epilogue's bounds in units of q / 1000 (+ 2): |m + t| and |r| above
constexpr int kMulAddSumBound = 1375, kMulAddOutBound = 2375;

struct MulAddNoProbe {
    PHA_HD void f64(double) const {}
};

// |v| of the signed word w
PHA_HD u64 small_magnitude(u64 w) { return (w >> 63) ? 0 - w : w; }
// [v] mod q for |v| < q
PHA_HD u64 small_lift(u64 w, u64 q) { return (w >> 63) ? q + w : w; }
// [k v] mod q, kq = k mod q
PHA_HD u64 small_lift_scaled(u64 w, u64 kq, const DModulus &m) {
    const u64 r = mul_mod(small_magnitude(w), kq, m);
    return (w >> 63) ? neg_mod(r, m.value) : r;
}

// x canonical
template <bool NEG>
PHA_HD u64 muladd_int(u64 x, u64 a, u64 b, bool has_p, u64 p, const DModulus &m) {
    u64 lo, hi;
    mul128(a, b, lo, hi);
    lo += x;
    hi += (lo < x);
    const u64 r = barrett128(lo, hi, m);
    if (!NEG) return r;
    const u64 n = neg_mod(r, m.value);
    return has_p ? add_mod(n, p, m.value) : n;
}
// x: the lazy double of the last round, |x| < 8 q
template <bool NEG, class Probe>
PHA_HD u64 muladd_fp(double x, u64 a, u64 b, bool has_p, u64 p, FpMod m, Probe &probe) {
    const double t = fp_reduce(x, m);
    const double s = fp_mulmod_light(fp_from_canon(a), fp_from_canon(b), m) + t;
    probe.f64(s);
    double r = s;
    if (NEG) r = has_p ? fp_from_canon(p) - s : -s;
    probe.f64(r);
    return fp_to_canon(r, m);
}

}  // namespace pha
