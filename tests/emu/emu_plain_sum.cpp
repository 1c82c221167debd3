// emu_plain_sum.cpp -- TEST-ONLY: the per-thread program of plain_sum_kernel (phantom-fhe_amd/csrc/pha_plain_sum.h, host/device
// functions) compiled for the host and run on one thread's worth of data: two adjacent coefficients of both polynomials, `terms`
// terms.  tests/test_emu_plain_sum.py compares the results with Python integers and checks the magnitude every accumulator
// reaches just before it is reduced.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "../../phantom-fhe_amd/csrc/pha_plain_sum.h"

using namespace pha;

namespace {

// term k: plain[2 k .. 2 k + 1], ct0[2 k ..], ct1[2 k ..] (the two coefficients of the plaintext and of the two polynomials)
struct HostSrc {
    const u64 *plain, *ct0, *ct1;
    void next(u64x2 &w, u64x2 &c0, u64x2 &c1) {
        w = u64x2{plain[0], plain[1]};
        c0 = u64x2{ct0[0], ct0[1]};
        c1 = u64x2{ct1[0], ct1[1]};
        plain += 2; ct0 += 2; ct1 += 2;
    }
};

// the largest value seen before a reduction: 128-bit integers as (hi, lo), doubles by magnitude
struct MaxProbe {
    u64 lo = 0, hi = 0;
    double mag = 0.0;
    uint64_t flushes = 0;
    void i128(u64 l, u64 h) {
        if (h > hi || (h == hi && l > lo)) { hi = h; lo = l; }
        flushes++;
    }
    void f64(double x) {
        if (std::fabs(x) > mag) mag = std::fabs(x);
        flushes++;
    }
};

DModulus make_modulus(u64 q) {   // floor(2^128 / q) as two words
    const unsigned __int128 top = ~(unsigned __int128)0;   // 2^128 - 1; q is odd and > 1, so floor((2^128 - 1) / q) == floor(2^128 / q)
    const unsigned __int128 r = top / q;
    return DModulus{q, (u64)r, (u64)(r >> 64)};
}

}  // namespace

extern "C" {

// terms per flush of the two back ends for modulus q
uint32_t emu_plain_sum_per(uint64_t q, int fp) { return fp ? plain_sum_per_fp(modulus_bits(q)) : plain_sum_per_int(modulus_bits(q)); }

// out[0..1] = c0 sums, out[2..3] = c1 sums of the two coefficients; acc (4 words: c0.x, c0.y, c1.x, c1.y) may be null.
// peak[0..1] = (lo, hi) of the largest 128-bit accumulator before a reduction (integer back end), peak[2] = the largest |double|
// (FP64 back end, an exact integer below 2^53 when the bound holds; stored rounded up), peak[3] = accumulators probed.
void emu_plain_sum(uint64_t q, int fp, uint32_t terms, const uint64_t *plain, const uint64_t *ct0, const uint64_t *ct1, const uint64_t *acc,
                   uint64_t *out, uint64_t *peak) {
    HostSrc src{plain, ct0, ct1};
    u64x2 a0{0, 0}, a1{0, 0}, r0, r1;
    if (acc) { a0 = u64x2{acc[0], acc[1]}; a1 = u64x2{acc[2], acc[3]}; }
    MaxProbe probe;
    if (fp) plain_sum_fp(src, terms, make_fpmod(q), modulus_bits(q), a0, a1, r0, r1, probe);
    else {
        const DModulus m = make_modulus(q);
        plain_sum_int(src, terms, m, a0, a1, r0, r1, probe);
    }
    out[0] = r0.x; out[1] = r0.y; out[2] = r1.x; out[3] = r1.y;
    peak[0] = probe.lo; peak[1] = probe.hi;
    peak[2] = (uint64_t)std::ceil(probe.mag);
    peak[3] = probe.flushes;
}

}
