// pha_ckks_fft.h -- the arithmetic of the CKKS encoder (src/fft.cu:44-77 butterflies, :114-125 twiddle index; src/rns_base.cu:49-153
// round and reduce): the radix-2 butterflies of the special FFT over complex doubles, the index of a butterfly's root of unity, and
// the rounding of one double coefficient into a residue.  Host/device like pha_arith.h and pha_bfv_lift.h, so that
// tests/emu/emu_ckks_fft.cpp compiles the very source the kernels of pha_ckks.hip run -- test-only on the host.
//
// "Bit-exact" here means: a complex product is (ar*br - ai*bi, ar*bi + ai*br) with every multiply, add and subtract rounded on its
// own.  Any tiling or radix that executes the same radix-2 butterfly graph then gives the same bits, which leaves the kernels free
// to group stages.  The rule is stated below as a pragma (as pha_arith.h does), so it does not depend on the build's flags.
#pragma once
#include "pha_arith.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace pha {

struct cplx {
    double re, im;
};

PHA_HD cplx c_add(cplx a, cplx b) { return cplx{a.re + b.re, a.im + b.im}; }
PHA_HD cplx c_sub(cplx a, cplx b) { return cplx{a.re - b.re, a.im - b.im}; }
PHA_HD cplx c_mul(cplx a, cplx b) {
    const double rr = a.re * b.re, ii = a.im * b.im, ri = a.re * b.im, ir = a.im * b.re;
    return cplx{rr - ii, ri + ir};
}

// inverse special FFT (encode): a, b <- a + b, (a - b) * w
PHA_HD void ckks_gs_bfly(cplx &a, cplx &b, cplx w) {
    const cplx s = c_add(a, b), d = c_sub(a, b);
    a = s;
    b = c_mul(d, w);
}
// forward special FFT (decode): a, b <- a + b * w, a - b * w
PHA_HD void ckks_ct_bfly(cplx &a, cplx &b, cplx w) {
    const cplx t = c_mul(b, w);
    b = c_sub(a, t);
    a = c_add(a, t);
}

PHA_HD u32 ckks_brev32(u32 x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x);
#else
    x = (x >> 16) | (x << 16);
    x = ((x & 0xff00ff00u) >> 8) | ((x & 0x00ff00ffu) << 8);
    x = ((x & 0xf0f0f0f0u) >> 4) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x & 0xccccccccu) >> 2) | ((x & 0x33333333u) << 2);
    return ((x & 0xaaaaaaaau) >> 1) | ((x & 0x55555555u) << 1);
#endif
}
// the low `bits` bits of x reversed
PHA_HD u32 ckks_brev(u32 x, u32 bits) { return bits ? ckks_brev32(x) >> (32 - bits) : 0; }

// Index into the table of M-th roots of the twiddle of butterfly group k of the stage whose pairs are 2^log_pairs apart, in a
// transform of 2^log_n points: (group[reverse of (k << log_pairs) over log_n - 1 bits] << log_pairs) mod M, group[i] = 5^i mod M.
// The forward transform (decode) takes roots[psi], the inverse (encode) roots[M - psi]; psi is an odd multiple of 2^log_pairs
// below M, so M - psi stays inside the table.  The product is formed in 32 bits: what that drops lies above the mask.
PHA_HD u32 ckks_psi(const u32 *group, u32 log_n, u32 log_pairs, u32 k, u32 m) {
    const u32 at = log_n >= 2 ? ckks_brev32(k << log_pairs) >> (33 - log_n) : 0;
    return (group[at] << log_pairs) & (m - 1);
}

// ---- one pass of the special FFT over a tile held in LDS (pha_ckks.hip: fft_pass_kernel; on the host the harness plays the
//      workgroup's threads one after the other, phase by phase) ---------------------------------------------------------------
enum { FFT_IN_INTERLEAVED = 0, FFT_IN_GATHER = 1, FFT_IN_SPLIT = 2 };
enum { FFT_OUT_INTERLEAVED = 0, FFT_OUT_SPLIT = 1, FFT_OUT_SCATTER = 2 };

struct FftPass {
    const double *in;
    double *out;
    size_t in_stride, out_stride;   // doubles between consecutive messages
    const cplx *roots;
    const u32 *group;
    u32 m, log_n;
    u32 log_tile, log_cols;         // log_cols == log_tile: a contiguous tile; below: rows of 2^log_cols adjacent columns, 2^lp0 apart
    u32 lp0, stages;                // the pass runs the stages whose pairs are 2^lp0 .. 2^(lp0 + stages - 1) apart
    int in_mode, out_mode;
    u32 values_size;                // FFT_IN_GATHER: points at or past it are zero
    double fix;                     // != 0: multiplies every stored component (the last pass of the inverse transform)
    u64 *maxbits;                   // per message, or null: max over the stored components of the bit pattern of |component|
};

// The plan: up to 2^13 points (128 KiB of complex doubles, inside the CU's 160 KiB of LDS) are ONE pass with the whole array in one
// tile.  A larger transform is a contiguous pass (tiles of 2^12 consecutive points: the stages whose pairs are 1 .. 2^11 apart) and
// a strided pass (tiles of n / 2^12 rows of 2^24 / n adjacent columns: the stages whose pairs are 2^12 and more apart); the inverse
// transform runs the contiguous pass first, the forward one the strided pass first.
constexpr u32 kFftSingleLog = 13, kFftTileLog = 12, kFftMaxLog = 2 * kFftTileLog;
PHA_HD u32 fft_pass_count(u32 log_n) { return log_n <= kFftSingleLog ? 1 : 2; }
PHA_HD void fft_pass_shape(FftPass &p, u32 log_n, bool inverse, u32 which) {
    p.log_n = log_n;
    if (log_n <= kFftSingleLog) {
        p.log_tile = p.log_cols = log_n; p.lp0 = 0; p.stages = log_n;
    } else if ((which == 0) == inverse) {
        p.log_tile = p.log_cols = kFftTileLog; p.lp0 = 0; p.stages = kFftTileLog;
    } else {
        p.log_tile = kFftTileLog; p.lp0 = kFftTileLog; p.stages = log_n - kFftTileLog; p.log_cols = kFftTileLog - p.stages;
    }
}

// point of the transform behind LDS slot i of tile `tile`
PHA_HD u32 fft_point(const FftPass &p, u32 tile, u32 i) {
    if (p.log_cols == p.log_tile) return (tile << p.log_tile) + i;
    return ((i >> p.log_cols) << p.lp0) + (tile << p.log_cols) + (i & ((1u << p.log_cols) - 1));
}

// first phase: the tile into LDS.  FFT_IN_GATHER is the bit reversal of encode: value i sits at point brev(i), the rest is zero
PHA_HD void fft_load(const FftPass &p, cplx *lds, u32 tile, u32 msg, u32 tid, u32 nthreads) {
    const u32 T = 1u << p.log_tile, n = 1u << p.log_n;
    const double *in = p.in + (size_t)msg * p.in_stride;
    for (u32 i = tid; i < T; i += nthreads) {
        const u32 g = fft_point(p, tile, i);
        cplx v{0.0, 0.0};
        if (p.in_mode == FFT_IN_GATHER) {
            const u32 j = ckks_brev(g, p.log_n);
            if (j < p.values_size) v = cplx{in[2 * (size_t)j], in[2 * (size_t)j + 1]};
        } else if (p.in_mode == FFT_IN_SPLIT) {
            v = cplx{in[g], in[(size_t)g + n]};
        } else {
            v = cplx{in[2 * (size_t)g], in[2 * (size_t)g + 1]};
        }
        lds[i] = v;
    }
}

// R consecutive stages of the pass, from its stage s0 up, on every group of 2^R LDS slots they connect: the group sits in
// registers, so R stages cost one LDS round trip.  The butterfly graph is the radix-2 one, stage by stage.
template <int R, bool INV>
PHA_HD void fft_group(const FftPass &p, cplx *lds, u32 tile, u32 s0, u32 tid, u32 nthreads) {
    const u32 q = s0 + (p.log_cols == p.log_tile ? 0 : p.log_cols);   // LDS distance (log) of stage s0's pairs
    const u32 units = 1u << (p.log_tile - R);
    for (u32 u = tid; u < units; u += nthreads) {
        const u32 base = ((u >> q) << (q + R)) | (u & ((1u << q) - 1));
        cplx x[1 << R];
#pragma unroll
        for (int e = 0; e < (1 << R); e++) x[e] = lds[base + ((u32)e << q)];
#pragma unroll
        for (int t = 0; t < R; t++) {
            const int s = INV ? t : R - 1 - t;   // inverse: pairs grow from stage to stage; forward: they shrink
            const u32 lp = p.lp0 + s0 + s;
#pragma unroll
            for (int e = 0; e < (1 << R); e++) {
                if (e & (1 << s)) continue;
                const u32 k = fft_point(p, tile, base + ((u32)e << q)) >> (lp + 1);
                const u32 psi = ckks_psi(p.group, p.log_n, lp, k, p.m);
                const cplx w = p.roots[INV ? p.m - psi : psi];
                if (INV) ckks_gs_bfly(x[e], x[e | (1 << s)], w);
                else ckks_ct_bfly(x[e], x[e | (1 << s)], w);
            }
        }
#pragma unroll
        for (int e = 0; e < (1 << R); e++) lds[base + ((u32)e << q)] = x[e];
    }
}

// one barrier-separated phase of the stages: the next (up to) three of them after `done`; returns how many it ran
template <bool INV>
PHA_HD u32 fft_stage_phase(const FftPass &p, cplx *lds, u32 tile, u32 done, u32 tid, u32 nthreads) {
    const u32 r = p.stages - done < 3 ? p.stages - done : 3;
    const u32 s0 = INV ? done : p.stages - done - r;
    if (r == 3) fft_group<3, INV>(p, lds, tile, s0, tid, nthreads);
    else if (r == 2) fft_group<2, INV>(p, lds, tile, s0, tid, nthreads);
    else fft_group<1, INV>(p, lds, tile, s0, tid, nthreads);
    return r;
}

// last phase: the tile out of LDS, scaled where the pass ends an inverse transform; FFT_OUT_SPLIT writes [re[0..n) | im[0..n)],
// FFT_OUT_SCATTER is the bit reversal of decode.  Returns this thread's max of the bit patterns of |component| (0 without maxbits).
PHA_HD u64 fft_store(const FftPass &p, const cplx *lds, u32 tile, u32 msg, u32 tid, u32 nthreads) {
    const u32 T = 1u << p.log_tile, n = 1u << p.log_n;
    double *out = p.out + (size_t)msg * p.out_stride;
    u64 mx = 0;
    for (u32 i = tid; i < T; i += nthreads) {
        const u32 g = fft_point(p, tile, i);
        cplx v = lds[i];
        if (p.fix != 0.0) v = cplx{v.re * p.fix, v.im * p.fix};
        if (p.maxbits) {
            const u64 a = as_u64(__builtin_fabs(v.re)), b = as_u64(__builtin_fabs(v.im));
            mx = mx > a ? mx : a;
            mx = mx > b ? mx : b;
        }
        if (p.out_mode == FFT_OUT_SPLIT) {
            out[g] = v.re;
            out[(size_t)g + n] = v.im;
        } else {
            const size_t j = p.out_mode == FFT_OUT_SCATTER ? ckks_brev(g, p.log_n) : g;
            out[2 * j] = v.re;
            out[2 * j + 1] = v.im;
        }
    }
    return mx;
}

// C round(): to the nearest integer, halves away from zero, without the double rounding of floor(x + 0.5): the fraction
// |x| - trunc(|x|) is exact below 2^52, and every double from 2^52 up is integral.
PHA_HD double ckks_round(double x) {
    const double a = __builtin_fabs(x);
    if (!(a < 4503599627370496.0)) return x;   // 2^52 and above (and NaN): already integral
    const double t = __builtin_trunc(a);
    const double r = (a - t >= 0.5) ? t + 1.0 : t;   // a - t is exact
    return __builtin_copysign(r, x);
}

// One coefficient whose rounded magnitude is below 2^64 (max_coeff_bit_count <= 64) modulo q: round, reduce the magnitude, negate.
// Only canonical words leave: a coefficient that rounds to -0.0 gives 0 (the reference writes q there), and so does a negative
// multiple of q.
PHA_HD u64 ckks_round_reduce64(double x, u64 q, u64 ratio1) {
    const double r = ckks_round(x);
    const u64 t = barrett64((u64)__builtin_fabs(r), q, ratio1);
    return (r < 0.0 && t) ? q - t : t;
}

// The same for a coefficient of any finite size: a double is mantissa * 2^shift exactly, so the residue is the mantissa's times
// 2^shift's, taken 32 bits of the shift at a time (what the reference's 128-bit and multi-word decompose kernels compute through
// fmod and division by 2^64).  Infinities and NaN never get here (the encoder refuses them); they give 0.
PHA_HD u64 ckks_round_reduce_wide(double x, const DModulus &m) {
    const double r = ckks_round(x);
    const u64 bits = as_u64(__builtin_fabs(r));
    const int e = (int)(bits >> 52);
    if (e == 0 || e == 0x7ff) return 0;   // |r| < 1 rounds to 0: r is integral, so a zero exponent field means r == 0
    const u64 man = (bits & 0xfffffffffffffull) | (1ull << 52);
    int shift = e - 1075;
    u64 t;
    if (shift <= 0) {
        t = barrett64(man >> -shift, m.value, m.ratio1);   // r is integral: the bits shifted out are zero
    } else {
        t = barrett64(man, m.value, m.ratio1);
        while (shift > 0) {
            const int s = shift < 32 ? shift : 32;
            t = barrett128(t << s, t >> (64 - s), m);
            shift -= s;
        }
    }
    return (r < 0.0 && t) ? m.value - t : t;
}

// max_coeff_bit_count of the encoder from the bit pattern of max |coefficient| (non-negative doubles order like their bit
// patterns, which is what the kernels reduce): ceil(log2(max(v, 1))) + 1, exact.  Infinity and NaN give a count above any modulus.
PHA_HD int ckks_bit_count(u64 max_bits) {
    const int e = (int)(max_bits >> 52);
    if (e >= 0x7ff) return 1 << 20;
    if (e < 1023) return 1;                                   // below 1
    const int lg = e - 1023;
    return ((max_bits & 0xfffffffffffffull) ? lg + 1 : lg) + 1;
}

}  // namespace pha
