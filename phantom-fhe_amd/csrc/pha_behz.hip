// pha_behz.hip -- BFV multiply, BEHZ variant, on gfx950.
//
// Reference: bfv_multiply_behz src/evaluate.cu:404-548; DRNSTool::fastbconv_m_tilde / sm_mrq / fast_floor /
// fastbconv_sk src/rns.cu:1249-1510; multiply_and_negated_add_rns_poly src/polymath.cu:606-634; constants
// src/rns.cu:392-560 (built in pha_context.hip, Context::behz).  The base conversions reuse the one-thread-per-
// coefficient converter of pha_rns.hip (its 128-bit accumulate form: the auxiliary primes are 61 bits wide), the
// transforms reuse the NTT kernels over the auxiliary table rows, and what remains are three element-wise kernels.
#include "../../include/phantom_amd.h"
#include "pha_internal.h"
#include "pha_ntt_core.h"

namespace pha {

// sm_mrq_kernel rns.cu:1290-1320: (x + q * r) * m_tilde^-1 mod Bsk with r = -x_mtilde * q^-1 mod m_tilde, centred
struct MrqArgs {
    u64 *dst;                // [polys][Bsk][N]
    const u64 *src;          // [polys][Bsk + 1][N], last limb modulo m_tilde
    const DModulus *mod;     // table base; Bsk limb j is row aux0 + j
    const u64 *prod_q_mod_bsk;
    const u64x2 *inv_mt_mod_bsk;
    u64x2 neg_inv_prod_q_mod_mt;
    uint32_t aux0, size_bsk, n;
    size_t dst_stride = 0;   // words between the polynomials of dst (0 = packed, size_bsk * n)
};
__global__ __launch_bounds__(256) void sm_mrq_kernel(const MrqArgs k) {
    const uint32_t j = blockIdx.y, coeff = blockIdx.x * 256 + threadIdx.x;
    const DModulus m = k.mod[k.aux0 + j];
    const u64 mt = (u64)1 << 32;
    const u64 *in = k.src + (size_t)blockIdx.z * (k.size_bsk + 1) * k.n;
    u64 r = shoup(in[(size_t)k.size_bsk * k.n + coeff], k.neg_inv_prod_q_mod_mt, mt);
    if (r >= (mt >> 1)) r += m.value - mt;
    u64 lo, hi;
    mul128(r, k.prod_q_mod_bsk[j], lo, hi);
    const u64 x = in[(size_t)j * k.n + coeff];
    lo += x;
    hi += lo < x;
    const size_t dz = k.dst_stride ? k.dst_stride : (size_t)k.size_bsk * k.n;
    k.dst[(size_t)blockIdx.z * dz + (size_t)j * k.n + coeff] = shoup(barrett128(lo, hi, m), k.inv_mt_mod_bsk[j], m.value);
}

// second half of bconv_fuse_sub_mul_unroll2_kernel rns.cu:1343-1386: (x_Bsk + (p - conv)) * prod(q)^-1 mod p
struct FloorArgs {
    u64 *dst;
    const u64 *x_bsk, *conv;
    const DModulus *mod;
    const u64x2 *scale;
    uint32_t aux0, n;
    size_t dst_stride = 0, x_stride = 0, conv_stride = 0;   // polynomial blockIdx.z
};
__global__ __launch_bounds__(256) void fast_floor_kernel(const FloorArgs k) {
    const uint32_t j = blockIdx.y, coeff = blockIdx.x * 256 + threadIdx.x;
    const u64 p = k.mod[k.aux0 + j].value;
    const size_t id = (size_t)j * k.n + coeff, z = blockIdx.z;
    // the sum is not reduced first (:1376-1378)
    k.dst[z * k.dst_stride + id] = shoup(k.x_bsk[z * k.x_stride + id] + (p - k.conv[z * k.conv_stride + id]), k.scale[j], p);
}

// alpha_sk (bconv_fuse_sub_mul_single_unroll2_kernel rns.cu:1421-1464) and the Shenoy-Kumaresan correction
// (multiply_and_negated_add_rns_poly polymath.cu:606-634) in one kernel over the q limbs
struct SkArgs {
    u64 *out_q;              // [Q][N]: FastBconv(x, B -> q) on entry, the result on exit
    const u64 *conv_msk;     // [N]   FastBconv(x, B -> {m_sk})
    const u64 *x_msk;        // [N]   the m_sk limb of the Bsk polynomial
    const DModulus *mod;
    const u64 *prod_b_mod_q;
    u64x2 inv_prod_b_mod_msk;
    u64 m_sk;
    uint32_t n;
    size_t out_stride = 0, conv_stride = 0, x_stride = 0;   // polynomial blockIdx.z
};
__global__ __launch_bounds__(256) void sk_fix_kernel(SkArgs k) {
    const uint32_t i = blockIdx.y, coeff = blockIdx.x * 256 + threadIdx.x;
    k.out_q += blockIdx.z * k.out_stride;
    k.conv_msk += blockIdx.z * k.conv_stride;
    k.x_msk += blockIdx.z * k.x_stride;
    const DModulus m = k.mod[i];
    u64 a = shoup(k.conv_msk[coeff] + (k.m_sk - k.x_msk[coeff]), k.inv_prod_b_mod_msk, k.m_sk);
    u64 pb = k.prod_b_mod_q[i];
    if (a > (k.m_sk >> 1)) a = k.m_sk - a;   // alpha_sk in [-m_sk/2, 0): -alpha * B is positive
    else pb = m.value - pb;                  // alpha_sk in [0, m_sk/2):  -alpha * B = alpha * (-B mod q)
    const size_t id = (size_t)i * k.n + coeff;
    k.out_q[id] = add_mod(k.out_q[id], mul_mod(a, pb, m), m.value);
}


// `polys` polynomials through one converter, phase 1 on load: dst + z * dst_stride <- src + z * src_stride
static void convert(Context &c, const BConv &conv, u64 *dst, size_t dst_stride, const u64 *src, size_t src_stride, uint32_t polys, hipStream_t s,
                    const BConvEpilogue *epi = nullptr) {
    BConvCall k = bconv_call(conv);
    k.polys = polys; k.dst = dst; k.dst_stride = dst_stride; k.src = src; k.src_stride = src_stride; k.epi = epi;
    launch_bconv(c, k, s);
}

// ---- the DRNSTool stages of the BEHZ multiply on `polys` polynomials per launch (blockIdx.z; strides in words).  The multiply
//      runs them on the 2 B or 3 B polynomials of a chunk, the pha_* step entries at the end of this file on one. ----
// fastbconv_m_tilde rns.cu:1249-1278: src [.][Q][N] -> dst [polys][Bsk + 1][N] packed.  Phase 1 with m_tilde * qhat^-1 (the
// converter's own scale-in factors, Context::behz), one conversion for all Bsk + 1 outputs
static void launch_fastbconv_m_tilde(Context &c, Behz &b, u64 *dst, const u64 *src, size_t src_stride, uint32_t polys, hipStream_t s) {
    convert(c, b.q_to_bskmt, dst, (size_t)(b.size_bsk + 1) * c.n, src, src_stride, polys, s);
}
// sm_mrq rns.cu:1326-1338: src [polys][Bsk + 1][N] packed -> dst [.][Bsk][N]
static void launch_sm_mrq(Context &c, Behz &b, u64 *dst, size_t dst_stride, const u64 *src, uint32_t polys, hipStream_t s) {
    const uint32_t n = (uint32_t)c.n;
    MrqArgs ma{dst, src, c.d_mod.p, b.prod_q_mod_bsk.p, b.inv_mt_mod_bsk.p, b.neg_inv_prod_q_mod_mt, b.aux0, b.size_bsk, n, dst_stride};
    hipLaunchKernelGGL(sm_mrq_kernel, dim3(n / 256, b.size_bsk, polys), dim3(256), 0, s, ma);
    check_launch();
}
// fast_floor rns.cu:1394-1419: (x_q [.][Q][N], x_bsk [.][Bsk][N]) -> dst [polys][Bsk][N] packed; conv [polys][Bsk][N] scratch
static void launch_fast_floor(Context &c, Behz &b, u64 *dst, const u64 *x_q, size_t q_stride, const u64 *x_bsk, size_t bsk_stride,
                              u64 *conv, uint32_t polys, hipStream_t s) {
    const uint32_t n = (uint32_t)c.n;
    const size_t bn = (size_t)b.size_bsk * n;
    convert(c, b.q_to_bsk, conv, bn, x_q, q_stride, polys, s);
    FloorArgs fa{dst, x_bsk, conv, c.d_mod.p, b.inv_prod_q_mod_bsk.p, b.aux0, n, bn, bsk_stride, bn};
    hipLaunchKernelGGL(fast_floor_kernel, dim3(n / 256, b.size_bsk, polys), dim3(256), 0, s, fa);
    check_launch();
}
// fastbconv_sk rns.cu:1470-1510: x [polys][Bsk][N] packed (B limbs, then the m_sk limb) -> out_q [polys][Q][N] packed; msk [polys][N] scratch
static void launch_fastbconv_sk(Context &c, Behz &b, u64 *out_q, const u64 *x, u64 *msk, uint32_t polys, hipStream_t s) {
    const uint32_t n = (uint32_t)c.n;
    const size_t qn = (size_t)b.size_q * n, bn = (size_t)b.size_bsk * n;
    convert(c, b.b_to_msk, msk, n, x, bn, polys, s);   // B -> m_sk
    convert(c, b.b_to_q, out_q, qn, x, bn, polys, s);
    SkArgs ka{out_q, msk, x + (size_t)b.size_b * n, c.d_mod.p, b.prod_b_mod_q.p, b.inv_prod_b_mod_msk, b.m_sk, n, qn, n, bn};
    hipLaunchKernelGGL(sk_fix_kernel, dim3(n / 256, b.size_q, polys), dim3(256), 0, s, ka);
    check_launch();
}

// ---- HPS variant (mul_tech_type::hps): bConv_HPS src/rns_bconv.cu:248-372, scaleAndRound_HPS_QR_R src/rns.cu:1700-1746.
// Floating point: the reference is built by nvcc with its default -fmad=true, so every `acc += double(x) * c` of
// its kernels is ONE fused multiply-add; the same fma chains are issued here (this file is compiled with
// -ffp-contract=off, the fusions are explicit).
struct HpsFixArgs {
    u64 *out;                // [osz][N]: FastBconv(y) on entry, minus v * prod(ibase) mod p_j on exit
    const u64 *y;            // [isz][N]  x_i * hat_i^-1 mod q_i
    const double *inv;       // [isz]     1 / q_i
    const u64 *alpha_mod;    // [isz + 1][osz]
    const DModulus *mod;
    const uint32_t *oprime;  // table rows of the output primes
    uint32_t isz, osz, n;
};
__global__ __launch_bounds__(256) void hps_fix_kernel(const HpsFixArgs k) {
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    double frac = 0.0;
    for (uint32_t i = 0; i < k.isz; i++) frac = __builtin_fma((double)k.y[(size_t)i * k.n + coeff], k.inv[i], frac);
    const size_t v = (size_t)llround(frac);
    for (uint32_t j = 0; j < k.osz; j++) {
        const u64 p = k.mod[k.oprime[j]].value;
        const size_t id = (size_t)j * k.n + coeff;
        k.out[id] = sub_mod(k.out[id], k.alpha_mod[v * k.osz + j], p);
    }
}

// sum_i x_i * tab[i] (i < count <= PAD) as a 128-bit number, carry-free: x_i arrives cut at bit SX (x0, x1), the uniform table
// entries are cut at bit SM on the way, partial products stay below 2^61 (halves of at most 31 and 30 bits) and the four partial
// sums are folded into the total every 8 terms -- four v_mad_u64_u32 per term instead of the nine of a 128-bit multiply-add.
template <int PAD, int SX, int SM>
__device__ __forceinline__ void split_dot(const u32 (&x0)[PAD], const u32 (&x1)[PAD], const u64 *tab, uint32_t count, u64 &lo, u64 &hi) {
    static_assert(SX + SM == 61, "halves of 30 and 31 bits");
#pragma unroll
    for (int base = 0; base < PAD; base += 8) {
        u64 ll = 0, lh = 0, hl = 0, hh = 0;
#pragma unroll
        for (int i = base; i < base + 8 && i < PAD; i++) {
            const u64 m = i < (int)count ? tab[i] : 0;
            const u32 m0 = (u32)m & ((1u << SM) - 1), m1 = (u32)(m >> SM);
            ll = (u64)x0[i] * m0 + ll;
            lh = (u64)x0[i] * m1 + lh;
            hl = (u64)x1[i] * m0 + hl;
            hh = (u64)x1[i] * m1 + hh;
        }
        lo += ll;
        hi += lo < ll;
        u64 t = lh << SM;
        lo += t;
        hi += (lo < t) + (lh >> (64 - SM));
        t = hl << SX;
        lo += t;
        hi += (lo < t) + (hl >> (64 - SX));
        t = hh << (SX + SM);
        lo += t;
        hi += (lo < t) + (hh >> (64 - SX - SM));
    }
}

struct ScaleRoundArgs {
    u64 *dst;                // [R][N]
    const u64 *src;          // [Q + R][N] coefficient form
    const double *frac;      // [Q]
    const u64 *tab;          // [R][Q + 1]
    const DModulus *mod;
    uint32_t size_q, size_r, aux0, n;
    size_t dst_stride = 0, src_stride = 0;   // polynomial blockIdx.y
};
// The carry alpha = floor(nu) < |Q| max q of one coefficient, modulo r_j.  The reference reduces it in place across the R limbs
// (rns.cu:1733): limb j receives ((alpha mod r_0) mod r_1 ...) mod r_j.  The first reduction is harmless (every limb then holds
// alpha - k r_0, a change of the result by less than |Q| r_0), but a later one that subtracts anything -- (alpha mod r_0) >= r_j, R
// descends from the smallest q -- reaches the limbs after j only: their residues then belong to no common integer and the
// coefficient is noise (once in r_0 / (r_0 - r_|Q|) coefficients: never at 60 bits, every few products at 36, every product at 30).
// Here every limb reduces alpha mod r_0 itself: the reference's words wherever those are consistent, the right ones elsewhere.
__device__ __forceinline__ u64 hps_carry(u64 &alpha, uint32_t j, const DModulus &m) {
    const u64 a = barrett64(alpha, m.value, m.ratio1);
    if (j == 0) alpha = a;
    return a;
}
// QPAD >= size_q: the Q residues of the coefficient stay in registers across the R limbs.  SPLIT: Q primes <= 60 bits and R
// primes <= 62: the carry-free dot product (residues cut at 30 bits, table entries at 31)
template <int QPAD, bool SPLIT>
__global__ __launch_bounds__(256) void hps_scale_round_kernel(ScaleRoundArgs k) {
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    k.src += blockIdx.y * k.src_stride;
    k.dst += blockIdx.y * k.dst_stride;
    u64 x[SPLIT ? 1 : QPAD];
    u32 x0[SPLIT ? QPAD : 1], x1[SPLIT ? QPAD : 1];
    double nu = 0.5;
#pragma unroll
    for (int i = 0; i < QPAD; i++) {
        u64 v = 0;
        if (i < (int)k.size_q) {
            v = k.src[(size_t)i * k.n + coeff];
            nu = __builtin_fma((double)v, k.frac[i], nu);
        }
        if (SPLIT) {
            x0[i] = (u32)v & 0x3fffffffu;
            x1[i] = (u32)(v >> 30);
        } else {
            x[i] = v;
        }
    }
    u64 alpha = (u64)nu;
    for (uint32_t j = 0; j < k.size_r; j++) {
        const DModulus m = k.mod[k.aux0 + j];
        const u64 *tab = k.tab + (size_t)j * (k.size_q + 1);
        u64 lo = 0, hi = 0;
        if constexpr (SPLIT) {
            split_dot<QPAD, 30, 31>(x0, x1, tab, k.size_q, lo, hi);
        } else {
#pragma unroll
            for (int i = 0; i < QPAD; i++)
                if (i < (int)k.size_q) mac128(x[i], tab[i], lo, hi);
        }
        mac128(k.src[(size_t)(k.size_q + j) * k.n + coeff], tab[k.size_q], lo, hi);
        const u64 v = barrett128(lo, hi, m);
        k.dst[(size_t)j * k.n + coeff] = add_mod(v, hps_carry(alpha, j, m), m.value);
    }
}
__global__ __launch_bounds__(256) void hps_scale_round_wide_kernel(ScaleRoundArgs k) {  // size_q > 32
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    k.src += blockIdx.y * k.src_stride;
    k.dst += blockIdx.y * k.dst_stride;
    double nu = 0.5;
    for (uint32_t i = 0; i < k.size_q; i++) nu = __builtin_fma((double)k.src[(size_t)i * k.n + coeff], k.frac[i], nu);
    u64 alpha = (u64)nu;
    for (uint32_t j = 0; j < k.size_r; j++) {
        const DModulus m = k.mod[k.aux0 + j];
        const u64 *tab = k.tab + (size_t)j * (k.size_q + 1);
        u64 lo = 0, hi = 0;
        for (uint32_t i = 0; i < k.size_q; i++) mac128(k.src[(size_t)i * k.n + coeff], tab[i], lo, hi);
        mac128(k.src[(size_t)(k.size_q + j) * k.n + coeff], tab[k.size_q], lo, hi);
        const u64 v = barrett128(lo, hi, m);
        k.dst[(size_t)j * k.n + coeff] = add_mod(v, hps_carry(alpha, j, m), m.value);
    }
}

// scaleAndRound_HPS_QlRl_Ql (src/rns.cu:1748-1796): [Q || Rl] coefficient form -> base Q, scaled by t / Rl and rounded;
// the carry alpha is reduced in place across the Q limbs exactly as :1783 does.
struct ScaleRoundQArgs {
    u64 *dst;                // [Q][N]
    const u64 *src;          // [Q + Rl][N]
    const double *frac;      // [Rl]
    const u64 *tab;          // [Q][Rl + 1]
    const DModulus *mod;
    uint32_t size_q, size_r, n;
    size_t dst_stride = 0, src_stride = 0;   // polynomial blockIdx.y
};
// RPAD >= size_r: the Rl residues of the coefficient stay in registers across the Q limbs (0 = re-read).  SPLIT (RPAD > 0): R
// primes <= 62 bits and Q primes <= 60: the carry-free dot product (residues cut at 31 bits, table entries at 30)
template <int RPAD, bool SPLIT>
__global__ __launch_bounds__(256) void hps_scale_round_q_kernel(ScaleRoundQArgs k) {
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    k.src += blockIdx.y * k.src_stride;
    k.dst += blockIdx.y * k.dst_stride;
    const u64 *src_r = k.src + (size_t)k.size_q * k.n + coeff;
    u64 x[RPAD && !SPLIT ? RPAD : 1];
    u32 x0[SPLIT ? RPAD : 1], x1[SPLIT ? RPAD : 1];
    double nu = 0.5;
    if (RPAD) {
#pragma unroll
        for (int j = 0; j < RPAD; j++) {
            u64 v = 0;
            if (j < (int)k.size_r) {
                v = src_r[(size_t)j * k.n];
                nu = __builtin_fma((double)v, k.frac[j], nu);
            }
            if (SPLIT) {
                x0[j] = (u32)v & 0x7fffffffu;
                x1[j] = (u32)(v >> 31);
            } else {
                x[j] = v;
            }
        }
    } else {
        for (uint32_t j = 0; j < k.size_r; j++) nu = __builtin_fma((double)src_r[(size_t)j * k.n], k.frac[j], nu);
    }
    u64 alpha = (u64)nu;
    for (uint32_t i = 0; i < k.size_q; i++) {
        const DModulus m = k.mod[i];
        const u64 *tab = k.tab + (size_t)i * (k.size_r + 1);
        u64 lo = 0, hi = 0;
        if constexpr (SPLIT) {
            split_dot<RPAD, 31, 30>(x0, x1, tab, k.size_r, lo, hi);
        } else if (RPAD) {
#pragma unroll
            for (int j = 0; j < RPAD; j++)
                if (j < (int)k.size_r) mac128(x[j], tab[j], lo, hi);
        } else {
            for (uint32_t j = 0; j < k.size_r; j++) mac128(src_r[(size_t)j * k.n], tab[j], lo, hi);
        }
        mac128(k.src[(size_t)i * k.n + coeff], tab[k.size_r], lo, hi);
        const u64 v = barrett128(lo, hi, m);
        alpha = barrett64(alpha, m.value, m.ratio1);
        k.dst[(size_t)i * k.n + coeff] = add_mod(v, alpha, m.value);
    }
}

static void launch_scale_round(Context &c, const ScaleRoundArgs &ka, hipStream_t s, uint32_t batch = 1) {
    // the carry-free dot product needs the residues (Q primes) below 2^60 and the table entries (R primes) below 2^62
    bool split = true;
    for (uint32_t i = 0; i < ka.size_q; i++) split = split && !(c.primes[i] >> 60);
    for (uint32_t j = 0; j < ka.size_r; j++) split = split && !(c.primes[ka.aux0 + j] >> 62);
    const dim3 grid(ka.n / 256, batch), block(256);
#define PHA_SR(P)                                                                                    \
    do {                                                                                             \
        if (split) hipLaunchKernelGGL((hps_scale_round_kernel<P, true>), grid, block, 0, s, ka);      \
        else hipLaunchKernelGGL((hps_scale_round_kernel<P, false>), grid, block, 0, s, ka);           \
    } while (0)
    if (ka.size_q <= 8) PHA_SR(8);
    else if (ka.size_q <= 16) PHA_SR(16);
    else if (ka.size_q <= 32) PHA_SR(32);
    else hipLaunchKernelGGL(hps_scale_round_wide_kernel, grid, block, 0, s, ka);
#undef PHA_SR
    check_launch();
}

void launch_bconv_phase1(Context &c, const BConv &conv, u64 *dst, const u64 *src, hipStream_t s);

// DBaseConverter::bConv_HPS on `batch` polynomials (strides in words): dst [osz][N] <- src [isz][N].  Up to 32 inputs the
// correction term rides in the conversion kernel (one launch for all the polynomials); wider bases: conversion, phase 1 and
// fix-up per polynomial, y [isz][N] scratch.
static void bconv_hps(Context &c, const BConv &conv, const double *inv, const u64 *alpha_mod,
                      u64 *dst, const u64 *src, u64 *y, hipStream_t s, uint32_t batch = 1, size_t dst_stride = 0,
                      size_t src_stride = 0) {
    const uint32_t n = (uint32_t)c.n;
    if (conv.isz <= 32) {
        BConvEpilogue e{};
        e.hps_inv = inv;
        e.hps_alpha = alpha_mod;
        convert(c, conv, dst, dst_stride, src, src_stride, batch, s, &e);
        return;
    }
    for (uint32_t b = 1; b < batch; b++) bconv_hps(c, conv, inv, alpha_mod, dst + b * dst_stride, src + b * src_stride, y, s);
    convert(c, conv, dst, 0, src, 0, 1, s);
    launch_bconv_phase1(c, conv, y, src, s);   // the fix-up needs the phase-1 values themselves
    HpsFixArgs fa{dst, y, inv, alpha_mod, c.d_mod.p, conv.d_oprime.p, conv.isz, conv.osz, n};
    hipLaunchKernelGGL(hps_fix_kernel, dim3(n / 256), dim3(256), 0, s, fa);
    check_launch();
}

// y_i = x_i * hat_i^-1 mod q_i for the input limbs of a converter (bconv_mult_kernel rns_bconv.cu:22-33)
struct Phase1Args {
    u64 *dst;
    const u64 *src;
    const DModulus *mod;
    const uint32_t *iprime;
    const u64x2 *hat_inv;
    uint32_t n;
};
__global__ __launch_bounds__(256) void bconv_phase1_kernel(const Phase1Args k) {
    const uint32_t i = blockIdx.y, coeff = blockIdx.x * 256 + threadIdx.x;
    const size_t id = (size_t)i * k.n + coeff;
    k.dst[id] = shoup(k.src[id], k.hat_inv[i], k.mod[k.iprime[i]].value);
}
void launch_bconv_phase1(Context &c, const BConv &conv, u64 *dst, const u64 *src, hipStream_t s) {
    Phase1Args k{dst, src, c.d_mod.p, conv.d_iprime.p, conv.hat_inv.p, (uint32_t)c.n};
    hipLaunchKernelGGL(bconv_phase1_kernel, dim3((unsigned)(c.n / 256), conv.isz), dim3(256), 0, s, k);
    check_launch();
}

static LimbSel qr_sel(uint32_t size_q, uint32_t size_r, uint32_t aux0) {  // [Q limbs || R limbs] buffers
    LimbSel s = plain_sel(0, size_q + size_r);
    s.remap_from = size_q;
    s.remap_add = aux0 - size_q;
    return s;
}

}  // namespace pha

using namespace pha;

// ExpandCRTBasis_Ql_Q (src/rns.cu:1810-1836): the Ql limbs times the product of the dropped primes, the dropped limbs zero.
// blockIdx.y over the |Q| limbs of dst; src has |Ql| limbs with the same limb pitch, so dst == src works in place.
struct ExpandArgs {
    u64 *dst;
    const u64 *src;
    const u64 *c, *c_shoup;
    const DModulus *mod;
    uint32_t size_ql, n;
    size_t poly_stride = 0;   // polynomial blockIdx.z of dst and src
};
__global__ __launch_bounds__(256) void hps_expand_kernel(const ExpandArgs k) {
    const uint32_t i = blockIdx.y, coeff = blockIdx.x * 256 + threadIdx.x;
    const size_t id = blockIdx.z * k.poly_stride + (size_t)i * k.n + coeff;
    k.dst[id] = i < k.size_ql ? shoup(k.src[id], u64x2{k.c[i], k.c_shoup[i]}, k.mod[i].value) : 0;
}
static void launch_scale_round_q(Context &c, u64 *dst, const u64 *src, const double *frac, const u64 *tab, uint32_t size_ql,
                                 uint32_t extra, hipStream_t s, uint32_t batch = 1, size_t dst_stride = 0, size_t src_stride = 0) {
    const uint32_t n = (uint32_t)c.n;
    ScaleRoundQArgs ka{dst, src, frac, tab, c.d_mod.p, size_ql, extra, n, dst_stride, src_stride};
    // the carry-free dot product needs the residues (primes size_ql .. size_ql + extra) below 2^62 and the table (Ql primes) below 2^60
    bool split = true;
    for (uint32_t i = 0; i < size_ql; i++) split = split && !(c.primes[i] >> 60);
    for (uint32_t j = 0; j < extra; j++) split = split && !(c.primes[size_ql + j] >> 62);
    const dim3 grid(n / 256, batch), block(256);
#define PHA_SRQ(P)                                                                                     \
    do {                                                                                               \
        if (split) hipLaunchKernelGGL((hps_scale_round_q_kernel<P, true>), grid, block, 0, s, ka);      \
        else hipLaunchKernelGGL((hps_scale_round_q_kernel<P, false>), grid, block, 0, s, ka);           \
    } while (0)
    if (extra <= 8) PHA_SRQ(8);
    else if (extra <= 16) PHA_SRQ(16);
    else if (extra <= 32) PHA_SRQ(32);
    else hipLaunchKernelGGL((hps_scale_round_q_kernel<0, false>), grid, block, 0, s, ka);
#undef PHA_SRQ
    check_launch();
}
static void launch_expand(Context &c, HpsQ &h, u64 *dst, const u64 *src, hipStream_t s, uint32_t batch = 1, size_t poly_stride = 0) {
    ExpandArgs ka{dst, src, h.drop_mod_q.p, h.drop_mod_q_shoup.p, c.d_mod.p, h.size_q, (uint32_t)c.n, poly_stride};
    hipLaunchKernelGGL(hps_expand_kernel, dim3((unsigned)(c.n / 256), h.size_q_full, batch), dim3(256), 0, s, ka);
    check_launch();
}

// dst[i] += src[i] * prod(dropped primes) on the Ql limbs only (ExpandCRTBasis_Ql_Q_add_to_ct, src/rns.cu:1838-1858)
__global__ __launch_bounds__(256) void hps_expand_add_kernel(const ExpandArgs k) {
    const uint32_t i = blockIdx.y, coeff = blockIdx.x * 256 + threadIdx.x;
    const size_t id = (size_t)i * k.n + coeff;
    const u64 q = k.mod[i].value;
    k.dst[id] = add_mod(shoup(k.src[id], u64x2{k.c[i], k.c_shoup[i]}, q), k.dst[id], q);
}
// `polys` polynomials, dst spaced dst_stride words and src spaced src_stride (the kernel takes one polynomial)
static void launch_expand_add(Context &c, HpsQ &h, u64 *dst, size_t dst_stride, const u64 *src, size_t src_stride, uint32_t polys,
                              hipStream_t s) {
    for (uint32_t p = 0; p < polys; p++) {
        ExpandArgs ka{dst + p * dst_stride, src + p * src_stride, h.drop_mod_q.p, h.drop_mod_q_shoup.p, c.d_mod.p, h.size_q, (uint32_t)c.n};
        hipLaunchKernelGGL(hps_expand_add_kernel, dim3((unsigned)(c.n / 256), h.size_q), dim3(256), 0, s, ka);
        check_launch();
    }
}

extern "C" int pha_scaleAndRound_HPS_Q_Ql(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ctx || !dst || !src) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql >= c.size_q) throw std::invalid_argument("at least one level has to be dropped");
    HpsQ &h = c.hps_overq((uint32_t)size_Ql);
    launch_scale_round_q(c, dst, src, h.frac_drop.p, h.div_mod_q_drop.p, h.size_q, h.drop, as_stream(stream));
    PHA_API_END
}

extern "C" int pha_ExpandCRTBasis_Ql_Q(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ctx || !dst || !src) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql >= c.size_q) throw std::invalid_argument("at least one level has to be dropped");
    launch_expand(c, c.hps_overq((uint32_t)size_Ql), dst, src, as_stream(stream));
    PHA_API_END
}

// keyswitch_inplace for BFV under hps_overq_leveled with levels dropped (src/eval_key_switch.cu:142-147, :170-175): c2 [Q][N] is
// scaled down to Ql, switched with the level's DRNSTool, and both halves are expanded to Q before they are added to ct [2][Q][N]
extern "C" int pha_keyswitch_inplace_bfv_leveled(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint64_t *c2,
                                                 const uint64_t *const *rlk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ctx || !ct || !c2 || !rlk) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql >= c.size_q) throw std::invalid_argument("at least one level has to be dropped");
    HpsQ &h = c.hps_overq((uint32_t)size_Ql);
    hipStream_t s = as_stream(stream);
    const size_t n = c.n, qln = size_Ql * n, qfn = (size_t)c.size_q * n;
    // buffers of this call (second arena: the inner key switch uses the stream's own): c2 at level l, the level's
    // key-switch result (c0, c1), one expanded polynomial
    u64 *c2l = c.scratch_outer(stream, 3 * qln + qfn), *res = c2l + qln, *full = res + 2 * qln;
    launch_scale_round_q(c, c2l, c2, h.frac_drop.p, h.div_mod_q_drop.p, h.size_q, h.drop, s);
    PHA_HIP(hipMemsetAsync(res, 0, 2 * qln * sizeof(u64), s));
    const int rc = pha_keyswitch_inplace(ctx, size_Ql, res, c2l, rlk, /*scheme bfv*/ 1, stream);
    if (rc != 0) throw std::runtime_error(pha_last_error());
    for (int p = 0; p < 2; p++) {
        launch_expand(c, h, full, res + (size_t)p * qln, s);
        launch_add(c, ct + (size_t)p * qfn, full, ct + (size_t)p * qfn, c.size_q, 0, s);
    }
    PHA_API_END
}

// ---- the BFV multiplies: ONE pipeline per variant, over `batch` independent pairs (the batched entries are an extension: the
//      reference loops over ciphertexts; the single-pair entries are the same pipeline at batch = 1) ------------------------------
// ct1, ct2 [batch][2][Q][N] -> dst [batch][3][Q][N], the ct3 layout of pha_relinearize_rotate_batched.  A chunk of C pairs goes
// through ONE set of launches: every stage covers its 2C or 3C polynomials (blockIdx.z, or y for the scale-and-round kernels), so the
// launch count does not depend on C, and there are no device-to-device copies.  Working buffers per chunk, L = |Q| + |aux| limbs:
//   xa [C][2][L][N] | xb [C][2][L][N] | xp [C][3][L][N] | stage scratch
// The operands' Q limbs are produced by the forward transform reading the caller's ciphertext out of place, the auxiliary limbs by
// the conversion straight into place; the tensor product writes xp (its [3]-polynomial pitch is what every later stage and dst
// share), in one launch over the Q rows and the auxiliary rows (launch_tensor_batched).  Every stage works per coefficient, so
// ciphertext b of a batch has the bits a single-pair call returns for pair b, whatever the chunk.
//
// Default pairs per chunk.  Measured at config 4 (N = 2^15, 30 data limbs, t = 1032193; B = 64, profiles/bfv_multiply_batched.md): per-op
// time falls steeply from chunk 1 to 4 (HPS 0.376 -> 0.264 ms) and stays within 3 % from 4 to 64; 8 is the fastest for BEHZ (0.3005 ms)
// and over-Q (0.2382) and 1.3 % behind 16 for HPS (0.2627 against 0.2592), with a working set of about 1 GB instead of 2.
constexpr size_t kBfvBatchChunk = 8;
constexpr size_t kBfvMaxChunk = 1024;   // 3 * chunk polynomials ride in grid z / y (limit 65535)

// refusals and strict checks shared by every multiply entry (`name`: the entry, for the strict message); returns the pairs per chunk
static size_t bfv_batched_begin(Context &c, const char *name, const u64 *ct1, const u64 *ct2, const u64 *dst, size_t batch,
                                size_t chunk, hipStream_t s) {
    const size_t qn = (size_t)c.size_q * c.n;
    if (overlaps(dst, batch * 3 * qn, ct1, batch * 2 * qn) || overlaps(dst, batch * 3 * qn, ct2, batch * 2 * qn))
        throw std::invalid_argument("dst must not overlap ct1 or ct2");
    if (strict_mode()) {   // large batches in pieces of at most 65534 polynomials (grid z); never skipped
        const std::string n1 = std::string(name) + " ct1", n2 = std::string(name) + " ct2";
        for (size_t b0 = 0; b0 < batch; b0 += 32767) {
            const uint32_t polys = (uint32_t)(2 * std::min<size_t>(32767, batch - b0));
            strict_operand(c, n1.c_str(), ct1 + b0 * 2 * qn, rows_plain(0, c.size_q), polys, qn, s);
            if (ct2 != ct1) strict_operand(c, n2.c_str(), ct2 + b0 * 2 * qn, rows_plain(0, c.size_q), polys, qn, s);
        }
    }
    if (chunk == 0) chunk = kBfvBatchChunk;
    return std::min(std::min(chunk, batch), kBfvMaxChunk);
}

static LimbSel qr_tail_sel(uint32_t size_q, uint32_t size_r, uint32_t aux0) {  // the auxiliary limbs of a [Q || aux] buffer
    LimbSel s = qr_sel(size_q, size_r, aux0);
    s.start = size_q;
    s.count = size_r;
    return s;
}

// forward transform of the Q limbs of `polys` polynomials, ct [.][Q_in][N] -> x [.][L][N], out of place
static void lift_q_ntt(Context &c, const u64 *ct, size_t ct_stride, u64 *x, size_t x_stride, uint32_t sq, uint32_t polys, hipStream_t s) {
    NttExtra xq;
    xq.batch = polys;
    xq.poly_stride = x_stride;
    xq.in_stride = ct_stride;
    ntt_forward(c, ct, x, x, plain_sel(0, sq), EPI_FWD_CANON, xq, s);
}

// bfv_multiply_hps with mul_tech hps (src/evaluate.cu:674-818)
static void hps_multiply(Context &c, Hps &h, const u64 *ct1, const u64 *ct2, u64 *dst, size_t batch, size_t chunk, const char *name,
                         void *stream) {
    hipStream_t s = as_stream(stream);
    const size_t C = bfv_batched_begin(c, name, ct1, ct2, dst, batch, chunk, s);
    const uint32_t n = (uint32_t)c.n, sq = h.size_q, sr = h.size_r, sqr = sq + sr;
    const size_t qn = (size_t)sq * n, rn = (size_t)sr * n, qrn = (size_t)sqr * n;
    const bool square = ct1 == ct2;
    // scratch: xa [C][2][Q+R] | xb [C][2][Q+R] | xp [C][3][Q+R] | tmp [C][3][R] | y [max(Q, R)] (wide bases only)
    u64 *xa = c.scratch(stream, C * (7 * qrn + 3 * rn) + std::max(qn, rn));
    u64 *xb = xa + C * 2 * qrn, *xp = xb + C * 2 * qrn, *tmp = xp + C * 3 * qrn, *y = tmp + C * 3 * rn;
    for (size_t b0 = 0; b0 < batch; b0 += C) {
        const uint32_t B = (uint32_t)std::min(C, batch - b0);
        // lift every input polynomial from base Q to Q || R (evaluate.cu:702-716, :733-748)
        for (int w = 0; w < (square ? 1 : 2); w++) {
            const u64 *ct = (w ? ct2 : ct1) + b0 * 2 * qn;
            u64 *x = w ? xb : xa;
            lift_q_ntt(c, ct, qn, x, qrn, sq, 2 * B, s);
            bconv_hps(c, h.q_to_r, h.q_inv.p, h.alpha_q_mod_r.p, x + qn, ct, y, s, 2 * B, qrn, qn);
            NttExtra xr;
            xr.batch = 2 * B;
            xr.poly_stride = qrn;
            ntt_forward(c, x, x, x, qr_tail_sel(sq, sr, h.aux0), EPI_FWD_CANON, xr, s);
        }
        launch_tensor_batched(c, xa, square ? xa : xb, xp, sqr, sq, h.aux0 - sq, square, B, s);
        NttExtra xi;
        xi.batch = 3 * B;
        xi.poly_stride = qrn;
        ntt_inverse(c, xp, xp, xp, qr_sel(sq, sr, h.aux0), EPI_INV_CANON, xi, s);
        // scale by t/Q and round into base R, then R -> Q (evaluate.cu:800-808)
        ScaleRoundArgs ka{tmp, xp, h.frac.p, h.div_mod_r.p, c.d_mod.p, sq, sr, h.aux0, n, rn, qrn};
        launch_scale_round(c, ka, s, 3 * B);
        bconv_hps(c, h.r_to_q, h.r_inv.p, h.alpha_r_mod_q.p, dst + b0 * 3 * qn, tmp, y, s, 3 * B, qn, rn);
    }
}

// bfv_multiply_hps with mul_tech hps_overq (h of the top level) or hps_overq_leveled with levels dropped (h of a lower level):
// src/evaluate.cu:674-818, the overq branches :709-711, :745-751, :790-795.  Operands and result are over the full base Q.
// ct1 == ct2 (the same pointer) is the reference's squaring shortcut (:720-731), kept as it is.  keep_c2_low (levels dropped,
// batch == 1: bfv_mul_relin_hps, :957-958) leaves the product's c2 at level l: only c0 and c1 are expanded to Q.
static void hps_overq_multiply(Context &c, HpsQ &h, const u64 *ct1, const u64 *ct2, u64 *dst, size_t batch, size_t chunk,
                               const char *name, void *stream, bool keep_c2_low = false) {
    hipStream_t s = as_stream(stream);
    const size_t C = bfv_batched_begin(c, name, ct1, ct2, dst, batch, chunk, s);
    const uint32_t n = (uint32_t)c.n, sq = h.size_q, sr = h.size_r, sqr = sq + sr, sqf = h.size_q_full;
    const size_t qn = (size_t)sq * n, rn = (size_t)sr * n, qrn = (size_t)sqr * n, qfn = (size_t)sqf * n;
    const bool square = ct1 == ct2;
    // scratch: xa [C][2][Ql+Rl] | xb [C][2][Ql+Rl] | xp [C][3][Ql+Rl] | y [max(Q, Rl)] (wide bases only)
    u64 *xa = c.scratch(stream, C * 7 * qrn + std::max(qfn, rn));
    u64 *xb = xa + C * 2 * qrn, *xp = xb + C * 2 * qrn, *y = xp + C * 3 * qrn;
    NttExtra xf;
    xf.poly_stride = qrn;
    for (size_t b0 = 0; b0 < batch; b0 += C) {
        const uint32_t B = (uint32_t)std::min(C, batch - b0);
        const u64 *in1 = ct1 + b0 * 2 * qfn, *in2 = ct2 + b0 * 2 * qfn;
        xf.batch = 2 * B;
        // first operand: (scaled down to Ql when levels are dropped, :709-710) exact lift to Ql || Rl
        if (h.drop) {
            launch_scale_round_q(c, xa, in1, h.frac_drop.p, h.div_mod_q_drop.p, sq, h.drop, s, 2 * B, qrn, qfn);
            bconv_hps(c, h.q_to_r, h.q_inv.p, h.alpha_q_mod_r.p, xa + qn, xa, y, s, 2 * B, qrn, qrn);
            ntt_forward(c, xa, xa, xa, qr_sel(sq, sr, h.aux0), EPI_FWD_CANON, xf, s);
        } else {
            lift_q_ntt(c, in1, qfn, xa, qrn, sq, 2 * B, s);
            bconv_hps(c, h.q_to_r, h.q_inv.p, h.alpha_q_mod_r.p, xa + qn, in1, y, s, 2 * B, qrn, qfn);
            ntt_forward(c, xa, xa, xa, qr_tail_sel(sq, sr, h.aux0), EPI_FWD_CANON, xf, s);
        }
        if (!square) {   // second operand: Q -> Rl by bConv_BEHZ_var1, then Rl -> Ql exactly (:745-751)
            convert(c, h.q_to_r_var1, xb + qn, qrn, in2, qfn, 2 * B, s);
            bconv_hps(c, h.r_to_q, h.r_inv.p, h.alpha_r_mod_q.p, xb, xb + qn, y, s, 2 * B, qrn, qrn);
            ntt_forward(c, xb, xb, xb, qr_sel(sq, sr, h.aux0), EPI_FWD_CANON, xf, s);
        }
        launch_tensor_batched(c, xa, square ? xa : xb, xp, sqr, sq, h.aux0 - sq, square, B, s);
        NttExtra xi;
        xi.batch = 3 * B;
        xi.poly_stride = qrn;
        ntt_inverse(c, xp, xp, xp, qr_sel(sq, sr, h.aux0), EPI_INV_CANON, xi, s);
        // scale by t / Rl and round straight into base Ql (:790-792), expand to Q (:794-795)
        u64 *out = dst + b0 * 3 * qfn;
        launch_scale_round_q(c, out, xp, h.frac.p, h.div_mod_q.p, sq, sr, s, 3 * B, qfn, qrn);
        if (h.drop) launch_expand(c, h, out, out, s, keep_c2_low ? 2u : 3 * B, qfn);
    }
}

// bfv_multiply_behz (src/evaluate.cu:447-548)
static void behz_multiply(Context &c, Behz &b, const u64 *ct1, const u64 *ct2, u64 *dst, size_t batch, size_t chunk, const char *name,
                          void *stream) {
    hipStream_t s = as_stream(stream);
    const size_t C = bfv_batched_begin(c, name, ct1, ct2, dst, batch, chunk, s);
    const uint32_t n = (uint32_t)c.n, sq = b.size_q, sk = b.size_bsk, sqk = sq + sk;
    const size_t qn = (size_t)sq * n, bn = (size_t)sk * n, qbn = (size_t)sqk * n;
    const bool square = ct1 == ct2;
    // scratch: xa [C][2][Q+Bsk] | xb [C][2][Q+Bsk] | xp [C][3][Q+Bsk] | tmp (lift [C][2][Bsk+1], later conv / floor / m_sk)
    const size_t tmp_words = std::max(2 * (bn + n), 6 * bn + 3 * (size_t)n);
    u64 *xa = c.scratch(stream, C * (7 * qbn + tmp_words));
    u64 *xb = xa + C * 2 * qbn, *xp = xb + C * 2 * qbn, *tmp = xp + C * 3 * qbn;
    for (size_t b0 = 0; b0 < batch; b0 += C) {
        const uint32_t B = (uint32_t)std::min(C, batch - b0);
        // BEHZ_mul_1 (evaluate.cu:404-441) for the 2 B polynomials of each operand: q -> Bsk u {m_tilde}, then the small Montgomery
        // reduction modulo q switches to base Bsk
        for (int w = 0; w < (square ? 1 : 2); w++) {
            const u64 *ct = (w ? ct2 : ct1) + b0 * 2 * qn;
            u64 *x = w ? xb : xa;
            lift_q_ntt(c, ct, qn, x, qbn, sq, 2 * B, s);
            launch_fastbconv_m_tilde(c, b, tmp, ct, qn, 2 * B, s);
            launch_sm_mrq(c, b, x + qn, qbn, tmp, 2 * B, s);
            NttExtra xk;
            xk.batch = 2 * B;
            xk.poly_stride = qbn;
            ntt_forward(c, x, x, x, qr_tail_sel(sq, sk, b.aux0), EPI_FWD_CANON, xk, s);
        }
        // step 4: tensor product in both bases (evaluate.cu:479-498), steps 5-6: inverse transforms fused with the multiplication by t
        launch_tensor_batched(c, xa, square ? xa : xb, xp, sqk, sq, b.aux0 - sq, square, B, s);
        NttExtra xi;
        xi.batch = 3 * B;
        xi.poly_stride = qbn;
        xi.scale = b.t_qb.p;
        xi.scale_shoup = b.t_qb_shoup.p;
        ntt_inverse(c, xp, xp, xp, qr_sel(sq, sk, b.aux0), EPI_INV_SCALE, xi, s);
        u64 *conv = tmp, *fl = tmp + (size_t)B * 3 * bn, *msk = fl + (size_t)B * 3 * bn;  // conv, fl [3B][Bsk][N], msk [3B][N]
        launch_fast_floor(c, b, fl, xp, qbn, xp + qn, qbn, conv, 3 * B, s);   // step 7
        launch_fastbconv_sk(c, b, dst + b0 * 3 * qn, fl, msk, 3 * B, s);      // step 8
    }
}

// Every entry: its own argument checks, then one call of its variant's pipeline (which refuses a dst overlapping an input and, in
// strict mode, checks both operands under the entry's name).

extern "C" int pha_bfv_multiply_behz(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ct1 || !ct2 || !dst) throw std::invalid_argument("null pointer");
    behz_multiply(ctx->c, ctx->c.behz(), ct1, ct2, dst, 1, 1, "bfv_multiply_behz", stream);
    PHA_API_END
}

extern "C" int pha_bfv_multiply_behz_batched(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst,
                                             size_t batch, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ct1 || !ct2 || !dst) throw std::invalid_argument("null pointer");
    if (batch == 0) return 0;
    behz_multiply(ctx->c, ctx->c.behz(), ct1, ct2, dst, batch, chunk, "bfv_multiply_behz_batched", stream);
    PHA_API_END
}

extern "C" int pha_bfv_multiply_hps(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ct1 || !ct2 || !dst) throw std::invalid_argument("null pointer");
    hps_multiply(ctx->c, ctx->c.hps(), ct1, ct2, dst, 1, 1, "bfv_multiply_hps", stream);
    PHA_API_END
}

extern "C" int pha_bfv_multiply_hps_batched(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst,
                                            size_t batch, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ct1 || !ct2 || !dst) throw std::invalid_argument("null pointer");
    if (batch == 0) return 0;
    hps_multiply(ctx->c, ctx->c.hps(), ct1, ct2, dst, batch, chunk, "bfv_multiply_hps_batched", stream);
    PHA_API_END
}

extern "C" int pha_bfv_multiply_hps_overq(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst,
                                          void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ct1 || !ct2 || !dst) throw std::invalid_argument("null pointer");
    hps_overq_multiply(ctx->c, ctx->c.hps_overq(), ct1, ct2, dst, 1, 1, "bfv_multiply_hps_overq", stream);
    PHA_API_END
}

extern "C" int pha_bfv_multiply_hps_overq_leveled(pha_context_t ctx, size_t size_Ql, const uint64_t *ct1, const uint64_t *ct2,
                                                  uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ct1 || !ct2 || !dst) throw std::invalid_argument("null pointer");
    if (size_Ql < 1 || size_Ql > ctx->c.size_q) throw std::invalid_argument("RNSBase is invalid");
    hps_overq_multiply(ctx->c, ctx->c.hps_overq((uint32_t)size_Ql), ct1, ct2, dst, 1, 1, "bfv_multiply_hps_overq_leveled", stream);
    PHA_API_END
}

extern "C" int pha_bfv_multiply_hps_overq_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct1, const uint64_t *ct2,
                                                  uint64_t *dst, size_t batch, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ct1 || !ct2 || !dst) throw std::invalid_argument("null pointer");
    if (size_Ql < 1 || size_Ql > ctx->c.size_q) throw std::invalid_argument("RNSBase is invalid");
    if (batch == 0) return 0;
    hps_overq_multiply(ctx->c, ctx->c.hps_overq((uint32_t)size_Ql), ct1, ct2, dst, batch, chunk, "bfv_multiply_hps_overq_batched", stream);
    PHA_API_END
}

// bfv_mul_relin_hps under hps_overq_leveled with levels dropped (src/evaluate.cu:822-1027): the product's c2 is left at
// level l, key-switched there, and the results go onto the Ql limbs of (c0, c1).  dst [2][Q][N].
extern "C" int pha_bfv_mul_relin_hps_overq_leveled(pha_context_t ctx, size_t size_Ql, const uint64_t *ct1, const uint64_t *ct2,
                                                   const uint64_t *const *rlk, uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!ct1 || !ct2 || !rlk || !dst) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql >= c.size_q) throw std::invalid_argument("at least one level has to be dropped");
    HpsQ &h = c.hps_overq((uint32_t)size_Ql);
    hipStream_t s = as_stream(stream);
    const size_t n = c.n, qln = size_Ql * n, qfn = (size_t)c.size_q * n;
    u64 *d3 = c.scratch_outer(stream, 3 * qfn + 2 * qln), *res = d3 + 3 * qfn;   // the inner calls use the stream's own arena
    hps_overq_multiply(c, h, ct1, ct2, d3, 1, 1, "bfv_mul_relin_hps_overq_leveled", stream, true);
    PHA_HIP(hipMemsetAsync(res, 0, 2 * qln * sizeof(u64), s));
    const int rc = pha_keyswitch_inplace(ctx, size_Ql, res, d3 + 2 * qfn, rlk, /*scheme bfv*/ 1, stream);
    if (rc != 0) throw std::runtime_error(pha_last_error());
    PHA_HIP(hipMemcpyAsync(dst, d3, 2 * qfn * sizeof(u64), hipMemcpyDeviceToDevice, s));
    launch_expand_add(c, h, dst, qfn, res, qln, 2, s);
    PHA_API_END
}

// ---- DBaseConverter as an object of the ABI (include/rns_bconv.cuh:13-87): a converter between two bases given as
//      rows of the context's prime table; bConv_BEHZ (rns_bconv.cu:212-229) and bConv_HPS (:248-372) on one polynomial ----
struct pha_base_converter {
    pha_context_t ctx;
    pha::BConv conv;
    pha::DevBuf<double> inv;          // 1 / q_i of the input base (src/host/rns.cu:321-323)
    pha::DevBuf<pha::u64> alpha_mod;  // [isz + 1][osz] alpha * prod(ibase) mod p_j (:459-466)
    // bConv_BEHZ_var1 (negPQHatInvModq / QInvModp, src/host/rns.cu:469-496): built on first use
    std::unique_ptr<pha::BConv> var1;
    std::mutex var1_lock;
    // exact_convert_array (src/rns_bconv.cu:374-431): ONE output modulus, which may be a raw value outside the prime table (the
    // plain modulus t of base_q_to_t_conv_, src/rns.cu:283-284)
    bool raw = false;                 // created by pha_base_converter_create_modulus: exact_convert_array only
    pha::DModulus out_mod{};          // the output modulus when osz == 1
    std::vector<uint32_t> irows;
    pha::DevBuf<pha::u64x2> x_hat_inv;   // [isz] qhat_i^-1 mod q_i (+ Shoup)
    pha::DevBuf<pha::u64> x_mat;         // [isz] qhat_i mod t
    pha::DevBuf<pha::u64> x_big;         // [isz] words of prod(ibase), little-endian
    pha::DevBuf<pha::u64> x_q;           // [isz] q_i
    bool x_ready = false;
};

namespace pha {
struct ExactArgs {
    u64 *dst;
    const u64 *src;
    const u64x2 *hat_inv;
    const u64 *mat, *big, *q;
    DModulus t;
    uint32_t isz, n;
};
// exact_convert_array_kernel src/rns_bconv.cu:374-414, one thread per coefficient.  The mid-loop reduction (:393-396) never
// fires in the reference (`i && reduction_threshold == 0` with reduction_threshold = 15) and is absent here; v is a sum of IEEE
// divisions in limb order; Q mod t by Horner over the words of prod(ibase), most significant first.
__global__ __launch_bounds__(256) void exact_convert_kernel(const ExactArgs k) {
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    u64 lo = 0, hi = 0, q_mod_t = 0;
    double v = 0.0;
    for (uint32_t i = 0; i < k.isz; i++) {
        const u64 qi = k.q[i];
        const u64 yi = shoup(k.src[(size_t)i * k.n + coeff], k.hat_inv[i], qi);
        mac128(yi, k.mat[i], lo, hi);
        q_mod_t = barrett128(k.big[k.isz - i - 1], q_mod_t, k.t);
        v += (double)yi / (double)qi;
    }
    const u64 inner = barrett128(lo, hi, k.t);
    const u64 rounded = (u64)round(v);
    k.dst[coeff] = sub_mod(inner, mul_mod(rounded, q_mod_t, k.t), k.t.value);
}
}  // namespace pha

// constants of exact_convert_array for (input rows, ONE output modulus): qhat_i^-1 mod q_i, qhat_i mod t, prod(ibase)
static void build_exact(pha::Context &c, pha_base_converter &h) {
    using namespace pha;
    const size_t isz = h.irows.size();
    std::vector<u64x2> hat_inv(isz);
    std::vector<u64> mat(isz), q(isz);
    Big big{1};
    const u64 t = h.out_mod.value;
    for (size_t i = 0; i < isz; i++) {
        const u64 qi = q[i] = c.primes[h.irows[i]];
        hat_inv[i] = h_pair(h_invmod(prod_mod(c.primes, h.irows, qi, i), qi), qi);
        mat[i] = prod_mod(c.primes, h.irows, t, i);
        big_mul(big, qi);
    }
    big.resize(isz);
    h.x_hat_inv.upload(hat_inv);
    h.x_mat.upload(mat);
    h.x_big.upload(big);
    h.x_q.upload(q);
    h.x_ready = true;
}

extern "C" {

int pha_base_converter_create(pha_context_t ctx, const uint32_t *ibase, size_t ibase_size, const uint32_t *obase,
                              size_t obase_size, pha_base_converter_t *out) {
    PHA_CTX_BEGIN(ctx)
    if (!ctx || !ibase || !obase || !out) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (ibase_size == 0 || ibase_size > 64 || obase_size == 0 || obase_size > 256) throw std::invalid_argument("RNSBase is invalid");
    std::vector<uint32_t> ip(ibase, ibase + ibase_size), op(obase, obase + obase_size);
    for (size_t i = 0; i < ip.size(); i++) {
        if (ip[i] >= c.rows) throw std::invalid_argument("modulus index out of range");
        for (size_t k = 0; k < i; k++)
            if (ip[k] == ip[i]) throw std::invalid_argument("RNSBase is not coprime");
    }
    for (uint32_t row : op)
        if (row >= c.rows) throw std::invalid_argument("modulus index out of range");
    PHA_HIP(hipSetDevice(c.device));
    auto h = std::make_unique<pha_base_converter>();
    h->ctx = ctx;
    build_bconv(c, h->conv, ip, op);
    h->inv.upload(inverse_doubles(c.primes, ip));
    h->alpha_mod.upload(alpha_table(c.primes, ip, op));
    h->irows = ip;
    if (op.size() == 1) h->out_mod = c.mods[op[0]];
    *out = h.release();
    PHA_API_END
}

int pha_base_converter_create_modulus(pha_context_t ctx, const uint32_t *ibase, size_t ibase_size, uint64_t out_modulus,
                                      pha_base_converter_t *out) {
    PHA_CTX_BEGIN(ctx)
    if (!ctx || !ibase || !out) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (ibase_size == 0 || ibase_size > 64) throw std::invalid_argument("RNSBase is invalid");
    if (out_modulus < 2 || (out_modulus >> 61)) throw std::invalid_argument("modulus is invalid");   // Modulus: 2 .. 61 bits
    std::vector<uint32_t> ip(ibase, ibase + ibase_size);
    for (size_t i = 0; i < ip.size(); i++) {
        if (ip[i] >= c.rows) throw std::invalid_argument("modulus index out of range");
        for (size_t k = 0; k < i; k++)
            if (ip[k] == ip[i]) throw std::invalid_argument("RNSBase is not coprime");
    }
    PHA_HIP(hipSetDevice(c.device));
    auto h = std::make_unique<pha_base_converter>();
    h->ctx = ctx;
    h->raw = true;
    h->irows = ip;
    h->out_mod = h_modulus(out_modulus);
    h->conv.isz = (uint32_t)ip.size();
    h->conv.osz = 1;
    *out = h.release();
    PHA_API_END
}

void pha_base_converter_destroy(pha_base_converter_t conv) {
    if (!conv) return;
    (void)hipSetDevice(conv->ctx->c.device);
    (void)hipDeviceSynchronize();
    delete conv;
}

int pha_bConv_BEHZ(pha_base_converter_t conv, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_API_BEGIN
    if (!conv || !dst || !src) throw std::invalid_argument("null pointer");
    if (conv->raw) throw std::invalid_argument("a converter to a raw modulus supports exact_convert_array only");
    Context &c = conv->ctx->c;
    convert(c, conv->conv, dst, 0, src, 0, 1, as_stream(stream));
    PHA_API_END
}

int pha_bConv_HPS(pha_base_converter_t conv, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_API_BEGIN
    if (!conv || !dst || !src) throw std::invalid_argument("null pointer");
    if (conv->raw) throw std::invalid_argument("a converter to a raw modulus supports exact_convert_array only");
    Context &c = conv->ctx->c;
    u64 *y = c.scratch(stream, (size_t)conv->conv.isz * c.n);
    bconv_hps(c, conv->conv, conv->inv.p, conv->alpha_mod.p, dst, src, y, as_stream(stream));
    PHA_API_END
}

// DBaseConverter::bConv_BEHZ_var1 (src/rns_bconv.cu:231-246): phase 1 with negPQHatInvModq, phase 2 with QInvModp
int pha_bConv_BEHZ_var1(pha_base_converter_t conv, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_API_BEGIN
    if (!conv || !dst || !src) throw std::invalid_argument("null pointer");
    if (conv->raw) throw std::invalid_argument("a converter to a raw modulus supports exact_convert_array only");
    Context &c = conv->ctx->c;
    PHA_HIP(hipSetDevice(c.device));
    {
        std::lock_guard<std::mutex> g(conv->var1_lock);
        if (!conv->var1) {
            auto v = std::make_unique<BConv>();
            build_bconv_var1(c, *v, conv->conv.iprime, conv->conv.oprime);
            conv->var1 = std::move(v);
        }
    }
    convert(c, *conv->var1, dst, 0, src, 0, 1, as_stream(stream));
    PHA_API_END
}

// DBaseConverter::exact_convert_array (src/rns_bconv.cu:416-431): src [ibase][N] -> dst [N], the output base is ONE modulus
int pha_exact_convert_array(pha_base_converter_t conv, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_API_BEGIN
    if (!conv || !dst || !src) throw std::invalid_argument("null pointer");
    if (conv->conv.osz != 1) throw std::invalid_argument("out base in exact_convert_array must be one.");   // :423-425
    Context &c = conv->ctx->c;
    PHA_HIP(hipSetDevice(c.device));
    {
        std::lock_guard<std::mutex> g(conv->var1_lock);
        if (!conv->x_ready) build_exact(c, *conv);
    }
    ExactArgs k{dst, src, conv->x_hat_inv.p, conv->x_mat.p, conv->x_big.p, conv->x_q.p, conv->out_mod, (uint32_t)conv->irows.size(),
                (uint32_t)c.n};
    hipLaunchKernelGGL(exact_convert_kernel, dim3((unsigned)(c.n / 256)), dim3(256), 0, as_stream(stream), k);
    check_launch();
    PHA_API_END
}

// ---- the DRNSTool steps of the BFV multiplies as entry points of their own (include/rns.cuh:167-200), ONE polynomial per call,
//      so that a caller written like bfv_multiply_behz / bfv_multiply_hps (src/evaluate.cu:447-548, :674-818) links against
//      this library step by step.  The whole multiplies above call the same stage launchers with 2 B or 3 B polynomials. ----
static void need_top(Context &c, size_t size_Ql, const char *what) {
    if (size_Ql != c.size_q) throw std::invalid_argument(std::string(what) + ": the auxiliary base exists at the top data level only");
}

int pha_tool_aux_sizes(pha_context_t ctx, size_t size_Ql, uint32_t *size_Bsk, uint32_t *size_R, uint32_t *size_Rl) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("RNSBase is invalid");
    if (size_Bsk) *size_Bsk = size_Ql == c.size_q ? c.behz().size_bsk : 0;
    if (size_R) *size_R = size_Ql == c.size_q ? c.hps().size_r : 0;
    if (size_Rl) *size_Rl = c.hps_overq((uint32_t)size_Ql).size_r;
    PHA_API_END
}

// DRNSTool::fastbconv_m_tilde src/rns.cu:1249-1278: src [Q][N] -> dst [Bsk + 1][N] (last limb modulo m_tilde)
int pha_fastbconv_m_tilde(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!dst || !src) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    need_top(c, size_Ql, "fastbconv_m_tilde");
    launch_fastbconv_m_tilde(c, c.behz(), dst, src, 0, 1, as_stream(stream));
    PHA_API_END
}

// DRNSTool::sm_mrq src/rns.cu:1326-1338 (kernel :1290-1320): src [Bsk + 1][N] -> dst [Bsk][N]
int pha_sm_mrq(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!dst || !src) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    need_top(c, size_Ql, "sm_mrq");
    launch_sm_mrq(c, c.behz(), dst, 0, src, 1, as_stream(stream));
    PHA_API_END
}

// DRNSTool::fast_floor src/rns.cu:1394-1419: input_base_q [Q][N], input_base_Bsk [Bsk][N] -> out_base_Bsk [Bsk][N]
int pha_fast_floor(pha_context_t ctx, size_t size_Ql, const uint64_t *input_base_q, const uint64_t *input_base_Bsk,
                   uint64_t *out_base_Bsk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!input_base_q || !input_base_Bsk || !out_base_Bsk) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    need_top(c, size_Ql, "fast_floor");
    Behz &b = c.behz();
    u64 *conv = c.scratch(stream, (size_t)b.size_bsk * c.n);
    launch_fast_floor(c, b, out_base_Bsk, input_base_q, 0, input_base_Bsk, 0, conv, 1, as_stream(stream));
    PHA_API_END
}

// DRNSTool::fastbconv_sk src/rns.cu:1470-1510: input_base_Bsk [Bsk][N] (B limbs, then the m_sk limb) -> out_base_q [Q][N]
int pha_fastbconv_sk(pha_context_t ctx, size_t size_Ql, const uint64_t *input_base_Bsk, uint64_t *out_base_q, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!input_base_Bsk || !out_base_q) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    need_top(c, size_Ql, "fastbconv_sk");
    Behz &b = c.behz();
    u64 *msk = c.scratch(stream, c.n);
    launch_fastbconv_sk(c, b, out_base_q, input_base_Bsk, msk, 1, as_stream(stream));
    PHA_API_END
}

// DRNSTool::scaleAndRound_HPS_QR_R src/rns.cu:1739-1746 (kernel :1700-1737): src [Q + R][N] -> dst [R][N]
int pha_scaleAndRound_HPS_QR_R(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!dst || !src) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    need_top(c, size_Ql, "scaleAndRound_HPS_QR_R");
    Hps &h = c.hps();
    ScaleRoundArgs ka{dst, src, h.frac.p, h.div_mod_r.p, c.d_mod.p, h.size_q, h.size_r, h.aux0, (uint32_t)c.n, 0, 0};
    launch_scale_round(c, ka, as_stream(stream), 1);
    PHA_API_END
}

// DRNSTool::scaleAndRound_HPS_QlRl_Ql src/rns.cu:1789-1796 (kernel :1749-1787): src [Ql + Rl][N] -> dst [Ql][N]
int pha_scaleAndRound_HPS_QlRl_Ql(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!dst || !src) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("RNSBase is invalid");
    HpsQ &h = c.hps_overq((uint32_t)size_Ql);
    launch_scale_round_q(c, dst, src, h.frac.p, h.div_mod_q.p, h.size_q, h.size_r, as_stream(stream));
    PHA_API_END
}

// DRNSTool::ExpandCRTBasis_Ql_Q_add_to_ct src/rns.cu:1850-1858 (kernel :1838-1848): dst [Ql limbs] += src [Ql][N] * prod(dropped)
int pha_ExpandCRTBasis_Ql_Q_add_to_ct(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!dst || !src) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql >= c.size_q) throw std::invalid_argument("at least one level has to be dropped");
    launch_expand_add(c, c.hps_overq((uint32_t)size_Ql), dst, 0, src, 0, 1, as_stream(stream));
    PHA_API_END
}

}  // extern "C"
