// pha_poly.hip -- residue-wise (dyadic) kernels over [limb][coeff] buffers.
//
// Reference: src/polymath.cu (one coefficient per thread, `twr = tid / N`, DModulus re-read per
// thread).  Here the limb is blockIdx.y, so the modulus and its Barrett ratio sit in SGPRs, and
// every thread moves two adjacent coefficients with 16-byte accesses (pure HBM streaming).
#include <algorithm>
#include <cstdint>

#include "../../include/phantom_amd.h"
#include "pha_internal.h"
#include "pha_plain_sum.h"

namespace pha {

constexpr int kEwThreads = 256;
constexpr int kEwPerThread = 2;

struct EwArgs {
    const u64 *a, *b, *d;
    u64 *r;
    u64 *r2;             // tensor product: where c2 goes (null = r + 2 * limbs * n, the reference layout)
    const u64 *s0, *s1;  // per-limb scalars (Shoup pair)
    const DModulus *mod;
    uint32_t n, limbs, mod_start;
    uint32_t poly_limbs;  // limbs between two polynomials of a ciphertext (0 = limbs)
    size_t za, zb, zr, zr2;   // blockIdx.z (batched tensor product): elements between consecutive ciphertexts of a / b / r / r2
    const FpInfo *fpinfo;     // [prime]: limbs below 2^50 form the tensor product in FP64 (r04)
    uint32_t remap_from, remap_add;   // limbs >= remap_from use table row mod_start + limb + remap_add ([Q || R] buffers, as LimbSel; 0, 0 = off)
};

// EW_TENSOR_NT (r06): the tensor product of a BATCH of ciphertexts: every word is read once and written once and the batch is larger
// than the MALL from two ciphertexts on (161 MB per pair at C3), so its loads and stores are nontemporal -- they stream past the L2 / MALL
// contents the neighbouring kernels live on.  One box, batched HomMul + relinearize + rescale with this and the batched inner product's
// streams nontemporal: 279.3 / 277.9 -> 275.5 / 274.8 us per op at B = 32, 283.8 / 281.7 -> 277.9 / 275.6 at B = 8
// (profiles/r06_experiments.md section 7).  A single ciphertext keeps the default policy: its c2 is read back from the MALL right away.
enum EwOp { EW_ADD, EW_SUB, EW_NEG, EW_MUL, EW_MULADD, EW_MULSCALAR, EW_TENSOR, EW_SQUARE, EW_TENSOR_NT };

typedef unsigned long long ew_v2 __attribute__((ext_vector_type(2)));
template <bool NT = false>
__device__ __forceinline__ u64x2 ld2(const u64 *p) {
    if (NT) {
        const ew_v2 t = __builtin_nontemporal_load(reinterpret_cast<const ew_v2 *>(p));
        return u64x2{t.x, t.y};
    }
    return *reinterpret_cast<const u64x2 *>(p);
}
template <bool NT = false>
__device__ __forceinline__ void st2(u64 *p, u64x2 v) {
    if (NT) {
        __builtin_nontemporal_store(ew_v2{v.x, v.y}, reinterpret_cast<ew_v2 *>(p));
        return;
    }
    *reinterpret_cast<u64x2 *>(p) = v;
}

template <int OP>
__global__ __launch_bounds__(kEwThreads) void ew_kernel(const EwArgs k) {
    const uint32_t limb = blockIdx.y;
    const uint32_t row = k.mod_start + limb + (limb >= k.remap_from ? k.remap_add : 0);
    const DModulus m = k.mod[row];
    const u64 q = m.value;
    const size_t idx = (size_t)limb * k.n + ((size_t)blockIdx.x * kEwThreads + threadIdx.x) * kEwPerThread;
    const size_t rc = (size_t)(k.poly_limbs ? k.poly_limbs : k.limbs) * k.n;  // stride between the polynomials of a ciphertext

    if (OP == EW_ADD) {  // add_rns_poly polymath.cu:41-56
        u64x2 x = ld2(k.a + idx), y = ld2(k.b + idx);
        st2(k.r + idx, u64x2{add_mod(x.x, y.x, q), add_mod(x.y, y.y, q)});
    } else if (OP == EW_SUB) {  // sub_rns_poly :109-124
        u64x2 x = ld2(k.a + idx), y = ld2(k.b + idx);
        st2(k.r + idx, u64x2{sub_mod(x.x, y.x, q), sub_mod(x.y, y.y, q)});
    } else if (OP == EW_NEG) {  // negate_rns_poly :17-32
        u64x2 x = ld2(k.a + idx);
        st2(k.r + idx, u64x2{neg_mod(x.x, q), neg_mod(x.y, q)});
    } else if (OP == EW_MUL) {  // multiply_rns_poly :156-172
        u64x2 x = ld2(k.a + idx), y = ld2(k.b + idx);
        st2(k.r + idx, u64x2{mul_mod(x.x, y.x, m), mul_mod(x.y, y.y, m)});
    } else if (OP == EW_MULADD) {  // multiply_and_add_rns_poly :225-244 (128-bit sum, one Barrett)
        u64x2 x = ld2(k.a + idx), y = ld2(k.b + idx), z = ld2(k.d + idx);
        u64 lo, hi, lo2, hi2;
        mul128(x.x, y.x, lo, hi);
        lo += z.x; hi += (lo < z.x);
        mul128(x.y, y.y, lo2, hi2);
        lo2 += z.y; hi2 += (lo2 < z.y);
        st2(k.r + idx, u64x2{barrett128(lo, hi, m), barrett128(lo2, hi2, m)});
    } else if (OP == EW_MULSCALAR) {  // multiply_scalar_rns_poly (Shoup) :198-213
        const u64x2 w{k.s0[limb], k.s1[limb]};
        u64x2 x = ld2(k.a + idx);
        st2(k.r + idx, u64x2{shoup(x.x, w, q), shoup(x.y, w, q)});
    } else if (OP == EW_TENSOR || OP == EW_TENSOR_NT) {  // tensor_prod_2x2_rns_poly :463-496; blockIdx.z walks a batch of ciphertexts (r04: one launch)
        const size_t z = blockIdx.z;
        const u64 *ka = k.a + z * k.za, *kb = k.b + z * k.zb;
        u64 *kr = k.r + z * k.zr, *kr2 = k.r2 ? k.r2 + z * k.zr2 : nullptr;
        constexpr bool NT = OP == EW_TENSOR_NT;
        u64x2 c00 = ld2<NT>(ka + idx), c01 = ld2<NT>(ka + idx + rc), c10 = ld2<NT>(kb + idx), c11 = ld2<NT>(kb + idx + rc);
        u64x2 d0, d1, d2;
        if (k.fpinfo && k.fpinfo[row].ok) {   // (uniform) r04: three exact FP64 products (fp_tensor_2x2, pha_arith.h) instead of
            // three Barrett-128 multiplies on 32-bit halves (~115 vector instructions per coefficient -> ~50); the same residues as :487-:494
            const FpInfo fi = k.fpinfo[row];
            const FpMod fm{fi.q, fi.qinv, false, false};
            u64 e[6];
            fp_tensor_2x2(c00.x, c01.x, c10.x, c11.x, fm, e[0], e[1], e[2]);
            fp_tensor_2x2(c00.y, c01.y, c10.y, c11.y, fm, e[3], e[4], e[5]);
            d0 = u64x2{e[0], e[3]}; d1 = u64x2{e[1], e[4]}; d2 = u64x2{e[2], e[5]};
            st2<NT>(kr + idx, d0);
            st2<NT>(kr + idx + rc, d1);
            st2<NT>(kr2 ? kr2 + idx : kr + idx + 2 * rc, d2);
            return;
        }
        d0.x = mul_mod(c00.x, c10.x, m); d0.y = mul_mod(c00.y, c10.y, m);
        d2.x = mul_mod(c01.x, c11.x, m); d2.y = mul_mod(c01.y, c11.y, m);
        // (c0 + c1) is not reduced before the multiply (q < 2^61), exactly like :487
        d1.x = mul_mod(c00.x + c01.x, c10.x + c11.x, m);
        d1.y = mul_mod(c00.y + c01.y, c10.y + c11.y, m);
        d1.x = csub(csub(d1.x + 2 * q - d0.x - d2.x, q), q);
        d1.y = csub(csub(d1.y + 2 * q - d0.y - d2.y, q), q);
        st2<NT>(kr + idx, d0);
        st2<NT>(kr + idx + rc, d1);
        st2<NT>(kr2 ? kr2 + idx : kr + idx + 2 * rc, d2);
    } else if (OP == EW_SQUARE) {  // tensor_square_2x2_rns_poly :500-529
        const size_t z = blockIdx.z;   // a batch of ciphertexts (za = zr = 0 for one)
        const u64 *ka = k.a + z * k.za;
        u64 *kr = k.r + z * k.zr;
        u64x2 c0 = ld2(ka + idx), c1 = ld2(ka + idx + rc);
        u64x2 d0, d1, d2;
        if (k.fpinfo && k.fpinfo[row].ok) {   // (uniform) the FP64 form: c0^2, 2 c0 c1, c1^2 (fp_square_2x2)
            const FpInfo fi = k.fpinfo[row];
            const FpMod fm{fi.q, fi.qinv, false, false};
            u64 e[6];
            fp_square_2x2(c0.x, c1.x, fm, e[0], e[1], e[2]);
            fp_square_2x2(c0.y, c1.y, fm, e[3], e[4], e[5]);
            d0 = u64x2{e[0], e[3]}; d1 = u64x2{e[1], e[4]}; d2 = u64x2{e[2], e[5]};
            st2(kr + idx, d0);
            st2(kr + idx + rc, d1);
            st2(kr + idx + 2 * rc, d2);
            return;
        }
        d0.x = mul_mod(c0.x, c0.x, m); d0.y = mul_mod(c0.y, c0.y, m);
        u64 lo, hi;
        mul128(c0.x, c1.x, lo, hi);
        d1.x = barrett128(lo << 1, (hi << 1) | (lo >> 63), m);
        mul128(c0.y, c1.y, lo, hi);
        d1.y = barrett128(lo << 1, (hi << 1) | (lo >> 63), m);
        d2.x = mul_mod(c1.x, c1.x, m); d2.y = mul_mod(c1.y, c1.y, m);
        st2(kr + idx, d0);
        st2(kr + idx + rc, d1);
        st2(kr + idx + 2 * rc, d2);
    }
}

template <int OP>
static void launch_ew(Context &c, EwArgs k, size_t limbs, size_t mod_start, hipStream_t s, size_t batch = 1) {
    if (limbs == 0 || batch == 0) return;
    // rows past size_qp are the auxiliary BFV bases (the reference's callers hand these kernels base_Bsk / base_Rl moduli,
    // src/evaluate.cu:489-497); they exist once a BFV multiply entry or pha_tool_aux_sizes has built them
    if (mod_start + limbs > c.rows) throw std::invalid_argument("modulus index out of range");
    k.mod = c.d_mod.p;
    k.fpinfo = c.d_fpinfo.p;
    k.n = (uint32_t)c.n;
    k.limbs = (uint32_t)limbs;
    k.mod_start = (uint32_t)mod_start;
    dim3 grid((unsigned)(c.n / (kEwThreads * kEwPerThread)), (unsigned)limbs, (unsigned)batch);
    hipLaunchKernelGGL((ew_kernel<OP>), grid, dim3(kEwThreads), 0, s, k);
    check_launch();
}

// tensor product over table rows [mod_start, mod_start + limbs) (pha_behz.hip: base q and base Bsk)
void launch_tensor(Context &c, const u64 *a, const u64 *b, u64 *r, size_t limbs, size_t mod_start, bool square,
                   hipStream_t s, size_t poly_limbs) {
    EwArgs k{};
    k.a = a; k.b = b; k.r = r;
    k.poly_limbs = (uint32_t)poly_limbs;
    if (limbs == 0) return;
    if (mod_start + limbs > c.rows) throw std::invalid_argument("modulus index out of range");
    k.mod = c.d_mod.p;
    k.n = (uint32_t)c.n;
    k.limbs = (uint32_t)limbs;
    k.mod_start = (uint32_t)mod_start;
    dim3 grid((unsigned)(c.n / (kEwThreads * kEwPerThread)), (unsigned)limbs);
    if (square) hipLaunchKernelGGL((ew_kernel<EW_SQUARE>), grid, dim3(kEwThreads), 0, s, k);
    else hipLaunchKernelGGL((ew_kernel<EW_TENSOR>), grid, dim3(kEwThreads), 0, s, k);
    check_launch();
}

// Batched BFV multiply (pha_behz.hip): the tensor product of `batch` ciphertext pairs over [Q || aux] working buffers in ONE launch.
// a, b: [batch][2][limbs][N]; r: [batch][3][limbs][N]; limbs >= remap_from take table row limb + remap_add (LimbSel's remap), so
// the Q rows and the auxiliary rows (R or Bsk) need no launch of their own.  From two pairs on the streams are nontemporal
// (EW_TENSOR_NT above); squaring (a == b) reads each operand once.
void launch_tensor_batched(Context &c, const u64 *a, const u64 *b, u64 *r, size_t limbs, uint32_t remap_from, uint32_t remap_add,
                           bool square, size_t batch, hipStream_t s) {
    if (limbs == 0 || batch == 0) return;
    if (batch > 65535) throw std::invalid_argument("batch out of range");
    const size_t last = limbs - 1 + (limbs - 1 >= remap_from ? remap_add : 0);
    if (last >= c.rows || (remap_from && remap_from - 1 >= c.rows)) throw std::invalid_argument("modulus index out of range");
    EwArgs k{};
    k.a = a; k.b = b; k.r = r;
    k.remap_from = remap_from;
    k.remap_add = remap_add;
    k.za = k.zb = 2 * limbs * c.n;
    k.zr = 3 * limbs * c.n;
    k.mod = c.d_mod.p;
    k.fpinfo = c.d_fpinfo.p;
    k.n = (uint32_t)c.n;
    k.limbs = (uint32_t)limbs;
    dim3 grid((unsigned)(c.n / (kEwThreads * kEwPerThread)), (unsigned)limbs, (unsigned)batch);
    if (square) hipLaunchKernelGGL((ew_kernel<EW_SQUARE>), grid, dim3(kEwThreads), 0, s, k);
    else if (batch >= 2) hipLaunchKernelGGL((ew_kernel<EW_TENSOR_NT>), grid, dim3(kEwThreads), 0, s, k);
    else hipLaunchKernelGGL((ew_kernel<EW_TENSOR>), grid, dim3(kEwThreads), 0, s, k);
    check_launch();
}

// ---- summed 2 x 2 tensor product (extension; lazy relinearization: sum the size-3 products, key-switch once per sum) ------------
// For every group g = blockIdx.z: (res01[g][0], res01[g][1], res2[g]) = sum over k < terms of tensor_prod_2x2(a[g][k], b[g][k]), the
// canonical residue of the sum in every word -- what tensor_prod_2x2_rns_poly (polymath.cu:463-496) followed by add_rns_poly
// (:41-56) gives in any order of addition.  One launch; the limb is blockIdx.y (modulus in SGPRs), two adjacent coefficients per
// thread, the loop over terms inside the thread.  Per term a thread reads four 16-byte words and writes nothing: the three sums stay
// in registers and are reduced once per `per` terms, not once per term.
//
// With d0 = sum a0 b0, d2 = sum a1 b1 and M = sum (a0 + a1)(b0 + b1) as INTEGERS, d1 = M - d0 - d2 >= 0 exactly (Karatsuba on the
// sums: three products per coefficient and term), so only the three final values are reduced.
//
// Integer limbs: 128-bit accumulators (mac128: v_mad_u64_u32 chains), one barrett128 per accumulator and flush -- it reduces ANY
// 128-bit value (the quotient estimate floor(x floor(2^128 / q) / 2^128) is short by at most 1).  Terms per flush, for q < 2^b
// (b = bit length of q, read from the modulus, not assumed): a0 + a1 and b0 + b1 are at most 2q - 2, one M product is at most
// (2q - 2)^2 = 4q^2 - 8q + 4, and M restarts after a flush from r0 + r1 + r2 <= 3q - 3 (the residues it stands for), so after T
// more terms M <= 3q + T (4q^2 - 8q + 4) < T 4q^2 < T 2^(2b + 2).  T = 2^(126 - 2b) keeps that below 2^128: 16 terms for the 61-bit
// primes (p61_a2), 64 at 60 bits, 2^26 at 50 bits (capped at 2^20); d0 and d2 (products below q^2) are smaller still.
//
// FP64 limbs (fpinfo.ok: q < 2^50): every product is reduced on the spot by fp_mulmod_light to an exact integer of a few q, as in
// fp_tensor_2x2 -- a double cannot hold the unreduced product -- and what is deferred is the re-centring and the canonical
// conversion: the centred values are summed in doubles, exact while the magnitude stays below 2^53.  Bounds for q < 2^b, b <= 50:
// a0 b0 and a1 b1 reduce to at most 0.875 q (pha_arith.h); for (a0 + a1)(b0 + b1), both factors below 2q, h = fl(Y W) < 2^(2b + 2),
// the quotient rint(fl(h fl(1/q))) is off by at most 3 * 2^-53 * 4q + 0.5 <= 2 (q <= 2^50), so |h - c q| <= 2q, and the error term
// l = Y W - h is at most ulp(h) / 2 <= 2^(2b - 52) <= q / 4: each M term is an exact integer of magnitude at most 2.25 q (2.5 q is
// what the interval below allows for).  A flush is fp_reduce (|result| <= q / 2 + 1 for |x| < 2^52.6), so T terms after one leave
// |M| <= q / 2 + 1 + T 2.5 q, and T = floor((14 * 2^(52 - b) - 6) / 25) keeps that below 1.4 * 2^52 < 2^52.5: 2 terms at 50 bits,
// 4 at 49, 2293 at 40.  The last flush is followed by d1 = M - d0 - d2 (at most 1.5 q + 3) and fp_to_canon of the three.
//
// Loads are nontemporal: every operand word is read exactly once (B_NT = false: operand b is shared by all groups -- batch stride
// 0 -- and keeps the default policy so that later groups may find it in the cache).  Stores follow EW_TENSOR_NT's rule by what reads
// the result next, the key switch: a result the Infinity Cache holds (one ciphertext at C3, 71 MB) is stored with the default
// policy, a larger one (ST_NT) streams past it.
struct SumArgs {
    const u64 *a, *b;
    u64 *r01, *r2;
    const DModulus *mod;
    const FpInfo *fpinfo;
    uint32_t n, limbs, terms;
    size_t ta, za, tb, zb;   // words between consecutive terms / groups of a and b
};

__device__ __forceinline__ void sub128(u64 &lo, u64 &hi, u64 blo, u64 bhi) {   // (hi:lo) -= (bhi:blo), no borrow out
    hi -= bhi + (lo < blo);
    lo -= blo;
}

template <bool B_NT, bool ST_NT>
__global__ __launch_bounds__(kEwThreads) void tensor_sum_kernel(const SumArgs k) {
    const uint32_t limb = blockIdx.y;
    const DModulus m = k.mod[limb];
    const u64 q = m.value;
    const size_t z = blockIdx.z;
    const size_t idx = (size_t)limb * k.n + ((size_t)blockIdx.x * kEwThreads + threadIdx.x) * kEwPerThread;
    const size_t rc = (size_t)k.limbs * k.n;
    const u64 *pa = k.a + z * k.za + idx, *pb = k.b + z * k.zb + idx;
    const int bits = 64 - __clzll((long long)q);   // q < 2^bits
    u64x2 d0, d1, d2;
    uint32_t t = 0;
    if (k.fpinfo[limb].ok) {   // (uniform)
        const FpInfo fi = k.fpinfo[limb];
        const FpMod fm{fi.q, fi.qinv, false, false};
        const u64 room = (14ull << (52 - bits)) - 6;          // bits <= 50
        const uint32_t per = (uint32_t)(room / 25 < (1u << 20) ? room / 25 : (1u << 20));
        double s0x = 0.0, s0y = 0.0, s2x = 0.0, s2y = 0.0, smx = 0.0, smy = 0.0;
        do {
            const uint32_t end = k.terms - t < per ? k.terms : t + per;
#pragma unroll 2
            for (; t < end; t++, pa += k.ta, pb += k.tb) {
                const u64x2 c00 = ld2<true>(pa), c01 = ld2<true>(pa + rc), c10 = ld2<B_NT>(pb), c11 = ld2<B_NT>(pb + rc);
                const double x0 = fp_from_canon(c00.x), x1 = fp_from_canon(c01.x), y0 = fp_from_canon(c10.x), y1 = fp_from_canon(c11.x);
                s0x += fp_mulmod_light(x0, y0, fm);
                s2x += fp_mulmod_light(x1, y1, fm);
                smx += fp_mulmod_light(x0 + x1, y0 + y1, fm);
                const double u0 = fp_from_canon(c00.y), u1 = fp_from_canon(c01.y), v0 = fp_from_canon(c10.y), v1 = fp_from_canon(c11.y);
                s0y += fp_mulmod_light(u0, v0, fm);
                s2y += fp_mulmod_light(u1, v1, fm);
                smy += fp_mulmod_light(u0 + u1, v0 + v1, fm);
            }
            s0x = fp_reduce(s0x, fm); s0y = fp_reduce(s0y, fm);
            s2x = fp_reduce(s2x, fm); s2y = fp_reduce(s2y, fm);
            smx = fp_reduce(smx, fm); smy = fp_reduce(smy, fm);
        } while (t < k.terms);
        d0 = u64x2{fp_to_canon(s0x, fm), fp_to_canon(s0y, fm)};
        d1 = u64x2{fp_to_canon(smx - s0x - s2x, fm), fp_to_canon(smy - s0y - s2y, fm)};
        d2 = u64x2{fp_to_canon(s2x, fm), fp_to_canon(s2y, fm)};
    } else {
        const int sh = 126 - 2 * bits;
        const uint32_t per = sh <= 0 ? 1u : (sh >= 20 ? 1u << 20 : 1u << sh);
        u64 a0x = 0, a0y = 0, a2x = 0, a2y = 0, amx = 0, amy = 0;      // low words; high words below
        u64 h0x = 0, h0y = 0, h2x = 0, h2y = 0, hmx = 0, hmy = 0;
        for (;;) {
            const uint32_t end = k.terms - t < per ? k.terms : t + per;
#pragma unroll 2
            for (; t < end; t++, pa += k.ta, pb += k.tb) {
                const u64x2 c00 = ld2<true>(pa), c01 = ld2<true>(pa + rc), c10 = ld2<B_NT>(pb), c11 = ld2<B_NT>(pb + rc);
                mac128(c00.x, c10.x, a0x, h0x);
                mac128(c01.x, c11.x, a2x, h2x);
                mac128(c00.x + c01.x, c10.x + c11.x, amx, hmx);   // unreduced sums, as polymath.cu:487 (q < 2^63)
                mac128(c00.y, c10.y, a0y, h0y);
                mac128(c01.y, c11.y, a2y, h2y);
                mac128(c00.y + c01.y, c10.y + c11.y, amy, hmy);
            }
            sub128(amx, hmx, a0x, h0x); sub128(amx, hmx, a2x, h2x);   // d1 = M - d0 - d2 as integers
            sub128(amy, hmy, a0y, h0y); sub128(amy, hmy, a2y, h2y);
            d0 = u64x2{barrett128(a0x, h0x, m), barrett128(a0y, h0y, m)};
            d1 = u64x2{barrett128(amx, hmx, m), barrett128(amy, hmy, m)};
            d2 = u64x2{barrett128(a2x, h2x, m), barrett128(a2y, h2y, m)};
            if (t >= k.terms) break;
            // restart from the residues: d0, d2, and M = d0 + d1 + d2 (carried into the high word: 3q may pass 2^64 at 63 bits)
            a0x = d0.x; a0y = d0.y; a2x = d2.x; a2y = d2.y;
            h0x = h0y = h2x = h2y = 0;
            amx = d0.x + d1.x; hmx = amx < d0.x; amx += d2.x; hmx += amx < d2.x;
            amy = d0.y + d1.y; hmy = amy < d0.y; amy += d2.y; hmy += amy < d2.y;
        }
    }
    u64 *r01 = k.r01 + z * 2 * rc + idx;
    st2<ST_NT>(r01, d0);
    st2<ST_NT>(r01 + rc, d1);
    st2<ST_NT>(k.r2 + z * rc + idx, d2);
}

// results up to this size are left to the Infinity Cache (256 MB) for the key switch that reads them next; larger ones stream past
constexpr size_t kSumCachedResultBytes = (size_t)128 << 20;

// launch only: the callers have validated (sum_check below)
static void launch_tensor_sum(Context &c, const SumOperand &a, const SumOperand &b, u64 *res01, u64 *res2, size_t cms, size_t terms,
                              size_t batch, hipStream_t s) {
    SumArgs k{a.p, b.p, res01, res2, c.d_mod.p, c.d_fpinfo.p, (uint32_t)c.n, (uint32_t)cms, (uint32_t)terms, a.ts, a.bs, b.ts, b.bs};
    const dim3 grid((unsigned)(c.n / (kEwThreads * kEwPerThread)), (unsigned)cms, (unsigned)batch), block(kEwThreads);
    const bool st_nt = batch * 3 * cms * c.n * sizeof(u64) > kSumCachedResultBytes, b_nt = !b.shared(batch);
    if (b_nt && st_nt) hipLaunchKernelGGL((tensor_sum_kernel<true, true>), grid, block, 0, s, k);
    else if (b_nt) hipLaunchKernelGGL((tensor_sum_kernel<true, false>), grid, block, 0, s, k);
    else if (st_nt) hipLaunchKernelGGL((tensor_sum_kernel<false, true>), grid, block, 0, s, k);
    else hipLaunchKernelGGL((tensor_sum_kernel<false, false>), grid, block, 0, s, k);
    check_launch();
}

// ---- plaintext-weighted sum of ciphertexts (extension; the linear layer with plaintext weights: one rescale per sum) --------------
// For every group g = blockIdx.z and both polynomials p: res[g][p] = acc[g][p] + sum over k < terms of plain[g][k] (.) ct[g][k][p]
// (acc optional), the canonical residue of the sum in every word -- what multiply_rns_poly (polymath.cu:156-172) followed by
// add_rns_poly (:41-56), or multiply_and_add_rns_poly (:225-244), gives in any order.  The geometry is tensor_sum_kernel's: one
// launch, the limb is blockIdx.y (modulus in SGPRs), two adjacent coefficients per thread, the loop over terms inside the thread.
// Per term a thread reads three 16-byte words (the plaintext's and the two polynomials') and writes nothing; the four sums (c0 and
// c1 of the two coefficients) stay in registers.  The thread program, its two back ends (128-bit integer accumulators; exact
// centred doubles on the limbs below 2^50) and the derivation of the terms per flush are in pha_plain_sum.h, which the host can
// compile (tests/emu/emu_plain_sum.cpp): 64 terms per flush at 61 bits and 256 at 60 bits (integer), 5 at 50 bits, 11 at 49 and
// 6552 at 40 (FP64).
//
// Cache policy, as above: operand words read once are loaded nontemporally (acc always is); an operand shared by all groups
// (batch stride 0 with batch > 1: PL_NT / CT_NT false) keeps the default policy so that later groups may find it in the cache;
// the result is stored with the default policy up to kSumCachedResultBytes and nontemporally (ST_NT) above it.
struct PlainSumArgs {
    const u64 *plain, *ct, *acc;   // acc may be null
    u64 *res;
    const DModulus *mod;
    const FpInfo *fpinfo;
    uint32_t n, limbs, terms;
    size_t tp, zp, tc, zc, za;     // words between consecutive terms / groups of plain and ct, groups of acc
};

template <bool PL_NT, bool CT_NT>
struct PlainSumSrc {
    const u64 *pp, *pc;
    size_t tp, tc, rc;
    __device__ __forceinline__ void next(u64x2 &w, u64x2 &c0, u64x2 &c1) {
        w = ld2<PL_NT>(pp);
        c0 = ld2<CT_NT>(pc);
        c1 = ld2<CT_NT>(pc + rc);
        pp += tp;
        pc += tc;
    }
};

template <bool PL_NT, bool CT_NT, bool ST_NT>
__global__ __launch_bounds__(kEwThreads, 8) void plain_sum_kernel(const PlainSumArgs k) {   // 8 waves per SIMD: at most 64 VGPRs
    const uint32_t limb = blockIdx.y;
    const DModulus m = k.mod[limb];
    const size_t z = blockIdx.z;
    const size_t idx = (size_t)limb * k.n + ((size_t)blockIdx.x * kEwThreads + threadIdx.x) * kEwPerThread;
    const size_t rc = (size_t)k.limbs * k.n;
    PlainSumSrc<PL_NT, CT_NT> src{k.plain + z * k.zp + idx, k.ct + z * k.zc + idx, k.tp, k.tc, rc};
    u64x2 a0{0, 0}, a1{0, 0}, r0, r1;
    if (k.acc) {   // (uniform)
        const u64 *pa = k.acc + z * k.za + idx;
        a0 = ld2<true>(pa);
        a1 = ld2<true>(pa + rc);
    }
    PlainSumNoProbe probe;
    if (k.fpinfo[limb].ok) {   // (uniform)
        const FpInfo fi = k.fpinfo[limb];
        plain_sum_fp(src, k.terms, FpMod{fi.q, fi.qinv, false, false}, modulus_bits(m.value), a0, a1, r0, r1, probe);
    } else {
        plain_sum_int(src, k.terms, m, a0, a1, r0, r1, probe);
    }
    u64 *r = k.res + z * 2 * rc + idx;   // (res == acc: this thread has read these very words above)
    st2<ST_NT>(r, r0);
    st2<ST_NT>(r + rc, r1);
}

// launch only: the callers have validated (sum_check below)
void launch_plain_sum(Context &c, const SumOperand &plain, const SumOperand &ct, const SumOperand &acc, u64 *res, size_t cms, size_t terms,
                      size_t batch, hipStream_t s) {
    PlainSumArgs k{plain.p,  ct.p,     acc.p, res,   c.d_mod.p, c.d_fpinfo.p, (uint32_t)c.n, (uint32_t)cms, (uint32_t)terms,
                   plain.ts, plain.bs, ct.ts, ct.bs, acc.bs};
    const dim3 grid((unsigned)(c.n / (kEwThreads * kEwPerThread)), (unsigned)cms, (unsigned)batch), block(kEwThreads);
    const bool st_nt = batch * 2 * cms * c.n * sizeof(u64) > kSumCachedResultBytes;
    const bool pl_nt = !plain.shared(batch), ct_nt = !ct.shared(batch);
#define PHA_PLAIN_SUM_LAUNCH(P, C, S) hipLaunchKernelGGL((plain_sum_kernel<P, C, S>), grid, block, 0, s, k)
    if (pl_nt && ct_nt) { if (st_nt) PHA_PLAIN_SUM_LAUNCH(true, true, true); else PHA_PLAIN_SUM_LAUNCH(true, true, false); }
    else if (pl_nt) { if (st_nt) PHA_PLAIN_SUM_LAUNCH(true, false, true); else PHA_PLAIN_SUM_LAUNCH(true, false, false); }
    else if (ct_nt) { if (st_nt) PHA_PLAIN_SUM_LAUNCH(false, true, true); else PHA_PLAIN_SUM_LAUNCH(false, true, false); }
    else { if (st_nt) PHA_PLAIN_SUM_LAUNCH(false, false, true); else PHA_PLAIN_SUM_LAUNCH(false, false, false); }
#undef PHA_PLAIN_SUM_LAUNCH
    check_launch();
}

// used by pha_rns.hip
void launch_add(Context &c, const u64 *a, const u64 *b, u64 *r, size_t limbs, size_t mod_start, hipStream_t s) {
    EwArgs k{};
    k.a = a; k.b = b; k.r = r;
    launch_ew<EW_ADD>(c, k, limbs, mod_start, s);
}

}  // namespace pha

using namespace pha;

// ---- the summed-product entries (extension): what they share on the host --------------------------------------------------------
// Every strided operand is a SumOperand view (pha_sum_operand.h: the address arithmetic, the layout refusals, the output-overlap
// walk and the strict-mode runs); the entries add what is theirs: the limb count, the batch one launch takes, their outputs.

// the refusals about everything but the outputs: terms, limb count, batch (the group is blockIdx.z of ONE launch), layout
static void sum_check(Context &c, std::initializer_list<SumOperand> ops, size_t cms, size_t terms, size_t batch) {
    sum_check_terms(terms);
    if (cms == 0 || cms > c.rows) throw std::invalid_argument("coeff_mod_size out of range");
    if (batch > 65535) throw std::invalid_argument("batch out of range");
    sum_check_layout(ops, terms);
}

// an output is aligned and touches no operand; the refusal calls operand i `what` (an absent operand is skipped)
struct SumInput {
    SumOperand op;
    const char *what;
};
static void sum_check_output(const char *name, const u64 *out, size_t out_words, std::initializer_list<SumInput> ins, size_t terms,
                             size_t batch) {
    if (reinterpret_cast<uintptr_t>(out) & 15) throw std::invalid_argument("buffers must be 16-byte aligned");
    for (const SumInput &in : ins)
        if (in.op.p && in.op.touches(out, out_words, terms, batch))
            throw std::invalid_argument(std::string(name) + " must not overlap " + in.what);
}

constexpr size_t kInnerProductChunk = 8;   // groups per set of launches, as the batched BFV multiplies (pha_behz.hip: kBfvBatchChunk)

// groups per set of launches of the whole-operation entries: what the batched key switch takes in one call
static size_t inner_product_chunk(Context &c, size_t size_Ql, size_t chunk, size_t batch) {
    if (chunk == 0) chunk = kInnerProductChunk;
    chunk = std::min<size_t>(std::min(chunk, batch), 1024);
    const size_t beta = c.tool((uint32_t)size_Ql).beta;
    while (chunk > 1 && (beta * chunk > 65535 || 2 * chunk > 65535)) chunk /= 2;
    return chunk;
}

// The whole operations: the summed tensor product of a chunk of groups, then ONE batched key switch for the chunk (the key
// switch is linear: relinearizing the sum is relinearizing every product, at 1 / terms of the cost).  The working buffers are the
// call's own (ONE scratch_outer claim: the key switch uses the stream's arena) and sized by the chunk; nothing is copied.
// What differs between the three entries, apart from the preconditions each checks itself, is the closing call:
enum class InnerProductClose {
    Rescale,     // pha_keyswitch_rescale_batched: the sums in scratch, dst [batch][2][Ql - 1][N]
    InPlace,     // pha_keyswitch_inplace_batched: (c0, c1) summed straight into dst [batch][2][Ql][N], which it completes in place
    ModSwitch,   // pha_keyswitch_mod_switch_batched (bgv): as Rescale
};
static int inner_product(pha_context_t ctx, InnerProductClose close, size_t size_Ql, const SumOperand &op1, const SumOperand &op2,
                         size_t terms, size_t batch, const u64 *const *rlk, int scheme, u64 *dst, size_t chunk, void *stream) {
    Context &c = ctx->c;
    const bool in_dst = close == InnerProductClose::InPlace;
    sum_check(c, {op1, op2}, size_Ql, terms, batch);
    const size_t ql_n = size_Ql * c.n, out_n = in_dst ? ql_n : ql_n - c.n;
    sum_check_output("dst", dst, batch * 2 * out_n, {{op1, "an operand ciphertext"}, {op2, "an operand ciphertext"}}, terms, batch);
    if (batch == 0) return 0;
    hipStream_t s = as_stream(stream);
    strict_sum_operand(c, "tensor_prod_2x2_sum operand1", op1, size_Ql, terms, batch, false, s);
    strict_sum_operand(c, "tensor_prod_2x2_sum operand2", op2, size_Ql, terms, batch, false, s);
    const size_t C = inner_product_chunk(c, size_Ql, chunk, batch);
    // the sums of a chunk: [C][2][Ql][N] | [C][Ql][N], or c2 alone
    u64 *work = c.scratch_outer(stream, C * (in_dst ? 1 : 3) * ql_n), *s2 = in_dst ? work : work + C * 2 * ql_n;
    for (size_t b0 = 0; b0 < batch; b0 += C) {
        const size_t B = std::min(C, batch - b0);
        u64 *out = dst + b0 * 2 * out_n, *s01 = in_dst ? out : work;
        launch_tensor_sum(c, op1.advanced(b0, 0), op2.advanced(b0, 0), s01, s2, size_Ql, terms, B, s);
        int rc = 0;
        switch (close) {
            case InnerProductClose::Rescale: rc = pha_keyswitch_rescale_batched(ctx, size_Ql, s01, s2, B, rlk, out, stream); break;
            case InnerProductClose::InPlace: rc = pha_keyswitch_inplace_batched(ctx, size_Ql, out, s2, B, rlk, scheme, stream); break;
            case InnerProductClose::ModSwitch: rc = pha_keyswitch_mod_switch_batched(ctx, size_Ql, s01, s2, B, rlk, out, stream); break;
        }
        if (rc != 0) return rc;   // (its message is the last error)
    }
    return 0;
}

// ---- plaintext-weighted sums (extension) -----------------------------------------------------------------------------------------
// The views of both entries: plaintext (g, k) is L N words at plain + g * bp + k * tp (sum_poly), ciphertext (g, k) 2 L N words at
// ct + g * bc + k * tc (sum_ct), acc (g) 2 L N words at acc + g * ba (sum_acc; absent when acc is null).
// An output may not touch a plaintext, a ciphertext or an addend (handed over as absent where out IS acc in acc's own layout, which
// the kernel allows)
static void plain_sum_check_output(const char *name, const u64 *out, size_t out_words, const SumOperand &plain, const SumOperand &ct,
                                   const SumOperand &acc, size_t terms, size_t batch) {
    sum_check_output(name, out, out_words,
                     {{plain, "a plaintext operand"},
                      {ct, "an operand ciphertext"},
                      {acc, "acc (other than res == acc with a stride of 2 * L * N)"}},
                     terms, batch);
}
// strict mode: every distinct buffer of the three operands; never skipped
static void plain_sum_strict(Context &c, const SumOperand &plain, const SumOperand &ct, const SumOperand &acc, size_t cms, size_t terms,
                             size_t batch, hipStream_t s) {
    strict_sum_operand(c, "multiply_plain_sum plain", plain, cms, terms, batch, false, s);
    strict_sum_operand(c, "multiply_plain_sum ct", ct, cms, terms, batch, false, s);
    strict_sum_operand(c, "multiply_plain_sum acc", acc, cms, 1, batch, false, s);
}

constexpr size_t kPlainSumChunk = 8;   // groups per set of launches of the rescale entry, as kInnerProductChunk

extern "C" {

int pha_add_rns_poly(pha_context_t ctx, const uint64_t *a, const uint64_t *b, uint64_t *r, size_t cms,
                     size_t mod_start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(a); need(b); need(r);
    strict_operand(ctx->c, "operand a", a, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    strict_operand(ctx->c, "operand b", b, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    launch_add(ctx->c, a, b, r, cms, mod_start, as_stream(stream));
    PHA_API_END
}
int pha_sub_rns_poly(pha_context_t ctx, const uint64_t *a, const uint64_t *b, uint64_t *r, size_t cms,
                     size_t mod_start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(a); need(b); need(r);
    strict_operand(ctx->c, "operand a", a, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    strict_operand(ctx->c, "operand b", b, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    EwArgs k{};
    k.a = a; k.b = b; k.r = r;
    launch_ew<EW_SUB>(ctx->c, k, cms, mod_start, as_stream(stream));
    PHA_API_END
}
int pha_negate_rns_poly(pha_context_t ctx, const uint64_t *a, uint64_t *r, size_t cms, size_t mod_start,
                        void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(a); need(r);
    strict_operand(ctx->c, "operand a", a, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    EwArgs k{};
    k.a = a; k.r = r;
    launch_ew<EW_NEG>(ctx->c, k, cms, mod_start, as_stream(stream));
    PHA_API_END
}
int pha_multiply_rns_poly(pha_context_t ctx, const uint64_t *a, const uint64_t *b, uint64_t *r, size_t cms,
                          size_t mod_start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(a); need(b); need(r);
    strict_operand(ctx->c, "operand a", a, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    strict_operand(ctx->c, "operand b", b, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    EwArgs k{};
    k.a = a; k.b = b; k.r = r;
    launch_ew<EW_MUL>(ctx->c, k, cms, mod_start, as_stream(stream));
    PHA_API_END
}
int pha_multiply_and_add_rns_poly(pha_context_t ctx, const uint64_t *a, const uint64_t *b, const uint64_t *d,
                                  uint64_t *r, size_t cms, size_t mod_start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(a); need(b); need(d); need(r);
    strict_operand(ctx->c, "operand a", a, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    strict_operand(ctx->c, "operand b", b, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    strict_operand(ctx->c, "operand d", d, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    EwArgs k{};
    k.a = a; k.b = b; k.d = d; k.r = r;
    launch_ew<EW_MULADD>(ctx->c, k, cms, mod_start, as_stream(stream));
    PHA_API_END
}
int pha_multiply_scalar_rns_poly(pha_context_t ctx, const uint64_t *a, const uint64_t *scalar,
                                 const uint64_t *scalar_shoup, uint64_t *r, size_t cms, size_t mod_start,
                                 void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(a); need(scalar); need(scalar_shoup); need(r);
    strict_operand(ctx->c, "operand a", a, rows_plain(mod_start, cms), 1, 0, as_stream(stream));
    EwArgs k{};
    k.a = a; k.s0 = scalar; k.s1 = scalar_shoup; k.r = r;
    launch_ew<EW_MULSCALAR>(ctx->c, k, cms, mod_start, as_stream(stream));
    PHA_API_END
}
int pha_tensor_prod_2x2_rns_poly(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *res,
                                 size_t cms, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op1); need(op2); need(res);
    strict_operand(ctx->c, "tensor_prod_2x2 operand1", op1, rows_plain(0, cms), 2, cms * ctx->c.n, as_stream(stream));
    strict_operand(ctx->c, "tensor_prod_2x2 operand2", op2, rows_plain(0, cms), 2, cms * ctx->c.n, as_stream(stream));
    EwArgs k{};
    k.a = op1; k.b = op2; k.r = res;
    launch_ew<EW_TENSOR>(ctx->c, k, cms, 0, as_stream(stream));
    PHA_API_END
}
int pha_tensor_prod_2x2_batched(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *res01,
                                uint64_t *res2, size_t cms, size_t batch, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op1); need(op2); need(res01); need(res2);
    const size_t ln = cms * ctx->c.n;
    if (batch > 65535) throw std::invalid_argument("batch out of range");
    if (2 * batch <= 65535) {
        strict_operand(ctx->c, "tensor_prod_2x2 operand1", op1, rows_plain(0, cms), (uint32_t)(2 * batch), ln, as_stream(stream));
        strict_operand(ctx->c, "tensor_prod_2x2 operand2", op2, rows_plain(0, cms), (uint32_t)(2 * batch), ln, as_stream(stream));
    }
    // one launch over the batch (blockIdx.z): r04 trace of 8 ciphertexts -- 8 launches of 35.7 us each against 30.7 us for a lone one
    EwArgs k{};
    k.a = op1; k.b = op2; k.r = res01; k.r2 = res2;
    k.za = k.zb = k.zr = 2 * ln;
    k.zr2 = ln;
    if (batch >= 2) launch_ew<EW_TENSOR_NT>(ctx->c, k, cms, 0, as_stream(stream), batch);
    else launch_ew<EW_TENSOR>(ctx->c, k, cms, 0, as_stream(stream), batch);
    PHA_API_END
}
int pha_tensor_prod_2x2_sum_batched(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *res01, uint64_t *res2,
                                    size_t cms, size_t terms, size_t batch, size_t op1_term_stride, size_t op1_batch_stride,
                                    size_t op2_term_stride, size_t op2_batch_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op1); need(op2); need(res01); need(res2);
    Context &c = ctx->c;
    const size_t ln = cms * c.n;
    const SumOperand a = sum_ct(op1, op1_term_stride, op1_batch_stride, ln, kSumCrowded),
                     b = sum_ct(op2, op2_term_stride, op2_batch_stride, ln, kSumCrowded);
    sum_check(c, {a, b}, cms, terms, batch);
    sum_check_output("res01", res01, batch * 2 * ln, {{a, "an operand ciphertext"}, {b, "an operand ciphertext"}}, terms, batch);
    sum_check_output("res2", res2, batch * ln, {{a, "an operand ciphertext"}, {b, "an operand ciphertext"}}, terms, batch);
    if (batch == 0) return 0;
    strict_sum_operand(c, "tensor_prod_2x2_sum operand1", a, cms, terms, batch, false, as_stream(stream));
    strict_sum_operand(c, "tensor_prod_2x2_sum operand2", b, cms, terms, batch, false, as_stream(stream));
    launch_tensor_sum(c, a, b, res01, res2, cms, terms, batch, as_stream(stream));
    PHA_API_END
}

// The three whole operations on encrypted operands: each checks what is its own (scheme, level, special modulus, plain modulus) and
// names its form; inner_product() above does the rest.
int pha_inner_product_relin_rescale_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *op1, const uint64_t *op2, size_t terms,
                                            size_t batch, size_t op1_term_stride, size_t op1_batch_stride, size_t op2_term_stride,
                                            size_t op2_batch_stride, const uint64_t *const *rlk, uint64_t *dst, size_t chunk,
                                            void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op1); need(op2); need(rlk); need(dst);
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("size_Ql out of range");
    if (c.size_p == 0) throw std::invalid_argument("context has no special modulus");
    if (size_Ql < 2) throw std::invalid_argument("cannot rescale the last remaining modulus");
    const size_t ln = size_Ql * c.n;
    return inner_product(ctx, InnerProductClose::Rescale, size_Ql, sum_ct(op1, op1_term_stride, op1_batch_stride, ln, kSumCrowded),
                         sum_ct(op2, op2_term_stride, op2_batch_stride, ln, kSumCrowded), terms, batch, rlk, 0, dst, chunk, stream);
    PHA_API_END
}

int pha_inner_product_relin_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *op1, const uint64_t *op2, size_t terms,
                                    size_t batch, size_t op1_term_stride, size_t op1_batch_stride, size_t op2_term_stride,
                                    size_t op2_batch_stride, const uint64_t *const *rlk, int scheme, uint64_t *dst, size_t chunk,
                                    void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op1); need(op2); need(rlk); need(dst);
    Context &c = ctx->c;
    if (scheme == PHA_SCHEME_BFV)
        throw std::invalid_argument("inner product of bfv ciphertexts is not supported: a bfv product is not an NTT-form tensor product");
    if (scheme != PHA_SCHEME_CKKS && scheme != PHA_SCHEME_BGV) throw std::invalid_argument("unsupported scheme");
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("size_Ql out of range");
    if (c.size_p == 0) throw std::invalid_argument("context has no special modulus");
    if (scheme == PHA_SCHEME_BGV && !c.tool((uint32_t)size_Ql).bgv_ready)
        throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
    const size_t ln = size_Ql * c.n;
    return inner_product(ctx, InnerProductClose::InPlace, size_Ql, sum_ct(op1, op1_term_stride, op1_batch_stride, ln, kSumCrowded),
                         sum_ct(op2, op2_term_stride, op2_batch_stride, ln, kSumCrowded), terms, batch, rlk, scheme, dst, chunk, stream);
    PHA_API_END
}
// bgv: the sums of a chunk, then ONE fused key switch + mod_switch_to_next for the chunk (pha_keyswitch_mod_switch_batched)
int pha_inner_product_relin_mod_switch_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *op1, const uint64_t *op2, size_t terms,
                                               size_t batch, size_t op1_term_stride, size_t op1_batch_stride, size_t op2_term_stride,
                                               size_t op2_batch_stride, const uint64_t *const *rlk, uint64_t *dst, size_t chunk,
                                               void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op1); need(op2); need(rlk); need(dst);
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("size_Ql out of range");
    if (c.size_p == 0) throw std::invalid_argument("context has no special modulus");
    if (size_Ql < 2) throw std::invalid_argument("cannot switch down the last remaining modulus");
    if (!c.tool((uint32_t)size_Ql).bgv_ready) throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
    const size_t ln = size_Ql * c.n;
    return inner_product(ctx, InnerProductClose::ModSwitch, size_Ql, sum_ct(op1, op1_term_stride, op1_batch_stride, ln, kSumCrowded),
                         sum_ct(op2, op2_term_stride, op2_batch_stride, ln, kSumCrowded), terms, batch, rlk, 0, dst, chunk, stream);
    PHA_API_END
}

int pha_multiply_plain_sum_batched(pha_context_t ctx, const uint64_t *plain, const uint64_t *ct, const uint64_t *acc, uint64_t *res,
                                   size_t cms, size_t terms, size_t batch, size_t plain_term_stride, size_t plain_batch_stride,
                                   size_t ct_term_stride, size_t ct_batch_stride, size_t acc_batch_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(plain); need(ct); need(res);
    Context &c = ctx->c;
    const size_t ln = cms * c.n;
    const SumOperand pl = sum_poly(plain, plain_term_stride, plain_batch_stride, ln, kPlainCrowded),
                     cts = sum_ct(ct, ct_term_stride, ct_batch_stride, ln, kCtCrowded), addend = sum_acc(acc, acc_batch_stride, ln);
    sum_check(c, {pl, cts, addend}, cms, terms, batch);
    const bool inplace = acc && res == acc && acc_batch_stride == 2 * ln;
    plain_sum_check_output("res", res, batch * 2 * ln, pl, cts, inplace ? SumOperand{} : addend, terms, batch);
    if (batch == 0) return 0;
    hipStream_t s = as_stream(stream);
    plain_sum_strict(c, pl, cts, addend, cms, terms, batch, s);
    launch_plain_sum(c, pl, cts, addend, res, cms, terms, batch, s);
    PHA_API_END
}

// The whole operation: the sums of a chunk of groups into this call's own work buffer (scratch_outer: the level drop uses the
// stream's arena), then the EXISTING level drop over the chunk's 2 * chunk polynomials straight into dst.  Nothing is copied.
int pha_plain_inner_product_rescale_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *plain, const uint64_t *ct,
                                            const uint64_t *acc, size_t terms, size_t batch, size_t plain_term_stride,
                                            size_t plain_batch_stride, size_t ct_term_stride, size_t ct_batch_stride,
                                            size_t acc_batch_stride, int scheme, uint64_t *dst, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(plain); need(ct); need(dst);
    Context &c = ctx->c;
    if (scheme == PHA_SCHEME_BFV)
        throw std::invalid_argument("plaintext inner product of bfv ciphertexts is not supported: a bfv plaintext product is not an "
                                    "NTT-form product of stored operands");
    if (scheme != PHA_SCHEME_CKKS && scheme != PHA_SCHEME_BGV) throw std::invalid_argument("unsupported scheme");
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("size_Ql out of range");
    if (size_Ql < 2) throw std::invalid_argument("cannot rescale the last remaining modulus");
    if (scheme == PHA_SCHEME_BGV && !c.tool((uint32_t)size_Ql).bgv_ready)
        throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
    const size_t ql_n = size_Ql * c.n, out_n = (size_Ql - 1) * c.n;
    const SumOperand pl = sum_poly(plain, plain_term_stride, plain_batch_stride, ql_n, kPlainCrowded),
                     cts = sum_ct(ct, ct_term_stride, ct_batch_stride, ql_n, kCtCrowded), addend = sum_acc(acc, acc_batch_stride, ql_n);
    sum_check(c, {pl, cts, addend}, size_Ql, terms, batch);
    plain_sum_check_output("dst", dst, batch * 2 * out_n, pl, cts, addend, terms, batch);
    if (batch == 0) return 0;
    hipStream_t s = as_stream(stream);
    plain_sum_strict(c, pl, cts, addend, size_Ql, terms, batch, s);
    const size_t C = std::min<size_t>(std::min(chunk ? chunk : kPlainSumChunk, batch), 32767);   // 2 C polynomials per level drop
    u64 *work = c.scratch_outer(stream, C * 2 * ql_n);   // the sums of a chunk: [C][2][Ql][N]
    for (size_t b0 = 0; b0 < batch; b0 += C) {
        const size_t B = std::min(C, batch - b0);
        launch_plain_sum(c, pl.advanced(b0, 0), cts.advanced(b0, 0), addend.advanced(b0, 0), work, size_Ql, terms, B, s);
        const int rc = scheme == PHA_SCHEME_CKKS
                           ? pha_divide_and_round_q_last_ntt(ctx, size_Ql, work, 2 * B, dst + b0 * 2 * out_n, stream)
                           : pha_mod_t_and_divide_q_last_ntt(ctx, size_Ql, work, 2 * B, dst + b0 * 2 * out_n, stream);
        if (rc != 0) return rc;   // (its message is the last error)
    }
    PHA_API_END
}
int pha_tensor_square_2x2_rns_poly(pha_context_t ctx, const uint64_t *op, uint64_t *res, size_t cms,
                                   void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op); need(res);
    strict_operand(ctx->c, "tensor_square_2x2 operand", op, rows_plain(0, cms), 2, cms * ctx->c.n, as_stream(stream));
    EwArgs k{};
    k.a = op; k.r = res;
    launch_ew<EW_SQUARE>(ctx->c, k, cms, 0, as_stream(stream));
    PHA_API_END
}
// tensor_prod_2x2_rns_poly / tensor_square_2x2_rns_poly with the reference's `modulus` pointer argument (polymath.cu:463-529) as a
// first table row: the BEHZ / HPS callers run them over base Bsk and base R (src/evaluate.cu:489-497, :763-777)
int pha_tensor_prod_2x2_rns_poly_at(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *res, size_t cms,
                                    size_t mod_start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op1); need(op2); need(res);
    strict_operand(ctx->c, "tensor_prod_2x2 operand1", op1, rows_plain(mod_start, cms), 2, cms * ctx->c.n, as_stream(stream));
    strict_operand(ctx->c, "tensor_prod_2x2 operand2", op2, rows_plain(mod_start, cms), 2, cms * ctx->c.n, as_stream(stream));
    launch_tensor(ctx->c, op1, op2, res, cms, mod_start, false, as_stream(stream), cms);
    PHA_API_END
}
int pha_tensor_square_2x2_rns_poly_at(pha_context_t ctx, const uint64_t *op, uint64_t *res, size_t cms, size_t mod_start,
                                      void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(op); need(res);
    strict_operand(ctx->c, "tensor_square_2x2 operand", op, rows_plain(mod_start, cms), 2, cms * ctx->c.n, as_stream(stream));
    launch_tensor(ctx->c, op, op, res, cms, mod_start, true, as_stream(stream), cms);
    PHA_API_END
}
int pha_add_to_ct(pha_context_t ctx, uint64_t *ct, const uint64_t *cx, size_t size_Ql, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(cx);
    strict_operand(ctx->c, "ct", ct, rows_plain(0, size_Ql), 1, 0, as_stream(stream));
    strict_operand(ctx->c, "cx", cx, rows_plain(0, size_Ql), 1, 0, as_stream(stream));
    launch_add(ctx->c, ct, cx, ct, size_Ql, 0, as_stream(stream));  // add_to_ct_kernel rns_bconv.cu:763-769
    PHA_API_END
}

}  // extern "C"
