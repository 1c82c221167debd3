// pha_hoist.hip -- hoisted rotations on gfx950: one mod-up shared by many Galois elements (pha_hoisting), the plaintext-weighted
// form (pha_hoisting_weighted), its baby-step / giant-step forms (pha_hoisting_weighted_bsgs, ..._blocks), and both hoisted forms for
// a batch of ciphertexts that share the keys (pha_hoisting_batched, pha_hoisting_weighted_batched), and the baby-step / giant-step
// form for such a batch (pha_hoisting_weighted_bsgs_batched).
//
// Two host drivers stand behind the seven entries.  hoist_batched_core() runs the plain and the weighted form: the single entries are
// a batch of one, in place, and a chunk of one ciphertext takes the one-ciphertext kernels.  The three BSGS entries build one BsgsCall
// (the plan of pha_hoist_plan.h: refusals, counts, host tables; the scratch claim; the upload) and run bsgs_baby_steps() and
// bsgs_giant_side() per set of row blocks or per chunk of ciphertexts.  Every entry claims its scratch once and no driver calls
// another.
//
// Reference: src/evaluate.cu:1670-1866.  The mod-up, the mod-down and the Galois launchers these entries call live in pha_rns.hip
// (declared in pha_internal.h).
#include "../../include/phantom_amd.h"
#include "pha_internal.h"
#include "pha_hoist_batched.h"
#include "pha_hoist_bsgs_batched.h"
#include "pha_hoist_plan.h"
#include <algorithm>
#include <cstddef>
#include <cstring>

namespace pha {
// ---- hoisted rotations (src/evaluate.cu:1670-1866): for every output coefficient, sum over the Galois
//      elements e and digits b of  modup_b[perm_e[k]] * key_{e,b}[k].  The reference materialises the
//      permuted digits and adds per-element inner products; here the permutation is a gather inside ONE
//      inner-product kernel and the accumulation over elements stays in the 128-bit registers
//      (n_elts * beta * 2^120 < 2^128 needs n_elts * beta < 256; larger sets are split by the driver). ----
struct HoistArgs {
    u64 *cx;                          // [2][QlP][N]
    const u64 *t_mod_up;              // [beta][QlP][N]
    const u64 *const *const *keys;    // device array [n_elts] of device arrays [beta] of keys [2][QP][N]
    const uint32_t *const *tables;    // device array [n_elts] of NTT-domain permutation tables
    const DModulus *mod;
    const uint32_t *qlp_prime;
    uint32_t n, beta, n_elts, accumulate;  // accumulate: add to what cx already holds (split calls)
    size_t qlp_n, qp_n;
};
// ---- weighted hoisted rotations (BASELINE config 5, build-defined: no reference counterpart): as above with a
//      plaintext weight per Galois element, multiplied in before the shared mod-down:
//      cx[k] = sum_e w_e[k] * (sum_b modup_b[perm_e[k]] * key_{e,b}[k] mod q).  The per-element inner product
//      is reduced once (Barrett) so that the weighted sum fits the 128-bit accumulator again. ----
struct HoistWArgs : HoistArgs {
    const u64 *const *weights;        // device array [n_elts] of weights [QlP][N] (NTT form)
};

// One kernel for the plain and the weighted form.  WEIGHTED: an element's digit sums go to a fresh accumulator, are reduced and
// multiplied by the element's weight into the running sums; otherwise they go straight to the running sums.
// BETA > 0: BETA is a template parameter and every load of an element (2 x BETA gathered digit words, 4 x BETA key words, the next
// element's permutation entry) is issued before the first multiply (r03: the run-time digit loop serialised one memory round trip
// per digit).  BETA = 0: any number of digits (run-time loop).
// Accumulator bounds: every product is below q_max^2; the driver launches at most acc_capacity() of them per sum.
template <int BETA, bool WEIGHTED>
__global__ __launch_bounds__(256) void hoist_inner_prod_kernel(const std::conditional_t<WEIGHTED, HoistWArgs, HoistArgs> k) {
    const uint32_t nid = blockIdx.y;
    const uint32_t twr = k.qlp_prime[nid];
    const DModulus m = k.mod[twr];
    const size_t coeff = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t out_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    KeyAcc acc;
    if (k.accumulate)
        acc.seed(*reinterpret_cast<const u64x2 *>(k.cx + out_id), *reinterpret_cast<const u64x2 *>(k.cx + out_id + k.qlp_n));
    uint2 idx = *reinterpret_cast<const uint2 *>(k.tables[0] + coeff);
    for (uint32_t e = 0; e < k.n_elts; e++) {
        const uint2 idx_next = *reinterpret_cast<const uint2 *>(k.tables[e + 1 < k.n_elts ? e + 1 : e] + coeff);
        const u64 *const *keys = k.keys[e];
        u64x2 w{};
        if constexpr (WEIGHTED) w = *reinterpret_cast<const u64x2 *>(k.weights[e] + out_id);
        KeyAcc part;
        KeyAcc &sums = WEIGHTED ? part : acc;   // where this element's digit sums go
        if constexpr (BETA > 0) {
            u64 v0[BETA], v1[BETA];
            u64x2 kb[BETA], ka[BETA];
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                const u64 *digit = k.t_mod_up + (size_t)i * k.qlp_n + (size_t)nid * k.n;
                const u64 *key = keys[i];
                v0[i] = digit[idx.x];
                v1[i] = digit[idx.y];
                kb[i] = *reinterpret_cast<const u64x2 *>(key + evk_id);
                ka[i] = *reinterpret_cast<const u64x2 *>(key + evk_id + k.qp_n);
            }
#pragma unroll
            for (int i = 0; i < BETA; i++) sums.mac(v0[i], v1[i], kb[i], ka[i]);
        } else {
            for (uint32_t i = 0; i < k.beta; i++) {
                const u64 *digit = k.t_mod_up + (size_t)i * k.qlp_n + (size_t)nid * k.n;
                const u64 v0 = digit[idx.x], v1 = digit[idx.y];
                const u64 *key = keys[i];
                sums.mac(v0, v1, *reinterpret_cast<const u64x2 *>(key + evk_id), *reinterpret_cast<const u64x2 *>(key + evk_id + k.qp_n));
            }
        }
        if constexpr (WEIGHTED) {
            u64x2 s, t;
            part.reduce(m, s, t);
            acc.mac_weighted(s, t, w);
        }
        idx = idx_next;
    }
    u64x2 r0, r1;
    acc.reduce(m, r0, r1);
    *reinterpret_cast<u64x2 *>(k.cx + out_id) = r0;
    *reinterpret_cast<u64x2 *>(k.cx + out_id + k.qlp_n) = r1;
}

// dst[limb][k] = sum_e src[limb][perm_e[k]] mod q  (c0 part of hoisting for ckks / bgv)
__global__ __launch_bounds__(256) void hoist_c0_kernel(u64 *dst, const u64 *src, const uint32_t *const *tables,
                                                       uint32_t n_elts, const DModulus *mod, uint32_t n) {
    const uint32_t limb = blockIdx.y;
    const u64 q = mod[limb].value;
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    u64 acc = 0;
    for (uint32_t e = 0; e < n_elts; e++) acc = add_mod(acc, src[(size_t)limb * n + tables[e][coeff]], q);
    dst[(size_t)limb * n + coeff] = acc;
}

// dst[p][limb][k] = sum_e w_e[limb][k] * src[p][limb][perm_e[k]] mod q.  blockIdx.z = polynomial: c0 takes every
// element, c1 only the main-diagonal ones (Galois element 1, identity permutation), whose list starts at first_c1.
__global__ __launch_bounds__(256) void hoist_weighted_c_kernel(u64 *dst, const u64 *src, const uint32_t *const *tables,
                                                               const u64 *const *weights, uint32_t n_elts,
                                                               uint32_t first_c1, const DModulus *mod, uint32_t n,
                                                               size_t poly_stride) {
    const uint32_t limb = blockIdx.y, p = blockIdx.z;
    const DModulus m = mod[limb];
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const size_t id = (size_t)limb * n + coeff;
    u64 lo = 0, hi = 0;
    uint32_t terms = 0;
    for (uint32_t e = p ? first_c1 : 0; e < n_elts; e++) {
        mac128(src[p * poly_stride + (size_t)limb * n + tables[e][coeff]], weights[e][id], lo, hi);
        if (++terms == 48) {           // products of two 61-bit residues: 48 * 2^122 stays below 2^128
            lo = barrett128(lo, hi, m);
            hi = 0;
            terms = 1;
        }
    }
    dst[p * poly_stride + id] = barrett128(lo, hi, m);
}

// ---- baby-step / giant-step form of the weighted hoisted rotations (BASELINE config 5, build-defined) -----------------------
//      out = sum_i rot_{G_i}( sum_j w_ij (.) rot_{B_j}(ct) ):  d = ng * nb diagonals from nb - 1 baby keys and ng - 1 giant keys
//      instead of d - 1 keys (24 GB of Galois keys per 128-diagonal block at C3 -> 4 GB).  "Double hoisting": the baby rotations
//      share ONE mod-up of c1 and their inner products stay in the extended base [Q_l || P]; every giant step i weights them with
//      its own plaintexts w_ij (given over [Q_l || P], as in pha_hoisting_weighted) and pays one mod-down; the giant rotations
//      share ONE final mod-down of the sum of their inner products.
// One thread = one coefficient of one limb; the accumulators of NG giant steps live in registers, so the baby keys, the gathered
// digits and the per-baby Barrett reductions are paid once for all of them.
struct BsgsArgs {
    u64 *acc;                         // [ng][2][QlP][N]
    const u64 *t_mod_up;              // [beta][QlP][N]
    const u64 *const *const *keys;    // device [nb]: key table of baby j ([beta] keys), null for the identity
    const uint32_t *const *tables;    // device [nb]: NTT-domain permutation of baby j
    const u64 *const *weights;        // device [ng][nb]: w_ij over [QlP][N], null = no such term
    const DModulus *mod;
    const uint32_t *qlp_prime;
    uint32_t n, beta, nb, g0;         // g0: first giant step of this launch
    size_t qlp_n, qp_n;
    const u64 *cc;                    // the input ciphertext (c0, c1), [2][Ql][N]
    const u64x2 *p_mod_q;             // [Ql] P mod q_j with its Shoup quotient
    uint32_t ql;
    size_t ql_n;
    const FpInfo *fpinfo;             // [prime]: limbs below 2^50 accumulate in doubles (r04)
};
// The c0 / c1 terms ride in the same accumulators: on a data limb j the value added is P * x mod q_j, which the mod-down that
// follows (it divides by P exactly: (cx_j - conv(cx_P)_j) P^-1) turns back into x, and on the P limbs P * x = 0 -- so
// moddown(acc + P * y) = moddown(acc) + y, word for word what a separate weighted sum over Q_l would add afterwards.
// Every load of a baby step (3 gathered digits, the c0 word, 2 x BETA key words, NG weights, the next step's permutation
// entry) is issued before the first multiply: the first version branched per giant step on a null weight and looped over the
// digits at run time, which serialised ~12 memory round trips per baby step (2.9 TB/s); missing weights now point at a zero
// plane supplied by the driver.
// r04: limbs whose prime is below 2^50 run the same sums in FP64 (pha_arith.h: residues as doubles with integer values, every
// product an exact fp_mulmod_light).  A 128-bit multiply-accumulate costs ~12 vector instructions on 32-bit halves and the two
// Barrett reductions per baby step ~55; here a product-and-add is 7 FP64 operations and there is nothing to reduce at the end of a
// step but two re-centrings: ~210 instead of ~340 instructions per baby step at NG = 8, and 2 NG instead of 4 NG accumulator
// register pairs.  Magnitudes: gathered digits, key words and weights are canonical (< q), so a digit product is below 0.875 q and
// BETA + 1 of them below 4.4 q; s and t are re-centred (<= q/2), a weighted term is then below 0.69 q, and the accumulators are
// re-centred every 8 baby steps (0.5 + 8 x 0.69 = 6.0 q < 8 q = 2^53): every value is an exact integer, the stored residues are
// the ones the integer form stores.
template <int NG, int BETA>
__device__ __forceinline__ void hoist_bsgs_body_fp(const BsgsArgs &k, uint32_t nid, uint32_t twr, const FpInfo fi) {
    const FpMod fm{fi.q, fi.qinv, false, false};
    const size_t coeff = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t out_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    const bool data_limb = nid < k.ql;          // uniform
    const double pqd = data_limb ? fp_from_canon(k.p_mod_q[nid].x) : 0.0;
    const u64 *cc0 = k.cc + (size_t)(data_limb ? nid : 0) * k.n;
    double al[NG], bl[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) al[g] = bl[g] = 0.0;
    uint32_t idx = k.tables[0][coeff];
    for (uint32_t j = 0; j < k.nb; j++) {
        const u64 *const *keys = k.keys[j];
        const uint32_t idx_next = k.tables[j + 1 < k.nb ? j + 1 : j][coeff];
        u64 wv[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) wv[g] = k.weights[(size_t)(k.g0 + g) * k.nb + j][out_id];
        const u64 x0 = cc0[idx];
        double s, t;
        if (keys) {   // uniform
            u64 v[BETA], kb[BETA], ka[BETA];
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                const u64 *key = keys[i];
                v[i] = k.t_mod_up[(size_t)i * k.qlp_n + (size_t)nid * k.n + idx];
                kb[i] = key[evk_id];
                ka[i] = key[evk_id + k.qp_n];
            }
            s = data_limb ? fp_mulmod_light(fp_from_canon(x0), pqd, fm) : 0.0;   // + P * rot_j(c0)
            t = 0.0;
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                const double vd = fp_from_canon(v[i]);
                s += fp_mulmod_light(vd, fp_from_canon(kb[i]), fm);
                t += fp_mulmod_light(vd, fp_from_canon(ka[i]), fm);
            }
        } else {      // identity baby step: (P c0, P c1) on the data limbs, nothing on the P limbs
            s = data_limb ? fp_mulmod_light(fp_from_canon(x0), pqd, fm) : 0.0;
            t = data_limb ? fp_mulmod_light(fp_from_canon(k.cc[k.ql_n + (size_t)nid * k.n + idx]), pqd, fm) : 0.0;
        }
        s = fp_reduce(s, fm);
        t = fp_reduce(t, fm);
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const double wd = fp_from_canon(wv[g]);
            al[g] += fp_mulmod_light(s, wd, fm);
            bl[g] += fp_mulmod_light(t, wd, fm);
        }
        if ((j & 7u) == 7u) {   // (uniform)
#pragma unroll
            for (int g = 0; g < NG; g++) {
                al[g] = fp_reduce(al[g], fm);
                bl[g] = fp_reduce(bl[g], fm);
            }
        }
        idx = idx_next;
    }
#pragma unroll
    for (int g = 0; g < NG; g++) {
        u64 *acc = k.acc + (size_t)(k.g0 + g) * 2 * k.qlp_n + out_id;
        acc[0] = fp_to_canon(al[g], fm);
        acc[k.qlp_n] = fp_to_canon(bl[g], fm);
    }
}

// integer limbs: accumulators [goff, goff + NG) of the launch
template <int NG, int BETA>
__device__ __forceinline__ void hoist_bsgs_body_int(const BsgsArgs &k, uint32_t nid, uint32_t twr, uint32_t goff) {
    const DModulus m = k.mod[twr];
    const size_t coeff = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t out_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    const bool data_limb = nid < k.ql;          // uniform
    const u64x2 pq = data_limb ? k.p_mod_q[nid] : u64x2{0, 0};
    const u64 *cc0 = k.cc + (size_t)(data_limb ? nid : 0) * k.n;   // (P limbs: any valid row, the value is multiplied by 0)
    u64 al[NG], ah[NG], bl[NG], bh[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) al[g] = ah[g] = bl[g] = bh[g] = 0;
    uint32_t idx = k.tables[0][coeff];
    for (uint32_t j = 0; j < k.nb; j++) {
        const u64 *const *keys = k.keys[j];
        const uint32_t idx_next = k.tables[j + 1 < k.nb ? j + 1 : j][coeff];
        // loads first
        u64 wv[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) wv[g] = k.weights[(size_t)(k.g0 + goff + g) * k.nb + j][out_id];
        const u64 x0 = cc0[idx];
        u64 s, t;
        if (keys) {   // uniform
            u64 v[BETA], kb[BETA], ka[BETA];
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                const u64 *key = keys[i];
                v[i] = k.t_mod_up[(size_t)i * k.qlp_n + (size_t)nid * k.n + idx];
                kb[i] = key[evk_id];
                ka[i] = key[evk_id + k.qp_n];
            }
            u64 sl = 0, sh = 0, tl = 0, th = 0;
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                mac128(v[i], kb[i], sl, sh);
                mac128(v[i], ka[i], tl, th);
            }
            s = barrett128(sl, sh, m);
            t = barrett128(tl, th, m);
            if (data_limb) s = add_mod(s, shoup(x0, pq, m.value), m.value);          // + P * rot_j(c0)
        } else {      // identity baby step: (P c0, P c1) on the data limbs, nothing on the P limbs
            s = data_limb ? shoup(x0, pq, m.value) : 0;
            t = data_limb ? shoup(k.cc[k.ql_n + (size_t)nid * k.n + idx], pq, m.value) : 0;
        }
#pragma unroll
        for (int g = 0; g < NG; g++) {
            mac128(s, wv[g], al[g], ah[g]);
            mac128(t, wv[g], bl[g], bh[g]);
        }
        idx = idx_next;
    }
#pragma unroll
    for (int g = 0; g < NG; g++) {
        u64 *acc = k.acc + (size_t)(k.g0 + goff + g) * 2 * k.qlp_n + out_id;
        acc[0] = barrett128(al[g], ah[g], m);
        acc[k.qlp_n] = barrett128(bl[g], bh[g], m);
    }
}

// NG accumulators per launch.  NG = 16 (r04): the FP64 limbs keep 16 (block, giant step) accumulators in 32 register pairs, so the
// baby keys are streamed once per 16 / ng row blocks; an integer limb would need 64 pairs for that and walks its baby steps twice
// with 8 accumulators each instead (16 of 60 limbs at the C3 set).
template <int NG, int BETA>
__global__ __launch_bounds__(256) void hoist_bsgs_inner_prod_kernel(const BsgsArgs k) {
    const uint32_t nid = blockIdx.y;
    const uint32_t twr = k.qlp_prime[nid];
    if (k.fpinfo) {   // (uniform) FP64 limbs
        const FpInfo fi = k.fpinfo[twr];
        if (fi.ok) {
            hoist_bsgs_body_fp<NG, BETA>(k, nid, twr, fi);
            return;
        }
    }
    if constexpr (NG > 8) {
        hoist_bsgs_body_int<8, BETA>(k, nid, twr, 0);
        hoist_bsgs_body_int<NG - 8, BETA>(k, nid, twr, 8);
    } else {
        hoist_bsgs_body_int<NG, BETA>(k, nid, twr, 0);
    }
}

// giant steps, part 1: ct0 = sum_i B_i0[perm_Gi], ct1 = sum over the identity giant steps of B_i1, and the dense operands
// g1[z] = B_i1[perm_Gi] of the keyed giant steps (z = their rank among the keyed ones)
// blockIdx.z = row block: its ng giant steps start at B + z * ng * 2 polynomials, its nk operands at g1 + z * nk, its output at ct + 2 z
__global__ __launch_bounds__(256) void bsgs_combine_kernel(u64 *ct, u64 *g1, const u64 *B, const uint32_t *const *tables,
                                                           const uint32_t *keyed_rank, uint32_t ng, uint32_t nk, const DModulus *mod,
                                                           uint32_t n, size_t poly_stride) {
    const uint32_t limb = blockIdx.y;
    ct += (size_t)blockIdx.z * 2 * poly_stride;
    g1 += (size_t)blockIdx.z * nk * poly_stride;
    B += (size_t)blockIdx.z * ng * 2 * poly_stride;
    const u64 q = mod[limb].value;
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const size_t id = (size_t)limb * n + coeff;
    u64 r0 = 0, r1 = 0;
    for (uint32_t i = 0; i < ng; i++) {
        const uint32_t from = tables[i][coeff];
        const u64 *b = B + (size_t)(2 * i) * poly_stride + (size_t)limb * n;
        r0 = add_mod(r0, b[from], q);
        const uint32_t z = keyed_rank[i];
        if (z == 0xffffffffu) r1 = add_mod(r1, b[poly_stride + coeff], q);     // identity giant step
        else g1[(size_t)z * poly_stride + id] = b[poly_stride + from];
    }
    ct[id] = r0;
    ct[poly_stride + id] = r1;
}

// giant steps, part 2: cx = sum_z <modup(g1[z]), key_z> in one pass (the inner products of nk key switches that share a mod-down)
struct MultiInnerArgs {
    u64 *cx;                        // [2][QlP][N]
    const u64 *t_mod_up;            // [nk][beta][QlP][N]
    const u64 *const *const *keys;  // device [nk] -> [beta]
    const DModulus *mod;
    const uint32_t *qlp_prime;
    uint32_t n, beta, nk;
    size_t qlp_n, qp_n;
};
__global__ __launch_bounds__(256) void inner_prod_multi_kernel(const MultiInnerArgs kk) {   // blockIdx.z = row block
    MultiInnerArgs k = kk;
    k.cx += (size_t)blockIdx.z * 2 * k.qlp_n;
    k.t_mod_up += (size_t)blockIdx.z * k.nk * k.beta * k.qlp_n;
    const uint32_t nid = blockIdx.y;
    const uint32_t twr = k.qlp_prime[nid];
    const DModulus m = k.mod[twr];
    const size_t coeff = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t c2_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    KeyAcc acc;
    for (uint32_t z = 0; z < k.nk; z++) {
        const u64 *const *keys = k.keys[z];
        for (uint32_t i = 0; i < k.beta; i++) {
            const u64 *key = keys[i];
            const u64x2 v = *reinterpret_cast<const u64x2 *>(k.t_mod_up + ((size_t)z * k.beta + i) * k.qlp_n + c2_id);
            acc.mac(v.x, v.y, *reinterpret_cast<const u64x2 *>(key + evk_id), *reinterpret_cast<const u64x2 *>(key + evk_id + k.qp_n));
        }
    }
    u64x2 r0, r1;
    acc.reduce(m, r0, r1);
    *reinterpret_cast<u64x2 *>(k.cx + c2_id) = r0;
    *reinterpret_cast<u64x2 *>(k.cx + c2_id + k.qlp_n) = r1;
}

// What an unreduced 128-bit accumulator holds: floor(2^128 / q_max^2) - 1 products of residues below q_max (255 for primes up to
// 60 bits, 63 for the 61-bit primes the context also accepts)
static size_t acc_capacity(const Context &c) {
    u64 qmax = 0;
    for (uint32_t i = 0; i < c.size_qp; i++) qmax = std::max(qmax, c.primes[i]);
    int qbits = 0;
    while (qbits < 64 && (qmax >> qbits)) qbits++;
    return qbits >= 64 ? 1 : ((size_t)1 << std::min(20, 128 - 2 * qbits)) - 1;
}

// The pointer tables of a call: host lists gathered into one buffer that upload() copies to `dev` (scratch words) in one go; add()
// hands back the typed device address the list will have there.
class PtrTable {
    std::vector<u64> host;
    u64 *dev;

public:
    explicit PtrTable(u64 *d) : dev(d) {}
    template <class T>
    const T *add(const std::vector<const void *> &list) {
        const T *at = reinterpret_cast<const T *>(dev + host.size());
        for (const void *p : list) host.push_back((u64)(uintptr_t)p);
        return at;
    }
    const uint32_t *add(const std::vector<uint32_t> &list) {   // two entries per word
        const uint32_t *at = reinterpret_cast<const uint32_t *>(dev + host.size());
        host.resize(host.size() + (list.size() + 1) / 2);
        std::memcpy(host.data() + host.size() - (list.size() + 1) / 2, list.data(), list.size() * sizeof(uint32_t));
        return at;
    }
    size_t words() const { return host.size(); }
    void upload(hipStream_t s) const {
        if (!host.empty()) PHA_HIP(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    }
};

// ---- hoisted rotations of a batch of ciphertexts that share keys, tables and weights (pha_hoisting_batched,
//      pha_hoisting_weighted_batched).  The thread program is pha_hoist_batched.h (replayed on the CPU by tests/emu): one thread
//      owns two adjacent coefficients of one limb for up to CB ciphertexts, blockIdx.z = group of CB ciphertexts of the chunk. ----
template <int BETA, int CB, bool WEIGHTED>
__global__ __launch_bounds__(256) void hoist_inner_prod_batched_kernel(const HoistBArgs k) {
    hoist_batched_thread<BETA, CB, WEIGHTED>(k, blockIdx.x * 256 + threadIdx.x, blockIdx.y, blockIdx.z);
}

// The c0 / (c0, c1) kernels' batched twins: a thread owns one coefficient of one limb for up to kHoistCGroup ciphertexts (blockIdx.z
// carries the group), so a permutation entry and a weight are read once per group.  Ciphertext b's polynomials are at src + b *
// src_stride and dst + b * dst_stride (+ poly_stride for c1).
constexpr uint32_t kHoistCGroup = 4;

// dst[b][0][limb][k] = sum_e src[b][limb][perm_e[k]] mod q, dst[b][1] = 0
__global__ __launch_bounds__(256) void hoist_c0_batched_kernel(u64 *dst, size_t dst_stride, const u64 *src, size_t src_stride,
                                                               const uint32_t *const *tables, uint32_t n_elts, const DModulus *mod,
                                                               uint32_t n, uint32_t n_ct, size_t poly_stride) {
    const uint32_t limb = blockIdx.y, first = blockIdx.z * kHoistCGroup;
    const uint32_t cnt = n_ct - first < kHoistCGroup ? n_ct - first : kHoistCGroup;   // (uniform)
    const u64 q = mod[limb].value;
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const u64 *row = src + (size_t)first * src_stride + (size_t)limb * n;
    u64 acc[kHoistCGroup] = {};
    for (uint32_t e = 0; e < n_elts; e++) {
        const uint32_t from = tables[e][coeff];
#pragma unroll
        for (uint32_t j = 0; j < kHoistCGroup; j++)
            if (j < cnt) acc[j] = add_mod(acc[j], row[(size_t)j * src_stride + from], q);
    }
#pragma unroll
    for (uint32_t j = 0; j < kHoistCGroup; j++)
        if (j < cnt) {
            u64 *d = dst + (size_t)(first + j) * dst_stride + (size_t)limb * n + coeff;
            d[0] = acc[j];
            d[poly_stride] = 0;
        }
}

// dst[b][p][limb][k] = sum_e w_e[limb][k] * src[b][p][limb][perm_e[k]] mod q.  blockIdx.z = 2 * group + p; elements and fold as
// hoist_weighted_c_kernel.
__global__ __launch_bounds__(256) void hoist_weighted_c_batched_kernel(u64 *dst, size_t dst_stride, const u64 *src, size_t src_stride,
                                                                       const uint32_t *const *tables, const u64 *const *weights,
                                                                       uint32_t n_elts, uint32_t first_c1, const DModulus *mod,
                                                                       uint32_t n, uint32_t n_ct, size_t poly_stride) {
    const uint32_t limb = blockIdx.y, p = blockIdx.z & 1, first = (blockIdx.z >> 1) * kHoistCGroup;
    const uint32_t cnt = n_ct - first < kHoistCGroup ? n_ct - first : kHoistCGroup;   // (uniform)
    const DModulus m = mod[limb];
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const size_t id = (size_t)limb * n + coeff;
    const u64 *row = src + (size_t)first * src_stride + p * poly_stride + (size_t)limb * n;
    u64 lo[kHoistCGroup] = {}, hi[kHoistCGroup] = {};
    uint32_t terms = 0;
    for (uint32_t e = p ? first_c1 : 0; e < n_elts; e++) {
        const uint32_t from = tables[e][coeff];
        const u64 w = weights[e][id];
#pragma unroll
        for (uint32_t j = 0; j < kHoistCGroup; j++)
            if (j < cnt) mac128(row[(size_t)j * src_stride + from], w, lo[j], hi[j]);
        if (++terms == 48) {           // products of two 61-bit residues: 48 * 2^122 stays below 2^128
#pragma unroll
            for (uint32_t j = 0; j < kHoistCGroup; j++) {
                lo[j] = barrett128(lo[j], hi[j], m);
                hi[j] = 0;
            }
            terms = 1;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kHoistCGroup; j++)
        if (j < cnt) dst[(size_t)(first + j) * dst_stride + p * poly_stride + id] = barrett128(lo[j], hi[j], m);
}

// All rotations' gather + inner products of n_ct ciphertexts (t_mod_up [n_ct][beta][QlP][N] -> cx [n_ct][2][QlP][N]) in one kernel per
// `per_call` Galois elements; a later launch adds to what cx holds.  d_w != null: the weighted form.  One ciphertext takes the
// one-ciphertext kernel, more take the batched one over groups of CB.
static void launch_hoist_inner_prod(Context &c, Tool &t, u64 *cx, const u64 *t_mod_up, const u64 *const *const *d_keys,
                                    const uint32_t *const *d_tabs, const u64 *const *d_w, size_t n_elts, size_t per_call, size_t n_ct,
                                    hipStream_t s) {
    const unsigned gx = (unsigned)(c.n / 512);
    for (size_t e0 = 0; e0 < n_elts; e0 += per_call) {
        HoistWArgs k{};
        HoistBArgs kb{};
        auto fill = [&](auto &x) {
            x.cx = cx; x.t_mod_up = t_mod_up; x.keys = d_keys + e0; x.tables = d_tabs + e0; x.weights = d_w ? d_w + e0 : nullptr;
            x.mod = c.d_mod.p; x.qlp_prime = t.d_qlp_prime.p; x.n = (uint32_t)c.n; x.beta = t.beta;
            x.n_elts = (uint32_t)std::min(per_call, n_elts - e0); x.accumulate = e0 ? 1 : 0;
            x.qlp_n = (size_t)t.size_qlp * c.n; x.qp_n = (size_t)c.size_qp * c.n;
        };
        fill(k);
        fill(kb);
        kb.n_ct = (uint32_t)n_ct;
        if (n_ct == 1)
            with_beta<0>(t.beta, [&](auto B) {
                constexpr int BETA = decltype(B)::value;
                const dim3 grid(gx, t.size_qlp), block(256);
                if (d_w) hipLaunchKernelGGL((hoist_inner_prod_kernel<BETA, true>), grid, block, 0, s, k);
                else hipLaunchKernelGGL((hoist_inner_prod_kernel<BETA, false>), grid, block, 0, s, static_cast<const HoistArgs &>(k));
            });
        else
            with_beta<0>(t.beta, [&](auto B) {
                constexpr int BETA = decltype(B)::value;
                constexpr int CBP = hoist_batched_cb(BETA, false), CBW = hoist_batched_cb(BETA, true);
                const unsigned cb = d_w ? CBW : CBP;
                const dim3 grid(gx, t.size_qlp, (unsigned)((n_ct + cb - 1) / cb)), block(256);
                if (d_w) hipLaunchKernelGGL((hoist_inner_prod_batched_kernel<BETA, CBW, true>), grid, block, 0, s, kb);
                else hipLaunchKernelGGL((hoist_inner_prod_batched_kernel<BETA, CBP, false>), grid, block, 0, s, kb);
            });
        check_launch();
    }
}

// The sums over c0 (d_w == null, NTT form: dst c0 = sum_e galois_e(c0), dst c1 = 0) or over (c0, c1) with the weights, for n_ct
// ciphertexts at dst + b * [2][Ql][N], read from src + b * src_stride: the one-ciphertext kernels for n_ct = 1, their batched twins else.
static void launch_hoist_c_sums(Context &c, size_t size_Ql, u64 *dst, const u64 *src, size_t src_stride, const uint32_t *const *d_tabs,
                                const u64 *const *d_w, size_t n_elts, size_t n_ks, size_t n_ct, hipStream_t s) {
    const uint32_t n = (uint32_t)c.n;
    const size_t ql_n = size_Ql * n;
    const unsigned gx = n / 256, gy = (unsigned)size_Ql, groups = (unsigned)((n_ct + kHoistCGroup - 1) / kHoistCGroup);
    if (d_w && n_ct == 1)
        hipLaunchKernelGGL(hoist_weighted_c_kernel, dim3(gx, gy, 2), dim3(256), 0, s, dst, src, d_tabs, d_w, (uint32_t)n_elts, (uint32_t)n_ks,
                           c.d_mod.p, n, ql_n);
    else if (d_w)
        hipLaunchKernelGGL(hoist_weighted_c_batched_kernel, dim3(gx, gy, 2 * groups), dim3(256), 0, s, dst, 2 * ql_n, src, src_stride, d_tabs,
                           d_w, (uint32_t)n_elts, (uint32_t)n_ks, c.d_mod.p, n, (uint32_t)n_ct, ql_n);
    else if (n_ct == 1)
        hipLaunchKernelGGL(hoist_c0_kernel, dim3(gx, gy), dim3(256), 0, s, dst, src, d_tabs, (uint32_t)n_elts, c.d_mod.p, n);
    else
        hipLaunchKernelGGL(hoist_c0_batched_kernel, dim3(gx, gy, groups), dim3(256), 0, s, dst, 2 * ql_n, src, src_stride, d_tabs,
                           (uint32_t)n_elts, c.d_mod.p, n, (uint32_t)n_ct, ql_n);
    check_launch();
    if (!d_w && n_ct == 1) PHA_HIP(hipMemsetAsync(dst + ql_n, 0, ql_n * sizeof(u64), s));   // (the batched twin writes c1 = 0 itself)
}

// Driver of the plain and the weighted form (weights == null: plain), single entries (a batch of one, in place) and batched ones.  Per
// chunk of cb ciphertexts: one mod-up of beta * cb digits (the digits' own limbs copied into t_mod_up -- the gather reads them through
// the permutation, so modup's own_in_place is off here whatever the key switch's own_in_place_ok() says), the inner-product launches,
// the c0 / (c0, c1) sums into out, one mod-down of 2 * cb polynomials added to them.  A chunk of one ciphertext takes the
// one-ciphertext kernels.
// Scratch: KsScratch of `chunk` ciphertexts | copy of the chunk's c0 [chunk][Ql][N] (plain; in place or bfv) resp. (c0, c1)
// [chunk][2][Ql][N] (weighted, in place) | pointer tables.
static void hoist_batched_core(Context &c, size_t size_Ql, const u64 *ct, size_t batch, const uint32_t *galois_elts, size_t n_elts,
                               const uint64_t *const *const *glk, const uint64_t *const *weights, int scheme, u64 *out, size_t chunk,
                               void *stream) {
    const bool weighted = weights != nullptr;
    const bool ntt_dom = ntt_domain_scheme(scheme);
    check_level(c, size_Ql, true);
    Tool &t = c.tool((uint32_t)size_Ql);
    hipStream_t s = as_stream(stream);
    const size_t n = c.n, ql_n = size_Ql * n, qlp_n = (size_t)t.size_qlp * n, ct_words = 2 * ql_n;
    const bool in_place = out == ct;
    if (!in_place && overlaps(out, batch * ct_words, ct, batch * ct_words))
        throw std::invalid_argument("out must be ct itself (in place) or must not overlap it");
    // every refusal before the first launch
    for (size_t e = 0; e < n_elts; e++) {
        check_galois_elt(c, galois_elts[e]);
        if (weighted && !weights[e]) throw std::invalid_argument("null weight");
    }
    for (size_t e = 0; e < n_elts; e++)
        if (!glk[e] && !(weighted && galois_elts[e] == 1)) throw std::logic_error("Galois key not present in hoisting");
    if (strict_mode()) {
        strict_operand(c, "hoisting ct", ct, rows_plain(0, size_Ql), (uint32_t)(2 * batch), ql_n, s);
        for (size_t e = 0; e < n_elts; e++) {
            if (glk[e]) strict_keys(c, "hoisting Galois key", glk[e], t.beta, (uint32_t)size_Ql, s);
            if (weighted) strict_operand(c, "hoisting weight", weights[e], rows_qlp(t.size_ql, c.size_q, c.size_p), 1, 0, s);
        }
    }
    if (!chunk) chunk = 8;
    chunk = std::min(std::min(chunk, batch), (size_t)65535 / std::max<size_t>(2, t.beta));
    // the elements in launch order: as given (plain); key-switched ones first, main-diagonal ones (element 1, no key) last (weighted)
    std::vector<const void *> tabs, keys, w_all;
    size_t n_ks = 0;
    for (int pass = 0; pass < (weighted ? 2 : 1); pass++)
        for (size_t e = 0; e < n_elts; e++) {
            const bool keyed = !weighted || galois_elts[e] != 1;
            if (weighted && keyed == (pass == 1)) continue;
            tabs.push_back(c.galois_table(galois_elts[e]));
            if (weighted) w_all.push_back(weights[e]);
            if (keyed) {
                keys.push_back(glk[e]);
                n_ks++;
            }
        }
    const size_t copy_polys = weighted ? (in_place ? 2 : 0) : ((in_place || !ntt_dom) ? 1 : 0);
    const size_t ks_words = KsScratch::words(c, t, chunk), copy_words = chunk * copy_polys * ql_n;
    u64 *base = c.scratch(stream, ks_words + copy_words + tabs.size() + w_all.size() + keys.size());
    const KsScratch k(base, c, t, chunk);
    u64 *cc = base + ks_words;
    PtrTable ptrs(cc + copy_words);
    const uint32_t *const *d_tabs = ptrs.add<const uint32_t *>(tabs);
    const u64 *const *d_w = weighted ? ptrs.add<const u64 *>(w_all) : nullptr;
    const u64 *const *const *d_keys = ptrs.add<const u64 *const *>(keys);
    ptrs.upload(s);
    // plain: acc_capacity / beta elements per launch.  Weighted: 63, whatever the primes: an element adds ONE reduced sum times a
    // weight, below 2^122 for the 61-bit primes the context accepts at most, so 63 of them fit (acc_capacity() / beta would split earlier)
    const size_t per_call = weighted ? 63 : std::max<size_t>(1, acc_capacity(c) / t.beta);

    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t cb = std::min(chunk, batch - b0);
        const u64 *in = ct + b0 * ct_words;
        u64 *o = out + b0 * ct_words;
        // what the sums over c0 (and c1) read once `o` is being written: the chunk itself, or its copy
        const u64 *src = in;
        size_t src_stride = ct_words;
        if (copy_polys == 2) {
            PHA_HIP(hipMemcpyAsync(cc, in, cb * ct_words * sizeof(u64), hipMemcpyDeviceToDevice, s));
            src = cc;
        } else if (copy_polys == 1) {
            if (cb == 1) PHA_HIP(hipMemcpyAsync(cc, in, ql_n * sizeof(u64), hipMemcpyDeviceToDevice, s));
            else PHA_HIP(hipMemcpy2DAsync(cc, ql_n * sizeof(u64), in, ct_words * sizeof(u64), ql_n * sizeof(u64), cb, hipMemcpyDeviceToDevice, s));
            src = cc;
            src_stride = ql_n;
        }
        if (n_ks) {
            modup(c, t, k.t_mod_up, in + ql_n, scheme, k.tmp, s, (uint32_t)cb, ct_words, nullptr, false);
            launch_hoist_inner_prod(c, t, k.cx, k.t_mod_up, d_keys, d_tabs, d_w, n_ks, per_call, cb, s);
        }
        if (ntt_dom) {
            launch_hoist_c_sums(c, size_Ql, o, src, src_stride, d_tabs, d_w, n_elts, n_ks, cb, s);
        } else {
            // coefficient-domain automorphism (src/galois.cu:20-39) of the chunk's dense c0 copy, one launch per element, and the adds
            PHA_HIP(hipMemsetAsync(o, 0, cb * ct_words * sizeof(u64), s));
            for (size_t e = 0; e < n_elts; e++) {
                launch_galois_coeff(c, k.tmp, cc, galois_elts[e], size_Ql, 0, cb, s);
                for (size_t b = 0; b < cb; b++) launch_add(c, o + b * ct_words, k.tmp + b * ql_n, o + b * ct_words, size_Ql, 0, s);
            }
        }
        if (n_ks) moddown_from_ntt(c, t, o, ql_n, k.cx, qlp_n, (uint32_t)(2 * cb), scheme, true, k.tmp, s);
    }
}

// ---- the fused baby-step kernel of the BSGS form for a batch of ciphertexts that share the baby keys, the tables and the weights
//      (pha_hoisting_weighted_bsgs_batched).  The thread program is pha_hoist_bsgs_batched.h (replayed on the CPU by tests/emu): one
//      thread owns one coefficient of one limb for NG giant-step accumulators of up to CB ciphertexts, blockIdx.z = group of CB
//      ciphertexts of the chunk. ----
static_assert(sizeof(BsgsBFp) == sizeof(FpInfo) && offsetof(BsgsBFp, qinv) == offsetof(FpInfo, qinv) &&
                  offsetof(BsgsBFp, ok) == offsetof(FpInfo, ok),
              "pha_hoist_bsgs_batched.h restates FpInfo");
template <int NG, int CB, int BETA>
__global__ __launch_bounds__(256) void hoist_bsgs_batched_kernel(const BsgsBArgs k) {
    hoist_bsgs_batched_thread<NG, CB, BETA>(k, blockIdx.x * 256 + threadIdx.x, blockIdx.y, blockIdx.z);
}

// ---- host side of the BSGS entries.  Block r (or ciphertext r) with weights w[i][j] gives out[r] = sum_i rot_{G_i}(sum_j w[i][j] (.)
//      rot_{B_j}(ct)).  The fused baby-step kernels treat the (unit, giant step) pairs as one list of accumulators, so the baby keys,
//      the gathered digits and the per-baby reductions are paid once for up to 16 of them; everything after them is batched over the
//      units.  Every unit's result is bit-identical to a call of its own. ----

// The plan of one API call (pha_hoist_plan.h): every refusal, then the strict-mode walk over n_ct ciphertexts, before the first launch
static BsgsPlan bsgs_plan(Context &c, Tool &t, const u64 *ct, size_t n_ct, const BsgsSteps &a, size_t lists, size_t units,
                          const char *unit_name, hipStream_t s) {
    BsgsPlan p(c.n, t.beta, acc_capacity(c), a, lists, units, unit_name, [&](uint32_t elt) { return c.galois_table(elt); });
    if (strict_mode()) {
        strict_operand(c, "hoisting ct", ct, rows_plain(0, t.size_ql), (uint32_t)(2 * n_ct), (size_t)t.size_ql * c.n, s);
        for (size_t j = 0; j < a.nb; j++)
            if (a.baby_glk[j]) strict_keys(c, "baby-step Galois key", a.baby_glk[j], t.beta, t.size_ql, s);
        for (size_t i = 0; i < a.ng; i++)
            if (a.giant_glk[i]) strict_keys(c, "giant-step Galois key", a.giant_glk[i], t.beta, t.size_ql, s);
        for (size_t i = 0; i < lists * a.nb; i++)
            if (a.weights[i]) strict_operand(c, "BSGS weight", a.weights[i], rows_qlp(t.size_ql, c.size_q, c.size_p), 1, 0, s);
    }
    return p;
}

// One API call on the device: the call's one scratch claim -- `units` row blocks of one ciphertext (cts = 1) or a chunk of `units`
// ciphertexts (cts = units) -- with the plan's tables uploaded into its pointer region.
struct BsgsCall {
    Context &c;
    Tool &t;
    const BsgsPlan &p;
    const int scheme;
    const hipStream_t s;
    const size_t n, ql_n, qlp_n;
    const BsgsScratch::Dims dims;
    const BsgsScratch m;
    const uint32_t *const *d_btab, *const *d_gtab, *d_rank;
    const u64 *const *const *d_bkeys, *const *const *d_gkeys;
    const u64 *const *d_w;

    BsgsCall(Context &c_, Tool &t_, const BsgsPlan &p_, size_t units, size_t cts, int scheme_, void *stream)
        : c(c_), t(t_), p(p_), scheme(scheme_), s(as_stream(stream)), n(c_.n), ql_n((size_t)t_.size_ql * n), qlp_n((size_t)t_.size_qlp * n),
          dims{ql_n, qlp_n, t_.beta, units, cts, p_.nb, p_.ng, p_.nk, p_.lists, p_.any_null},
          m(c_.scratch(stream, BsgsScratch::words(dims)), dims) {
        std::vector<const void *> w = p.weights;
        if (p.any_null) {   // missing weights point at a zero plane
            PHA_HIP(hipMemsetAsync(m.zero, 0, qlp_n * sizeof(u64), s));
            for (auto &x : w)
                if (!x) x = m.zero;
        }
        PtrTable ptrs(m.ptrs);
        d_btab = ptrs.add<const uint32_t *>(p.btab);
        d_bkeys = ptrs.add<const u64 *const *>(p.bkeys);
        d_w = ptrs.add<const u64 *>(w);
        d_gtab = ptrs.add<const uint32_t *>(p.gtab);
        d_gkeys = ptrs.add<const u64 *const *>(p.gkeys);
        d_rank = ptrs.add(p.rank);
        if (ptrs.words() > BsgsScratch::ptr_words(dims)) throw std::logic_error("BSGS pointer tables do not fit their region");
        ptrs.upload(s);
    }
};

// Baby steps of `cts` ciphertexts at `in`: one mod-up of their c1 polynomials (the digits' own limbs copied -- the gather reads them
// through the permutation), then every accumulator list's weighted sum of the hoisted inner products (and of the c0 / c1 terms,
// pre-multiplied by P) into acc, in one pass over the baby keys per NG lists: the one-ciphertext kernel over the plan's lists (the
// (row block, giant step) pairs), or the batched kernel over groups of CB ciphertexts with ng lists each (pha_hoist_bsgs_batched.h).
static void bsgs_baby_steps(const BsgsCall &b, const u64 *in, size_t cts) {
    Context &c = b.c;
    Tool &t = b.t;
    const BsgsPlan &p = b.p;
    const size_t n = b.n;
    if (p.nbk) modup(c, t, b.m.t_mod_up, in + b.ql_n, b.scheme, b.m.tmp, b.s, (uint32_t)cts, 2 * b.ql_n, nullptr, false);
    BsgsArgs k{};     // the one-ciphertext kernel's arguments and the batched kernel's: the same fields, the batch's on top
    BsgsBArgs kb{};
    auto fill = [&](auto &x) {
        x.acc = b.m.acc; x.t_mod_up = b.m.t_mod_up; x.keys = b.d_bkeys; x.tables = b.d_btab; x.weights = b.d_w; x.mod = c.d_mod.p;
        x.qlp_prime = t.d_qlp_prime.p; x.n = (uint32_t)n; x.beta = t.beta; x.nb = (uint32_t)p.nb; x.qlp_n = b.qlp_n;
        x.qp_n = (size_t)c.size_qp * n; x.cc = in; x.p_mod_q = t.p_mod_q2.p; x.ql = t.size_ql; x.ql_n = b.ql_n;
    };
    fill(k);
    fill(kb);
    k.fpinfo = c.d_fpinfo.p;
    kb.fpinfo = reinterpret_cast<const BsgsBFp *>(c.d_fpinfo.p);
    kb.g_total = (uint32_t)p.lists; kb.cc_stride = 2 * b.ql_n; kb.n_ct = (uint32_t)cts;
    // NG lists per launch, from list g0 on: launch(BETA, NG) issues one kernel
    auto ladder = [&](auto &&launch) {
        for (size_t g0 = 0; g0 < p.lists;) {
            k.g0 = kb.g0 = (uint32_t)g0;
            with_beta<4>(t.beta, [&](auto Bt) {   // (beta <= 4: the plan refuses anything else)
                g0 += with_ng(p.lists - g0, [&](auto Ng) { launch(Bt, Ng); });
            });
            check_launch();
        }
    };
    if (cts == 1)
        ladder([&](auto Bt, auto Ng) {
            constexpr int BETA = decltype(Bt)::value, NG = decltype(Ng)::value;
            hipLaunchKernelGGL((hoist_bsgs_inner_prod_kernel<NG, BETA>), dim3((unsigned)(n / 256), t.size_qlp), dim3(256), 0, b.s, k);
        });
    else
        ladder([&](auto Bt, auto Ng) {
            constexpr int BETA = decltype(Bt)::value, NG = decltype(Ng)::value, CB = hoist_bsgs_batched_cb(BETA, NG);
            hipLaunchKernelGGL((hoist_bsgs_batched_kernel<NG, CB, BETA>),
                               dim3((unsigned)(n / 256), t.size_qlp, (unsigned)((cts + CB - 1) / CB)), dim3(256), 0, b.s, kb);
        });
}

// Giant steps of `units` row blocks or ciphertexts, ng accumulator lists each: B = moddown(acc) in one batched launch set, the
// permutations (every unit in one launch: the first write to `out`), then per unit ONE mod-down for the sum of its key-switch inner
// products, added to out.
static void bsgs_giant_side(const BsgsCall &b, size_t units, u64 *out) {
    Context &c = b.c;
    Tool &t = b.t;
    const BsgsPlan &p = b.p;
    const BsgsScratch &m = b.m;
    const size_t n = b.n;
    moddown_from_ntt(c, t, m.B, b.ql_n, m.acc, b.qlp_n, (uint32_t)(2 * p.ng * units), b.scheme, false, m.tmp, b.s);
    hipLaunchKernelGGL(bsgs_combine_kernel, dim3((unsigned)(n / 256), t.size_ql, (unsigned)units), dim3(256), 0, b.s, out, m.g1, m.B, b.d_gtab,
                       b.d_rank, (uint32_t)p.ng, (uint32_t)p.nk, c.d_mod.p, (uint32_t)n, b.ql_n);
    check_launch();
    if (p.nk) {
        modup(c, t, m.mu_g, m.g1, b.scheme, m.tmp, b.s, (uint32_t)(units * p.nk));
        MultiInnerArgs k{m.cx, m.mu_g, b.d_gkeys, c.d_mod.p, t.d_qlp_prime.p, (uint32_t)n, t.beta, (uint32_t)p.nk, b.qlp_n, (size_t)c.size_qp * n};
        hipLaunchKernelGGL(inner_prod_multi_kernel, dim3((unsigned)(n / 512), t.size_qlp, (unsigned)units), dim3(256), 0, b.s, k);
        check_launch();
        moddown_from_ntt(c, t, out, b.ql_n, m.cx, b.qlp_n, (uint32_t)(2 * units), b.scheme, true, m.tmp, b.s);
    }
}

// pha_hoisting_weighted_bsgs (one block, in place) and ..._blocks: `blocks` row blocks that share the input ciphertext and every Galois
// key, blocks * ng accumulator lists on the one-ciphertext kernel
static void bsgs_blocks(Context &c, size_t size_Ql, const u64 *ct, size_t blocks, const BsgsSteps &a, u64 *out, int scheme, void *stream) {
    Tool &t = c.tool((uint32_t)size_Ql);
    const BsgsPlan p = bsgs_plan(c, t, ct, 1, a, blocks * a.ng, blocks, "row blocks", as_stream(stream));
    const BsgsCall b(c, t, p, blocks, 1, scheme, stream);
    bsgs_baby_steps(b, ct, 1);
    bsgs_giant_side(b, blocks, out);
}

// pha_hoisting_weighted_bsgs_batched: `batch` ciphertexts that share every key, table and weight, `chunk` of them per set of launches
// (scratch per call: BsgsScratch of `chunk` ciphertexts).  A chunk of one ciphertext -- chunk = 1, or a tail of one -- takes the
// one-ciphertext baby-step kernel.
static void bsgs_batched(Context &c, size_t size_Ql, const u64 *ct, size_t batch, const BsgsSteps &a, int scheme, u64 *out, size_t chunk,
                         void *stream) {
    Tool &t = c.tool((uint32_t)size_Ql);
    const size_t ct_words = 2 * size_Ql * c.n;
    const BsgsPlan p = bsgs_plan(c, t, ct, batch, a, a.ng, 1, "giant steps", as_stream(stream));
    if (!chunk) chunk = 4;
    chunk = std::min(std::min(chunk, batch), std::min((size_t)65535 / (2 * a.ng), (size_t)65535 / std::max<size_t>(1, p.nk * t.beta)));
    const BsgsCall b(c, t, p, chunk, chunk, scheme, stream);
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t cb = std::min(chunk, batch - b0);
        bsgs_baby_steps(b, ct + b0 * ct_words, cb);
        bsgs_giant_side(b, cb, out + b0 * ct_words);
    }
}

}  // namespace pha

using namespace pha;

extern "C" {

int pha_hoisting(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint32_t *galois_elts, size_t n_elts,
                 const uint64_t *const *const *glk, int scheme, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(galois_elts); need(glk);
    if (n_elts == 0) throw std::invalid_argument("steps must not be empty");
    hoist_batched_core(ctx->c, size_Ql, ct, 1, galois_elts, n_elts, glk, nullptr, scheme, ct, 1, stream);
    PHA_API_END
}

int pha_hoisting_weighted(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint32_t *galois_elts, size_t n_elts,
                          const uint64_t *const *const *glk, const uint64_t *const *weights, int scheme, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(galois_elts); need(glk); need(weights);
    if (n_elts == 0) throw std::invalid_argument("steps must not be empty");
    if (!ntt_domain_scheme(scheme)) throw std::invalid_argument("weighted hoisting takes NTT-form ciphertexts (ckks / bgv)");
    hoist_batched_core(ctx->c, size_Ql, ct, 1, galois_elts, n_elts, glk, weights, scheme, ct, 1, stream);
    PHA_API_END
}

int pha_hoisting_weighted_bsgs(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint32_t *baby_elts, size_t n_baby,
                               const uint64_t *const *const *baby_glk, const uint32_t *giant_elts, size_t n_giant,
                               const uint64_t *const *const *giant_glk, const uint64_t *const *weights, int scheme, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(baby_elts); need(baby_glk); need(giant_elts); need(giant_glk); need(weights);
    if (n_baby == 0 || n_giant == 0) throw std::invalid_argument("steps must not be empty");
    if (!ntt_domain_scheme(scheme)) throw std::invalid_argument("weighted hoisting takes NTT-form ciphertexts (ckks / bgv)");
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    bsgs_blocks(c, size_Ql, ct, 1, {baby_elts, n_baby, baby_glk, giant_elts, n_giant, giant_glk, weights}, ct, scheme, stream);
    PHA_API_END
}

int pha_hoisting_weighted_bsgs_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t batch, const uint32_t *baby_elts,
                                       size_t n_baby, const uint64_t *const *const *baby_glk, const uint32_t *giant_elts, size_t n_giant,
                                       const uint64_t *const *const *giant_glk, const uint64_t *const *weights, int scheme, uint64_t *out,
                                       size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(baby_elts); need(baby_glk); need(giant_elts); need(giant_glk); need(weights); need(out);
    if (n_baby == 0 || n_giant == 0) throw std::invalid_argument("steps must not be empty");
    if (!ntt_domain_scheme(scheme)) throw std::invalid_argument("weighted hoisting takes NTT-form ciphertexts (ckks / bgv)");
    if (batch == 0) return 0;
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    const size_t words = batch * 2 * size_Ql * c.n;
    if (out != ct && overlaps(out, words, ct, words)) throw std::invalid_argument("out must be ct itself (in place) or must not overlap it");
    bsgs_batched(c, size_Ql, ct, batch, {baby_elts, n_baby, baby_glk, giant_elts, n_giant, giant_glk, weights}, scheme, out, chunk, stream);
    PHA_API_END
}

int pha_hoisting_weighted_bsgs_blocks(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t n_blocks, const uint32_t *baby_elts,
                                      size_t n_baby, const uint64_t *const *const *baby_glk, const uint32_t *giant_elts, size_t n_giant,
                                      const uint64_t *const *const *giant_glk, const uint64_t *const *weights, uint64_t *out, int scheme,
                                      void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(baby_elts); need(baby_glk); need(giant_elts); need(giant_glk); need(weights); need(out);
    if (n_blocks == 0) return 0;
    if (n_baby == 0 || n_giant == 0) throw std::invalid_argument("steps must not be empty");
    if (!ntt_domain_scheme(scheme)) throw std::invalid_argument("weighted hoisting takes NTT-form ciphertexts (ckks / bgv)");
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    const size_t ql_n = size_Ql * c.n;
    if (overlaps(out, n_blocks * 2 * ql_n, ct, 2 * ql_n)) throw std::invalid_argument("out must not overlap ct");
    bsgs_blocks(c, size_Ql, ct, n_blocks, {baby_elts, n_baby, baby_glk, giant_elts, n_giant, giant_glk, weights}, out, scheme, stream);
    PHA_API_END
}

int pha_hoisting_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t batch, const uint32_t *galois_elts, size_t n_elts,
                         const uint64_t *const *const *glk, int scheme, uint64_t *out, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(galois_elts); need(glk); need(out);
    if (n_elts == 0) throw std::invalid_argument("steps must not be empty");
    if (batch == 0) return 0;
    hoist_batched_core(ctx->c, size_Ql, ct, batch, galois_elts, n_elts, glk, nullptr, scheme, out, chunk, stream);
    PHA_API_END
}

int pha_hoisting_weighted_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t batch, const uint32_t *galois_elts,
                                  size_t n_elts, const uint64_t *const *const *glk, const uint64_t *const *weights, int scheme,
                                  uint64_t *out, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(galois_elts); need(glk); need(weights); need(out);
    if (n_elts == 0) throw std::invalid_argument("steps must not be empty");
    if (!ntt_domain_scheme(scheme)) throw std::invalid_argument("weighted hoisting takes NTT-form ciphertexts (ckks / bgv)");
    if (batch == 0) return 0;
    hoist_batched_core(ctx->c, size_Ql, ct, batch, galois_elts, n_elts, glk, weights, scheme, out, chunk, stream);
    PHA_API_END
}

}  // extern "C"
