// pha_hoist_bsgs_batched.h -- the per-thread program of hoist_bsgs_batched_kernel (pha_hoist.hip): the fused baby-step kernel of the
// baby-step / giant-step hoisted rotations for a group of up to CB ciphertexts that share the baby keys, the permutation tables and
// the weights (pha_hoisting_weighted_bsgs_batched).  Host/device functions like pha_hoist_batched.h, from "which words does this
// thread load" to "which words does it store", so that tests/emu/emu_hoist_bsgs_batched.cpp replays the very source the kernel runs
// on ordinary host arrays (test-only; the product never executes it on the host).  It needs pha_arith.h alone and declares the few
// plain structs it takes itself.
//
// One thread = one coefficient of one limb of [Q_l || P] for NG giant-step accumulators [g0, g0 + NG) of each of the ciphertexts
// [group * CB, min((group + 1) * CB, n_ct)) of the launch.  The two bodies are those of hoist_bsgs_body_fp / hoist_bsgs_body_int
// (pha_hoist.hip) with one more index, and give every ciphertext the words the one-ciphertext kernel gives it:
//   FP body       limbs whose prime is below 2^50: 2 NG CB doubles, re-centred every 8 baby steps.  Magnitudes are per ciphertext
//                 and those stated at hoist_bsgs_body_fp: BETA + 1 digit products below 4.4 q, s and t re-centred (<= q / 2), a
//                 weighted term below 0.69 q, 0.5 + 8 x 0.69 = 6.0 q < 8 q = 2^53 between two re-centrings.
//   integer body  the other limbs: 128-bit sums, 4 NG CB words.  A thread holds at most 8 (giant step, ciphertext) sets at a time
//                 and walks the baby steps once per 8 of them, as the one-ciphertext kernel does for NG = 16.  Per sum: one s * w
//                 product per baby ENTRY, each below q_max^2 -- the driver admits nb + 1 <= floor(2^128 / q_max^2) - 1.
// Loads of a baby step: ONCE the next permutation entry, the 2 BETA key words and the NG weight words; per ciphertext the BETA
// gathered digit words and the c0 word (an identity step: the c0 and c1 words).  All of them are issued before the step's first
// multiply.  A ciphertext the last group does not have issues no load and no store.  Missing weights point at a zero plane.
//
// Words loaded per (limb, coefficient, keyed baby step, ciphertext) of a full group over G giant steps (derived from this source, not
// counted):  ceil(G / NG) (2 BETA + NG + CB (BETA + 1)) / CB, against ceil(G / NG) (3 BETA + NG + 1) of the one-ciphertext kernel.
#pragma once
#include "pha_arith.h"

namespace pha {

// per-prime constants of the FP64 path (the layout of the context's table)
struct BsgsBFp {
    double q, qinv;
    uint32_t ok, pad;
};

struct BsgsBArgs {
    u64 *acc;                         // [n_ct][g_total][2][QlP][N]
    const u64 *t_mod_up;              // [n_ct][beta][QlP][N]
    const u64 *const *const *keys;    // [nb]: key table of baby j ([beta] keys [2][QP][N]), null for the identity
    const uint32_t *const *tables;    // [nb]: NTT-domain permutation of baby j
    const u64 *const *weights;        // [g_total][nb]: w_ij over [QlP][N] (a zero plane where there is no such term)
    const DModulus *mod;              // [prime]
    const uint32_t *qlp_prime;        // limb of [Q_l || P] -> prime
    uint32_t n, beta, nb, g0;         // g0: first giant step of this launch
    uint32_t g_total, n_ct;           // giant steps per ciphertext (accumulator stride), ciphertexts of the launch
    size_t qlp_n, qp_n;
    const u64 *cc;                    // the input ciphertexts (c0, c1): ciphertext b at cc + b * cc_stride, [2][Ql][N]
    size_t cc_stride;
    const u64x2 *p_mod_q;             // [Ql] P mod q_j with its Shoup quotient
    uint32_t ql;
    size_t ql_n;
    const BsgsBFp *fpinfo;            // [prime]: limbs below 2^50 accumulate in doubles; null: every limb takes the integer body
};

// Ciphertexts per thread for each instantiation the library launches: at most 16 FP accumulator sets per thread, whatever the digit
// count.  No candidate spills to scratch memory (compiler report); 32 sets (NG = 8 with CB = 4, NG = 16 with CB = 2) halve the
// occupancy and measured slower than 16 (profiles/bsgs_batched.md)
constexpr int hoist_bsgs_batched_cb(int beta, int ng) { return (void)beta, ng >= 16 ? 1 : ng >= 8 ? 2 : 4; }

// FP64 limbs.  coeff: coefficient of the limb, nid: limb of [Q_l || P], twr: its prime, first / cnt: the group's ciphertexts
template <int NG, int CB, int BETA>
PHA_HD void hoist_bsgs_batched_fp(const BsgsBArgs &k, uint32_t coeff, uint32_t nid, uint32_t twr, uint32_t first, uint32_t cnt,
                                  const BsgsBFp fi) {
    const FpMod fm{fi.q, fi.qinv, false, false};
    const size_t out_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    const bool data_limb = nid < k.ql;          // uniform
    const double pqd = data_limb ? fp_from_canon(k.p_mod_q[nid].x) : 0.0;
    const u64 *cc0 = k.cc + (size_t)first * k.cc_stride + (size_t)(data_limb ? nid : 0) * k.n;   // (P limbs: any valid row)
    const u64 *row = k.t_mod_up + (size_t)first * k.beta * k.qlp_n + (size_t)nid * k.n;
    double al[CB][NG], bl[CB][NG];
#pragma unroll
    for (int c = 0; c < CB; c++)
#pragma unroll
        for (int g = 0; g < NG; g++) al[c][g] = bl[c][g] = 0.0;
    uint32_t idx = k.tables[0][coeff];
    for (uint32_t j = 0; j < k.nb; j++) {
        const u64 *const *keys = k.keys[j];
        const uint32_t idx_next = k.tables[j + 1 < k.nb ? j + 1 : j][coeff];
        // loads first
        u64 wv[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) wv[g] = k.weights[(size_t)(k.g0 + g) * k.nb + j][out_id];
        u64 x0[CB] = {};
#pragma unroll
        for (int c = 0; c < CB; c++)
            if ((uint32_t)c < cnt) x0[c] = cc0[(size_t)c * k.cc_stride + idx];
        double s[CB] = {}, t[CB] = {};
        if (keys) {   // uniform
            u64 kb[BETA], ka[BETA];
            u64 v[CB][BETA] = {};
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                const u64 *key = keys[i];
                kb[i] = key[evk_id];
                ka[i] = key[evk_id + k.qp_n];
            }
#pragma unroll
            for (int c = 0; c < CB; c++)
                if ((uint32_t)c < cnt) {
#pragma unroll
                    for (int i = 0; i < BETA; i++) v[c][i] = row[(size_t)(c * BETA + i) * k.qlp_n + idx];
                }
#pragma unroll
            for (int c = 0; c < CB; c++)
                if ((uint32_t)c < cnt) {
                    s[c] = data_limb ? fp_mulmod_light(fp_from_canon(x0[c]), pqd, fm) : 0.0;   // + P * rot_j(c0)
                    t[c] = 0.0;
#pragma unroll
                    for (int i = 0; i < BETA; i++) {
                        const double vd = fp_from_canon(v[c][i]);
                        s[c] += fp_mulmod_light(vd, fp_from_canon(kb[i]), fm);
                        t[c] += fp_mulmod_light(vd, fp_from_canon(ka[i]), fm);
                    }
                }
        } else {      // identity baby step: (P c0, P c1) on the data limbs, nothing on the P limbs
            u64 x1[CB] = {};
#pragma unroll
            for (int c = 0; c < CB; c++)
                if ((uint32_t)c < cnt && data_limb) x1[c] = cc0[(size_t)c * k.cc_stride + k.ql_n + idx];
#pragma unroll
            for (int c = 0; c < CB; c++)
                if ((uint32_t)c < cnt) {
                    s[c] = data_limb ? fp_mulmod_light(fp_from_canon(x0[c]), pqd, fm) : 0.0;
                    t[c] = data_limb ? fp_mulmod_light(fp_from_canon(x1[c]), pqd, fm) : 0.0;
                }
        }
#pragma unroll
        for (int c = 0; c < CB; c++)
            if ((uint32_t)c < cnt) {
                const double sc = fp_reduce(s[c], fm), tc = fp_reduce(t[c], fm);
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    const double wd = fp_from_canon(wv[g]);
                    al[c][g] += fp_mulmod_light(sc, wd, fm);
                    bl[c][g] += fp_mulmod_light(tc, wd, fm);
                }
                if ((j & 7u) == 7u) {   // (uniform)
#pragma unroll
                    for (int g = 0; g < NG; g++) {
                        al[c][g] = fp_reduce(al[c][g], fm);
                        bl[c][g] = fp_reduce(bl[c][g], fm);
                    }
                }
            }
        idx = idx_next;
    }
#pragma unroll
    for (int c = 0; c < CB; c++)
        if ((uint32_t)c < cnt) {
#pragma unroll
            for (int g = 0; g < NG; g++) {
                u64 *acc = k.acc + ((size_t)(first + c) * k.g_total + k.g0 + g) * 2 * k.qlp_n + out_id;
                acc[0] = fp_to_canon(al[c][g], fm);
                acc[k.qlp_n] = fp_to_canon(bl[c][g], fm);
            }
        }
}

// integer limbs: accumulators [goff, goff + NG) of the launch for the ciphertexts [first, first + cnt), cnt <= CB
template <int NG, int CB, int BETA>
PHA_HD void hoist_bsgs_batched_int(const BsgsBArgs &k, uint32_t coeff, uint32_t nid, uint32_t twr, uint32_t first, uint32_t cnt,
                                   uint32_t goff) {
    const DModulus m = k.mod[twr];
    const size_t out_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    const bool data_limb = nid < k.ql;          // uniform
    const u64x2 pq = data_limb ? k.p_mod_q[nid] : u64x2{0, 0};
    const u64 *cc0 = k.cc + (size_t)first * k.cc_stride + (size_t)(data_limb ? nid : 0) * k.n;   // (P limbs: any valid row)
    const u64 *row = k.t_mod_up + (size_t)first * k.beta * k.qlp_n + (size_t)nid * k.n;
    u64 al[CB][NG], ah[CB][NG], bl[CB][NG], bh[CB][NG];
#pragma unroll
    for (int c = 0; c < CB; c++)
#pragma unroll
        for (int g = 0; g < NG; g++) al[c][g] = ah[c][g] = bl[c][g] = bh[c][g] = 0;
    uint32_t idx = k.tables[0][coeff];
    for (uint32_t j = 0; j < k.nb; j++) {
        const u64 *const *keys = k.keys[j];
        const uint32_t idx_next = k.tables[j + 1 < k.nb ? j + 1 : j][coeff];
        // loads first
        u64 wv[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) wv[g] = k.weights[(size_t)(k.g0 + goff + g) * k.nb + j][out_id];
        u64 x0[CB] = {};
#pragma unroll
        for (int c = 0; c < CB; c++)
            if ((uint32_t)c < cnt) x0[c] = cc0[(size_t)c * k.cc_stride + idx];
        u64 s[CB] = {}, t[CB] = {};
        if (keys) {   // uniform
            u64 kb[BETA], ka[BETA];
            u64 v[CB][BETA] = {};
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                const u64 *key = keys[i];
                kb[i] = key[evk_id];
                ka[i] = key[evk_id + k.qp_n];
            }
#pragma unroll
            for (int c = 0; c < CB; c++)
                if ((uint32_t)c < cnt) {
#pragma unroll
                    for (int i = 0; i < BETA; i++) v[c][i] = row[(size_t)(c * BETA + i) * k.qlp_n + idx];
                }
#pragma unroll
            for (int c = 0; c < CB; c++)
                if ((uint32_t)c < cnt) {
                    u64 sl = 0, sh = 0, tl = 0, th = 0;
#pragma unroll
                    for (int i = 0; i < BETA; i++) {
                        mac128(v[c][i], kb[i], sl, sh);
                        mac128(v[c][i], ka[i], tl, th);
                    }
                    s[c] = barrett128(sl, sh, m);
                    t[c] = barrett128(tl, th, m);
                    if (data_limb) s[c] = add_mod(s[c], shoup(x0[c], pq, m.value), m.value);          // + P * rot_j(c0)
                }
        } else {      // identity baby step: (P c0, P c1) on the data limbs, nothing on the P limbs
            u64 x1[CB] = {};
#pragma unroll
            for (int c = 0; c < CB; c++)
                if ((uint32_t)c < cnt && data_limb) x1[c] = cc0[(size_t)c * k.cc_stride + k.ql_n + idx];
#pragma unroll
            for (int c = 0; c < CB; c++)
                if ((uint32_t)c < cnt) {
                    s[c] = data_limb ? shoup(x0[c], pq, m.value) : 0;
                    t[c] = data_limb ? shoup(x1[c], pq, m.value) : 0;
                }
        }
#pragma unroll
        for (int c = 0; c < CB; c++)
            if ((uint32_t)c < cnt) {
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    mac128(s[c], wv[g], al[c][g], ah[c][g]);
                    mac128(t[c], wv[g], bl[c][g], bh[c][g]);
                }
            }
        idx = idx_next;
    }
#pragma unroll
    for (int c = 0; c < CB; c++)
        if ((uint32_t)c < cnt) {
#pragma unroll
            for (int g = 0; g < NG; g++) {
                u64 *acc = k.acc + ((size_t)(first + c) * k.g_total + k.g0 + goff + g) * 2 * k.qlp_n + out_id;
                acc[0] = barrett128(al[c][g], ah[c][g], m);
                acc[k.qlp_n] = barrett128(bl[c][g], bh[c][g], m);
            }
        }
}

// coeff: coefficient of the limb (blockIdx.x * 256 + threadIdx.x), nid: limb of [Q_l || P] (blockIdx.y), group: blockIdx.z
template <int NG, int CB, int BETA>
PHA_HD void hoist_bsgs_batched_thread(const BsgsBArgs &k, uint32_t coeff, uint32_t nid, uint32_t group) {
    const uint32_t twr = k.qlp_prime[nid];
    const uint32_t first = group * CB;
    const uint32_t cnt = k.n_ct - first < (uint32_t)CB ? k.n_ct - first : (uint32_t)CB;   // (uniform) ciphertexts this group has
    if (k.fpinfo) {   // (uniform) FP64 limbs
        const BsgsBFp fi = k.fpinfo[twr];
        if (fi.ok) {
            hoist_bsgs_batched_fp<NG, CB, BETA>(k, coeff, nid, twr, first, cnt, fi);
            return;
        }
    }
    // at most 8 sets of 128-bit sums per walk over the baby steps: NGI giant steps x CBI ciphertexts
    constexpr int NGI = NG > 8 ? 8 : NG;
    constexpr int CBI = 8 / NGI < CB ? 8 / NGI : CB;
    for (uint32_t coff = 0; coff < cnt; coff += CBI) {
        const uint32_t sub = cnt - coff < (uint32_t)CBI ? cnt - coff : (uint32_t)CBI;
        for (uint32_t goff = 0; goff < (uint32_t)NG; goff += NGI) hoist_bsgs_batched_int<NGI, CBI, BETA>(k, coeff, nid, twr, first + coff, sub, goff);
    }
}

}  // namespace pha
