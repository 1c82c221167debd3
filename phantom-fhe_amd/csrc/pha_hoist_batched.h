// pha_hoist_batched.h -- the per-thread program of hoist_inner_prod_batched_kernel (pha_hoist.hip): the gather + inner product of the
// hoisted rotations for a group of up to CB ciphertexts that share the Galois keys, the permutation tables and (weighted form) the
// plaintext weights.  Host/device functions like pha_arith.h and pha_plain_sum.h, from "which words does this thread load" to "which
// words does it store", so that tests/emu/emu_hoist_batched.cpp replays the very source the kernel runs on ordinary host arrays
// (test-only; the product never executes it on the host).
//
// One thread = two adjacent coefficients of one limb of [Q_l || P] for the ciphertexts [group * CB, min((group + 1) * CB, n_ct)) of
// the launch: CB KeyAcc sets (four 128-bit sums each).  Per Galois element it loads ONCE the permutation pair, the 4 x BETA key
// words and (weighted) the weight pair, then gathers 2 x BETA digit words per ciphertext; every load of an element is issued before
// its first multiply (BETA > 0).  A ciphertext the last group does not have issues no load and no store.
//
// Words moved per (limb, coefficient, keyed element), G = ciphertexts per group:  G * beta gathered digit words + 2 * beta key words
// (+ 1 weight word): per ciphertext beta + 2 beta / G (+ 1 / G), against 3 beta (+ 1) of the one-ciphertext kernel.
//
// Accumulator bounds are per ciphertext and those of hoist_inner_prod_kernel: every product is of two canonical residues, below
// q_max^2, and a 128-bit sum holds floor(2^128 / q_max^2) - 1 of them on top of a seed below q_max.  Plain form: n_elts * beta
// products per sum and launch (the driver launches acc_capacity / beta elements at a time; `accumulate` seeds a later launch from
// cx).  Weighted form: an element's beta digit products go to a fresh sum, are reduced (Barrett) and enter the running sum as ONE
// product with the weight: n_elts products per launch (the driver launches 63 at a time).
#pragma once
#include "pha_arith.h"

namespace pha {

struct alignas(8) u32x2 {
    uint32_t x, y;
};

struct HoistBArgs {
    u64 *cx;                          // [n_ct][2][QlP][N]
    const u64 *t_mod_up;              // [n_ct][beta][QlP][N]
    const u64 *const *const *keys;    // array [n_elts] of arrays [beta] of keys [2][QP][N]
    const uint32_t *const *tables;    // array [n_elts] of NTT-domain permutation tables [N]
    const u64 *const *weights;        // weighted form: array [n_elts] of weights [QlP][N] (NTT form)
    const DModulus *mod;              // [prime]
    const uint32_t *qlp_prime;        // limb of [Q_l || P] -> prime
    uint32_t n, beta, n_elts, accumulate;  // accumulate: add to what cx already holds (split calls)
    uint32_t n_ct;                    // ciphertexts of the launch
    size_t qlp_n, qp_n;
};

// Ciphertexts per thread for each instantiation the library launches (BETA = 0: the run-time digit loop), chosen from the compiler's
// resource report so that nothing spills to scratch memory (profiles/hoisting_batched.md)
constexpr int hoist_batched_cb(int beta, bool weighted) { return weighted && beta == 4 ? 2 : 4; }

PHA_HD u64x2 hb_ld2(const u64 *p) { return *reinterpret_cast<const u64x2 *>(p); }
PHA_HD void hb_st2(u64 *p, u64x2 v) { *reinterpret_cast<u64x2 *>(p) = v; }

// pair: which coefficient pair of the limb (blockIdx.x * 256 + threadIdx.x), nid: limb of [Q_l || P], group: blockIdx.z
template <int BETA, int CB, bool WEIGHTED>
PHA_HD void hoist_batched_thread(const HoistBArgs &k, uint32_t pair, uint32_t nid, uint32_t group) {
    const uint32_t twr = k.qlp_prime[nid];
    const DModulus m = k.mod[twr];
    const size_t coeff = (size_t)pair * 2;
    const size_t out_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    const uint32_t first = group * CB;
    const uint32_t cnt = k.n_ct - first < (uint32_t)CB ? k.n_ct - first : (uint32_t)CB;   // (uniform) ciphertexts this group has
    // digit i of the group's ciphertext j: row + (j * beta + i) * qlp_n; its sums: cx + j * 2 * qlp_n (+ qlp_n)
    const u64 *row = k.t_mod_up + (size_t)first * k.beta * k.qlp_n + (size_t)nid * k.n;
    u64 *cx = k.cx + (size_t)first * 2 * k.qlp_n + out_id;
    KeyAcc acc[CB];
    if (k.accumulate) {
#pragma unroll
        for (int j = 0; j < CB; j++)
            if ((uint32_t)j < cnt) acc[j].seed(hb_ld2(cx + (size_t)j * 2 * k.qlp_n), hb_ld2(cx + (size_t)j * 2 * k.qlp_n + k.qlp_n));
    }
    u32x2 idx = *reinterpret_cast<const u32x2 *>(k.tables[0] + coeff);
    for (uint32_t e = 0; e < k.n_elts; e++) {
        const u32x2 idx_next = *reinterpret_cast<const u32x2 *>(k.tables[e + 1 < k.n_elts ? e + 1 : e] + coeff);
        const u64 *const *keys = k.keys[e];
        u64x2 w{};
        if constexpr (WEIGHTED) w = hb_ld2(k.weights[e] + out_id);
        if constexpr (BETA > 0) {
            u64x2 kb[BETA], ka[BETA];
            u64 v0[CB][BETA] = {}, v1[CB][BETA] = {};
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                const u64 *key = keys[i];
                kb[i] = hb_ld2(key + evk_id);
                ka[i] = hb_ld2(key + evk_id + k.qp_n);
            }
#pragma unroll
            for (int j = 0; j < CB; j++)
                if ((uint32_t)j < cnt) {
#pragma unroll
                    for (int i = 0; i < BETA; i++) {
                        const u64 *digit = row + (size_t)(j * BETA + i) * k.qlp_n;
                        v0[j][i] = digit[idx.x];
                        v1[j][i] = digit[idx.y];
                    }
                }
#pragma unroll
            for (int j = 0; j < CB; j++)
                if ((uint32_t)j < cnt) {
                    KeyAcc part;
                    KeyAcc &sums = WEIGHTED ? part : acc[j];   // where this element's digit sums go
#pragma unroll
                    for (int i = 0; i < BETA; i++) sums.mac(v0[j][i], v1[j][i], kb[i], ka[i]);
                    if constexpr (WEIGHTED) {
                        u64x2 s, t;
                        part.reduce(m, s, t);
                        acc[j].mac_weighted(s, t, w);
                    }
                }
        } else {
            KeyAcc part[CB];
            for (uint32_t i = 0; i < k.beta; i++) {
                const u64 *key = keys[i];
                const u64x2 kb = hb_ld2(key + evk_id), ka = hb_ld2(key + evk_id + k.qp_n);
                u64 v0[CB] = {}, v1[CB] = {};
#pragma unroll
                for (int j = 0; j < CB; j++)
                    if ((uint32_t)j < cnt) {
                        const u64 *digit = row + ((size_t)j * k.beta + i) * k.qlp_n;
                        v0[j] = digit[idx.x];
                        v1[j] = digit[idx.y];
                    }
#pragma unroll
                for (int j = 0; j < CB; j++)
                    if ((uint32_t)j < cnt) (WEIGHTED ? part[j] : acc[j]).mac(v0[j], v1[j], kb, ka);
            }
            if constexpr (WEIGHTED) {
#pragma unroll
                for (int j = 0; j < CB; j++)
                    if ((uint32_t)j < cnt) {
                        u64x2 s, t;
                        part[j].reduce(m, s, t);
                        acc[j].mac_weighted(s, t, w);
                    }
            }
        }
        idx = idx_next;
    }
#pragma unroll
    for (int j = 0; j < CB; j++)
        if ((uint32_t)j < cnt) {
            u64x2 r0, r1;
            acc[j].reduce(m, r0, r1);
            hb_st2(cx + (size_t)j * 2 * k.qlp_n, r0);
            hb_st2(cx + (size_t)j * 2 * k.qlp_n + k.qlp_n, r1);
        }
}

}  // namespace pha
