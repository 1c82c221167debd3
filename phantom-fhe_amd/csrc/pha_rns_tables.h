// pha_rns_tables.h -- the constants of the RNS tools as functions from rows of the prime table to std::vectors.
//
// Host C++ only, no HIP: pha_context.hip calls these and uploads what they return; tests/emu/emu_rns_tables.cpp compiles the
// same header with g++ and tests/test_emu_rns_tables.py holds every table against Python big integers.  `primes` is the
// context's prime table (the QP chain, then the auxiliary moduli); a base is a list of its rows.
// Reference: the DRNSTool constructor (src/rns.cu:66-975) and the converters' host tables (src/host/rns.cu:282-337,438-497).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "pha_arith.h"

namespace pha {

typedef unsigned __int128 u128;
typedef std::vector<uint32_t> Rows;

constexpr int kBcRowPad = 16;  // row pitch (entries) of the split base-conversion matrix

// ---- single-word number theory ----------------------------------------------------------------
inline u64 h_mulmod(u64 a, u64 b, u64 q) { return (u64)(((u128)a * b) % q); }
// extended Euclid (the reference's try_invert_uint_mod is xgcd as well, src/host/numth.cu)
inline u64 h_invmod(u64 a, u64 q) {
    __int128 t = 0, nt = 1, r = q, nr = a % q;
    while (nr) {
        __int128 k = r / nr;
        __int128 tmp = t - k * nt; t = nt; nt = tmp;
        tmp = r - k * nr; r = nr; nr = tmp;
    }
    if (r != 1) throw std::logic_error("value is not invertible modulo q");
    if (t < 0) t += q;
    return (u64)t;
}
inline u64 h_shoup(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
inline u64x2 h_pair(u64 v, u64 q) { return u64x2{v, h_shoup(v, q)}; }
inline int h_bits(u64 v) { return v ? 64 - __builtin_clzll(v) : 0; }

// prod(primes[rows]) mod m, optionally without one position of the base
inline u64 prod_mod(const std::vector<u64> &primes, const Rows &rows, u64 m, size_t skip = (size_t)-1) {
    u64 p = 1 % m;
    for (size_t k = 0; k < rows.size(); k++)
        if (k != skip) p = h_mulmod(p, primes[rows[k]] % m, m);
    return p;
}
inline Rows row_range(uint32_t first, uint32_t count) {
    Rows r(count);
    for (uint32_t i = 0; i < count; i++) r[i] = first + i;
    return r;
}

// ---- little-endian multi-word integers ----------------------------------------------------------
typedef std::vector<u64> Big;
inline void big_mul(Big &b, u64 m) {
    u64 carry = 0;
    for (auto &w : b) { const u128 t = (u128)w * m + carry; w = (u64)t; carry = (u64)(t >> 64); }
    if (carry) b.push_back(carry);
}
inline u64 big_mod(const Big &b, u64 m) {
    u128 rem = 0;
    for (size_t i = b.size(); i-- > 0;) rem = ((rem << 64) | b[i]) % m;
    return (u64)rem;
}
inline void big_div(Big &b, u64 m) {
    u128 rem = 0;
    for (size_t i = b.size(); i-- > 0;) { const u128 cur = (rem << 64) | b[i]; b[i] = (u64)(cur / m); rem = cur % m; }
}
inline int big_bits(const Big &b) {
    size_t top = b.size();
    while (top > 1 && !b[top - 1]) top--;
    return (int)(top - 1) * 64 + h_bits(b[top - 1]);
}

// ---- converter constants (DBaseConverter, src/host/rns.cu:282-337,438-457) ---------------------------------------------
struct BConvTables {
    std::vector<u64x2> hat_inv;   // [isz] in_scale * qhat_i^-1 mod q_i (+Shoup)
    std::vector<u64> mat;         // [osz][isz] out_scale_j * qhat_i mod p_j
    std::vector<uint32_t> mat30;  // [osz][row_pad][2] halves of mat (Montgomery form when mont), rows zero-padded
    std::vector<u64> oninv;       // [osz] -p_j^-1 mod 2^64 when mont, else 0
    int split_kind = 0;           // BConv::split_kind (pha_internal.h)
    bool mont = false, r90 = false;
    uint32_t row_pad = kBcRowPad;
};

// The carry-free form of a converter (the rule in front of BConv::split_kind) and the tables cut for it.  family_isz: the widest
// converter of those launched together (mod-up digits take one kind).
inline void bconv_split_tables(const std::vector<u64> &primes, const Rows &ip, const Rows &op, uint32_t family_isz, BConvTables &b) {
    const uint32_t isz = (uint32_t)ip.size(), osz = (uint32_t)op.size();
    int by = 0, bm = 0;       // residues of the input primes are below 2^by, matrix entries (residues of the output moduli) below 2^bm
    for (uint32_t row : ip) by = std::max(by, h_bits(primes[row] - 1));
    for (uint32_t row : op) bm = std::max(bm, h_bits(primes[row] - 1));
    uint32_t sm = 30;         // the matrix entries are cut at this bit
    b.split_kind = 0;
    b.row_pad = kBcRowPad;
    const uint32_t widest = std::max(isz, family_isz);
    if (widest <= (uint32_t)kBcRowPad && by <= 60 && bm <= 60) b.split_kind = 1;
    else if (widest <= 32 && by <= 60 && bm <= 62) { b.split_kind = 2; sm = 31; }
    else if (widest <= 32 && by <= 62 && bm <= 60) { b.split_kind = 3; sm = 30; }
    if (b.split_kind >= 2 && isz > (uint32_t)kBcRowPad) b.row_pad = 32;
    // Montgomery form for the split-accumulator kernel: rows hold qhat_i * 2^64 mod p_j, so that REDC of the accumulated
    // sum gives sum_i y_i * qhat_i mod p_j directly (valid for odd p_j; the BEHZ converter with m_tilde = 2^32 keeps Barrett)
    // and for sum_i y_i * entry < 2^64 p_j: 16 inputs of 60 bits, or in general sum_i q_i < 2^64
    u128 sum_q = 0;
    for (uint32_t row : ip) sum_q += primes[row];
    b.mont = b.split_kind == 1 || (b.split_kind != 0 && (sum_q >> 64) == 0);
    for (uint32_t row : op) b.mont = b.mont && (primes[row] & 1);
    // r06: with at most 15 inputs and the 30 / 30 cuts the kernels reduce word by word in base 2^30 straight from the four split
    // accumulators (mont_redc90_split, pha_arith.h): the rows then carry 2^90.  A sixteenth term would overflow its first step.
    b.r90 = b.mont && b.split_kind == 1 && widest <= 15;
    b.oninv.assign(osz, 0);
    if (b.mont)
        for (uint32_t j = 0; j < osz; j++) {
            const u64 pj = primes[op[j]];
            u64 inv = pj;                                        // Newton: inv * pj = 1 mod 2^(3 * 2^k)
            for (int it = 0; it < 6; it++) inv *= 2 - pj * inv;
            b.oninv[j] = 0 - inv;
        }
    b.mat30.assign((size_t)osz * b.row_pad * 2, 0u);
    if (isz <= b.row_pad)
        for (uint32_t j = 0; j < osz; j++)
            for (uint32_t i = 0; i < isz; i++) {
                u64 m = b.mat[(size_t)j * isz + i];
                if (b.mont) {
                    const u64 pj = primes[op[j]];
                    m = (u64)((((u128)m) << 64) % pj);
                    if (b.r90) m = (u64)((((u128)m) << 26) % pj);   // 2^64 * 2^26 = 2^90
                }
                b.mat30[((size_t)j * b.row_pad + i) * 2] = (uint32_t)(m & ((1u << sm) - 1));
                b.mat30[((size_t)j * b.row_pad + i) * 2 + 1] = (uint32_t)(m >> sm);
            }
}

// q-hat_i^-1 mod q_i and q-hat_i mod p_j for an (ibase -> obase) converter.
// out_scale (optional, [osz]): row j of the matrix is multiplied by out_scale[j] mod p_j, i.e. the converter delivers
// out_scale[j] * (converted value) mod p_j at no extra cost (pha_keyswitch_rescale: P^-1 mod q_j).  in_scale: the phase-1 factors
// carry it, i.e. the converter takes x and converts in_scale * x (BEHZ: m_tilde).
inline BConvTables bconv_tables(const std::vector<u64> &primes, const Rows &ip, const Rows &op, const std::vector<u64> *out_scale = nullptr,
                                u64 in_scale = 1, uint32_t family_isz = 0) {
    const uint32_t isz = (uint32_t)ip.size(), osz = (uint32_t)op.size();
    BConvTables b;
    b.hat_inv.resize(isz);
    for (uint32_t i = 0; i < isz; i++) {
        const u64 qi = primes[ip[i]];
        u64 inv = h_invmod(prod_mod(primes, ip, qi, i), qi);
        if (in_scale != 1) inv = h_mulmod(in_scale % qi, inv, qi);
        b.hat_inv[i] = h_pair(inv, qi);
    }
    b.mat.resize((size_t)osz * isz);
    for (uint32_t j = 0; j < osz; j++) {
        const u64 pj = primes[op[j]];
        for (uint32_t i = 0; i < isz; i++) {
            const u64 h = prod_mod(primes, ip, pj, i);
            b.mat[(size_t)j * isz + i] = out_scale ? h_mulmod((*out_scale)[j] % pj, h, pj) : h;
        }
    }
    bconv_split_tables(primes, ip, op, family_isz, b);
    return b;
}

// bConv_BEHZ_var1 (src/rns_bconv.cu:231-246, constants src/host/rns.cu:469-496): the quotient-style conversion
// x -> about P * x / Q in base P: phase 1 multiplies by -P * qhat_i^-1 mod q_i, the matrix is q_i^-1 mod p_j.
inline BConvTables bconv_tables_var1(const std::vector<u64> &primes, const Rows &ip, const Rows &op) {
    const uint32_t isz = (uint32_t)ip.size(), osz = (uint32_t)op.size();
    BConvTables b;
    b.hat_inv.resize(isz);
    for (uint32_t i = 0; i < isz; i++) {
        const u64 qi = primes[ip[i]];
        const u64 v = qi - h_mulmod(prod_mod(primes, op, qi), h_invmod(prod_mod(primes, ip, qi, i), qi), qi);
        b.hat_inv[i] = h_pair(v, qi);
    }
    b.mat.resize((size_t)osz * isz);
    for (uint32_t j = 0; j < osz; j++) {
        const u64 pj = primes[op[j]];
        for (uint32_t i = 0; i < isz; i++) b.mat[(size_t)j * isz + i] = h_invmod(primes[ip[i]] % pj, pj);
    }
    bconv_split_tables(primes, ip, op, 0, b);
    return b;
}

// ---- hybrid key switch (src/rns.cu:66-200) --------------------------------------------------------------------------------
// v[i] = prod(primes[num]) mod q_i, or its inverse, for the data limbs i < count
inline std::vector<u64> prod_mod_limbs(const std::vector<u64> &primes, const Rows &num, uint32_t count, bool invert) {
    std::vector<u64> v(count);
    for (uint32_t i = 0; i < count; i++) {
        const u64 p = prod_mod(primes, num, primes[i]);
        v[i] = invert ? h_invmod(p, primes[i]) : p;
    }
    return v;
}
inline std::vector<u64> shoup_of(const std::vector<u64> &primes, const Rows &rows, const std::vector<u64> &v) {
    std::vector<u64> s(v.size());
    for (size_t i = 0; i < v.size(); i++) s[i] = h_shoup(v[i], primes[rows[i]]);
    return s;
}
inline std::vector<u64x2> pairs_of(const std::vector<u64> &primes, const Rows &rows, const std::vector<u64> &v) {
    std::vector<u64x2> s(v.size());
    for (size_t i = 0; i < v.size(); i++) s[i] = h_pair(v[i], primes[rows[i]]);
    return s;
}
// The digits of level size_ql (rns.cu:152-190): digit b's own limbs [b alpha, min((b + 1) alpha, Ql)) of [Ql || P] are its inputs,
// every other limb an output; all of them take one carry-free form (family_isz = alpha).  qlp_prime: limb -> row.
struct DigitTables {
    Rows ip, op;
    BConvTables conv;
};
inline std::vector<DigitTables> digit_tables(const std::vector<u64> &primes, const Rows &qlp_prime, uint32_t size_ql, uint32_t alpha) {
    std::vector<DigitTables> d((size_ql + alpha - 1) / alpha);
    for (uint32_t b = 0; b < (uint32_t)d.size(); b++) {
        const uint32_t s = alpha * b, len = std::min(alpha, size_ql - s);
        for (uint32_t j = 0; j < (uint32_t)qlp_prime.size(); j++) (j >= s && j < s + len ? d[b].ip : d[b].op).push_back(qlp_prime[j]);
        d[b].conv = bconv_tables(primes, d[b].ip, d[b].op, nullptr, 1, alpha);
    }
    return d;
}
// partQlHatInv_mod_Ql_concat: the digits' phase-1 factors by data limb
inline std::vector<u64x2> part_hat_inv(const std::vector<DigitTables> &digits) {
    std::vector<u64x2> v;
    for (const DigitTables &d : digits) v.insert(v.end(), d.conv.hat_inv.begin(), d.conv.hat_inv.end());
    return v;
}

// ---- HPS / HPS-over-Q (src/rns.cu:687-975) -------------------------------------------------------------------------------------
// [|ibase| + 1][|obase|]: a * prod(ibase) mod p_j (src/host/rns.cu:459-466)
inline std::vector<u64> alpha_table(const std::vector<u64> &primes, const Rows &ibase, const Rows &obase) {
    const size_t isz = ibase.size(), osz = obase.size();
    std::vector<u64> t((isz + 1) * osz);
    for (size_t j = 0; j < osz; j++) {
        const u64 p = primes[obase[j]], m = prod_mod(primes, ibase, p);
        for (size_t a = 0; a <= isz; a++) t[a * osz + j] = h_mulmod(a, m, p);
    }
    return t;
}
inline std::vector<double> inverse_doubles(const std::vector<u64> &primes, const Rows &rows) {
    std::vector<double> v(rows.size());
    for (size_t i = 0; i < rows.size(); i++) v[i] = 1.0 / (double)primes[rows[i]];
    return v;
}
// Scale-and-round tables from base `away` || `keep` into base `keep`: over S = away u keep, x_s = factor * prod(keep) * (S / s)^-1
// mod s as a big integer.  frac [|away|] = the fraction of x_a / a; tab [|keep|][|away| + 1]: column a = floor(x_a / a) mod keep_k,
// the last column floor(x_k / keep_k) mod keep_k.  (HPS: t R / (Q R) into R, rns.cu:727-790; over Q: t Ql / (Ql Rl) into Ql,
// :836-885; levels dropped: Ql / Q into Ql, :918-972)
inline void scale_round_tables(const std::vector<u64> &primes, const Rows &away, const Rows &keep, u64 factor, std::vector<double> &frac,
                               std::vector<u64> &tab) {
    const size_t na = away.size(), nk = keep.size();
    Rows all(away);
    all.insert(all.end(), keep.begin(), keep.end());
    frac.assign(na, 0.0);
    tab.assign(nk * (na + 1), 0);
    for (size_t i = 0; i < na + nk; i++) {
        const u64 si = primes[all[i]];
        Big x{1};
        for (uint32_t row : keep) big_mul(x, primes[row]);
        if (factor != 1) big_mul(x, factor);
        big_mul(x, h_invmod(prod_mod(primes, all, si, i), si));
        if (i < na) frac[i] = (double)big_mod(x, si) / (double)si;
        big_div(x, si);
        if (i < na)
            for (size_t k = 0; k < nk; k++) tab[k * (na + 1) + i] = big_mod(x, primes[keep[k]]);
        else
            tab[(i - na) * (na + 1) + na] = big_mod(x, si);
    }
}

// ---- BEHZ (src/rns.cu:392-560) ---------------------------------------------------------------------------------------------------
// |B|: one prime more than |Q| when 32 + |t| + |prod(q)| bits do not fit (rns.cu:398-406)
inline uint32_t behz_size_b(const std::vector<u64> &primes, uint32_t size_q, u64 plain_t) {
    Big acc{1};
    for (uint32_t i = 0; i < size_q; i++) big_mul(acc, primes[i]);
    return size_q + ((32 + h_bits(plain_t) + big_bits(acc) >= 61 * (int)size_q + 61) ? 1 : 0);
}
struct BehzTables {
    std::vector<u64x2> inv_prod_q_mod_bsk, inv_mt_mod_bsk;   // [Bsk]
    std::vector<u64> prod_q_mod_bsk;                         // [Bsk]
    std::vector<u64> prod_b_mod_q;                           // [Q]
    std::vector<u64> t_qb, t_qb_shoup;                       // [Q + Bsk]
    u64x2 neg_inv_prod_q_mod_mt, inv_prod_b_mod_msk;
};
// the bases: Q = rows [0, size_q), B = [aux0, aux0 + size_b), m_sk = row aux0 + size_b, m_tilde (a power of two) the row after it
inline BehzTables behz_tables(const std::vector<u64> &primes, uint32_t size_q, uint32_t aux0, uint32_t size_b, u64 plain_t) {
    const uint32_t size_bsk = size_b + 1;
    const Rows q = row_range(0, size_q), b = row_range(aux0, size_b);
    const u64 m_sk = primes[aux0 + size_b], m_tilde = primes[aux0 + size_bsk];
    BehzTables t;
    for (uint32_t j = 0; j < size_bsk; j++) {
        const u64 p = primes[aux0 + j], pq = prod_mod(primes, q, p);
        t.prod_q_mod_bsk.push_back(pq);                                    // :548-553
        t.inv_prod_q_mod_bsk.push_back(h_pair(h_invmod(pq, p), p));        // :508-518
        t.inv_mt_mod_bsk.push_back(h_pair(h_invmod(m_tilde % p, p), p));   // :537-546
    }
    for (uint32_t i = 0; i < size_q; i++) t.prod_b_mod_q.push_back(prod_mod(primes, b, primes[i]));
    // t (:467-479) by limb of a [Q || Bsk] buffer: one inverse transform over both bases multiplies by it.  Stored reduced: the
    // reference keeps t itself, whose Shoup quotient floor(t 2^64 / q_i) does not fit 64 bits once t >= q_i (t < 2^60 may exceed a
    // data prime; the Bsk primes have 61 bits).  For t < q_i the words are the reference's.
    for (uint32_t i = 0; i < size_q + size_bsk; i++) {
        const u64 prime = primes[i < size_q ? i : aux0 + i - size_q];
        t.t_qb.push_back(plain_t % prime);
        t.t_qb_shoup.push_back(h_shoup(plain_t % prime, prime));
    }
    const u64 inv_q_mt = h_invmod(prod_mod(primes, q, m_tilde), m_tilde);
    t.neg_inv_prod_q_mod_mt = h_pair((m_tilde - inv_q_mt) % m_tilde, m_tilde);
    t.inv_prod_b_mod_msk = h_pair(h_invmod(prod_mod(primes, b, m_sk), m_sk), m_sk);
    return t;
}

// ---- plain-modulus constants of one level (src/rns.cu:196-324) -----------------------------------------------------------------
struct PlainTables {
    u64x2 inv_q_last_mod_t, pinv_mod_t, neg_ql_mod_t;   // (value, Shoup) modulo t; pinv_mod_t only with special primes
    std::vector<u64> q_last_mod_q;                      // [ql - 1] q_last mod q_i
    std::vector<u64> p_hat_mod_t;                       // [alpha] row of base_P_to_t_conv
    std::vector<u64> t_inv_mod_q;                       // [ql] t^-1 mod q_i (rns.cu:308-324)
    std::vector<u64> plain_upper_half_increment;        // [ql] q_i - t
};
inline PlainTables plain_tables(const std::vector<u64> &primes, uint32_t size_ql, const Rows &p, u64 pt) {
    PlainTables t{};
    const u64 q_last = primes[size_ql - 1];
    t.inv_q_last_mod_t = h_pair(h_invmod(q_last % pt, pt), pt);       // :200-212
    for (uint32_t i = 0; i + 1 < size_ql; i++) t.q_last_mod_q.push_back(q_last % primes[i]);
    if (!p.empty()) {                                                 // :270-284
        for (size_t k = 0; k < p.size(); k++) t.p_hat_mod_t.push_back(prod_mod(primes, p, pt, k));
        t.pinv_mod_t = h_pair(h_invmod(prod_mod(primes, p, pt), pt), pt);
    }
    // BFV enc / add / sub (:292-324): -Ql mod t and t^-1 mod q_i; q_i - t for the plain lift
    t.neg_ql_mod_t = h_pair(pt - prod_mod(primes, row_range(0, size_ql), pt), pt);
    for (uint32_t i = 0; i < size_ql; i++) {
        t.t_inv_mod_q.push_back(h_invmod(pt % primes[i], primes[i]));
        t.plain_upper_half_increment.push_back(primes[i] - pt);
    }
    return t;
}

// ---- decryption at one level (pha_decrypt.h) -------------------------------------------------------------------------------------
// The BFV scale-and-round: h = ceil(bits of the widest q_i / 2); per limb i, with A_i = t [qhat_i^-1]_{q_i} and B_i = t [qhat_i^-1 2^h]_{q_i}
// as 128-bit integers (t < 2^60, q_i < 2^61: below 2^121), itab [L][2] = floor(A_i / q_i) mod t, floor(B_i / q_i) mod t and frac [L][2]
// = (A_i mod q_i) / q_i, (B_i mod q_i) / q_i.  A fraction r / q is taken as floor(r 2^64 / q), exact in 128 bits, and converted once:
// within 2^-64 + 2^-54 < 2^-52 of its true value (no division of two doubles).
struct DecryptRoundTables {
    int h = 0;
    std::vector<double> frac;   // [L][2]
    std::vector<u64> itab;      // [L][2]
};
inline DecryptRoundTables decrypt_round_tables(const std::vector<u64> &primes, uint32_t size_ql, u64 t) {
    DecryptRoundTables d;
    const Rows q = row_range(0, size_ql);
    int bits = 0;
    for (uint32_t i = 0; i < size_ql; i++) bits = std::max(bits, h_bits(primes[i]));
    d.h = (bits + 1) / 2;
    d.frac.resize(2 * (size_t)size_ql);
    d.itab.resize(2 * (size_t)size_ql);
    for (uint32_t i = 0; i < size_ql; i++) {
        const u64 qi = primes[i];
        const u64 inv = h_invmod(prod_mod(primes, q, qi, i), qi);
        const u64 both[2] = {inv, h_mulmod(inv, (u64)(((u128)1 << d.h) % qi), qi)};
        for (int p = 0; p < 2; p++) {
            const u128 a = (u128)t * both[p];
            d.itab[2 * i + p] = (u64)((a / qi) % t);
            const u64 fix = (u64)((((u128)(u64)(a % qi)) << 64) / qi);   // floor(r 2^64 / q_i), r < q_i
            d.frac[2 * i + p] = (double)fix * 0x1p-64;
        }
    }
    return d;
}
// The BGV tail, exact_convert_array to t (src/rns_bconv.cu:374-431, constants src/host/rns.cu:282-337): qhat_i^-1 mod q_i, qhat_i mod t,
// Q mod t
struct DecryptModTTables {
    std::vector<u64x2> hat_inv;   // [L]
    std::vector<u64> mat;         // [L]
    u64 q_mod_t = 0;
};
inline DecryptModTTables decrypt_mod_t_tables(const std::vector<u64> &primes, uint32_t size_ql, u64 t) {
    DecryptModTTables d;
    const Rows q = row_range(0, size_ql);
    for (uint32_t i = 0; i < size_ql; i++) {
        const u64 qi = primes[i];
        d.hat_inv.push_back(h_pair(h_invmod(prod_mod(primes, q, qi, i), qi), qi));
        d.mat.push_back(prod_mod(primes, q, t, i));
    }
    d.q_mod_t = prod_mod(primes, q, t);
    return d;
}

// ---- mixed-radix tables of the noise kernels (pha_noise.h) ------------------------------------------------------------------------
// Over the first `size` primes, ONE set for every level (digit a_j depends on q_0 .. q_j only): inv [size][size], entry i * size + j
// (i < j) = (q_i^-1 mod q_j, Shoup), zero elsewhere; lift [size] = q_j ceil(2^61 / q_j), the multiple of q_j in [2^61, 2^61 + q_j).
struct NoiseTables {
    uint32_t size = 0;
    std::vector<u64x2> inv;
    std::vector<u64> lift;
};
inline NoiseTables noise_tables(const std::vector<u64> &primes, uint32_t size) {
    NoiseTables t;
    t.size = size;
    t.inv.assign((size_t)size * size, u64x2{0, 0});
    t.lift.resize(size);
    for (uint32_t j = 0; j < size; j++) {
        const u64 qj = primes[j];
        if (qj >> 61) throw std::invalid_argument("the noise kernels take moduli below 2^61");
        t.lift[j] = qj * ((((u64)1 << 61) + qj - 1) / qj);
        for (uint32_t i = 0; i < j; i++) t.inv[(size_t)i * size + j] = h_pair(h_invmod(primes[i] % qj, qj), qj);
    }
    return t;
}
// Per level: the mixed-radix digits of (Q_l - 1) / 2 (repeated division of the big integer by q_0, q_1, ...), bitcount(Q_l), and
// scalar mod q_i for the factor the norm is taken with (t can exceed a 41-bit limb).
struct NoiseLevelTables {
    std::vector<u64> half;   // [size_ql]
    int q_bits = 0;
};
inline NoiseLevelTables noise_level_tables(const std::vector<u64> &primes, uint32_t size_ql) {
    NoiseLevelTables t;
    Big q{1};
    for (uint32_t i = 0; i < size_ql; i++) big_mul(q, primes[i]);
    t.q_bits = big_bits(q);
    Big h(q);                // (Q - 1) / 2 = Q >> 1 for odd Q
    for (size_t w = 0; w < h.size(); w++) h[w] = (h[w] >> 1) | (w + 1 < h.size() ? h[w + 1] << 63 : 0);
    t.half.resize(size_ql);
    for (uint32_t i = 0; i < size_ql; i++) {
        t.half[i] = big_mod(h, primes[i]);
        big_div(h, primes[i]);
    }
    return t;
}
inline std::vector<u64> noise_scalar_table(const std::vector<u64> &primes, uint32_t size_ql, u64 scalar) {
    std::vector<u64> s(size_ql);
    for (uint32_t i = 0; i < size_ql; i++) s[i] = scalar % primes[i];
    return s;
}

}  // namespace pha
