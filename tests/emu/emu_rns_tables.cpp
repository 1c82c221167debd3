// emu_rns_tables.cpp -- TEST-ONLY: the tool constants of phantom-fhe_amd/csrc/pha_rns_tables.h (the very functions pha_context.hip
// uploads the results of), compiled for the host and handed out as flat arrays.  tests/test_emu_rns_tables.py holds the expected
// values, computed from the definitions with Python integers.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../phantom-fhe_amd/csrc/pha_rns_tables.h"

using namespace pha;

namespace {
std::vector<u64> vec(const uint64_t *p, size_t n) { return std::vector<u64>(p, p + n); }
Rows rows(const uint32_t *p, size_t n) { return Rows(p, p + n); }
template <class T>
void put(T *dst, const std::vector<T> &v) { if (!v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T)); }
void put_pairs(uint64_t *dst, const std::vector<u64x2> &v) {
    for (size_t i = 0; i < v.size(); i++) { dst[2 * i] = v[i].x; dst[2 * i + 1] = v[i].y; }
}
// meta[4] = split_kind, mont, r90, row_pad; mat30 [osz][row_pad][2]
void put_conv(const BConvTables &b, uint64_t *hat_inv, uint64_t *mat, uint32_t *mat30, uint64_t *oninv, uint32_t *meta) {
    put_pairs(hat_inv, b.hat_inv);
    put(mat, b.mat);
    put(mat30, b.mat30);
    put(oninv, b.oninv);
    meta[0] = (uint32_t)b.split_kind; meta[1] = b.mont; meta[2] = b.r90; meta[3] = b.row_pad;
}
}  // namespace

extern "C" {

// var1 != 0: bconv_tables_var1 (out_scale, in_scale and family_isz unused)
int emu_bconv(const uint64_t *primes, size_t np, const uint32_t *ip, size_t isz, const uint32_t *op, size_t osz, const uint64_t *out_scale,
              uint64_t in_scale, uint32_t family_isz, int var1, uint64_t *hat_inv, uint64_t *mat, uint32_t *mat30, uint64_t *oninv,
              uint32_t *meta) {
    const std::vector<u64> pr = vec(primes, np), os = out_scale ? vec(out_scale, osz) : std::vector<u64>();
    const BConvTables b = var1 ? bconv_tables_var1(pr, rows(ip, isz), rows(op, osz))
                               : bconv_tables(pr, rows(ip, isz), rows(op, osz), out_scale ? &os : nullptr, in_scale, family_isz);
    put_conv(b, hat_inv, mat, mat30, oninv, meta);
    return 0;
}

// digit b of level size_ql; returns the digit count.  ip / op receive the digit's rows (isz_osz[2] their counts)
int emu_digit(const uint64_t *primes, size_t np, const uint32_t *qlp_prime, size_t size_qlp, uint32_t size_ql, uint32_t alpha, uint32_t b,
              uint32_t *ip, uint32_t *op, uint32_t *isz_osz, uint64_t *hat_inv, uint64_t *mat, uint32_t *mat30, uint64_t *oninv, uint32_t *meta,
              uint64_t *part_hat_inv_out) {
    const std::vector<DigitTables> d = digit_tables(vec(primes, np), rows(qlp_prime, size_qlp), size_ql, alpha);
    put(ip, d[b].ip);
    put(op, d[b].op);
    isz_osz[0] = (uint32_t)d[b].ip.size();
    isz_osz[1] = (uint32_t)d[b].op.size();
    put_conv(d[b].conv, hat_inv, mat, mat30, oninv, meta);
    put_pairs(part_hat_inv_out, part_hat_inv(d));
    return (int)d.size();
}

void emu_prod_mod_limbs(const uint64_t *primes, size_t np, const uint32_t *num, size_t nnum, uint32_t count, int invert, uint64_t *out) {
    put(out, prod_mod_limbs(vec(primes, np), rows(num, nnum), count, invert != 0));
}

void emu_alpha_table(const uint64_t *primes, size_t np, const uint32_t *ib, size_t isz, const uint32_t *ob, size_t osz, uint64_t *out) {
    put(out, alpha_table(vec(primes, np), rows(ib, isz), rows(ob, osz)));
}

void emu_scale_round(const uint64_t *primes, size_t np, const uint32_t *away, size_t na, const uint32_t *keep, size_t nk, uint64_t factor,
                     double *frac, uint64_t *tab) {
    std::vector<double> f;
    std::vector<u64> t;
    scale_round_tables(vec(primes, np), rows(away, na), rows(keep, nk), factor, f, t);
    put(frac, f);
    put(tab, t);
}

uint32_t emu_behz_size_b(const uint64_t *primes, uint32_t size_q, uint64_t plain_t) { return behz_size_b(vec(primes, size_q), size_q, plain_t); }

// pairs_bsk [2][Bsk][2]: inv_prod_q_mod_bsk, inv_mt_mod_bsk; words_bsk [Bsk]: prod_q_mod_bsk; words_q [Q]: prod_b_mod_q;
// t_qb [2][Q + Bsk]: value, Shoup; scalars [2][2]: neg_inv_prod_q_mod_mt, inv_prod_b_mod_msk
void emu_behz(const uint64_t *primes, size_t np, uint32_t size_q, uint32_t aux0, uint32_t size_b, uint64_t plain_t, uint64_t *pairs_bsk,
              uint64_t *words_bsk, uint64_t *words_q, uint64_t *t_qb, uint64_t *scalars) {
    const BehzTables t = behz_tables(vec(primes, np), size_q, aux0, size_b, plain_t);
    const size_t bsk = size_b + 1;
    put_pairs(pairs_bsk, t.inv_prod_q_mod_bsk);
    put_pairs(pairs_bsk + 2 * bsk, t.inv_mt_mod_bsk);
    put(words_bsk, t.prod_q_mod_bsk);
    put(words_q, t.prod_b_mod_q);
    put(t_qb, t.t_qb);
    put(t_qb + size_q + bsk, t.t_qb_shoup);
    put_pairs(scalars, {t.neg_inv_prod_q_mod_mt, t.inv_prod_b_mod_msk});
}

// scalars [3][2]: inv_q_last_mod_t, pinv_mod_t, neg_ql_mod_t; q_last_mod_q [ql - 1]; p_hat_mod_t [|p|]; t_inv_mod_q [ql]; inc [ql]
void emu_plain(const uint64_t *primes, size_t np, uint32_t size_ql, const uint32_t *p, size_t size_p, uint64_t plain_t, uint64_t *scalars,
               uint64_t *q_last_mod_q, uint64_t *p_hat_mod_t, uint64_t *t_inv_mod_q, uint64_t *inc) {
    const PlainTables t = plain_tables(vec(primes, np), size_ql, rows(p, size_p), plain_t);
    put_pairs(scalars, {t.inv_q_last_mod_t, t.pinv_mod_t, t.neg_ql_mod_t});
    put(q_last_mod_q, t.q_last_mod_q);
    put(p_hat_mod_t, t.p_hat_mod_t);
    put(t_inv_mod_q, t.t_inv_mod_q);
    put(inc, t.plain_upper_half_increment);
}

}
