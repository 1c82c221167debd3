// pha_plain.hip -- ciphertext (+|-|*) plaintext on raw buffers: the device work of add_plain_inplace /
// sub_plain_inplace / multiply_plain_inplace (src/evaluate.cu:1105-1226, 1228-1340, src/scalingvariant.cu:10-60) with
// the per-level constants of DRNSTool (src/rns.cu:292-324) taken from the context.  Compositions of the kernels in
// pha_poly_ext.hip / pha_ntt.hip; the host mirror (host/phantom.h) keeps the reference's checks and metadata.
#include "../../include/phantom_amd.h"
#include "pha_internal.h"
#include "pha_ntt_core.h"

#include <algorithm>

using namespace pha;

static Tool &plain_tool(Context &c, size_t size_Ql) {
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("RNSBase is invalid");
    if (!c.plain_t) throw std::invalid_argument("the context has no plain modulus (pha_context_set_plain_modulus)");
    return c.tool((uint32_t)size_Ql);
}

// the level checks pha_bfv_multiply_plain makes: a level of the context, a plain modulus, t below every q_i of the level
// (no per-level tool is built: the lift's constants are t and the primes themselves)
static void bfv_sum_level(Context &c, size_t size_Ql) {
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("RNSBase is invalid");
    if (!c.plain_t) throw std::invalid_argument("the context has no plain modulus (pha_context_set_plain_modulus)");
    for (uint32_t i = 0; i < size_Ql; i++)
        if (c.primes[i] <= c.plain_t) throw std::invalid_argument("the plain lift needs t below every q_i");
}

// out (i) = NTT(centred lift of plain (i)) for i < count: one launch pair per piece of at most 65535 plaintexts (grid z)
static void launch_bfv_lift(Context &c, size_t size_Ql, const u64 *plain, size_t count, size_t plain_stride, u64 *out,
                            size_t out_stride, hipStream_t s) {
    constexpr size_t kPiece = 65535;
    for (size_t i0 = 0; i0 < count; i0 += kPiece) {
        NttExtra x;
        x.batch = (uint32_t)std::min(kPiece, count - i0);
        x.poly_stride = x.batch > 1 ? out_stride : size_Ql * c.n;
        x.pro_src = plain + i0 * plain_stride;   // every limb of plaintext z lifts the same N words modulo its own prime
        x.pro_stride = plain_stride;
        x.pro_lift_t = c.plain_t;
        u64 *o = out + i0 * out_stride;
        ntt_forward(c, o, o, o, plain_sel(0, size_Ql), EPI_FWD_CANON, x, s);
    }
}

constexpr size_t kBfvSumChunk = 8;   // groups per inverse transform, as kPlainSumChunk (pha_poly.hip)
// Terms per slab: the work buffer holds chunk * slab ciphertexts in NTT form (8 x 4 x 15 MiB = 480 MiB at N = 2^15 with 30 limbs,
// half as much again for raw plaintexts), and a slab costs one more pass over the partial sums in res (32 bytes per coefficient
// and limb, against 44 per term), so 4 terms keep that pass below a fifth of the sum's traffic.
constexpr size_t kBfvSumSlab = 4;

// The pipeline behind pha_bfv_multiply_plain_sum_batched (raw == false: plain (g, k) is [L][N], lifted and in NTT form) and
// pha_bfv_plain_inner_product_batched (raw == true: [N] words below t).  Slabs of terms outside, chunks of groups inside, so that
// an operand shared between the groups is transformed once per slab for ALL groups; the NTT-form partial sums live in res
// (plain_sum_kernel's acc == res mode) and a chunk is taken back to coefficient form right behind its last slab.
static void bfv_plain_sum(Context &c, size_t size_Ql, const SumOperand &plain, bool raw, const SumOperand &ct, const SumOperand &acc,
                          u64 *res, size_t terms, size_t batch, size_t chunk, size_t slab, void *stream) {
    need(plain.p); need(ct.p); need(res);
    bfv_sum_level(c, size_Ql);
    const size_t ln = size_Ql * c.n;
    sum_check_terms(terms);
    sum_check_layout({plain, ct, acc}, terms, res);
    const size_t res_words = batch * 2 * ln;
    if (plain.touches(res, res_words, terms, batch)) throw std::invalid_argument("res must not overlap a plaintext operand");
    if (ct.touches(res, res_words, terms, batch)) throw std::invalid_argument("res must not overlap an operand ciphertext");
    if (acc.p && acc.touches(res, res_words, 1, batch)) throw std::invalid_argument("res must not overlap acc");
    if (batch == 0) return;
    hipStream_t s = as_stream(stream);
    strict_sum_operand(c, raw ? "bfv_plain_inner_product plain" : "bfv_multiply_plain_sum plain", plain, size_Ql, terms, batch, raw, s);
    strict_sum_operand(c, raw ? "bfv_plain_inner_product ct" : "bfv_multiply_plain_sum ct", ct, size_Ql, terms, batch, false, s);
    strict_sum_operand(c, raw ? "bfv_plain_inner_product acc" : "bfv_multiply_plain_sum acc", acc, size_Ql, 1, batch, false, s);
    const size_t tp = plain.ts, tc = ct.ts;
    // 2 * chunk polynomials per inverse and 2 * slab per forward launch: both within a launch's grid
    const size_t C = std::min<size_t>(std::min(chunk ? chunk : kBfvSumChunk, batch), 32767);
    const size_t S = std::min<size_t>(std::min(slab ? slab : kBfvSumSlab, terms), 32767);
    const bool ct_shared = ct.bs == 0, pl_shared = plain.bs == 0;
    const size_t wct_words = (ct_shared ? 1 : C) * S * 2 * ln, wpl_words = raw ? (pl_shared ? 1 : C) * S * ln : 0;
    u64 *wct = c.scratch_outer(stream, wct_words + wpl_words), *wpl = wct + wct_words;
    const LimbSel sel = plain_sel(0, size_Ql);
    // NTT form of the K terms from k0 on of one group's ciphertexts / plaintexts, into the work buffer
    auto forward_ct = [&](const u64 *src, size_t K, u64 *dst) {
        NttExtra x;
        x.poly_stride = x.in_stride = ln;
        if (K == 1 || tc == 2 * ln) {   // the terms' 2 K polynomials lie in a row: one launch pair
            x.batch = (uint32_t)(2 * K);
            ntt_forward(c, src, dst, dst, sel, EPI_FWD_CANON, x, s);
        } else {
            x.batch = 2;
            for (size_t k = 0; k < K; k++) ntt_forward(c, src + k * tc, dst + k * 2 * ln, dst + k * 2 * ln, sel, EPI_FWD_CANON, x, s);
        }
    };
    for (size_t k0 = 0; k0 < terms; k0 += S) {
        const size_t K = std::min(S, terms - k0);
        const bool first = k0 == 0, last = k0 + K == terms;
        if (ct_shared) forward_ct(ct.at(0, k0), K, wct);
        if (raw && pl_shared) launch_bfv_lift(c, size_Ql, plain.at(0, k0), K, tp, wpl, ln, s);
        for (size_t b0 = 0; b0 < batch; b0 += C) {
            const size_t B = std::min(C, batch - b0);
            for (size_t g = 0; g < B; g++) {
                if (!ct_shared) forward_ct(ct.at(b0 + g, k0), K, wct + g * S * 2 * ln);
                if (raw && !pl_shared) launch_bfv_lift(c, size_Ql, plain.at(b0 + g, k0), K, tp, wpl + g * S * ln, ln, s);
            }
            u64 *r = res + b0 * 2 * ln;
            // the work buffers hold a group's slab densely: [S] lifted plaintexts, [S] ciphertexts; the partial sums are res itself
            const SumOperand w_plain = raw ? sum_poly(wpl, ln, pl_shared ? 0 : S * ln, ln, nullptr) : plain.advanced(b0, k0),
                             w_ct = sum_ct(wct, 2 * ln, ct_shared ? 0 : S * 2 * ln, ln, nullptr),
                             partial = sum_acc(first ? nullptr : r, 2 * ln, ln);
            launch_plain_sum(c, w_plain, w_ct, partial, r, size_Ql, K, B, s);
            if (!last) continue;
            NttExtra x;   // the chunk's 2 B polynomials back to coefficient form, in place; group g adds acc (g) in the final store
            x.batch = (uint32_t)(2 * B);
            x.poly_stride = ln;
            if (acc.p) {
                x.aux = acc.at(b0, 0);
                x.aux_stride = ln;
                x.aux_pair_stride = acc.bs;
            }
            ntt_inverse(c, r, r, r, sel, acc.p ? EPI_INV_CANON_ADD : EPI_INV_CANON, x, s);
        }
    }
}

extern "C" {

int pha_bfv_add_plain(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint64_t *plain, int subtract, void *stream) {
    PHA_CTX_BEGIN(ctx)   // multiply_add_plain_with_scaling_variant / multiply_sub_plain_with_scaling_variant
    need(ct); need(plain);
    Context &c = ctx->c;
    Tool &t = plain_tool(c, size_Ql);
    if (subtract)
        rc(pha_bfv_sub_timesQ_overt(ctx, ct, plain, t.neg_ql_mod_t.x, t.neg_ql_mod_t.y, t.t_inv_mod_q.p,
                                    t.t_inv_mod_q_shoup.p, c.plain_t, size_Ql, stream));
    else
        rc(pha_bfv_add_timesQ_overt(ctx, ct, plain, t.neg_ql_mod_t.x, t.neg_ql_mod_t.y, t.t_inv_mod_q.p,
                                    t.t_inv_mod_q_shoup.p, c.plain_t, size_Ql, stream));
    PHA_API_END
}

int pha_bfv_multiply_plain(pha_context_t ctx, size_t size_Ql, uint64_t *ct, size_t cipher_size, const uint64_t *plain,
                           void *stream) {
    PHA_CTX_BEGIN(ctx)   // multiply_plain_normal evaluate.cu:1256-1300
    need(ct); need(plain);
    Context &c = ctx->c;
    Tool &t = plain_tool(c, size_Ql);
    for (uint32_t i = 0; i < size_Ql; i++)
        if (c.primes[i] <= c.plain_t) throw std::invalid_argument("the plain lift needs t below every q_i");
    if (cipher_size == 0) return 0;
    if (cipher_size > 65535) throw std::invalid_argument("cipher_size out of range");
    const size_t ln = size_Ql * c.n;
    u64 *temp = c.scratch(stream, ln);
    // centred lift of the plaintext into every limb (:1283-1285), then NTT
    rc(pha_abs_plain_rns_poly(ctx, plain, (c.plain_t + 1) >> 1, t.plain_upper_half_increment.p, temp, size_Ql, stream));
    rc(pha_nwt_2d_radix8_forward_inplace(ctx, temp, size_Ql, 0, stream));
    // (c_i * pt): NTT, pointwise product, inverse NTT -- all polynomials per launch
    rc(pha_nwt_2d_radix8_forward_inplace_batched(ctx, ct, size_Ql, 0, cipher_size, ln, stream));
    for (size_t i = 0; i < cipher_size; i++) rc(pha_multiply_rns_poly(ctx, ct + i * ln, temp, ct + i * ln, size_Ql, 0, stream));
    rc(pha_nwt_2d_radix8_backward_inplace_batched(ctx, ct, size_Ql, 0, cipher_size, ln, stream));
    PHA_API_END
}

int pha_bgv_lift_plain(pha_context_t ctx, size_t size_Ql, const uint64_t *plain, uint64_t *out, void *stream) {
    PHA_CTX_BEGIN(ctx)   // the modup_fuse loop of evaluate.cu:1150-1154 / 1208-1212 / 1319-1323, every limb in one launch
    need(plain); need(out);
    Context &c = ctx->c;
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("RNSBase is invalid");
    NttExtra x;
    x.pro_src = plain;   // each limb transforms the same N coefficients, reduced modulo its own prime on load
    ntt_forward(c, out, out, out, plain_sel(0, size_Ql), EPI_FWD_CANON, x, as_stream(stream));
    PHA_API_END
}

// ---- BFV plaintext-weighted sums: one forward transform per term, one inverse per sum (extension) -------
// Sum_k iNTT(NTT(ct_k) (.) NTT(pt_k)) = iNTT(Sum_k NTT(ct_k) (.) NTT(pt_k)) word for word: the transform is an exact linear map
// modulo each prime and every stored word is canonical.  So the per-term inverse transforms and add passes of the loop of
// pha_bfv_multiply_plain + pha_add_rns_poly collapse into the one-launch plain_sum_kernel (pha_poly.hip) over NTT-form operands
// and ONE inverse transform, which adds acc in its final store (EPI_INV_CANON_ADD); the plaintexts are lifted in the load of
// their forward transform (PRO_LIFT).

int pha_bfv_lift_plain_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *plain, size_t count, size_t plain_stride,
                               uint64_t *out, size_t out_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(plain); need(out);
    Context &c = ctx->c;
    bfv_sum_level(c, size_Ql);
    const size_t ln = size_Ql * c.n;
    if ((plain_stride | out_stride) & 1) throw std::invalid_argument("strides must be even (16-byte loads)");
    if ((reinterpret_cast<uintptr_t>(plain) | reinterpret_cast<uintptr_t>(out)) & 15)
        throw std::invalid_argument("buffers must be 16-byte aligned");
    if (count > 1 && out_stride < ln) throw std::invalid_argument("out stride below L * N: the lifted plaintexts overlap");
    if (count == 0) return 0;
    if (sum_poly(plain, plain_stride, 0, c.n, nullptr).touches(out, (count - 1) * out_stride + ln, count, 1))
        throw std::invalid_argument("out must not overlap a plaintext operand");
    hipStream_t s = as_stream(stream);
    strict_plain(c, "bfv_lift_plain plain", plain, c.plain_t, count > 1 && plain_stride == 0 ? 1 : count, plain_stride, s);
    launch_bfv_lift(c, size_Ql, plain, count, plain_stride, out, out_stride, s);
    PHA_API_END
}

int pha_bfv_multiply_plain_sum_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *plain_ntt, const uint64_t *ct,
                                       const uint64_t *acc, uint64_t *res, size_t terms, size_t batch, size_t plain_term_stride,
                                       size_t plain_batch_stride, size_t ct_term_stride, size_t ct_batch_stride,
                                       size_t acc_batch_stride, size_t chunk, size_t slab, void *stream) {
    PHA_CTX_BEGIN(ctx)
    const size_t ln = size_Ql * ctx->c.n;
    bfv_plain_sum(ctx->c, size_Ql, sum_poly(plain_ntt, plain_term_stride, plain_batch_stride, ln, kPlainCrowded), false,
                  sum_ct(ct, ct_term_stride, ct_batch_stride, ln, kCtCrowded), sum_acc(acc, acc_batch_stride, ln), res, terms, batch, chunk,
                  slab, stream);
    PHA_API_END
}

int pha_bfv_plain_inner_product_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *plain, const uint64_t *ct,
                                        const uint64_t *acc, uint64_t *res, size_t terms, size_t batch, size_t plain_term_stride,
                                        size_t plain_batch_stride, size_t ct_term_stride, size_t ct_batch_stride,
                                        size_t acc_batch_stride, size_t chunk, size_t slab, void *stream) {
    PHA_CTX_BEGIN(ctx)
    const size_t ln = size_Ql * ctx->c.n;
    bfv_plain_sum(ctx->c, size_Ql, sum_poly(plain, plain_term_stride, plain_batch_stride, ctx->c.n, kRawPlainCrowded), true,
                  sum_ct(ct, ct_term_stride, ct_batch_stride, ln, kCtCrowded), sum_acc(acc, acc_batch_stride, ln), res, terms, batch, chunk,
                  slab, stream);
    PHA_API_END
}

}  // extern "C"
