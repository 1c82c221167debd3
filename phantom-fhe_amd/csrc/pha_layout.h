// pha_layout.h -- what the entries of the secret-key layer (pha_decrypt.hip, pha_noise.hip, pha_encrypt.hip, pha_prng.hip) refuse before
// they launch anything, one function per entry, over ContextShape, a plain description of the context.  EncBuf and check_layout() ask
// whether the elements of a strided batch overlap, whether strides are even and bases aligned and whether an output touches an input;
// phase_chunk() gives the chunk size and work-buffer stride of the phase front end.  Host C++ only, no HIP, nothing dereferenced but
// the prime table, no heap off the throw path: tests/cpp/test_layout.cpp compiles this header alone and sweeps it under the address and
// undefined-behaviour sanitizers (tests/test_layout.py).
#pragma once
#include <string>

#include "../../include/phantom_amd.h"   // PHA_SCHEME_*
#include "pha_sum_operand.h"             // overlaps(); <algorithm>, <cstdint>, <initializer_list>, <stdexcept>

namespace pha {

struct ContextShape {
    size_t n;
    uint32_t size_q, size_p, size_qp;
    uint64_t plain_t;         // 0: none
    const uint64_t *primes;   // [size_qp]: Q, then P
};

inline void need(const void *p) {
    if (!p) throw std::invalid_argument("null device pointer");
}
// rows [first, first + rows) of a table of `table` rows; a level: the first size_Ql of the size_q data primes
inline void check_rns_level(size_t rows, size_t table, size_t first = 0) {
    if (rows < 1 || first > table || rows > table - first) throw std::invalid_argument("RNSBase is invalid");
}
inline void need_plain_modulus(const ContextShape &cx) {
    if (!cx.plain_t) throw std::invalid_argument("the context has no plain modulus (pha_context_set_plain_modulus)");
}
inline bool ntt_domain_scheme(int scheme) {   // ckks / bgv: true, bfv: false; throws on anything else
    if (scheme != PHA_SCHEME_CKKS && scheme != PHA_SCHEME_BGV && scheme != PHA_SCHEME_BFV) throw std::invalid_argument("unsupported scheme");
    return scheme != PHA_SCHEME_BFV;
}
inline void check_scheme(const ContextShape &cx, int scheme) {
    if (!ntt_domain_scheme(scheme) || scheme == PHA_SCHEME_BGV) need_plain_modulus(cx);
}
inline void check_degree(const ContextShape &cx) {
    if (cx.n < 8) throw std::invalid_argument("poly_modulus_degree below 8: a generator block is eight words");
}
constexpr uint64_t kEncryptMinPrime = (uint64_t)1 << 17, kNoiseMinPrime = 22;   // the smallest prime a sample may meet; 0: any
inline void check_prime_floor(const ContextShape &cx, size_t first, size_t rows, uint64_t min_prime) {
    for (size_t y = 0; min_prime && y < rows; y++)
        if (cx.primes[first + y] < min_prime)
            throw std::invalid_argument(min_prime == kNoiseMinPrime ? "a sample of magnitude 21 needs every prime of the rows used above 21"
                                                                    : "a sample of magnitude 2^16 needs every prime of the rows used at or above 2^17");
}
// the rows of a polynomial at a level: the first size_Ql data primes, then (special) the special primes
inline void check_rows(const ContextShape &cx, size_t size_Ql, bool special, uint64_t min_prime) {
    check_rns_level(size_Ql, cx.size_q);
    if (special && cx.size_p == 0) throw std::invalid_argument("context has no special modulus");
    check_prime_floor(cx, 0, size_Ql, min_prime);
    if (special) check_prime_floor(cx, cx.size_q, cx.size_p, min_prime);
}

struct EncBuf {
    const char *name;
    const void *p;          // null: absent (an optional result)
    size_t words, stride;   // one element in 8-byte words, and the words between consecutive elements (0: shared)
    bool may_share;         // a stride of 0 is allowed
    bool out = false;       // written: must not touch what is read, nor an earlier output
    unsigned align = 16;    // of p, in bytes: 16 (its stride must be even), or the size of its own words
    const char *crowded = nullptr;   // the refusal of a stride below `words`; null: "<name> stride below the size of an element ..."
    bool in_place_ok = false;        // an output may be this buffer itself, at this stride
};
inline size_t span(const EncBuf &b, size_t count) { return count ? (b.stride ? (count - 1) * b.stride : 0) + b.words : 0; }
constexpr size_t kMaxCount = 65535;   // a launch carries the element in blockIdx.z

inline void check_count(size_t count, size_t max = kMaxCount, const char *refusal = "count out of range") {
    if (count > max) throw std::invalid_argument(refusal);
}
inline void check_crowded(const EncBuf &b, size_t count) {
    if (count > 1 && b.stride < b.words && !(b.may_share && b.stride == 0))
        throw std::invalid_argument(b.crowded ? std::string(b.crowded) : std::string(b.name) + " stride below the size of an element: the elements overlap");
}
inline void check_even(std::initializer_list<EncBuf> bufs, bool stores) {   // of the buffers accessed 16 bytes at a time
    for (const EncBuf &b : bufs)
        if (b.align == 16 && (b.stride & 1)) throw std::invalid_argument(stores ? "strides must be even (16-byte stores)" : "strides must be even (16-byte loads)");
}
inline void check_aligned(std::initializer_list<EncBuf> bufs) {   // the 16-byte buffers first, then the ones aligned to their words
    uintptr_t wide = 0, narrow = 0;
    for (const EncBuf &b : bufs) (b.align == 16 ? wide : narrow) |= reinterpret_cast<uintptr_t>(b.p) & (b.align - 1);
    if (wide) throw std::invalid_argument("buffers must be 16-byte aligned");
    if (narrow) throw std::invalid_argument("buffers must be aligned to their words");
}
// every output against every input and every output before it, in list order; result i may take the place of element i of an in_place_ok input
inline void check_overlap(std::initializer_list<EncBuf> bufs, size_t count) {
    auto words = [](const EncBuf &b) { return static_cast<const uint64_t *>(b.p); };
    for (const EncBuf *o = bufs.begin(); count && o != bufs.end(); o++)
        for (const EncBuf *b = bufs.begin(); o->out && b != bufs.end(); b++)
            if ((!b->out || b < o) && o->p && b->p && !(b->in_place_ok && o->p == b->p && (count == 1 || o->stride == b->stride)) &&
                overlaps(words(*o), span(*o, count), words(*b), span(*b, count)))
                throw std::invalid_argument(std::string(o->name) + " must not overlap " + b->name);
}
// Strides, alignment, overlap of the buffers of one batched entry -- nothing else, in this order
inline void check_layout(std::initializer_list<EncBuf> bufs, size_t count) {
    for (const EncBuf &b : bufs) check_crowded(b, count);
    check_even(bufs, false);
    check_aligned(bufs);
    check_overlap(bufs, count);
}

struct CtBatch {
    const uint64_t *ct;
    size_t cipher_size, batch, ct_stride;
    const uint64_t *sk_powers;
    size_t n_powers;
};
constexpr size_t kPhaseBatchMax = 4 * (size_t)65535;   // kPhaseGroup ciphertexts per workgroup row (pha_decrypt.h), the row in blockIdx.z
constexpr const char *kNoiseLimbCap = "the noise entries take levels of at most 64 limbs";
inline EncBuf ct_buf(const ContextShape &cx, size_t size_Ql, const CtBatch &b, bool in_place_ok) {
    return EncBuf{"ct", b.ct, b.cipher_size * size_Ql * cx.n, b.ct_stride, false, false, 16, "ct stride below cipher_size * L * N: the ciphertexts overlap", in_place_ok};
}
inline EncBuf sk_buf(const ContextShape &cx, size_t size_Ql, const CtBatch &b) {   // s^i at i * size_QP * N, L rows of each
    return EncBuf{"sk_powers", b.sk_powers, (b.cipher_size - 2) * (size_t)cx.size_qp * cx.n + size_Ql * cx.n, 0, true};
}
// what an entry over a CtBatch refuses after its null pointers (the noise budget: after the scheme); max_limbs: the noise entry's cap, 0: none
inline void check_ct_batch(const ContextShape &cx, size_t size_Ql, const CtBatch &b, bool need_t, size_t max_limbs) {
    check_rns_level(size_Ql, cx.size_q);
    if (max_limbs && size_Ql > max_limbs) throw std::invalid_argument(kNoiseLimbCap);
    if (need_t) need_plain_modulus(cx);
    if (b.cipher_size < 2 || b.cipher_size > 65535) throw std::invalid_argument("cipher_size out of range");
    if (b.n_powers < b.cipher_size - 1) throw std::invalid_argument("sk_powers holds fewer powers than the ciphertext has polynomials beyond c0");
    check_count(b.batch, kPhaseBatchMax, "batch out of range");
}
// the three decrypt entries.  out_words: L * N for the phase, N for the plaintexts; in_place_ok: dst may be ct itself (result b in c0 (b)'s place)
inline void check_decrypt(const ContextShape &cx, size_t size_Ql, const CtBatch &b, const uint64_t *dst, size_t dst_stride, size_t out_words,
                          bool in_place_ok, bool need_t) {
    need(b.ct); need(b.sk_powers); need(dst);
    check_ct_batch(cx, size_Ql, b, need_t, 0);
    check_layout({sk_buf(cx, size_Ql, b), ct_buf(cx, size_Ql, b, in_place_ok),
                  EncBuf{"dst", dst, out_words, dst_stride, false, true, 16, "dst stride below the size of a result: the results overlap"}}, b.batch);
}
// pha_invariant_noise_budget_batched; returns whether the scheme keeps ciphertexts in NTT form.  budget: 4-byte words, counted in pairs
inline bool check_noise_budget(const ContextShape &cx, size_t size_Ql, const CtBatch &b, int scheme, const int32_t *budget, const uint64_t *norm,
                               size_t max_limbs) {
    need(b.ct); need(b.sk_powers); need(budget);
    const bool ntt_form = ntt_domain_scheme(scheme);
    check_ct_batch(cx, size_Ql, b, scheme != PHA_SCHEME_CKKS, max_limbs);
    check_layout({ct_buf(cx, size_Ql, b, false), sk_buf(cx, size_Ql, b), EncBuf{"budget", budget, (b.batch + 1) / 2, 0, true, true, 4},
                  EncBuf{"norm", norm, b.batch * size_Ql, 0, true, true, 8}}, b.batch);
    return ntt_form;
}
// pha_poly_infty_norm_batched (any count: the entry cuts it into launches itself)
inline void check_poly_norm(const ContextShape &cx, size_t size_Ql, const uint64_t *src, size_t count, size_t src_stride, const uint64_t *norm,
                            const uint32_t *bits, size_t max_limbs) {
    need(src); need(bits);
    check_rns_level(size_Ql, cx.size_q);
    if (size_Ql > max_limbs) throw std::invalid_argument(kNoiseLimbCap);
    check_layout({EncBuf{"src", src, size_Ql * cx.n, src_stride, false, false, 8, "src stride below L * N: the polynomials overlap"},
                  EncBuf{"norm", norm, count * size_Ql, 0, true, true, 8}, EncBuf{"bits", bits, (count + 1) / 2, 0, true, true, 4}}, count);
}

// the encrypt entries.  pk == false: key = sk_ntt, e [N], no u; plain_words == 0: no plaintext (the zero encryption).  pk == true: key = the
// public key [2][QP][N], u [N], e [2][N]; the special primes are checked, ct has the level's rows alone
inline void check_encrypt(const ContextShape &cx, size_t size_Ql, bool special, bool pk, int scheme, const uint64_t *key, const uint64_t *u,
                          size_t u_stride, const uint64_t *e, size_t e_stride, const uint64_t *plain, size_t plain_words, size_t plain_stride,
                          const uint64_t *ct, size_t ct_stride, size_t count) {
    need(key); need(e); need(ct);
    if (pk) need(u);
    if (plain_words) need(plain);
    check_rows(cx, size_Ql, special, kEncryptMinPrime);
    check_scheme(cx, scheme);
    check_count(count);
    const size_t n = cx.n, rows = size_Ql + (special && !pk ? cx.size_p : 0), k = pk ? 2 : 1;
    check_layout({EncBuf{"ct", ct, 2 * rows * n, ct_stride, false, true, 16, "ct stride below the size of a ciphertext: the ciphertexts overlap"},
                  EncBuf{pk ? "pk" : "sk_ntt", key, k * cx.size_qp * n, 0, true}, EncBuf{"u", u, pk ? n : 0, u_stride, !pk},
                  EncBuf{"e", e, k * n, e_stride, false}, EncBuf{"plain", plain, plain_words, plain_stride, true}}, count);
}

// one polynomial over rows [mod_start, mod_start + cms) of the QP table (the reference's layout)
inline void check_sample_ref(const ContextShape &cx, const uint64_t *out, const uint8_t *seed, size_t cms, size_t mod_start, uint64_t min_prime) {
    need(out); need(seed);
    check_degree(cx);
    check_rns_level(cms, cx.size_qp, mod_start);
    if (cms > kMaxCount) throw std::invalid_argument("coeff_mod_size out of range");
    check_prime_floor(cx, mod_start, cms, min_prime);
    check_aligned({EncBuf{"out", out, 0, 0, true}, EncBuf{"seeds", seed, 0, 0, true}});
}
// `count` elements of out_words words (with a level: after its rows are checked; size_Ql == 0 with uniform == false: [N] signed words)
inline void check_sample_batch(const ContextShape &cx, bool uniform, size_t size_Ql, bool special, const uint8_t *seeds, size_t count,
                               const uint64_t *out, size_t out_stride) {
    need(seeds); need(out);
    check_degree(cx);
    if (uniform) check_rows(cx, size_Ql, special, 0);
    const EncBuf o{"out", out, uniform ? (size_Ql + (special ? cx.size_p : 0)) * cx.n : cx.n, out_stride, false};
    check_count(count);
    check_even({o}, true);
    check_crowded(o, count);
    check_aligned({o, EncBuf{"seeds", seeds, 0, 0, true}});
}
// pha_generate_kswitch_keys_seeded; bgv_ready(): asked of the entry's tables, once the context is known to have them.  Returns dnum
template <class F>
inline size_t check_kswitch(const ContextShape &cx, const uint64_t *sk_ntt, const uint64_t *new_keys, size_t n_keys, size_t new_key_stride,
                            const uint8_t *seeds, const uint64_t *evk, size_t evk_stride, int scheme, F &&bgv_ready) {
    need(sk_ntt); need(new_keys); need(seeds); need(evk);
    check_degree(cx);
    if (cx.size_p == 0) throw std::invalid_argument("context has no special modulus");
    if (cx.size_q % cx.size_p) throw std::invalid_argument("#Q must be a multiple of special_modulus_size");
    if (ntt_domain_scheme(scheme) && scheme == PHA_SCHEME_BGV && !bgv_ready()) throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
    const size_t dnum = cx.size_q / cx.size_p, qp_n = (size_t)cx.size_qp * cx.n, count = n_keys * dnum;
    check_count(n_keys, kMaxCount / dnum, "n_keys out of range");
    const EncBuf evk_b{"evk", evk, 2 * qp_n, evk_stride, false, true, 16, "evk stride below 2 * size_QP * N: the components overlap"};
    const EncBuf keys_b{"new_keys", new_keys, (size_t)cx.size_q * cx.n, new_key_stride, false, false, 16, "new_key stride below size_Q * N: the keys overlap"};
    check_even({evk_b, keys_b}, true);
    check_crowded(evk_b, count);
    check_crowded(keys_b, n_keys);
    check_aligned({evk_b, EncBuf{"seeds", seeds, 0, 0, true}, EncBuf{"sk_ntt", sk_ntt, qp_n, 0, true}, keys_b});
    if (count && (overlaps(evk, span(evk_b, count), sk_ntt, qp_n) || overlaps(evk, span(evk_b, count), new_keys, span(keys_b, n_keys))))
        throw std::invalid_argument("evk must not overlap an input");
    return dnum;
}

// the phase front end (pha_decrypt.hip phase_to_coeff).  C: ciphertexts per set of launches -- the chunk argument (0: the default), the
// batch, and the grid's 65535 polynomials: one per ciphertext in NTT form, k - 1 forward transforms per ciphertext under bfv.  wst:
// work-buffer words per ciphertext, [L][N] or [k - 1][L][N]; the work buffer takes C * wst words
struct PhaseChunk { size_t C, wst; };
inline PhaseChunk phase_chunk(bool ntt_form, size_t cipher_size, size_t ln, size_t batch, size_t chunk, size_t default_chunk) {
    const size_t km1 = cipher_size - 1, cap = ntt_form ? 65535 : std::max<size_t>(65535 / km1, 1);
    return PhaseChunk{std::min(std::min(chunk ? chunk : default_chunk, batch), cap), ntt_form ? ln : km1 * ln};
}

}  // namespace pha
