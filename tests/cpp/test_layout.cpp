// test_layout.cpp -- TEST-ONLY, host only (no device is touched): phantom-fhe_amd/csrc/pha_layout.h, the host-side refusals of the
// secret-key layer.  Built with -fsanitize=address,undefined and run by tests/test_layout.py.  Every pointer lies inside one arena (or
// is null, or is never reached by a comparison) and none is dereferenced but the prime table.
//   overlap:  check_overlap() equals the brute-force, word-by-word intersection of the two extents for an output slid across and past
//             both ends of an input, for 8-byte results and for arrays of 4-byte words counted in pairs, with the in-place exemption
//             present and absent.
//   refusals: every refusal the header decides, alone, with its exception class and full text.
//   order:    per entry a table of its refusals in the order the entry made them before the header existed (read from that source);
//             for every position i the arguments break rule i and every later rule that can be broken with it, and message i is raised.
//             The decrypt entries and the noise budget have tables of their own: the shared prefix and the noise entry's four
//             differences are asserted on the tables.  Every entry of the four files calls ONE function of the header for what
//             it refuses without a device (key generation asks its tables about bgv through a callable), and each has its table here.
//   chunk:    phase_chunk() against the formulas the three chunked entries used to write out.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <typeinfo>
#include <vector>

#include "../../phantom-fhe_amd/csrc/pha_layout.h"

using namespace pha;

static int bad = 0;
#define EXPECT(cond, ...)             \
    do {                              \
        if (!(cond)) {                \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            bad++;                    \
        }                             \
    } while (0)

static std::vector<uint64_t> arena(1 << 16);
static const uint64_t *at(size_t word) { return arena.data() + word; }
static const void *off_by(const void *p, size_t bytes) { return reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(p) + bytes); }

static const uint64_t *base_of(const EncBuf &b) { return static_cast<const uint64_t *>(b.p); }

static void refused(const std::string &what, const char *text, const std::function<void()> &fn) {
    try {
        fn();
        EXPECT(false, "%s: accepted, want \"%s\"", what.c_str(), text);
    } catch (const std::exception &e) {
        EXPECT(typeid(e) == typeid(std::invalid_argument), "%s: threw %s", what.c_str(), typeid(e).name());
        EXPECT(std::strcmp(e.what(), text) == 0, "%s: says \"%s\", want \"%s\"", what.c_str(), e.what(), text);
    }
}
static void accepted(const char *what, const std::function<void()> &fn) {
    try {
        fn();
    } catch (const std::exception &e) {
        EXPECT(false, "%s: refused with \"%s\"", what, e.what());
    }
}

// ---- overlap against the definition ---------------------------------------------------------------------------------------------------
// the words of a buffer's extent: from the first word of its first element to the last word of its last, the padding between strided
// elements included (the entries have always refused a result that lies in an operand's padding)
static std::set<const uint64_t *> words_of(const EncBuf &b, size_t count) {
    std::set<const uint64_t *> w;
    const size_t elements = b.stride ? count : (count ? 1 : 0);
    for (const uint64_t *p = base_of(b); elements && p < base_of(b) + (elements - 1) * b.stride + b.words; p++) w.insert(p);
    return w;
}
// the words the elements themselves occupy, by definition: a result that shares one of them with an input must be refused whatever
// the extents say (the converse does not hold: padding counts as occupied)
static std::set<const uint64_t *> element_words(const EncBuf &b, size_t count) {
    std::set<const uint64_t *> w;
    for (size_t i = 0; i < (b.stride ? count : (count ? 1 : 0)); i++)
        for (size_t k = 0; k < b.words; k++) w.insert(base_of(b) + i * b.stride + k);
    return w;
}
static bool refuses_overlap(const EncBuf &in, const EncBuf &out, size_t count) {
    try {
        check_overlap({in, out}, count);
        return false;
    } catch (const std::invalid_argument &e) {
        EXPECT(std::string(e.what()) == "out must not overlap in", "overlap: says \"%s\"", e.what());
        return true;
    }
}
static size_t sweep_overlap() {
    size_t layouts = 0;
    const uint64_t *base = at(256);
    for (size_t words : {2, 4})
    for (size_t count = 0; count <= 3; count++)
    for (size_t stride : {(size_t)0, words, words + 2})
    for (int in_place_ok = 0; in_place_ok < 2; in_place_ok++) {
        EncBuf in{"in", base, words, stride, stride == 0};
        in.in_place_ok = in_place_ok != 0;
        const std::set<const uint64_t *> in_words = words_of(in, count);
        const size_t reach = 2 * (words + 2) + words;   // past the last word of the largest case
        // strided 8-byte results: before, inside, abutting, after; one coincides with the input (offset 0, the input's own stride)
        for (size_t out_words : {(size_t)1, words})
        for (size_t out_stride : {out_words, stride, words + 2}) {
            if (out_stride < out_words) continue;
            for (const uint64_t *p = base - 3 * (words + 2) - 2; p < base + reach + 2; p++) {
                const EncBuf out{"out", p, out_words, out_stride, false, true};
                bool want = false;
                for (const uint64_t *w : words_of(out, count)) want = want || in_words.count(w);
                if (in_place_ok && p == base && (count == 1 || out_stride == stride)) want = false;   // the exemption, by its definition
                const bool got = refuses_overlap(in, out, count);
                bool shared_word = false;
                for (const uint64_t *w : element_words(out, count)) shared_word = shared_word || element_words(in, count).count(w);
                if (shared_word && !(in_place_ok && p == base)) EXPECT(got, "overlap: a result that shares a word with an input was accepted (at %td)", p - base);
                EXPECT(got == want, "overlap: words %zu count %zu stride %zu in-place %d, out %zu words every %zu at %td: got %d, want %d", words,
                       count, stride, in_place_ok, out_words, out_stride, p - base, (int)got, (int)want);
            }
            layouts++;
        }
        // a dense array of `count` 4-byte words, counted as (count + 1) / 2 words
        for (const uint64_t *p = base - 4; p < base + reach + 2; p++) {
            const EncBuf out{"out", p, (count + 1) / 2, 0, true, true, 4};   // as the noise entries describe budget / bits
            bool want = false;
            for (size_t k = 0; k < (count + 1) / 2 && count; k++) want = want || in_words.count(p + k);
            if (in_place_ok && p == base && (count == 1 || stride == 0)) want = false;
            const bool got = refuses_overlap(in, out, count);
            EXPECT(got == want, "overlap: words %zu count %zu stride %zu, 4-byte array at %td: got %d, want %d", words, count, stride, p - base, (int)got, (int)want);
        }
        layouts++;
    }
    return layouts;
}

// ---- the entries over a batch of ciphertexts --------------------------------------------------------------------------------------------
static const char *kNull = "null device pointer", *kLevel = "RNSBase is invalid", *kScheme = "unsupported scheme";
static const char *kNoT = "the context has no plain modulus (pha_context_set_plain_modulus)", *kCipher = "cipher_size out of range";
static const char *kPowers = "sk_powers holds fewer powers than the ciphertext has polynomials beyond c0", *kBatch = "batch out of range";
static const char *kCtCrowded = "ct stride below cipher_size * L * N: the ciphertexts overlap";
static const char *kDstCrowded = "dst stride below the size of a result: the results overlap";
static const char *kAligned16 = "buffers must be 16-byte aligned", *kAlignedWords = "buffers must be aligned to their words";
static const char *kEvenLoads = "strides must be even (16-byte loads)", *kEvenStores = "strides must be even (16-byte stores)";
static const char *kCap = "the noise entries take levels of at most 64 limbs";

static std::vector<uint64_t> primes(71, ((uint64_t)1 << 40) + 1);   // values matter to the prime floors only
static ContextShape shape(uint32_t size_q, uint32_t size_p, uint64_t t) { return ContextShape{8, size_q, size_p, size_q + size_p, t, primes.data()}; }
static bool has(uint32_t mask, int rule) { return (mask >> rule) & 1; }
static uint32_t from(int i, int rules) { return ((1u << rules) - 1) & ~((1u << i) - 1); }   // rule i and every later one

// The decrypt entries, rules in the order of the former decrypt_check().  phase: pha_decrypt_phase_batched (a result is L * N words and
// may take c0's place; no plain modulus needed); else pha_bgv_decrypt_batched / pha_bfv_decrypt_batched
static const std::vector<const char *> kPhaseTable{kNull, kLevel, kCipher, kPowers, kBatch, kCtCrowded, kDstCrowded, kEvenLoads, kAligned16,
                                                   "dst must not overlap sk_powers", "dst must not overlap ct"};
static const std::vector<const char *> kDecryptTable{kNull, kLevel, kNoT, kCipher, kPowers, kBatch, kCtCrowded, kDstCrowded, kEvenLoads,
                                                     kAligned16, "dst must not overlap sk_powers", "dst must not overlap ct"};
static void call_decrypt(bool phase, uint32_t mask) {
    int r = 0;
    const bool null = has(mask, r++), level = has(mask, r++), no_t = phase ? false : has(mask, r++), cipher = has(mask, r++),
               powers = has(mask, r++), batch = has(mask, r++), ct_crowded = has(mask, r++), dst_crowded = has(mask, r++), odd = has(mask, r++),
               unaligned = has(mask, r++), on_sk = has(mask, r++), on_ct = has(mask, r++);
    const ContextShape cx = shape(3, 1, no_t ? 0 : 65537);
    const size_t size_Ql = level ? 4 : 2, k = cipher ? 65536 : 3, ln = size_Ql * cx.n, ct_words = k * ln, out_words = phase ? ln : cx.n;
    const uint64_t *ct = at(1024), *sk = on_sk && on_ct ? ct : at(8192), *dst = on_ct ? ct + 2 : on_sk ? sk + 2 : at(16384);
    const CtBatch b{null ? nullptr : ct, k, batch ? kPhaseBatchMax + 1 : 3, ct_words + (ct_crowded ? -2 : 2) + (odd ? 1 : 0), sk, powers ? 0 : k - 1};
    check_decrypt(cx, size_Ql, b, unaligned ? dst + 1 : dst, out_words + (dst_crowded ? -2 : 2), out_words, phase, !phase);
}

// pha_invariant_noise_budget_batched, rules in the order the entry wrote them out.  The context has 70 data primes, so that a level
// can be valid and above 64 limbs
static const std::vector<const char *> kNoiseTable{kNull, kScheme, kLevel, kCap, kNoT, kCipher, kPowers, kBatch, kCtCrowded, kEvenLoads, kAligned16,
                                                   kAlignedWords, "budget must not overlap ct", "budget must not overlap sk_powers",
                                                   "norm must not overlap ct", "norm must not overlap sk_powers", "norm must not overlap budget"};
static void call_noise(uint32_t mask) {
    int r = 0;
    const bool null = has(mask, r++), scheme = has(mask, r++), level = has(mask, r++), cap = has(mask, r++), no_t = has(mask, r++),
               cipher = has(mask, r++), powers = has(mask, r++), batch = has(mask, r++), ct_crowded = has(mask, r++), odd = has(mask, r++),
               unaligned = has(mask, r++), unaligned_words = has(mask, r++), b_ct = has(mask, r++), b_sk = has(mask, r++), n_ct = has(mask, r++),
               n_sk = has(mask, r++), n_b = has(mask, r++);
    const ContextShape cx = shape(70, 1, no_t ? 0 : 65537);
    const size_t size_Ql = level ? 71 : cap ? 65 : 2, k = cipher ? 65536 : 3, ct_words = k * size_Ql * cx.n;
    const uint64_t *ct = at(1024), *sk = b_ct && b_sk ? ct : at(8192);
    const uint64_t *budget = b_ct ? ct + 2 : b_sk ? sk + 2 : at(16384), *norm = n_ct ? ct + 4 : n_sk ? sk + 4 : n_b ? budget : at(20480);
    const CtBatch b{ct, k, batch ? kPhaseBatchMax + 1 : 3, ct_words + (ct_crowded ? -2 : 2) + (odd ? 1 : 0), unaligned ? sk + 1 : sk, powers ? 0 : k - 1};
    check_noise_budget(cx, size_Ql, b, scheme ? 7 : PHA_SCHEME_BFV, static_cast<const int32_t *>(null ? nullptr : off_by(budget, unaligned_words ? 2 : 0)),
                       static_cast<const uint64_t *>(off_by(norm, unaligned_words ? 4 : 0)), 64);
}

// pha_poly_infty_norm_batched
static const std::vector<const char *> kNormTable{kNull, kLevel, kCap, "src stride below L * N: the polynomials overlap", kAlignedWords,
                                                  "norm must not overlap src", "bits must not overlap src", "bits must not overlap norm"};
static void call_norm(uint32_t mask) {
    int r = 0;
    const bool null = has(mask, r++), level = has(mask, r++), cap = has(mask, r++), crowded = has(mask, r++), unaligned = has(mask, r++),
               n_src = has(mask, r++), b_src = has(mask, r++), b_n = has(mask, r++);
    const ContextShape cx = shape(70, 1, 0);
    const size_t size_Ql = level ? 71 : cap ? 65 : 2, ln = size_Ql * cx.n;
    const uint64_t *src = at(1024), *norm = n_src ? src + 2 : at(8192), *bits = b_src ? src + 4 : b_n ? norm : at(16384);
    check_poly_norm(cx, size_Ql, null ? nullptr : src, 3, crowded ? ln - 1 : ln + 1 /* odd strides are fine here */, norm,
                    static_cast<const uint32_t *>(off_by(bits, unaligned ? 2 : 0)), 64);
}

// pha_encrypt_symmetric_batched (with_plain; bgv: plain is N words and may be shared) and pha_encrypt_zero_symmetric_batched (over
// the special primes too)
static const char *kFloor17 = "a sample of magnitude 2^16 needs every prime of the rows used at or above 2^17";
static const char *kCount = "count out of range", *kCtSize = "ct stride below the size of a ciphertext: the ciphertexts overlap";
static const char *kNoP = "context has no special modulus", *kDegree = "poly_modulus_degree below 8: a generator block is eight words";
static const std::vector<const char *> kEncryptTable{kNull, kLevel, kFloor17, kScheme, kNoT, kCount, kCtSize,
                                                     "e stride below the size of an element: the elements overlap",
                                                     "plain stride below the size of an element: the elements overlap", kEvenLoads, kAligned16,
                                                     "ct must not overlap sk_ntt", "ct must not overlap e", "ct must not overlap plain"};
static const std::vector<const char *> kEncryptZeroTable{kNull, kLevel, kNoP, kFloor17, kScheme, kNoT, kCount, kCtSize,
                                                         "e stride below the size of an element: the elements overlap", kEvenLoads, kAligned16,
                                                         "ct must not overlap sk_ntt", "ct must not overlap e"};
static std::vector<uint64_t> small_primes(4, 65537);
static void call_encrypt(bool with_plain, uint32_t mask) {
    int r = 0;
    const bool null = has(mask, r++), level = has(mask, r++), no_p = with_plain ? false : has(mask, r++), floor = has(mask, r++),
               scheme = has(mask, r++), no_t = has(mask, r++), count = has(mask, r++), ct_crowded = has(mask, r++), e_crowded = has(mask, r++),
               p_crowded = with_plain ? has(mask, r++) : false, odd = has(mask, r++), unaligned = has(mask, r++), on_sk = has(mask, r++),
               on_e = has(mask, r++), on_p = with_plain ? has(mask, r++) : false;
    ContextShape cx = shape(3, no_p ? 0 : 1, no_t ? 0 : 65537);
    if (floor) cx.primes = small_primes.data();
    const size_t size_Ql = level ? 4 : 2, n = cx.n, words = 2 * (size_Ql + (with_plain ? 0 : cx.size_p)) * n, B = count ? 65536 : 3;
    const uint64_t *ct = at(1024), *sk = on_sk ? ct + 2 : at(8192), *e = on_e ? ct + 4 : at(16384), *plain = on_p ? ct + 6 : at(20480);
    check_encrypt(cx, size_Ql, !with_plain, false, scheme ? 0 : PHA_SCHEME_BGV, null ? nullptr : sk, nullptr, 0, e, n + (e_crowded ? -2 : 2) + (odd ? 1 : 0),
                  with_plain ? plain : nullptr, with_plain ? n : 0, p_crowded ? n - 2 : (with_plain ? n + 2 : 0), unaligned ? ct + 1 : ct,
                  words + (ct_crowded ? -2 : 2), B);
}
// pha_encrypt_asymmetric_batched (ckks: plain is L * N words)
static const std::vector<const char *> kAsymmetricTable{kNull, kLevel, kNoP, kFloor17, kScheme, kNoT, kCount, kCtSize,
                                                        "u stride below the size of an element: the elements overlap",
                                                        "e stride below the size of an element: the elements overlap",
                                                        "plain stride below the size of an element: the elements overlap", kEvenLoads, kAligned16,
                                                        "ct must not overlap pk", "ct must not overlap u", "ct must not overlap e", "ct must not overlap plain"};
static void call_asymmetric(uint32_t mask) {
    int r = 0;
    const bool null = has(mask, r++), level = has(mask, r++), no_p = has(mask, r++), floor = has(mask, r++), scheme = has(mask, r++),
               no_t = has(mask, r++), count = has(mask, r++), ct_crowded = has(mask, r++), u_crowded = has(mask, r++), e_crowded = has(mask, r++),
               p_crowded = has(mask, r++), odd = has(mask, r++), unaligned = has(mask, r++), on_pk = has(mask, r++), on_u = has(mask, r++),
               on_e = has(mask, r++), on_p = has(mask, r++);
    ContextShape cx = shape(3, no_p ? 0 : 1, no_t ? 0 : 65537);
    if (floor) cx.primes = small_primes.data();
    const size_t size_Ql = level ? 4 : 2, n = cx.n, ln = size_Ql * n;
    const uint64_t *ct = at(1024), *pk = on_pk ? ct + 2 : at(8192), *u = on_u ? ct + 4 : at(12288), *e = on_e ? ct + 6 : at(16384),
                   *plain = on_p ? ct + 8 : at(20480);
    check_encrypt(cx, size_Ql, true, true, scheme ? 0 : PHA_SCHEME_BFV, null ? nullptr : pk, u, n + (u_crowded ? -2 : 2), e,
                  2 * n + (e_crowded ? -2 : 2) + (odd ? 1 : 0), plain, n, p_crowded ? n - 2 : n + 2, unaligned ? ct + 1 : ct,
                  2 * ln + (ct_crowded ? -2 : 2), count ? 65536 : 3);
}

// the batched samplers: pha_sample_uniform_batched (rows of a level) and pha_sample_{ternary,error}_signed_batched ([N] signed words)
static const char *kOutCrowded = "out stride below the size of an element: the elements overlap";
static const std::vector<const char *> kUniformTable{kNull, kDegree, kLevel, kNoP, kCount, kEvenStores, kOutCrowded, kAligned16};
static const std::vector<const char *> kSignedTable{kNull, kDegree, kCount, kEvenStores, kOutCrowded, kAligned16};
static void call_sample_batch(bool uniform, uint32_t mask) {
    int r = 0;
    const bool null = has(mask, r++), degree = has(mask, r++), level = uniform ? has(mask, r++) : false, special = uniform ? has(mask, r++) : false,
               count = has(mask, r++), odd = has(mask, r++), crowded = has(mask, r++), unaligned = has(mask, r++);
    ContextShape cx = shape(3, special ? 0 : 1, 0);
    if (degree) cx.n = 4;
    const size_t size_Ql = level ? 4 : 2, words = uniform ? (size_Ql + cx.size_p) * cx.n : cx.n;
    const uint64_t *out = at(1024), *seeds = at(8192);
    check_sample_batch(cx, uniform, uniform ? size_Ql : 0, uniform, static_cast<const uint8_t *>(null ? nullptr : (unaligned ? off_by(seeds, 8) : seeds)),
                       count ? 65536 : 3, out, words + (crowded ? -2 : 2) + (odd ? 1 : 0));
}
// pha_sample_error_poly (pha_sample_ternary_poly, pha_sample_uniform_poly: no prime floor); 65536 rows need a table no context has
static const std::vector<const char *> kRefTable{kNull, kDegree, kLevel, "coeff_mod_size out of range",
                                                 "a sample of magnitude 21 needs every prime of the rows used above 21", kAligned16};
static std::vector<uint64_t> many_small(70001, 19);
static void call_sample_ref(uint32_t mask) {
    int r = 0;
    const bool null = has(mask, r++), degree = has(mask, r++), level = has(mask, r++), many = has(mask, r++), floor = has(mask, r++),
               unaligned = has(mask, r++);
    ContextShape cx{degree ? (size_t)4 : 8, 70000, 1, 70001, 0, floor ? many_small.data() : nullptr};
    const size_t cms = level ? 70002 : many ? 65536 : 2;
    check_sample_ref(cx, null ? nullptr : (unaligned ? at(1) : at(0)), (const uint8_t *)at(64), cms, 0, floor ? kNoiseMinPrime : 0);
}
// pha_generate_kswitch_keys_seeded; whether bgv is ready is the entry's to say (its tables), asked at its place in the order
static const std::vector<const char *> kKswitchTable{kNull, kDegree, kNoP, "#Q must be a multiple of special_modulus_size", kScheme,
                                                     "bgv needs a plain modulus (pha_context_set_plain_modulus)", "n_keys out of range",
                                                     kEvenStores, "evk stride below 2 * size_QP * N: the components overlap",
                                                     "new_key stride below size_Q * N: the keys overlap", kAligned16, "evk must not overlap an input"};
static void call_kswitch(uint32_t mask) {
    int r = 0;
    const bool null = has(mask, r++), degree = has(mask, r++), no_p = has(mask, r++), ragged = has(mask, r++), scheme = has(mask, r++),
               not_ready = has(mask, r++), keys = has(mask, r++), odd = has(mask, r++), evk_crowded = has(mask, r++), key_crowded = has(mask, r++), unaligned = has(mask, r++),
               overlap = has(mask, r++);
    ContextShape cx = shape(ragged ? 3 : 4, no_p ? 0 : 2, 0);
    if (degree) cx.n = 4;
    const size_t qp_n = (size_t)cx.size_qp * cx.n, q_n = (size_t)cx.size_q * cx.n, n_keys = keys ? 65535 : 2;
    const uint64_t *sk = at(1024), *new_keys = at(2048), *evk = overlap ? sk + 2 : at(8192);
    const uint8_t *seeds = (const uint8_t *)at(4096);
    const uint64_t *sk_arg = null ? nullptr : (unaligned ? sk + 1 : sk);
    const size_t dnum = check_kswitch(cx, sk_arg, new_keys, n_keys, q_n + (key_crowded ? -2 : 2), seeds, evk, 2 * qp_n + (evk_crowded ? -2 : 2) + (odd ? 1 : 0),
                                      scheme ? 0 : PHA_SCHEME_BGV, [&] { return !not_ready; });
    EXPECT(dnum == 2, "kswitch: dnum %zu", dnum);
}

static void check_table(const char *entry, const std::vector<const char *> &table, const std::function<void(uint32_t)> &call) {
    const int rules = (int)table.size();
    accepted(entry, [&] { call(0); });
    for (int i = 0; i < rules; i++) {
        refused(std::string(entry) + ", rule " + std::to_string(i) + " alone", table[i], [&] { call(1u << i); });
        refused(std::string(entry) + ", rule " + std::to_string(i) + " and every later one", table[i], [&] { call(from(i, rules)); });
    }
}

// the noise entry refuses what the decrypt entries refuse, in their order, but for four differences
static void check_tables_agree() {
    std::vector<const char *> shared;
    for (const char *m : kNoiseTable)
        if (m != kScheme && m != kCap && m != kAlignedWords && std::strncmp(m, "budget", 6) && std::strncmp(m, "norm", 4)) shared.push_back(m);
    std::vector<const char *> want;
    for (const char *m : kDecryptTable)
        if (m != kDstCrowded && std::strncmp(m, "dst must", 8)) want.push_back(m);
    EXPECT(shared == want, "tables: the noise entry's shared refusals are not the decrypt entries', in their order");
    EXPECT(kNoiseTable[1] == kScheme && kNoiseTable[2] == kLevel, "tables: the noise entry checks the scheme before the level");
    EXPECT(kNoiseTable[3] == kCap && kNoiseTable[4] == kNoT, "tables: the noise entry's 64-limb cap is part of its level check");
    for (const char *m : kNoiseTable) EXPECT(m != kDstCrowded, "tables: the noise entry has no dst-stride rule");
    EXPECT(kNoiseTable[10] == kAligned16 && kNoiseTable[11] == kAlignedWords, "tables: the noise entry's word-alignment rule follows the 16-byte one");
    std::vector<const char *> phase = kDecryptTable;
    phase.erase(phase.begin() + 2);
    EXPECT(phase == kPhaseTable, "tables: the phase entry refuses what the bgv / bfv entries refuse, but for the plain modulus");
}

// ---- refusals no table reaches, and what must be accepted ----------------------------------------------------------------------------
static void check_singles() {
    const ContextShape cx = shape(3, 1, 65537), ckks = shape(3, 1, 0), big = shape(70, 1, 65537);
    const uint64_t *ct = at(1024), *sk = at(8192), *dst = at(16384);
    const size_t ln = 2 * cx.n;
    const CtBatch b{ct, 3, 3, 3 * ln + 2, sk, 2};
    auto with = [](CtBatch v, size_t k, size_t batch, size_t stride) { v.cipher_size = k; v.batch = batch; v.ct_stride = stride; return v; };
    refused("level 0", kLevel, [&] { check_decrypt(cx, 0, b, dst, ln, ln, true, false); });
    refused("cipher_size 1", kCipher, [&] { check_decrypt(cx, 2, with(b, 1, 3, 3 * ln), dst, ln, ln, true, false); });
    refused("null sk_powers", kNull, [&] { CtBatch v = b; v.sk_powers = nullptr; check_decrypt(cx, 2, v, dst, ln, ln, true, false); });
    refused("null dst", kNull, [&] { check_decrypt(cx, 2, b, nullptr, ln, ln, true, false); });
    refused("odd dst stride", kEvenLoads, [&] { check_decrypt(cx, 2, b, dst, ln + 1, ln, true, false); });
    refused("sk_powers off by 8 bytes", kAligned16, [&] { CtBatch v = b; v.sk_powers = sk + 1; check_decrypt(cx, 2, v, dst, ln, ln, true, false); });
    // the in-place exemption: dst == ct at ct's stride (any stride for one ciphertext), for the phase entry alone
    accepted("phase in place", [&] { check_decrypt(cx, 2, b, ct, b.ct_stride, ln, true, false); });
    accepted("phase in place, one ciphertext", [&] { check_decrypt(cx, 2, with(b, 3, 1, 0), ct, 0, ln, true, false); });
    refused("phase in place at another stride", "dst must not overlap ct", [&] { check_decrypt(cx, 2, b, ct, b.ct_stride + 2, ln, true, false); });
    refused("phase onto c1", "dst must not overlap ct", [&] { check_decrypt(cx, 2, b, ct + ln, b.ct_stride, ln, true, false); });
    refused("decrypt in place", "dst must not overlap ct", [&] { check_decrypt(cx, 2, b, ct, b.ct_stride, cx.n, false, true); });
    refused("phase onto sk_powers, one ciphertext", "dst must not overlap sk_powers", [&] { check_decrypt(cx, 2, with(b, 3, 1, 0), sk, 0, ln, true, false); });
    accepted("dst abuts ct", [&] { check_decrypt(cx, 2, b, ct + 2 * b.ct_stride + 3 * ln, ln, ln, true, false); });
    accepted("empty batch, overlapping", [&] { check_decrypt(cx, 2, with(b, 3, 0, 0), ct + 2, 0, ln, true, false); });
    accepted("the largest batch", [&] { check_count(kPhaseBatchMax, kPhaseBatchMax, "batch out of range"); });
    // the noise budget: ckks needs no plain modulus, norm is optional, an empty batch is accepted before the overlaps
    accepted("noise, ckks without t", [&] { EXPECT(check_noise_budget(ckks, 2, b, PHA_SCHEME_CKKS, (const int32_t *)dst, nullptr, 64), "ckks is NTT form"); });
    accepted("noise, bfv", [&] { EXPECT(!check_noise_budget(cx, 2, b, PHA_SCHEME_BFV, (const int32_t *)dst, dst + 64, 64), "bfv is coefficient form"); });
    refused("noise, bgv without t", kNoT, [&] { check_noise_budget(ckks, 2, b, PHA_SCHEME_BGV, (const int32_t *)dst, nullptr, 64); });
    accepted("noise, 64 limbs", [&] { check_noise_budget(big, 64, with(b, 3, 1, 0), PHA_SCHEME_BGV, (const int32_t *)dst, nullptr, 64); });
    accepted("noise, budget abuts norm", [&] { check_noise_budget(cx, 2, b, PHA_SCHEME_BFV, (const int32_t *)dst, dst + 2, 64); });
    refused("noise, norm on the budget's second pair", "norm must not overlap budget",
            [&] { check_noise_budget(cx, 2, b, PHA_SCHEME_BFV, (const int32_t *)dst, dst + 1, 64); });
    accepted("noise, budget off by 4 bytes", [&] { check_noise_budget(cx, 2, b, PHA_SCHEME_BFV, (const int32_t *)off_by(dst, 4), nullptr, 64); });
    accepted("poly norm without norm", [&] { check_poly_norm(cx, 2, ct, 3, ln, nullptr, (const uint32_t *)dst, 64); });
    accepted("any count of polynomials", [&] { check_poly_norm(cx, 2, at(60000), 70000, ln, nullptr, (const uint32_t *)at(0), 64); });
    // rows and schemes
    std::vector<uint64_t> mixed{((uint64_t)1 << 17) + 29, 131071, 23, 19};   // Q = the first three, P = the last
    const ContextShape m{8, 3, 1, 4, 65537, mixed.data()};
    accepted("a prime of 2^17 + 29", [&] { check_rows(m, 1, false, kEncryptMinPrime); });
    refused("a prime of 2^17 - 1", kFloor17, [&] { check_rows(m, 2, false, kEncryptMinPrime); });
    refused("a small special prime", kFloor17, [&] { check_rows(m, 1, true, kEncryptMinPrime); });
    accepted("uniform rows over any primes", [&] { check_rows(m, 3, true, 0); });
    refused("special rows without P", "context has no special modulus", [&] { check_rows(shape(3, 0, 0), 1, true, kEncryptMinPrime); });
    const char *k21 = kRefTable[4];
    accepted("noise residues modulo 23", [&] { check_sample_ref(m, at(0), (const uint8_t *)at(64), 1, 2, kNoiseMinPrime); });
    refused("noise residues modulo 19", k21, [&] { check_sample_ref(m, at(0), (const uint8_t *)at(64), 2, 2, kNoiseMinPrime); });
    accepted("ternary residues modulo 19", [&] { check_sample_ref(m, at(0), (const uint8_t *)at(64), 4, 0, 0); });
    refused("no rows", kLevel, [&] { check_sample_ref(m, at(0), (const uint8_t *)at(64), 0, 0, 0); });
    refused("rows from past the table", kLevel, [&] { check_sample_ref(m, at(0), (const uint8_t *)at(64), 1, 5, 0); });
    refused("rows past the table's end", kLevel, [&] { check_sample_ref(m, at(0), (const uint8_t *)at(64), 3, 2, 0); });
    const ContextShape wide{8, 70000, 1, 70001, 0, nullptr};
    refused("65536 rows", "coeff_mod_size out of range", [&] { check_sample_ref(wide, at(0), (const uint8_t *)at(64), 65536, 0, 0); });
    accepted("ckks without t", [&] { check_scheme(ckks, PHA_SCHEME_CKKS); });
    accepted("bfv with t", [&] { check_scheme(cx, PHA_SCHEME_BFV); });
    refused("bgv without t", kNoT, [&] { check_scheme(ckks, PHA_SCHEME_BGV); });
    refused("bfv without t", kNoT, [&] { check_scheme(ckks, PHA_SCHEME_BFV); });
    refused("scheme 0", kScheme, [&] { check_scheme(cx, 0); });
    // pha_generate_kswitch_keys_seeded: its own texts through the same pieces
    const EncBuf evk{"evk", ct, 16, 14, false, true, 16, "evk stride below 2 * size_QP * N: the components overlap"};
    const EncBuf keys{"new_keys", sk, 8, 9, false, false, 16, "new_key stride below size_Q * N: the keys overlap"};
    refused("odd new_key stride", kEvenStores, [&] { check_even({evk, keys}, kEvenStores); });
    refused("evk components overlap", "evk stride below 2 * size_QP * N: the components overlap", [&] { check_crowded(evk, 2); });
    accepted("one evk component at any stride", [&] { check_crowded(evk, 1); });
    refused("asymmetric: u elements overlap", "u stride below the size of an element: the elements overlap", [&] { check_crowded(EncBuf{"u", sk, 8, 6, false}, 2); });
    refused("a shared e", "e stride below the size of an element: the elements overlap", [&] { check_crowded(EncBuf{"e", sk, 8, 0, false}, 2); });
    accepted("a shared plain", [&] { check_crowded(EncBuf{"plain", sk, 8, 0, true}, 2); });
    refused("asymmetric: ct on pk", "ct must not overlap pk", [&] { check_overlap({EncBuf{"ct", ct, 8, 8, false, true}, EncBuf{"pk", ct + 23, 8, 0, true}}, 3); });
    accepted("ct abuts pk", [&] { check_overlap({EncBuf{"ct", ct, 8, 8, false, true}, EncBuf{"pk", ct + 24, 8, 0, true}}, 3); });
}

// ---- chunk size and work-buffer words against the formulas the three chunked entries wrote out ---------------------------------------------
static size_t check_chunks() {
    size_t cases = 0;
    const size_t ln = 3 * 4096, kDefault = 8;
    for (size_t k : {2, 3, 65535})
    for (size_t batch : {1, 8, 9, 65536})
    for (size_t chunk : {0, 1, 3, 1000000}) {
        const size_t km1 = k - 1;
        const size_t c_ntt = std::min<size_t>(std::min(chunk ? chunk : kDefault, batch), 65535);
        const size_t c_bfv = std::min<size_t>(std::min(chunk ? chunk : kDefault, batch), 65535 / km1 ? 65535 / km1 : 1);
        const PhaseChunk ntt = phase_chunk(true, k, ln, batch, chunk, kDefault), bfv = phase_chunk(false, k, ln, batch, chunk, kDefault);
        EXPECT(ntt.C == c_ntt && ntt.wst == ln && ntt.C * ntt.wst == c_ntt * ln, "chunk: NTT form, k %zu batch %zu chunk %zu: %zu x %zu", k, batch, chunk, ntt.C, ntt.wst);
        EXPECT(bfv.C == c_bfv && bfv.wst == km1 * ln && bfv.C * bfv.wst == c_bfv * km1 * ln, "chunk: bfv, k %zu batch %zu chunk %zu: %zu x %zu", k, batch, chunk, bfv.C, bfv.wst);
        EXPECT(ntt.C >= 1 && bfv.C >= 1 && bfv.C * km1 <= std::max<size_t>(65535, km1), "chunk: outside the grid");
        cases++;
    }
    return cases;
}

int main() {
    EXPECT((reinterpret_cast<uintptr_t>(arena.data()) & 15) == 0, "the arena is not 16-byte aligned");
    const size_t layouts = sweep_overlap();
    check_table("decrypt_phase", kPhaseTable, [](uint32_t m) { call_decrypt(true, m); });
    check_table("bgv / bfv decrypt", kDecryptTable, [](uint32_t m) { call_decrypt(false, m); });
    check_table("noise_budget", kNoiseTable, call_noise);
    check_table("poly_infty_norm", kNormTable, call_norm);
    check_table("encrypt_symmetric", kEncryptTable, [](uint32_t m) { call_encrypt(true, m); });
    check_table("encrypt_zero_symmetric", kEncryptZeroTable, [](uint32_t m) { call_encrypt(false, m); });
    check_table("encrypt_asymmetric", kAsymmetricTable, call_asymmetric);
    check_table("sample_uniform_batched", kUniformTable, [](uint32_t m) { call_sample_batch(true, m); });
    check_table("sample_signed_batched", kSignedTable, [](uint32_t m) { call_sample_batch(false, m); });
    check_table("sample_ref", kRefTable, call_sample_ref);
    check_table("generate_kswitch_keys_seeded", kKswitchTable, call_kswitch);
    check_tables_agree();
    check_singles();
    const size_t chunks = check_chunks();
    if (bad) {
        std::printf("FAILED: %d expectation(s)\n", bad);
        return 1;
    }
    std::printf("layout OK (%zu layouts, %zu chunk cases): overlap, refusals, their order, chunks\n", layouts, chunks);
    return 0;
}
