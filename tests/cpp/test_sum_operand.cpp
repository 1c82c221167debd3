// test_sum_operand.cpp -- TEST-ONLY, host only (no device is touched): SumOperand of phantom-fhe_amd/csrc/pha_sum_operand.h, the view of
// a strided operand behind the summed-product entries.  Built with -fsanitize=address,undefined and run by tests/test_sum_operand.py.
// Every pointer lies inside one arena and none is dereferenced.
//   touches:  equals the brute-force intersection of word sets for an output window slid across and past both ends of the operand's
//             span; false, without a wrapped span, for an empty batch or no terms.
//   strict:   the runs visit every distinct polynomial exactly once and nothing else (a shared operand once, not per group), none
//             longer than its cap (3 and 4 injected); at the real cap, 32767 / 32768 / 65535 / 65536 terms give the run lists of the
//             loops the entries used to write out (restated below as formulas).
//   advanced: the view moved by (g0, k0) addresses element (g0 + g, k0 + k) of the original.
//   refusals: exception class and exact text, one defect per case, and the first in order for two defects at once.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>
#include <typeinfo>
#include <vector>

#include "../../phantom-fhe_amd/csrc/pha_sum_operand.h"

using pha::SumOperand;

static int bad = 0;
#define EXPECT(cond, ...)             \
    do {                              \
        if (!(cond)) {                \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            bad++;                    \
        }                             \
    } while (0)

static std::vector<uint64_t> arena(1 << 20);   // 8 MiB: 65536 terms of 4 words at a stride of 6, twice, fit
typedef std::tuple<const uint64_t *, size_t, size_t> Run;   // base, polynomials, words between them

static std::vector<Run> runs_of(const SumOperand &op, size_t terms, size_t batch, size_t cap = 0) {
    std::vector<Run> r;
    auto take = [&](const uint64_t *base, size_t polys, size_t stride) { r.emplace_back(base, polys, stride); };
    if (cap) op.strict_runs(terms, batch, take, cap);
    else op.strict_runs(terms, batch, take);
    return r;
}

// the small sweep: words 2, 4; one- and two-polynomial elements; terms and batch 0 .. 3; term stride words, words + 2, and 0 at one
// term or none; batch stride 0 (shared), dense, dense + 2
template <class F>
static size_t sweep(F &&fn) {
    size_t cases = 0;
    for (size_t words : {2, 4})
    for (size_t polys : {1, 2})
    for (size_t terms = 0; terms <= 3; terms++)
    for (size_t batch = 0; batch <= 3; batch++)
    for (size_t ts : {words, words + 2, (size_t)0}) {
        if (ts == 0 && terms > 1) continue;
        const size_t dense = terms * ts;
        for (size_t bs : {(size_t)0, dense, dense + 2}) {
            fn(SumOperand{arena.data() + 64, ts, bs, words, polys, "crowded"}, terms, batch);
            cases++;
        }
    }
    return cases;
}

// the words of the operand, by definition: every group of a batch has `terms` elements; with bs == 0 all groups share one set
static std::vector<const uint64_t *> element_starts(const SumOperand &op, size_t terms, size_t batch) {
    std::vector<const uint64_t *> e;
    const size_t groups = op.bs ? batch : (batch ? 1 : 0);
    for (size_t g = 0; g < groups; g++)
        for (size_t k = 0; k < terms; k++) e.push_back(op.p + g * op.bs + k * op.ts);
    return e;
}

static void check_touches(const SumOperand &op, size_t terms, size_t batch) {
    const std::vector<const uint64_t *> elts = element_starts(op, terms, batch);
    const size_t span = 3 * (3 * (op.words + 2) + 2) + op.words;   // beyond the last word of the largest case
    for (size_t out_words : {(size_t)1, (size_t)2, op.words + 1}) {
        for (const uint64_t *out = op.p - out_words - 2; out < op.p + span + 2; out++) {
            bool want = false;
            for (const uint64_t *e : elts)
                for (size_t w = 0; w < op.words; w++) want = want || (e + w >= out && e + w < out + out_words);
            const bool got = op.touches(out, out_words, terms, batch);
            EXPECT(got == want, "touches: words %zu terms %zu batch %zu ts %zu bs %zu window %td + %zu: got %d, want %d", op.words, terms, batch,
                   op.ts, op.bs, out - op.p, out_words, (int)got, (int)want);
            if (batch == 0 || terms == 0) EXPECT(!got, "touches: true for an empty operand (batch %zu, terms %zu)", batch, terms);
        }
    }
}

static void check_runs_cover(const SumOperand &op, size_t terms, size_t batch) {
    const size_t pw = op.words / op.polys;
    std::vector<const uint64_t *> want;
    for (const uint64_t *e : element_starts(op, terms, batch))
        for (size_t h = 0; h < op.polys; h++) want.push_back(e + h * pw);
    std::sort(want.begin(), want.end());
    for (size_t cap : {(size_t)3, (size_t)4, (size_t)0}) {
        std::vector<const uint64_t *> got;
        for (const Run &r : runs_of(op, terms, batch, cap)) {
            const size_t limit = cap ? cap : pha::kStrictRunPolys;
            EXPECT(std::get<1>(r) >= 1 && std::get<1>(r) <= limit, "strict: a run of %zu polynomials at a cap of %zu", std::get<1>(r), limit);
            for (size_t i = 0; i < std::get<1>(r); i++) got.push_back(std::get<0>(r) + i * std::get<2>(r));
        }
        std::sort(got.begin(), got.end());
        EXPECT(got == want, "strict: words %zu polys %zu terms %zu batch %zu ts %zu bs %zu cap %zu: %zu polynomials visited, %zu distinct ones exist",
               op.words, op.polys, terms, batch, op.ts, op.bs, cap, got.size(), want.size());
    }
}

// at the real cap: the loops the entries used to write out, as formulas.  ln = words of one polynomial
static void check_runs_at_real_caps() {
    const size_t ln = 2;
    for (size_t terms : {32767, 32768, 65535, 65536})
    for (size_t batch : {1, 2}) {
        for (size_t ts : {2 * ln, 2 * ln + 2}) {   // ciphertext operands: dense rows, or c0 of every term and then c1
            for (size_t bs : {(size_t)0, terms * ts}) {
                const SumOperand op{arena.data(), ts, bs, 2 * ln, 2, "crowded"};
                std::vector<Run> want;
                for (size_t g = 0; g < (bs ? batch : 1); g++) {
                    const uint64_t *base = op.p + g * bs;
                    if (terms == 1 || ts == 2 * ln) {
                        for (size_t k0 = 0; k0 < terms; k0 += 32767)
                            want.emplace_back(base + k0 * 2 * ln, 2 * std::min<size_t>(32767, terms - k0), ln);
                    } else {
                        for (size_t half = 0; half < 2; half++)
                            for (size_t k0 = 0; k0 < terms; k0 += 65535)
                                want.emplace_back(base + half * ln + k0 * ts, std::min<size_t>(65535, terms - k0), ts);
                    }
                }
                EXPECT(runs_of(op, terms, batch) == want, "strict: ciphertext runs at %zu terms, batch %zu, ts %zu, bs %zu differ", terms, batch, ts, bs);
            }
        }
        for (size_t tp : {ln, ln + 2}) {           // one-polynomial operands
            for (size_t bp : {(size_t)0, terms * tp}) {
                const SumOperand op{arena.data(), tp, bp, ln, 1, "crowded"};
                std::vector<Run> want;
                for (size_t g = 0; g < (bp ? batch : 1); g++)
                    for (size_t k0 = 0; k0 < terms; k0 += 65535)
                        want.emplace_back(op.p + g * bp + k0 * tp, std::min<size_t>(65535, terms - k0), tp);
                EXPECT(runs_of(op, terms, batch) == want, "strict: plaintext runs at %zu terms, batch %zu, tp %zu, bp %zu differ", terms, batch, tp, bp);
            }
        }
    }
    // without a cap (raw plaintexts: their count cuts a group's terms itself) a one-polynomial operand is one run per group
    const SumOperand raw{arena.data(), 4, 65536 * 4, 2, 1, "crowded"};
    const std::vector<Run> whole{Run(raw.p, 65536, 4), Run(raw.p + 65536 * 4, 65536, 4)};
    EXPECT(runs_of(raw, 65536, 2, SIZE_MAX) == whole, "strict: the uncapped runs of a one-polynomial operand differ");
    // an addend: one ciphertext per group, the two polynomials in a row
    const SumOperand acc{arena.data(), 0, 10, 2 * ln, 2, nullptr};
    const std::vector<Run> want{Run(acc.p, 2, ln), Run(acc.p + 10, 2, ln), Run(acc.p + 20, 2, ln)};
    EXPECT(runs_of(acc, 1, 3) == want, "strict: the runs of an addend differ");
}

static void check_advanced(const SumOperand &op, size_t, size_t) {
    for (size_t g0 = 0; g0 < 3; g0++)
    for (size_t k0 = 0; k0 < 3; k0++) {
        const SumOperand v = op.advanced(g0, k0);
        EXPECT(v.ts == op.ts && v.bs == op.bs && v.words == op.words && v.polys == op.polys && v.crowded == op.crowded,
               "advanced: a field other than the base changed");
        for (size_t g = 0; g < 3; g++)
            for (size_t k = 0; k < 3; k++)
                EXPECT(v.at(g, k) == op.at(g0 + g, k0 + k), "advanced (%zu, %zu): element (%zu, %zu) is not the original's", g0, k0, g, k);
    }
    SumOperand none = op;
    none.p = nullptr;
    EXPECT(none.advanced(2, 1).p == nullptr, "advanced: an absent operand became present");
}

template <class F>
static void refused(const char *what, const char *text, F &&fn) {
    try {
        fn();
        EXPECT(false, "refusals: %s was accepted", what);
    } catch (const std::exception &e) {
        EXPECT(typeid(e) == typeid(std::invalid_argument), "refusals: %s threw %s", what, typeid(e).name());
        EXPECT(std::strcmp(e.what(), text) == 0, "refusals: %s says \"%s\", want \"%s\"", what, e.what(), text);
    }
}

static void check_refusals() {
    const char *kEven = "strides must be even (16-byte loads)", *kAligned = "buffers must be 16-byte aligned";
    const char *kSum = "term stride below 2 * L * N: the terms of an operand overlap";
    const char *kPlainL = "plain term stride below L * N: the terms of plain overlap", *kPlainN = "plain term stride below N: the terms of plain overlap";
    const char *kCt = "ct term stride below 2 * L * N: the terms of ct overlap";
    const uint64_t *base = arena.data();   // 16-byte aligned (the allocator's alignment), as is base + 2 k
    EXPECT((reinterpret_cast<uintptr_t>(base) & 15) == 0, "the arena is not 16-byte aligned");
    const size_t ln = 4, terms = 3;
    const SumOperand plain{base, ln, terms * ln, ln, 1, kPlainL}, ct{base + 64, 2 * ln, terms * 2 * ln, 2 * ln, 2, kCt},
        acc{base + 256, 0, 2 * ln, 2 * ln, 2, nullptr}, none{nullptr, 0, 2 * ln, 2 * ln, 2, nullptr};
    auto with = [](SumOperand o, size_t ts, size_t bs, const uint64_t *p) { o.ts = ts; o.bs = bs; o.p = p; return o; };
    // nothing wrong: accepted, an absent addend and one term at a term stride of 0 included
    pha::sum_check_terms(1);
    pha::sum_check_terms(0xffffffffull);
    pha::sum_check_layout({plain, ct, acc}, terms, base + 512);
    pha::sum_check_layout({plain, ct, none}, terms);
    pha::sum_check_layout({with(plain, 0, 0, plain.p), with(ct, 0, 0, ct.p), acc}, 1);
    pha::sum_check_layout({plain, ct, with(acc, 0, 0, acc.p)}, terms);   // an addend has no term stride to refuse
    // one defect per case
    refused("no terms", "terms must be at least 1", [&] { pha::sum_check_terms(0); });
    refused("2^32 terms", "terms out of range", [&] { pha::sum_check_terms(0x100000000ull); });
    refused("odd plain term stride", kEven, [&] { pha::sum_check_layout({with(plain, ln + 1, plain.bs, plain.p), ct, acc}, terms); });
    refused("odd plain batch stride", kEven, [&] { pha::sum_check_layout({with(plain, ln, plain.bs + 1, plain.p), ct, acc}, terms); });
    refused("odd ct term stride", kEven, [&] { pha::sum_check_layout({plain, with(ct, 2 * ln + 1, ct.bs, ct.p), acc}, terms); });
    refused("odd ct batch stride", kEven, [&] { pha::sum_check_layout({plain, with(ct, 2 * ln, ct.bs + 1, ct.p), acc}, terms); });
    refused("odd acc batch stride", kEven, [&] { pha::sum_check_layout({plain, ct, with(acc, 0, 2 * ln + 1, acc.p)}, terms); });
    refused("odd stride of an absent acc", kEven, [&] { pha::sum_check_layout({plain, ct, with(none, 0, 2 * ln + 1, nullptr)}, terms); });
    refused("plain off by 8 bytes", kAligned, [&] { pha::sum_check_layout({with(plain, plain.ts, plain.bs, plain.p + 1), ct, acc}, terms); });
    refused("ct off by 8 bytes", kAligned, [&] { pha::sum_check_layout({plain, with(ct, ct.ts, ct.bs, ct.p + 1), acc}, terms); });
    refused("acc off by 8 bytes", kAligned, [&] { pha::sum_check_layout({plain, ct, with(acc, 0, acc.bs, acc.p + 1)}, terms); });
    refused("the output off by 8 bytes", kAligned, [&] { pha::sum_check_layout({plain, ct, acc}, terms, base + 513); });
    refused("plain terms overlap", kPlainL, [&] { pha::sum_check_layout({with(plain, ln - 2, plain.bs, plain.p), ct, acc}, terms); });
    refused("plain term stride 0", kPlainL, [&] { pha::sum_check_layout({with(plain, 0, plain.bs, plain.p), ct, acc}, 2); });
    SumOperand raw = plain;
    raw.crowded = kPlainN;
    refused("raw plain terms overlap", kPlainN, [&] { pha::sum_check_layout({with(raw, ln - 2, raw.bs, raw.p), ct, acc}, terms); });
    refused("ct terms overlap", kCt, [&] { pha::sum_check_layout({plain, with(ct, 2 * ln - 2, ct.bs, ct.p), acc}, terms); });
    SumOperand a = ct, b = ct;
    a.crowded = b.crowded = kSum;
    refused("operand 1 terms overlap", kSum, [&] { pha::sum_check_layout({with(a, 2 * ln - 2, a.bs, a.p), b}, terms); });
    refused("operand 2 terms overlap", kSum, [&] { pha::sum_check_layout({a, with(b, 0, b.bs, b.p)}, terms); });
    // two defects at once: parity before alignment before the term strides, and those in the order of the operands
    refused("odd stride and misaligned", kEven, [&] { pha::sum_check_layout({with(plain, ln + 1, plain.bs, plain.p + 1), ct, acc}, terms); });
    refused("odd ct stride and plain terms overlap", kEven,
            [&] { pha::sum_check_layout({with(plain, ln - 2, plain.bs, plain.p), with(ct, ct.ts, ct.bs + 1, ct.p), acc}, terms); });
    refused("misaligned output and ct terms overlap", kAligned,
            [&] { pha::sum_check_layout({plain, with(ct, 2 * ln - 2, ct.bs, ct.p), acc}, terms, base + 513); });
    refused("plain and ct terms overlap", kPlainL,
            [&] { pha::sum_check_layout({with(plain, ln - 2, plain.bs, plain.p), with(ct, 2 * ln - 2, ct.bs, ct.p), acc}, terms); });
    refused("everything at once", kEven,
            [&] { pha::sum_check_layout({with(plain, ln - 1, plain.bs, plain.p + 1), with(ct, 2 * ln - 2, ct.bs, ct.p), acc}, terms, base + 513); });
}

int main() {
    EXPECT(pha::overlaps(arena.data(), 4, arena.data() + 3, 1) && !pha::overlaps(arena.data(), 4, arena.data() + 4, 1) &&
               !pha::overlaps(arena.data() + 4, 0, arena.data(), 4) && pha::overlaps(arena.data() + 1, 1, arena.data(), 4),
           "overlaps: wrong at an edge");
    const size_t cases = sweep([](const SumOperand &op, size_t terms, size_t batch) {
        check_touches(op, terms, batch);
        check_runs_cover(op, terms, batch);
        check_advanced(op, terms, batch);
    });
    check_runs_at_real_caps();
    check_refusals();
    if (bad) {
        std::printf("FAILED: %d expectation(s)\n", bad);
        return 1;
    }
    std::printf("SumOperand OK (%zu layouts): touches, strict runs, advanced views, refusals\n", cases);
    return 0;
}
