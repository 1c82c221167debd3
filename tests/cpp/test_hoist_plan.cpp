// test_hoist_plan.cpp -- TEST-ONLY, host only (no device is touched): BsgsScratch and BsgsPlan of phantom-fhe_amd/csrc/pha_hoist_plan.h,
// the host side of the baby-step / giant-step hoisted rotations.  Built with -fsanitize=address,undefined and run by
// tests/test_hoist_plan.py.
//   layout: for a sweep of (units, nb, ng, nk, beta, any_null), both forms (row blocks of one ciphertext, a chunk of ciphertexts), the
//           regions follow each other in the documented order without a gap, have the documented sizes, and the last one ends at
//           base + words(): what the hand-summed expressions of the two former drivers gave.
//   plan:   counts, orderings, the rank table, the zero-plane flag, and every refusal with its exception class and message.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../phantom-fhe_amd/csrc/pha_hoist_plan.h"

using pha::BsgsPlan;
using pha::BsgsScratch;

static int bad = 0;
#define EXPECT(cond, ...)             \
    do {                              \
        if (!(cond)) {                \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            bad++;                    \
        }                             \
    } while (0)

static size_t check_layouts() {
    std::vector<uint64_t> arena;   // the regions' first and last words are written: a region outside the claim trips the sanitizer
    size_t cases = 0;
    const size_t n = 8;
    for (size_t ql : {1, 3})
    for (size_t beta : {1, 2, 4})
    for (size_t units : {1, 2, 5})
    for (size_t nb : {1, 4})
    for (size_t ng : {1, 3, 9})
    for (size_t nk = 0; nk <= ng; nk += (ng > 2 ? ng / 2 : 1))
    for (int any_null = 0; any_null < 2; any_null++)
    for (int batched = 0; batched < 2; batched++) {
        const size_t ql_n = ql * n, qlp_n = (ql + 2) * n, cts = batched ? units : 1, lists = batched ? ng : units * ng, G = units * ng;
        const BsgsScratch::Dims d{ql_n, qlp_n, beta, units, cts, nb, ng, nk, lists, any_null != 0};
        const size_t ptrs = (2 * nb + lists * nb + ng + nk + (ng + 1) / 2 + 31) / 32 * 32;   // whole 256-byte lines
        // the former drivers' sums: bsgs_core without its (c0, c1) copy (tmp = 2 G), bsgs_batched_core
        const size_t want = 2 * G * ql_n + cts * beta * qlp_n + G * 2 * qlp_n + G * 2 * ql_n + units * nk * ql_n + units * nk * beta * qlp_n +
                            units * 2 * qlp_n + ptrs + (any_null ? qlp_n : 0);
        const size_t words = BsgsScratch::words(d);
        arena.assign(words + 1, 0);
        uint64_t *base = arena.data();
        const BsgsScratch s(base, d);
        const uint64_t *at[] = {s.tmp, s.t_mod_up, s.acc, s.B, s.g1, s.mu_g, s.cx, s.ptrs, s.zero, base + words};
        const size_t size[] = {2 * G * ql_n, cts * beta * qlp_n, G * 2 * qlp_n, G * 2 * ql_n, units * nk * ql_n, units * nk * beta * qlp_n,
                               units * 2 * qlp_n, ptrs, any_null ? qlp_n : 0};
        bool ok = words == want && s.tmp == base;
        for (int r = 0; r < 9; r++) {
            ok = ok && at[r + 1] == at[r] + size[r];
            if (ok && size[r]) {
                const_cast<uint64_t *>(at[r])[0] += 1;
                const_cast<uint64_t *>(at[r])[size[r] - 1] += 1;
            }
        }
        // tmp holds what every mod-up and mod-down of the call asks for
        ok = ok && size[0] >= cts * ql_n && size[0] >= units * nk * ql_n && size[0] >= 2 * units * ql_n;
        ok = ok && arena[words] == 0;
        EXPECT(ok, "BsgsScratch (ql %zu, beta %zu, units %zu, nb %zu, ng %zu, nk %zu, null %d, batched %d): words %zu, want %zu", ql, beta, units,
               nb, ng, nk, any_null, batched, words, want);
        cases++;
    }
    return cases;
}

struct Call {
    std::vector<uint32_t> baby, giant;
    std::vector<const uint64_t *const *> bk, gk;
    std::vector<const uint64_t *> w;
    size_t n = 4096, beta = 3, max_terms = 255, units = 1;
    const char *unit_name = "row blocks";
    BsgsPlan plan() const {
        const pha::BsgsSteps a{baby.data(), baby.size(), bk.data(), giant.data(), giant.size(), gk.data(), w.data()};
        return BsgsPlan(n, beta, max_terms, a, w.size() / baby.size(), units, unit_name,
                        [](uint32_t e) { return reinterpret_cast<const void *>((uintptr_t)e << 8); });
    }
};

// 1: std::invalid_argument, 2: std::logic_error, with the message
template <class E>
static void refused(const char *what, const Call &c, const char *msg) {
    try {
        c.plan();
        EXPECT(false, "%s: not refused", what);
    } catch (const E &e) {
        EXPECT(std::strstr(e.what(), msg) == e.what(), "%s: message \"%s\"", what, e.what());
    } catch (const std::exception &e) {
        EXPECT(false, "%s: another exception class, \"%s\"", what, e.what());
    }
}

static void check_plans() {
    static const uint64_t word = 0;
    static const uint64_t *const key[4] = {&word, &word, &word, &word};
    Call ok;
    ok.baby = {1, 5, 25, 125};
    ok.giant = {625, 1, 3125};
    ok.bk = {nullptr, key, key + 1, key + 2};
    ok.gk = {key + 3, nullptr, key};
    ok.w.assign(2 * 3 * 4, &word);   // two row blocks
    ok.units = 2;
    {
        const BsgsPlan p = ok.plan();
        EXPECT(p.nb == 4 && p.ng == 3 && p.lists == 6 && p.nbk == 3 && p.nk == 2 && !p.any_null, "plan: counts");
        EXPECT(p.rank == (std::vector<uint32_t>{0, 0xffffffffu, 1}), "plan: ranks");
        EXPECT(p.gkeys == (std::vector<const void *>{key + 3, key}), "plan: keyed giant steps in order");
        EXPECT(p.bkeys == (std::vector<const void *>{nullptr, key, key + 1, key + 2}), "plan: baby keys, null for the identity");
        EXPECT(p.btab[2] == reinterpret_cast<const void *>((uintptr_t)25 << 8) && p.gtab[2] == reinterpret_cast<const void *>((uintptr_t)3125 << 8),
               "plan: tables in the order given");
        EXPECT(p.weights.size() == 24, "plan: weights");
    }
    {
        Call c = ok;
        c.w[7] = nullptr;
        c.bk[0] = key;   // a key for the identity is ignored
        const BsgsPlan p = c.plan();
        EXPECT(p.any_null && p.bkeys[0] == nullptr && p.nbk == 3, "plan: missing weight, key of the identity");
    }
    Call c = ok;
    c.baby[2] = 4;
    refused<std::invalid_argument>("even baby element", c, "Galois element is not valid");
    c = ok;
    c.giant[0] = 2 * 4096 + 1;
    refused<std::invalid_argument>("giant element >= 2N", c, "Galois element is not valid");
    c = ok;
    c.bk[1] = nullptr;
    refused<std::logic_error>("missing baby key", c, "Galois key not present in hoisting");
    c = ok;
    c.gk[2] = nullptr;
    refused<std::logic_error>("missing giant key", c, "Galois key not present in hoisting");
    c = ok;
    c.max_terms = 4;   // nb + 1 = 5 products
    refused<std::invalid_argument>("accumulator capacity", c, "too many steps for one call: the 128-bit accumulators hold");
    c = ok;
    c.max_terms = 5;   // nk * beta = 6 products
    refused<std::invalid_argument>("accumulator capacity, giant side", c, "too many steps for one call");
    c = ok;
    c.units = 65535 / 6 + 1;   // units * nk * beta > 65535
    refused<std::invalid_argument>("grid limit", c, "too many row blocks for one call");
    c.unit_name = "giant steps";
    refused<std::invalid_argument>("grid limit", c, "too many giant steps for one call");
    c = ok;
    c.beta = 5;
    refused<std::invalid_argument>("five digits", c, "more than 4 key-switch digits");
    c.max_terms = 5;   // several defects: the capacity is reported before the digit count
    refused<std::invalid_argument>("order of refusals", c, "too many steps");
}

int main() {
    const size_t cases = check_layouts();
    check_plans();
    if (!bad) std::printf("BsgsScratch layout OK (%zu cases), BsgsPlan OK\n", cases);
    return bad ? 1 : 0;
}
