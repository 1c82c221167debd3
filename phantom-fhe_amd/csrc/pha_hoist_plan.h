// pha_hoist_plan.h -- what the baby-step / giant-step hoisted rotations decide on the host before the first launch: BsgsPlan (every
// refusal, the counts, the host tables in launch order) and BsgsScratch (where the regions of the call's one scratch claim lie).
//
// Host C++ only, no HIP: pha_hoist.hip builds both once per API call; tests/cpp/test_hoist_plan.cpp compiles this header alone and
// sweeps them under the address and undefined-behaviour sanitizers (tests/test_hoist_plan.py).
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace pha {

// What every BSGS entry is handed: nb baby entries and ng giant steps with their key tables (null for element 1), weights [lists][nb]
struct BsgsSteps {
    const uint32_t *baby_elts;
    size_t nb;
    const uint64_t *const *const *baby_glk;
    const uint32_t *giant_elts;
    size_t ng;
    const uint64_t *const *const *giant_glk;
    const uint64_t *const *weights;
};

// out = sum_i rot_{G_i}(sum_j w_ij (.) rot_{B_j}(ct)) for `lists` = ng (one ciphertext, or every ciphertext of a batch) or blocks * ng
// (row blocks that share the ciphertext) lists of nb weights.  Ordering of the input and the output (every BSGS entry, in place
// included): the first write to out is the combine kernel's, after the last read of ct -- by the mod-up and the baby-step kernel,
// earlier on the same stream; a later chunk of a batch reads only its own ciphertexts.  So no entry copies its ciphertexts.
struct BsgsPlan {
    size_t nb, ng, lists;
    size_t nbk = 0, nk = 0;            // keyed (non-identity) baby entries and giant steps
    bool any_null = false;             // a missing weight: the baby-step kernels read a zero plane in its place
    std::vector<const void *> btab, bkeys, gtab, gkeys;   // [nb] tables, [nb] key tables (null: identity), [ng] tables, [nk] key tables
    std::vector<uint32_t> rank;        // [ng] rank of a giant step among the keyed ones, 0xffffffff: identity
    std::vector<const void *> weights; // [lists][nb], null where there is no such term

    // n: ring degree; max_terms: products an unreduced 128-bit accumulator holds (acc_capacity()); units: what shares one launch with
    // the keyed giant steps on blockIdx.z -- the row blocks, or 1 for a batch (whose chunk is cut to fit afterwards); unit_name: how
    // the grid refusal calls them; table_of(elt): the NTT-domain permutation table of a valid element.
    template <class TableOf>
    BsgsPlan(size_t n, size_t beta, size_t max_terms, const BsgsSteps &a, size_t lists_, size_t units, const char *unit_name,
             TableOf &&table_of)
        : nb(a.nb), ng(a.ng), lists(lists_), btab(a.nb), bkeys(a.nb), gtab(a.ng), rank(a.ng), weights(a.weights, a.weights + lists_ * a.nb) {
        const uint32_t *baby_elts = a.baby_elts, *giant_elts = a.giant_elts;
        const uint64_t *const *const *baby_glk = a.baby_glk, *const *const *giant_glk = a.giant_glk;
        auto valid = [&](uint32_t elt) {
            if (!(elt & 1) || elt >= 2 * n) throw std::invalid_argument("Galois element is not valid");
        };
        for (size_t j = 0; j < nb; j++) valid(baby_elts[j]);
        for (size_t i = 0; i < ng; i++) valid(giant_elts[i]);
        for (size_t j = 0; j < nb; j++) {
            if (baby_elts[j] != 1 && !baby_glk[j]) throw std::logic_error("Galois key not present in hoisting");
            nbk += baby_elts[j] != 1;
        }
        for (size_t i = 0; i < ng; i++) {
            if (giant_elts[i] != 1 && !giant_glk[i]) throw std::logic_error("Galois key not present in hoisting");
            nk += giant_elts[i] != 1;
        }
        // what the unreduced 128-bit accumulators of the fused baby-step kernels hold: one s * w product per baby ENTRY (identity
        // entries and repeated elements included) plus the P-scaled c0 / c1 term, each below q_max^2 (2^122 for 61-bit primes: 63
        // fit); the giant steps' key products likewise (2^120 each for 60-bit primes)
        if (nb + 1 > max_terms || nk * beta > max_terms || nbk > 255)
            throw std::invalid_argument("too many steps for one call: the 128-bit accumulators hold floor(2^128 / q_max^2) - 1 products (at most "
                                        "254 baby entries for primes up to 60 bits, 62 for 61-bit primes)");
        if (2 * lists > 65535 || units * nk * beta > 65535) throw std::invalid_argument(std::string("too many ") + unit_name + " for one call");
        if (beta > 4) throw std::invalid_argument("more than 4 key-switch digits are not supported by the baby-step / giant-step form");
        for (const void *p : weights) any_null = any_null || !p;
        for (size_t j = 0; j < nb; j++) {
            btab[j] = table_of(baby_elts[j]);
            bkeys[j] = baby_elts[j] == 1 ? nullptr : baby_glk[j];
        }
        for (size_t i = 0; i < ng; i++) {
            gtab[i] = table_of(giant_elts[i]);
            rank[i] = giant_elts[i] == 1 ? 0xffffffffu : (uint32_t)gkeys.size();
            if (giant_elts[i] != 1) gkeys.push_back(giant_glk[i]);
        }
    }
};

// The one scratch claim of a BSGS call, sized for its largest set of launches: `units` row blocks of one ciphertext (cts = 1), or a
// chunk of `units` ciphertexts (cts = units); every unit has ng accumulator lists.
//   tmp [2 ng units][Ql][N] | mod-up [cts][beta][QlP][N] | acc [units][ng][2][QlP][N] | B [units][ng][2][Ql][N] | g1 [units][nk][Ql][N] |
//   giant mod-up [units][nk][beta][QlP][N] | cx [units][2][QlP][N] | pointers | zero plane [QlP][N] (missing weights only)
// tmp serves the mod-ups (cts resp. units * nk polynomials) and the mod-downs (2 ng units resp. 2 units); the first mod-down's is the
// largest of them, because cts <= units and nk <= ng.
struct BsgsScratch {
    struct Dims {
        size_t ql_n, qlp_n, beta, units, cts, nb, ng, nk, lists;
        bool any_null;
    };
    enum { kRegions = 9 };
    uint64_t *tmp, *t_mod_up, *acc, *B, *g1, *mu_g, *cx, *ptrs, *zero;

    // pointer region: baby tables, baby key tables, weights, giant tables, giant key tables (a word each), the ranks (half a word
    // each); rounded up to 256 bytes, so that the zero plane behind it is cleared by one aligned fill
    static size_t ptr_words(const Dims &d) { return (2 * d.nb + d.lists * d.nb + d.ng + d.nk + (d.ng + 1) / 2 + 31) / 32 * 32; }
    // the regions' sizes in words, in the order of the members: words() and the constructor both walk this list
    static std::array<size_t, kRegions> sizes(const Dims &d) {
        return {2 * d.ng * d.units * d.ql_n,
                d.cts * d.beta * d.qlp_n,
                d.units * d.ng * 2 * d.qlp_n,
                d.units * d.ng * 2 * d.ql_n,
                d.units * d.nk * d.ql_n,
                d.units * d.nk * d.beta * d.qlp_n,
                d.units * 2 * d.qlp_n,
                ptr_words(d),
                d.any_null ? d.qlp_n : 0};
    }
    static size_t words(const Dims &d) {
        size_t w = 0;
        for (size_t r : sizes(d)) w += r;
        return w;
    }
    BsgsScratch(uint64_t *base, const Dims &d) {
        uint64_t **const region[kRegions] = {&tmp, &t_mod_up, &acc, &B, &g1, &mu_g, &cx, &ptrs, &zero};
        const std::array<size_t, kRegions> w = sizes(d);
        for (int r = 0; r < kRegions; r++) {
            *region[r] = base;
            base += w[r];
        }
    }
};

}  // namespace pha
