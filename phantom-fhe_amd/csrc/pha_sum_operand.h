// pha_sum_operand.h -- what the summed-product entries (pha_poly.hip, pha_plain.hip) decide about a strided operand on the host:
// SumOperand, the view "element (g, k) is `words` words at p + g * bs + k * ts", with the address arithmetic of the chunk and slab
// loops, the layout refusals, the output-overlap test and the enumeration strict mode walks.  Also the one range test overlaps().
//
// Host C++ only, no HIP and nothing dereferenced: tests/cpp/test_sum_operand.cpp compiles this header alone and sweeps it under the
// address and undefined-behaviour sanitizers (tests/test_sum_operand.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <stdexcept>

namespace pha {

// do [a, a + na) and [b, b + nb) share a word?
inline bool overlaps(const uint64_t *a, size_t na, const uint64_t *b, size_t nb) { return a < b + nb && b < a + na; }

// polynomials one strict-mode count takes: the polynomial is blockIdx.z, and a grid's z extent ends at 65535
constexpr size_t kStrictRunPolys = 65535;

struct SumOperand {
    const uint64_t *p = nullptr;    // null: the operand is absent (an optional addend)
    size_t ts = 0, bs = 0;          // words between consecutive terms / groups; bs == 0: one set of terms shared by all groups
    size_t words = 0;               // of one element
    size_t polys = 1;               // polynomials of one element, words / polys each: 2 for a ciphertext
    const char *crowded = nullptr;  // the refusal of a term stride below `words`; null: one element per group, no term stride

    const uint64_t *at(size_t g, size_t k) const { return p + g * bs + k * ts; }
    size_t groups(size_t batch) const { return bs ? batch : std::min<size_t>(batch, 1); }   // distinct ones
    // the view whose element (g, k) is this one's (g0 + g, k0 + k)
    SumOperand advanced(size_t g0, size_t k0) const {
        SumOperand v = *this;
        if (p) v.p = at(g0, k0);
        return v;
    }
    bool shared(size_t batch) const { return bs == 0 && batch > 1; }   // the launchers' cache policy: later groups re-read it

    // does out [out_words] touch any element?  The span of all of them first: the usual call is answered by one comparison
    bool touches(const uint64_t *out, size_t out_words, size_t terms, size_t batch) const {
        const size_t G = groups(batch);
        if (G == 0 || terms == 0) return false;
        if (!overlaps(out, out_words, p, (G - 1) * bs + (terms - 1) * ts + words)) return false;
        for (size_t g = 0; g < G; g++)
            for (size_t k = 0; k < terms; k++)
                if (overlaps(out, out_words, at(g, k), words)) return true;
        return false;
    }

    // strict mode: fn(base, polynomials, words between them) for runs that cover every distinct polynomial once, at most `cap` a
    // run.  Two-polynomial elements that lie in a row (one term, or a term stride of `words`) go as [terms][2] rows of cap / 2
    // terms; any other layout polynomial by polynomial: c0 of every term, then c1
    template <class F>
    void strict_runs(size_t terms, size_t batch, F &&fn, size_t cap = kStrictRunPolys) const {
        const size_t pw = words / polys, G = groups(batch);
        for (size_t g = 0; g < G; g++) {
            if (polys == 2 && (terms == 1 || ts == words)) {
                const size_t row = cap / 2;
                for (size_t k0 = 0; k0 < terms; k0 += row) fn(at(g, k0), 2 * std::min(row, terms - k0), pw);
            } else {
                for (size_t half = 0; half < polys; half++)
                    for (size_t k0 = 0; k0 < terms; k0 += cap) fn(at(g, k0) + half * pw, std::min(cap, terms - k0), ts);
            }
        }
    }
};

// The refusals every summed-product entry makes about its term count and about where its operands lie, in this order; an entry's
// own (limb count, batch) go between the two calls.
inline void sum_check_terms(size_t terms) {
    if (terms == 0) throw std::invalid_argument("terms must be at least 1");
    if (terms > 0xffffffffull) throw std::invalid_argument("terms out of range");
}
// also_aligned: a buffer whose alignment is refused along with the operands' (null: none)
inline void sum_check_layout(std::initializer_list<SumOperand> ops, size_t terms, const uint64_t *also_aligned = nullptr) {
    size_t strides = 0;
    uintptr_t bases = reinterpret_cast<uintptr_t>(also_aligned);
    for (const SumOperand &o : ops) {
        strides |= o.ts | o.bs;
        bases |= reinterpret_cast<uintptr_t>(o.p);
    }
    if (strides & 1) throw std::invalid_argument("strides must be even (16-byte loads)");
    if (bases & 15) throw std::invalid_argument("buffers must be 16-byte aligned");
    for (const SumOperand &o : ops)
        if (terms > 1 && o.crowded && o.ts < o.words) throw std::invalid_argument(o.crowded);
}

}  // namespace pha
