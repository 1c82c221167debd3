// emu_prng.cpp -- TEST-ONLY: the per-thread programs of the seeded samplers (phantom-fhe_amd/csrc/pha_prng.h, the very functions the
// kernels of pha_prng.hip call) compiled for the host.  tests/test_emu_prng.py compares their words with the numpy restatement
// (tests/prng_restatement.py).
#include <cstddef>
#include <cstdint>
#include "../../phantom-fhe_amd/csrc/pha_prng.h"

using namespace pha;

namespace {

u64 ratio1_of(u64 q) { return (u64)((~(unsigned __int128)0 / q) >> 64); }   // the high word of floor(2^128 / q)

}  // namespace

extern "C" {

int emu_prng_seed_bytes() { return kPrngSeedBytes; }
int emu_prng_group_words() { return kPrngGroupWords; }

void emu_quarter_round(uint32_t *v) { prng_quarter_round(v[0], v[1], v[2], v[3]); }

// out [count][16]: the blocks of (seed, nonces[k])
void emu_blocks(const uint8_t *seed, const uint64_t *nonces, size_t count, uint32_t *out) {
    const PrngKey key = prng_load_key(seed);
    for (size_t k = 0; k < count; k++) {
        const PrngBlock b = prng_block(key, nonces[k]);
        for (int i = 0; i < 16; i++) out[16 * k + i] = b.w[i];
    }
}

// coefficients 0 .. n - 1 of the ternary (which == 0) or noise sample: the signed word, and the residue modulo q
void emu_small(const uint8_t *seed, int which, uint64_t q, size_t n, uint64_t *signed_out, uint64_t *residue_out) {
    const PrngKey key = prng_load_key(seed);
    for (size_t i = 0; i < n; i++) {
        const PrngBlock b = prng_block(key, i);
        const int v = which == 0 ? prng_ternary_value(b.w[0]) : prng_error_value(b.w[0], b.w[1]);
        signed_out[i] = prng_signed_word(v);
        residue_out[i] = prng_residue(v, q);
    }
}

uint64_t emu_max_multiple(uint64_t q) { return prng_max_multiple(q, ratio1_of(q)); }

// the exact reduction the uniform rule stores with
void emu_reduce(uint64_t q, const uint64_t *words, size_t count, uint64_t *out) {
    for (size_t k = 0; k < count; k++) out[k] = barrett64(words[k], q, ratio1_of(q));
}

// rows [rows][n] as prng_uniform_kernel forms them: row y modulo primes[y], group g = y * (n / 8) + j; tries [rows][n / 8]
void emu_uniform(const uint8_t *seed, const uint64_t *primes, size_t rows, size_t n, uint64_t *out, uint32_t *tries) {
    const PrngKey key = prng_load_key(seed);
    const size_t groups = n / kPrngGroupWords;
    for (size_t y = 0; y < rows; y++)
        for (size_t j = 0; j < groups; j++) {
            u64 w[kPrngGroupWords];
            tries[y * groups + j] = prng_uniform_group(key, y * groups + j, (u64)n * rows, primes[y], ratio1_of(primes[y]), w);
            for (int i = 0; i < kPrngGroupWords; i++) out[y * n + j * kPrngGroupWords + i] = w[i];
        }
}

}  // extern "C"
