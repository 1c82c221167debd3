// emu_noise.cpp -- TEST-ONLY: the per-thread programs of the noise kernels (phantom-fhe_amd/csrc/pha_noise.h, host/device functions)
// and their host-built tables (pha_rns_tables.h noise_tables / noise_level_tables) compiled for the host.  tests/test_emu_noise.py
// compares every stage with Python integers.  With -DEMU_NOISE_MAIN the file is a stand-alone program (primes on the command line)
// that sweeps the same programs over constructed columns and word patterns: built with -fsanitize=undefined, it guards the shifts
// of the bit count.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../phantom-fhe_amd/csrc/pha_noise.h"
#include "../../phantom-fhe_amd/csrc/pha_rns_tables.h"

using namespace pha;

namespace {

DModulus make_modulus(u64 q) {   // floor(2^128 / q) as two words (q is no power of two)
    const unsigned __int128 r = ~(unsigned __int128)0 / q;
    return DModulus{q, (u64)r, (u64)(r >> 64)};
}

struct HostCol {
    u64 *p;
    u64 &operator()(uint32_t i) const { return p[i]; }
};
struct HostWords {
    const u64 *p;
    u64 operator()(uint32_t i) const { return p[i]; }
};
struct HostInv {
    const u64x2 *inv;
    uint32_t pitch;
    u64x2 operator()(uint32_t i, uint32_t j) const { return inv[(size_t)i * pitch + j]; }
};

// One coefficient through every stage, as norm_kernel and finish_kernel run them.  The tables are built over `size` >= L primes: the
// level uses its prefix.
struct Pipeline {
    std::vector<u64> primes;
    NoiseTables base;
    Pipeline(const uint64_t *p, uint32_t size) : primes(p, p + size), base(noise_tables(primes, size)) {}
    // x [L] canonical residues; digits / mag [L]; words [L]; returns the sign decision, *bits = the magnitude's bit count
    bool run(uint32_t L, u64 scalar, const u64 *x, u64 *digits, u64 *mag, u64 *words, uint32_t *bits) const {
        const NoiseLevelTables lvl = noise_level_tables(primes, L);
        const std::vector<u64> scal = noise_scalar_table(primes, L, scalar);
        std::vector<u64> col(L);
        for (uint32_t i = 0; i < L; i++) col[i] = scalar != 1 ? mul_mod(x[i], scal[i], make_modulus(primes[i])) : x[i];
        HostCol c{col.data()};
        const HostWords q{primes.data()};
        noise_garner(c, L, q, HostInv{base.inv.data(), base.size}, HostWords{base.lift.data()});
        for (uint32_t i = 0; i < L; i++) digits[i] = col[i];
        const bool neg = noise_magnitude(c, L, q, HostWords{lvl.half.data()});
        for (uint32_t i = 0; i < L; i++) mag[i] = col[i];
        noise_horner(HostWords{col.data()}, L, q, words);
        *bits = noise_bits(words, L);
        return neg;
    }
};

}  // namespace

extern "C" {

uint32_t emu_noise_max_limbs() { return kNoiseMaxLimbs; }

// inv [size][size][2] (value, Shoup; zero unless i < j), lift [size]
void emu_noise_tables(const uint64_t *primes, uint32_t size, uint64_t *inv, uint64_t *lift) {
    const NoiseTables t = noise_tables(std::vector<u64>(primes, primes + size), size);
    for (size_t k = 0; k < (size_t)size * size; k++) { inv[2 * k] = t.inv[k].x; inv[2 * k + 1] = t.inv[k].y; }
    for (uint32_t j = 0; j < size; j++) lift[j] = t.lift[j];
}

// half [L]: the mixed-radix digits of (Q_l - 1) / 2; returns bitcount(Q_l)
int emu_noise_level(const uint64_t *primes, uint32_t L, uint64_t *half) {
    const NoiseLevelTables t = noise_level_tables(std::vector<u64>(primes, primes + L), L);
    for (uint32_t i = 0; i < L; i++) half[i] = t.half[i];
    return t.q_bits;
}

// x [L][count] canonical residues over the first L of `size` primes -> digits, mag [count][L] (mixed radix), neg [count], words
// [count][L] (little-endian), bits [count], budget [count]
void emu_noise_columns(const uint64_t *primes, uint32_t size, uint32_t L, uint64_t scalar, const uint64_t *x, size_t count, uint64_t *digits,
                       uint64_t *mag, uint32_t *neg, uint64_t *words, uint32_t *bits, int32_t *budget) {
    const Pipeline p(primes, size);
    const int q_bits = noise_level_tables(p.primes, L).q_bits;
    std::vector<u64> col(L);
    for (size_t j = 0; j < count; j++) {
        for (uint32_t i = 0; i < L; i++) col[i] = x[(size_t)i * count + j];
        neg[j] = p.run(L, scalar, col.data(), digits + j * L, mag + j * L, words + j * L, bits + j);
        budget[j] = noise_budget(q_bits, bits[j]);
    }
}

// the index of the maximum of `count` digit vectors [count][L] as the kernels find it: noise_greater, the first maximum kept
size_t emu_noise_argmax(const uint64_t *digits, size_t count, uint32_t L) {
    size_t best = 0;
    for (size_t c = 1; c < count; c++)
        if (noise_greater(HostWords{digits + c * L}, HostWords{digits + best * L}, L)) best = c;
    return best;
}

uint32_t emu_noise_bits(const uint64_t *words, uint32_t L) { return noise_bits(words, L); }

}

#ifdef EMU_NOISE_MAIN
// argv[1 ..]: the primes.  Every prefix L: the columns 0, 1, q_i - 1 (Q - 1), half, half + 1 and pseudo-random ones, with scalars 1
// and 2^59 - 55; then the bit count over word patterns at both ends of a word.
int main(int argc, char **argv) {
    std::vector<u64> primes;
    for (int i = 1; i < argc; i++) primes.push_back(strtoull(argv[i], nullptr, 10));
    const uint32_t size = (uint32_t)primes.size();
    if (!size) return 2;
    const Pipeline p(primes.data(), size);
    u64 state = 0x9E3779B97F4A7C15ull, checksum = 0;
    for (uint32_t L = 1; L <= size; L++) {
        const NoiseLevelTables lvl = noise_level_tables(primes, L);
        std::vector<u64> x(L), digits(L), mag(L), words(L);
        for (int pattern = 0; pattern < 16; pattern++)
            for (u64 scalar : {(u64)1, ((u64)1 << 59) - 55}) {
                for (uint32_t i = 0; i < L; i++) {
                    state = state * 6364136223846793005ull + 1442695040888963407ull;
                    x[i] = pattern == 0 ? 0 : pattern == 1 ? 1 % primes[i] : pattern == 2 ? primes[i] - 1 : (state >> 3) % primes[i];
                }
                uint32_t bits = 0;
                const bool neg = p.run(L, scalar, x.data(), digits.data(), mag.data(), words.data(), &bits);
                if (pattern == 0 && (neg || bits != 0)) return 3;
                if (pattern == 2 && scalar == 1 && (!neg || bits != 1 || words[0] != 1)) return 4;   // Q - 1: magnitude 1
                if (noise_budget(lvl.q_bits, bits) < 0) return 5;
                checksum += bits + words[0];
            }
    }
    const u64 top = (u64)1 << 63;
    const u64 pat[][3] = {{0, 0, 0}, {1, 0, 0}, {top, 0, 0}, {~(u64)0, 0, 0}, {0, 1, 0}, {0, top, 0}, {0, 0, 1}, {~(u64)0, ~(u64)0, ~(u64)0}};
    const uint32_t want[] = {0, 1, 64, 64, 65, 128, 129, 192};
    for (int k = 0; k < 8; k++)
        if (noise_bits(pat[k], 3) != want[k]) return 6;
    if (noise_budget(10, 192) != 0 || noise_budget(100, 0) != 99) return 7;
    printf("emu_noise ok %llu\n", (unsigned long long)checksum);
    return 0;
}
#endif
