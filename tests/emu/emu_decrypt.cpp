// emu_decrypt.cpp -- TEST-ONLY: the per-thread programs of the decryption kernels (phantom-fhe_amd/csrc/pha_decrypt.h, host/device
// functions) and their tables (pha_rns_tables.h) compiled for the host.  tests/test_emu_decrypt.py compares the results with Python
// integers and checks the magnitude every accumulator of the phase program reaches just before it is reduced.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../phantom-fhe_amd/csrc/pha_decrypt.h"
#include "../../phantom-fhe_amd/csrc/pha_rns_tables.h"

using namespace pha;

namespace {

// one thread's words: ct [G][k][2] (ciphertext g, polynomial i, the two coefficients), sk [k - 1][2] (s^1 first)
struct HostPhaseSrc {
    const u64 *ct, *sk;
    uint32_t k;
    u64x2 c(int g, uint32_t i) const { const u64 *p = ct + ((size_t)g * k + i) * 2; return u64x2{p[0], p[1]}; }
    u64x2 s(uint32_t i) const { const u64 *p = sk + (size_t)(i - 1) * 2; return u64x2{p[0], p[1]}; }
};

struct MaxProbe {
    u64 lo = 0, hi = 0;
    double mag = 0.0;
    uint64_t probes = 0;
    void i128(u64 l, u64 h) {
        if (h > hi || (h == hi && l > lo)) { hi = h; lo = l; }
        probes++;
    }
    void f64(double x) {
        if (std::fabs(x) > mag) mag = std::fabs(x);
        probes++;
    }
};

DModulus make_modulus(u64 q) {   // floor(2^128 / q) as two words (q is no power of two)
    const unsigned __int128 r = ~(unsigned __int128)0 / q;
    return DModulus{q, (u64)r, (u64)(r >> 64)};
}

template <int G, int K>
void run_phase(HostPhaseSrc &src, u64 q, int fp, uint32_t k, bool with_c0, u64x2 *r, MaxProbe &probe) {
    if (fp) phase_fp<G, K>(src, k, with_c0, make_fpmod(q), modulus_bits(q), r, probe);
    else phase_int<G, K>(src, k, with_c0, make_modulus(q), r, probe);
}
template <int G>
void run_phase_k(HostPhaseSrc &src, u64 q, int fp, uint32_t k, int specialised, bool with_c0, u64x2 *r, MaxProbe &probe) {
    if (specialised && k == 2) run_phase<G, 2>(src, q, fp, k, with_c0, r, probe);
    else if (specialised && k == 3) run_phase<G, 3>(src, q, fp, k, with_c0, r, probe);
    else run_phase<G, 0>(src, q, fp, k, with_c0, r, probe);
}

struct HostLimbSrc {
    const u64 *p;
    size_t stride;
    u64 operator()(uint32_t i) const { return p[(size_t)i * stride]; }
};

}  // namespace

extern "C" {

int emu_phase_group() { return kPhaseGroup; }
uint32_t emu_decrypt_max_limbs() { return kDecryptMaxLimbs; }
// terms per flush of the two phase programs for modulus q, as the header computes them
uint32_t emu_phase_per(uint64_t q, int fp) { return fp ? plain_sum_per_fp(modulus_bits(q)) : plain_sum_per_int(modulus_bits(q)); }

// out [G][2]; peak as emu_plain_sum: (lo, hi) of the largest 128-bit accumulator, the largest |double| rounded up, accumulators probed.
// specialised != 0: k = 2 / 3 run the instantiations the kernel launches for them; 0: the run-time loop.
void emu_phase(uint64_t q, int fp, int G, uint32_t k, int specialised, int with_c0, const uint64_t *ct, const uint64_t *sk, uint64_t *out,
               uint64_t *peak) {
    HostPhaseSrc src{ct, sk, k};
    u64x2 r[kPhaseGroup];
    MaxProbe probe;
    switch (G) {
        case 4: run_phase_k<4>(src, q, fp, k, specialised, with_c0 != 0, r, probe); break;
        case 3: run_phase_k<3>(src, q, fp, k, specialised, with_c0 != 0, r, probe); break;
        case 2: run_phase_k<2>(src, q, fp, k, specialised, with_c0 != 0, r, probe); break;
        default: run_phase_k<1>(src, q, fp, k, specialised, with_c0 != 0, r, probe); break;
    }
    for (int g = 0; g < G; g++) { out[2 * g] = r[g].x; out[2 * g + 1] = r[g].y; }
    peak[0] = probe.lo; peak[1] = probe.hi;
    peak[2] = (uint64_t)std::ceil(probe.mag);
    peak[3] = probe.probes;
}

// the four table sets of the scale-and-round over primes [L] (frac, itab: [L][2]) and its split point
int emu_round_tables(const uint64_t *primes, uint32_t L, uint64_t t, double *frac, uint64_t *itab) {
    const DecryptRoundTables d = decrypt_round_tables(std::vector<u64>(primes, primes + L), L, t);
    for (size_t i = 0; i < 2 * (size_t)L; i++) { frac[i] = d.frac[i]; itab[i] = d.itab[i]; }
    return d.h;
}

// x [L][count] canonical residues -> out [count], fsum [count] (the fraction sum as computed)
void emu_scale_round(const uint64_t *primes, uint32_t L, uint64_t t, const uint64_t *x, size_t count, uint64_t *out, double *fsum) {
    const DecryptRoundTables d = decrypt_round_tables(std::vector<u64>(primes, primes + L), L, t);
    const DModulus tm = make_modulus(t);
    for (size_t j = 0; j < count; j++) {
        HostLimbSrc src{x + j, count};
        out[j] = decrypt_scale_round(src, L, d.h, d.frac.data(), d.itab.data(), tm, fsum + j);
    }
}

// hat_inv [L][2] (value, Shoup), mat [L], returns Q mod t
uint64_t emu_mod_t_tables(const uint64_t *primes, uint32_t L, uint64_t t, uint64_t *hat_inv, uint64_t *mat) {
    const DecryptModTTables d = decrypt_mod_t_tables(std::vector<u64>(primes, primes + L), L, t);
    for (uint32_t i = 0; i < L; i++) { hat_inv[2 * i] = d.hat_inv[i].x; hat_inv[2 * i + 1] = d.hat_inv[i].y; mat[i] = d.mat[i]; }
    return d.q_mod_t;
}

void emu_mod_t(const uint64_t *primes, uint32_t L, uint64_t t, uint64_t factor, const uint64_t *x, size_t count, uint64_t *out) {
    const DecryptModTTables d = decrypt_mod_t_tables(std::vector<u64>(primes, primes + L), L, t);
    const DModulus tm = make_modulus(t);
    for (size_t j = 0; j < count; j++) {
        HostLimbSrc src{x + j, count};
        out[j] = decrypt_mod_t_convert(src, L, d.hat_inv.data(), d.mat.data(), primes, d.q_mod_t, tm, factor);
    }
}

}
