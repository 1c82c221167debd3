// emu_hoist_batched.cpp -- TEST-ONLY: the per-thread program of hoist_inner_prod_batched_kernel (phantom-fhe_amd/csrc/
// pha_hoist_batched.h, host/device functions) compiled for the host.  emu_hoist_batched() replays EVERY thread of a toy launch --
// grid (N / 512, limbs of [Q_l || P], ceil(n_ct / CB)) x 256 threads -- on ordinary host arrays; tests/test_emu_hoist_batched.py
// compares every output word with Python integers and checks canary words around the buffers.
// With -DEMU_HOIST_BATCHED_MAIN the file is a stand-alone program (its own main) for a sanitizer build: exact-size heap buffers, so
// that a tail group that loaded or stored a word of a ciphertext it does not have would be reported.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../phantom-fhe_amd/csrc/pha_hoist_batched.h"

using namespace pha;

namespace {

DModulus make_modulus(u64 q) {   // floor(2^128 / q) as two words
    const unsigned __int128 top = ~(unsigned __int128)0;   // 2^128 - 1; q is odd and > 1, so floor((2^128 - 1) / q) == floor(2^128 / q)
    const unsigned __int128 r = top / q;
    return DModulus{q, (u64)r, (u64)(r >> 64)};
}

template <int BETA, int CB, bool WEIGHTED>
void replay(const HoistBArgs &k, uint32_t limbs) {
    const uint32_t groups = (k.n_ct + CB - 1) / CB;
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t nid = 0; nid < limbs; nid++)
            for (uint32_t pair = 0; pair < k.n / 2; pair++) hoist_batched_thread<BETA, CB, WEIGHTED>(k, pair, nid, g);
}

template <int BETA, int CB>
void replay_w(const HoistBArgs &k, uint32_t limbs, bool weighted) {
    if (weighted) replay<BETA, CB, true>(k, limbs);
    else replay<BETA, CB, false>(k, limbs);
}

template <int BETA>
bool replay_cb(const HoistBArgs &k, uint32_t limbs, int cb, bool weighted) {
    switch (cb) {
        case 1: replay_w<BETA, 1>(k, limbs, weighted); return true;
        case 2: replay_w<BETA, 2>(k, limbs, weighted); return true;
        case 4: replay_w<BETA, 4>(k, limbs, weighted); return true;
        default: return false;
    }
}

}  // namespace

extern "C" {

// ciphertexts per thread of the instantiation the library launches for `beta` digits (beta > 4: the run-time digit loop, BETA = 0)
int emu_hoist_batched_cb(int beta, int weighted) { return hoist_batched_cb(beta > 4 ? 0 : beta, weighted != 0); }

// One launch.  cx [n_ct][2][limbs][n] (read when accumulate), t_mod_up [n_ct][beta][limbs][n], keys [n_elts][beta][2][n_primes][n],
// tables [n_elts][n], weights [n_elts][limbs][n] (weighted only), primes [n_primes], qlp_prime [limbs].  Returns 0, or -1 for a
// (beta, cb) without an instantiation.
int emu_hoist_batched(int beta, int cb, int weighted, uint32_t n, uint32_t limbs, uint32_t n_primes, uint32_t n_elts, uint32_t n_ct,
                      int accumulate, uint64_t *cx, const uint64_t *t_mod_up, const uint64_t *keys, const uint32_t *tables,
                      const uint64_t *weights, const uint64_t *primes, const uint32_t *qlp_prime) {
    std::vector<DModulus> mod(n_primes);
    for (uint32_t i = 0; i < n_primes; i++) mod[i] = make_modulus(primes[i]);
    const size_t qlp_n = (size_t)limbs * n, qp_n = (size_t)n_primes * n;
    std::vector<const u64 *> key_ptrs((size_t)n_elts * beta);
    std::vector<const u64 *const *> key_tabs(n_elts);
    std::vector<const uint32_t *> tabs(n_elts);
    std::vector<const u64 *> ws(n_elts);
    for (uint32_t e = 0; e < n_elts; e++) {
        for (int i = 0; i < beta; i++) key_ptrs[(size_t)e * beta + i] = keys + ((size_t)e * beta + i) * 2 * qp_n;
        key_tabs[e] = key_ptrs.data() + (size_t)e * beta;
        tabs[e] = tables + (size_t)e * n;
        ws[e] = weighted ? weights + (size_t)e * qlp_n : nullptr;
    }
    HoistBArgs k{};
    k.cx = cx; k.t_mod_up = t_mod_up; k.keys = key_tabs.data(); k.tables = tabs.data(); k.weights = weighted ? ws.data() : nullptr;
    k.mod = mod.data(); k.qlp_prime = qlp_prime; k.n = n; k.beta = (uint32_t)beta; k.n_elts = n_elts; k.accumulate = accumulate ? 1 : 0;
    k.n_ct = n_ct; k.qlp_n = qlp_n; k.qp_n = qp_n;
    switch (beta > 4 ? 0 : beta) {
        case 0: return replay_cb<0>(k, limbs, cb, weighted != 0) ? 0 : -1;
        case 1: return replay_cb<1>(k, limbs, cb, weighted != 0) ? 0 : -1;
        case 2: return replay_cb<2>(k, limbs, cb, weighted != 0) ? 0 : -1;
        case 3: return replay_cb<3>(k, limbs, cb, weighted != 0) ? 0 : -1;
        case 4: return replay_cb<4>(k, limbs, cb, weighted != 0) ? 0 : -1;
    }
    return -1;
}

}

#ifdef EMU_HOIST_BATCHED_MAIN
#include <cstdio>
#include <cstdlib>

// every (beta, CB, form) at the tail-group sizes, buffers of exactly n_ct ciphertexts on the heap, all operands q - 1 (the result
// is then one word per limb: seed + products mod q, computed here with 128-bit integers)
int main() {
    const uint32_t n = 1024, limbs = 3, n_primes = 4;
    const uint64_t primes[4] = {1125899906826241ull, 2305843009213554689ull, 1125899906629633ull, 2305843009213489153ull};
    const uint32_t qlp_prime[3] = {0, 1, 3};
    int bad = 0;
    for (int beta = 1; beta <= 5; beta++)
        for (int weighted = 0; weighted < 2; weighted++)
            for (int cb : {1, 2, 4})
                for (uint32_t n_ct : {(uint32_t)cb - 1, (uint32_t)cb, (uint32_t)cb + 1, 2 * (uint32_t)cb + 1}) {
                    if (!n_ct) continue;
                    const uint32_t n_elts = weighted ? 63 : 63 / beta;
                    std::vector<uint64_t> cx((size_t)n_ct * 2 * limbs * n), mu((size_t)n_ct * beta * limbs * n),
                        keys((size_t)n_elts * beta * 2 * n_primes * n), w((size_t)n_elts * limbs * n);
                    std::vector<uint32_t> tables((size_t)n_elts * n);
                    for (uint32_t e = 0; e < n_elts; e++)
                        for (uint32_t i = 0; i < n; i++) tables[(size_t)e * n + i] = (i * (2 * e + 1) + e) & (n - 1);
                    for (size_t z = 0; z < cx.size(); z++) cx[z] = primes[qlp_prime[(z / n) % limbs]] - 1;
                    for (size_t z = 0; z < mu.size(); z++) mu[z] = primes[qlp_prime[(z / n) % limbs]] - 1;
                    for (size_t z = 0; z < w.size(); z++) w[z] = primes[qlp_prime[(z / n) % limbs]] - 1;
                    for (size_t z = 0; z < keys.size(); z++) keys[z] = primes[(z / n) % n_primes] - 1;
                    if (emu_hoist_batched(beta, cb, weighted, n, limbs, n_primes, n_elts, n_ct, 1, cx.data(), mu.data(), keys.data(),
                                          tables.data(), w.data(), primes, qlp_prime))
                        return 2;
                    for (size_t z = 0; z < cx.size(); z++) {
                        const unsigned __int128 q = primes[qlp_prime[(z / n) % limbs]], m1 = q - 1;
                        const unsigned __int128 inner = (unsigned __int128)beta * (m1 * m1 % q) % q;   // an element's reduced digit sum
                        const unsigned __int128 want = weighted ? (m1 + (unsigned __int128)n_elts * (inner * m1 % q)) % q
                                                                : (m1 + (unsigned __int128)n_elts * beta * (m1 * m1 % q)) % q;
                        if (cx[z] != (uint64_t)want) bad++;
                    }
                }
    std::printf("emu_hoist_batched: %d wrong word(s)\n", bad);
    return bad ? 1 : 0;
}
#endif
