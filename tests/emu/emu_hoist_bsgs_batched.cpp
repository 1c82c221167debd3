// emu_hoist_bsgs_batched.cpp -- TEST-ONLY: the per-thread program of hoist_bsgs_batched_kernel (phantom-fhe_amd/csrc/
// pha_hoist_bsgs_batched.h, host/device functions) compiled for the host.  emu_hoist_bsgs_batched() replays EVERY thread of a toy
// launch -- grid (N / 256, limbs of [Q_l || P], ceil(n_ct / CB)) x 256 threads -- on ordinary host arrays;
// tests/test_emu_hoist_bsgs_batched.py compares every output word with Python integers and checks canary words around the buffers.
// With -DEMU_HOIST_BSGS_BATCHED_MAIN the file is a stand-alone program (its own main) for a sanitizer build: exact-size heap
// buffers, so that a tail group that loaded or stored a word of a ciphertext it does not have would be reported.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../phantom-fhe_amd/csrc/pha_hoist_bsgs_batched.h"

using namespace pha;

namespace {

DModulus make_modulus(u64 q) {   // floor(2^128 / q) as two words
    const unsigned __int128 top = ~(unsigned __int128)0;   // 2^128 - 1; q is odd and > 1, so floor((2^128 - 1) / q) == floor(2^128 / q)
    const unsigned __int128 r = top / q;
    return DModulus{q, (u64)r, (u64)(r >> 64)};
}

template <int NG, int CB, int BETA>
void replay(const BsgsBArgs &k, uint32_t limbs) {
    const uint32_t groups = (k.n_ct + CB - 1) / CB;
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t nid = 0; nid < limbs; nid++)
            for (uint32_t coeff = 0; coeff < k.n; coeff++) hoist_bsgs_batched_thread<NG, CB, BETA>(k, coeff, nid, g);
}

// the library's CB for every (NG, BETA); NG = 2 also with the other group widths (CB is a tuning choice, the words must not depend on it)
template <int NG, int BETA>
bool replay_cb(const BsgsBArgs &k, uint32_t limbs, int cb) {
    constexpr int LIB = hoist_bsgs_batched_cb(BETA, NG);
    if (cb == LIB) {
        replay<NG, LIB, BETA>(k, limbs);
        return true;
    }
    if constexpr (NG == 2) {
        switch (cb) {
            case 1: replay<NG, 1, BETA>(k, limbs); return true;
            case 2: replay<NG, 2, BETA>(k, limbs); return true;
            case 4: replay<NG, 4, BETA>(k, limbs); return true;
        }
    }
    return false;
}

template <int BETA>
bool replay_ng(const BsgsBArgs &k, uint32_t limbs, int ng, int cb) {
    switch (ng) {
        case 1: return replay_cb<1, BETA>(k, limbs, cb);
        case 2: return replay_cb<2, BETA>(k, limbs, cb);
        case 4: return replay_cb<4, BETA>(k, limbs, cb);
        case 8: return replay_cb<8, BETA>(k, limbs, cb);
        case 16: return replay_cb<16, BETA>(k, limbs, cb);
    }
    return false;
}

}  // namespace

extern "C" {

// ciphertexts per thread of the instantiation the library launches for NG accumulators and `beta` digits
int emu_hoist_bsgs_batched_cb(int beta, int ng) { return hoist_bsgs_batched_cb(beta, ng); }

// One launch: the accumulators [g0, g0 + ng) of n_ct ciphertexts.  acc [n_ct][g_total][2][limbs][n], t_mod_up [n_ct][beta][limbs][n],
// keys [nb][beta][2][n_primes][n] with keyed[j] = 0 for an identity baby step (its key words are never read), tables [nb][n],
// weights [g_total][nb][limbs][n] with has_w[i * nb + j] = 0 for a missing weight (its words are never read: the harness points it at a
// zero plane, as the driver does), cc [n_ct][2][ql][n], primes [n_primes], qlp_prime [limbs], p_mod_q [ql].  Limbs below 2^50 take
// the FP body.  Returns 0, or -1 for an (ng, cb, beta) without an instantiation.
int emu_hoist_bsgs_batched(int ng, int cb, int beta, uint32_t n, uint32_t limbs, uint32_t ql, uint32_t n_primes, uint32_t nb,
                           uint32_t g_total, uint32_t g0, uint32_t n_ct, uint64_t *acc, const uint64_t *t_mod_up, const uint64_t *keys,
                           const uint8_t *keyed, const uint32_t *tables, const uint64_t *weights, const uint8_t *has_w,
                           const uint64_t *cc, const uint64_t *primes, const uint32_t *qlp_prime, const uint64_t *p_mod_q) {
    std::vector<DModulus> mod(n_primes);
    std::vector<BsgsBFp> fp(n_primes);
    for (uint32_t i = 0; i < n_primes; i++) {
        mod[i] = make_modulus(primes[i]);
        const FpMod fm = make_fpmod(primes[i]);
        fp[i] = BsgsBFp{fm.q, fm.qinv, (primes[i] >> 50) == 0 ? 1u : 0u, 0u};
    }
    std::vector<u64x2> pq(ql);
    for (uint32_t l = 0; l < ql; l++)
        pq[l] = u64x2{p_mod_q[l], (u64)((((unsigned __int128)p_mod_q[l]) << 64) / primes[qlp_prime[l]])};
    const size_t qlp_n = (size_t)limbs * n, qp_n = (size_t)n_primes * n;
    std::vector<u64> zero(qlp_n, 0);
    std::vector<const u64 *> key_ptrs((size_t)nb * beta);
    std::vector<const u64 *const *> key_tabs(nb);
    std::vector<const uint32_t *> tabs(nb);
    std::vector<const u64 *> ws((size_t)g_total * nb);
    for (uint32_t j = 0; j < nb; j++) {
        for (int i = 0; i < beta; i++) key_ptrs[(size_t)j * beta + i] = keys + ((size_t)j * beta + i) * 2 * qp_n;
        key_tabs[j] = keyed[j] ? key_ptrs.data() + (size_t)j * beta : nullptr;
        tabs[j] = tables + (size_t)j * n;
    }
    for (size_t z = 0; z < ws.size(); z++) ws[z] = has_w[z] ? weights + z * qlp_n : zero.data();
    BsgsBArgs k{};
    k.acc = acc; k.t_mod_up = t_mod_up; k.keys = key_tabs.data(); k.tables = tabs.data(); k.weights = ws.data(); k.mod = mod.data();
    k.qlp_prime = qlp_prime; k.n = n; k.beta = (uint32_t)beta; k.nb = nb; k.g0 = g0; k.g_total = g_total; k.n_ct = n_ct;
    k.qlp_n = qlp_n; k.qp_n = qp_n; k.cc = cc; k.cc_stride = (size_t)2 * ql * n; k.p_mod_q = pq.data(); k.ql = ql;
    k.ql_n = (size_t)ql * n; k.fpinfo = fp.data();
    switch (beta) {
        case 1: return replay_ng<1>(k, limbs, ng, cb) ? 0 : -1;
        case 2: return replay_ng<2>(k, limbs, ng, cb) ? 0 : -1;
        case 3: return replay_ng<3>(k, limbs, ng, cb) ? 0 : -1;
        case 4: return replay_ng<4>(k, limbs, ng, cb) ? 0 : -1;
    }
    return -1;
}

}

#ifdef EMU_HOIST_BSGS_BATCHED_MAIN
#include <cstdio>
#include <cstdlib>

// every (NG, BETA) at the library's CB and the tail-group sizes, buffers of exactly n_ct ciphertexts on the heap, all operands q - 1,
// an identity baby step in the middle, 62 baby entries (the result is then one word per limb and polynomial, computed here with
// 128-bit integers)
int main() {
    const uint32_t n = 1024, limbs = 3, ql = 2, n_primes = 4, nb = 62, ident = 30;
    const uint64_t primes[4] = {1099511590913ull, 1152921504606830593ull, 1125899906826241ull, 2305843009213554689ull};
    const uint32_t qlp_prime[3] = {0, 1, 3};
    const uint64_t p_mod_q[2] = {primes[3] % primes[0], primes[3] % primes[1]};
    int bad = 0;
    for (int beta = 1; beta <= 4; beta++)
        for (int ng : {1, 2, 4, 8, 16}) {
            const int cb = emu_hoist_bsgs_batched_cb(beta, ng);
            for (uint32_t n_ct : {(uint32_t)cb - 1, (uint32_t)cb, (uint32_t)cb + 1, 2 * (uint32_t)cb + 1}) {
                if (!n_ct) continue;
                const uint32_t g_total = (uint32_t)ng + 1, g0 = 1;
                std::vector<uint64_t> acc((size_t)n_ct * g_total * 2 * limbs * n, 7), mu((size_t)n_ct * beta * limbs * n),
                    keys((size_t)nb * beta * 2 * n_primes * n), w((size_t)g_total * nb * limbs * n), cc((size_t)n_ct * 2 * ql * n);
                std::vector<uint32_t> tables((size_t)nb * n);
                std::vector<uint8_t> keyed(nb, 1), has_w((size_t)g_total * nb, 1);
                keyed[ident] = 0;
                for (uint32_t j = 0; j < nb; j++)
                    for (uint32_t i = 0; i < n; i++) tables[(size_t)j * n + i] = j == ident ? i : ((i * (2 * j + 1) + j) & (n - 1));
                for (size_t z = 0; z < mu.size(); z++) mu[z] = primes[qlp_prime[(z / n) % limbs]] - 1;
                for (size_t z = 0; z < w.size(); z++) w[z] = primes[qlp_prime[(z / n) % limbs]] - 1;
                for (size_t z = 0; z < cc.size(); z++) cc[z] = primes[qlp_prime[(z / n) % ql]] - 1;
                for (size_t z = 0; z < keys.size(); z++) keys[z] = primes[(z / n) % n_primes] - 1;
                if (emu_hoist_bsgs_batched(ng, cb, beta, n, limbs, ql, n_primes, nb, g_total, g0, n_ct, acc.data(), mu.data(), keys.data(),
                                           keyed.data(), tables.data(), w.data(), has_w.data(), cc.data(), primes, qlp_prime, p_mod_q))
                    return 2;
                for (size_t z = 0; z < acc.size(); z++) {
                    const uint32_t l = (uint32_t)((z / n) % limbs), poly = (uint32_t)((z / ((size_t)limbs * n)) % 2),
                                   g = (uint32_t)((z / ((size_t)2 * limbs * n)) % g_total);
                    const unsigned __int128 q = primes[qlp_prime[l]], m1 = q - 1;
                    const unsigned __int128 pc = l < ql ? (unsigned __int128)p_mod_q[l] * m1 % q : 0;       // P * c0 = P * c1
                    const unsigned __int128 inner = (unsigned __int128)beta * (m1 * m1 % q) % q;             // a keyed step's digit sum
                    const unsigned __int128 s_keyed = poly == 0 ? (inner + pc) % q : inner;
                    const unsigned __int128 want = ((nb - 1) * (s_keyed * m1 % q) + pc * m1 % q) % q;
                    if (acc[z] != (g < g0 ? 7 : (uint64_t)want)) bad++;
                }
            }
        }
    std::printf("emu_hoist_bsgs_batched: %d wrong word(s)\n", bad);
    return bad ? 1 : 0;
}
#endif
