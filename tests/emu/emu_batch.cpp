// emu_batch.cpp -- TEST-ONLY: the arithmetic, the index math and the pass phases of the BFV / BGV batch encoder
// (phantom-fhe_amd/csrc/pha_batch.h, host/device functions: the very source the kernels of pha_batch.hip run) compiled for the host.
// A workgroup's threads are played one after the other, phase by phase (a phase ends where the kernel has its barrier).
// tests/test_emu_batch.py compares the results with the restatement (tests/batch_restatement.py), word for word.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../phantom-fhe_amd/csrc/pha_batch.h"

using namespace pha;

extern "C" {

void emu_batch_index_map(uint32_t log_n, uint64_t *out) { batch_index_map(log_n, out); }
uint64_t emu_batch_sign_rule(uint64_t v, uint64_t t) { return batch_sign_rule(v, t); }
uint32_t emu_batch_threads(uint32_t log_tile) { return nwt_threads(log_tile); }

// One whole transform of 2^log_n words modulo t through the kernels' plan and phases with `nthreads` threads per workgroup (0: the
// kernels' own count per tile): tw = the direction's table as (value, Shoup) pairs, perm = the inverse index map, in / out as the
// modes say, `mid` (2^log_n words) between the passes of a two-pass transform.  Returns the number of passes.
uint32_t emu_batch_nwt(int inverse, uint32_t log_n, uint64_t t, const uint64_t *tw_pairs, uint64_t ninv, uint64_t ninv_shoup,
                       const uint32_t *perm, const uint64_t *in, int in_mode, uint32_t values_size, uint64_t *mid, uint64_t *out,
                       int out_mode, uint32_t nthreads) {
    NwtPass p{};
    p.tw = reinterpret_cast<const u64x2 *>(tw_pairs);
    p.perm = perm;
    p.q = t;
    p.ninv = u64x2{ninv, ninv_shoup};
    const u32 passes = nwt_pass_count(log_n);
    for (u32 which = 0; which < passes; which++) {
        const bool first = which == 0, last = which + 1 == passes;
        nwt_pass_shape(p, log_n, inverse != 0, which);
        p.in = first ? in : mid;
        p.in_mode = first ? in_mode : (int)NWT_IN_PLAIN;
        p.values_size = values_size;
        p.out = last ? out : mid;
        p.out_mode = last ? out_mode : (int)NWT_OUT_LAZY;
        const u32 threads = nthreads ? nthreads : nwt_threads(p.log_tile);
        std::vector<u64> lds((size_t)1 << p.log_tile);
        for (u32 tile = 0; tile < (1u << (log_n - p.log_tile)); tile++) {
            for (u32 th = 0; th < threads; th++) nwt_load(p, lds.data(), tile, 0, th, threads);
            for (u32 done = 0; done < p.stages;) {
                u32 r = 0;
                for (u32 th = 0; th < threads; th++)
                    r = inverse ? nwt_stage_phase<true>(p, lds.data(), tile, done, th, threads)
                                : nwt_stage_phase<false>(p, lds.data(), tile, done, th, threads);
                done += r;
            }
            for (u32 th = 0; th < threads; th++) {
                if (inverse) nwt_store<true>(p, lds.data(), tile, 0, th, threads);
                else nwt_store<false>(p, lds.data(), tile, 0, th, threads);
            }
        }
    }
    return passes;
}

// decode's gather and encode's permutation as passes of their own
void emu_batch_gather(uint64_t *out, const uint64_t *src, const uint32_t *index_map, uint32_t n) {
    for (u32 i = 0; i < n; i++) batch_gather_word(out, src, index_map, i);
}
void emu_batch_permute(uint64_t *buf, const uint64_t *values, const uint32_t *perm, uint32_t values_size, uint64_t t, uint32_t n) {
    for (u32 g = 0; g < n; g++) batch_permute_word(buf, values, perm, values_size, t, g);
}

}  // extern "C"

#ifdef EMU_BATCH_MAIN
// stand-alone run for a sanitizer build: a round trip through gather, stages, scale and scatter at 2^12 and 2^15 with t = 2^16 + 1
// (a batching prime up to N = 2^15; psi found by search).  Exit status 0: decode(encode(v)) == v.
#include <cstdio>
static u64 mulmod(u64 a, u64 b, u64 q) { return (u64)(((unsigned __int128)a * b) % q); }
static u64 powmod(u64 a, u64 e, u64 q) {
    u64 r = 1;
    for (; e; e >>= 1, a = mulmod(a, a, q))
        if (e & 1) r = mulmod(r, a, q);
    return r;
}
int main() {
    const u64 t = 65537;
    for (u32 log_n : {12u, 15u}) {
        const u32 n = 1u << log_n;
        u64 psi = 0;
        for (u64 g = 3; !psi; g += 2) {
            const u64 r = powmod(g, (t - 1) / (2 * n), t);
            if (powmod(r, n, t) == t - 1) psi = r;
        }
        const u64 ipsi = powmod(psi, t - 2, t), ninv = powmod(n % t, t - 2, t);
        std::vector<u64> tw(2 * (size_t)n), itw(2 * (size_t)n), map(n), v(n), plain(n), mid(n), back(n);
        u64 pw = 1, ipw = 1;
        for (u32 k = 0; k < n; k++) {
            const u32 at = batch_brev(k, log_n);
            tw[2 * at] = pw; tw[2 * at + 1] = (u64)(((unsigned __int128)pw << 64) / t);
            itw[2 * at] = ipw; itw[2 * at + 1] = (u64)(((unsigned __int128)ipw << 64) / t);
            pw = mulmod(pw, psi, t); ipw = mulmod(ipw, ipsi, t);
        }
        batch_index_map(log_n, map.data());
        std::vector<u32> inv(n);
        for (u32 i = 0; i < n; i++) inv[map[i]] = i;
        for (u32 i = 0; i < n; i++) v[i] = (i * 2654435761u) % t;
        emu_batch_nwt(1, log_n, t, itw.data(), ninv, (u64)(((unsigned __int128)ninv << 64) / t), inv.data(), v.data(), NWT_IN_GATHER, n - 3,
                      mid.data(), plain.data(), NWT_OUT_CANON, 0);
        emu_batch_nwt(0, log_n, t, tw.data(), ninv, 0, inv.data(), plain.data(), NWT_IN_PLAIN, 0, mid.data(), back.data(), NWT_OUT_SCATTER, 0);
        for (u32 i = 0; i < n; i++)
            if (back[i] != (i < n - 3 ? v[i] : 0)) { std::printf("mismatch at %u (N = 2^%u)\n", i, log_n); return 1; }
    }
    std::printf("emu_batch round trips OK\n");
    return 0;
}
#endif
