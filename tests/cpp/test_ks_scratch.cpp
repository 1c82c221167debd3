// test_ks_scratch.cpp -- TEST-ONLY, host only (no device is touched): the key switch's scratch layout, KsScratch of
// phantom-fhe_amd/csrc/pha_internal.h, against the expressions the key-switch entries of pha_rns.hip wrote out by hand before it
// existed:
//     words = B * (2 * ql_n + beta * qlp_n + 2 * qlp_n)
//     tmp = base, t_mod_up = base + B * 2 * ql_n, cx = t_mod_up + B * beta * qlp_n          (ql_n = Ql * N, qlp_n = QlP * N)
// and the documented layout tmp [B][2][Ql][N] | t_mod_up [B][beta][QlP][N] | cx [B][2][QlP][N]: the regions follow each other without
// a gap and cx ends at base + words, where a caller's own regions begin.  Built and run by tests/test_ks_scratch.py.
#include <cstdint>
#include <cstdio>

#include "../../phantom-fhe_amd/csrc/pha_internal.h"

using pha::KsScratch;
using pha::u64;

struct Case {
    uint32_t ql, qlp, beta;   // as the entries hold them: Tool::size_ql, size_qlp, beta
    size_t n;
    uint32_t B;
};

int main() {
    const Case cases[] = {
        {6, 8, 3, 4096, 1},
        {7, 10, 3, 8192, 4},
        {45, 60, 3, 65536, 32},
        {63, 64, 63, 4096, 1024},   // beta * B = 64512: the most digit polynomials the batched entries admit (63 x 1024 <= 65535 < 64 x 1024)
    };
    // the pointers are compared, never dereferenced: the largest case spans 2^37 bytes
    u64 *const base = reinterpret_cast<u64 *>(uintptr_t(1) << 44);
    int bad = 0;
    for (const Case &k : cases) {
        const size_t ql_n = (size_t)k.ql * k.n, qlp_n = (size_t)k.qlp * k.n;
        const size_t words = k.B * (2 * ql_n + (size_t)k.beta * qlp_n + 2 * qlp_n);
        const size_t got = KsScratch::words(k.ql, k.qlp, k.beta, k.n, k.B);
        const KsScratch s(base, k.ql, k.qlp, k.beta, k.n, k.B);
        u64 *tmp = base, *t_mod_up = base + k.B * 2 * ql_n, *cx = t_mod_up + k.B * (size_t)k.beta * qlp_n;
        const bool ok = got == words && s.tmp == tmp && s.t_mod_up == t_mod_up && s.cx == cx &&
                        s.t_mod_up == s.tmp + (size_t)k.B * 2 * k.ql * k.n &&                  // tmp      [B][2][Ql][N]
                        s.cx == s.t_mod_up + (size_t)k.B * k.beta * k.qlp * k.n &&             // t_mod_up [B][beta][QlP][N]
                        base + got == s.cx + (size_t)k.B * 2 * k.qlp * k.n;                    // cx       [B][2][QlP][N]
        if (!ok) {
            std::printf("KsScratch (ql %u, qlp %u, beta %u, n %zu, B %u): words %zu, want %zu; offsets %td %td %td, want 0 %td %td\n", k.ql,
                        k.qlp, k.beta, k.n, k.B, got, words, s.tmp - base, s.t_mod_up - base, s.cx - base, t_mod_up - base, cx - base);
            bad++;
        }
    }
    if (!bad) std::printf("KsScratch layout OK (%zu cases)\n", sizeof(cases) / sizeof(cases[0]));
    return bad ? 1 : 0;
}
