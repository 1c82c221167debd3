// emu_ntt_order.cpp -- TEST-ONLY: the work maps of the batched NTT launch pair (phantom-fhe_amd/csrc/pha_ntt_core.h: ZloopMap,
// PassOrder and the rules that build them -- the very functions the launchers and ntt_pass_kernel call) compiled for the host.
// emu_ntt_order() builds the maps of one launch the way forward_impl / inverse_impl do and decodes EVERY block of the strided
// pass's grid in dispatch order (x fastest, then y, then z), and a margin of blocks past its end; tests/test_emu_ntt_order.py proves the bijection and the order from the lists.
#include <cstddef>
#include <cstdint>
#include "../../phantom-fhe_amd/csrc/pha_ntt_core.h"

using namespace pha;

namespace {

struct Geometry {
    uint32_t tiles_s, tiles_c, waves_c;   // tiles per limb of the strided / contiguous pass, wavefronts per contiguous workgroup
};
template <int LOGN, int V>
Geometry geometry_of() {
    using P1 = typename NttPlan<LOGN, V>::P1;
    using Z2 = typename NttPlan<LOGN, V == 4 ? 3 : V>::P2;   // (forward_impl: plan 4 takes plan 3's contiguous pass here)
    return Geometry{(uint32_t)((1u << LOGN) >> P1::LOGTILE), (uint32_t)((1u << LOGN) >> Z2::LOGTILE), (uint32_t)(Z2::THREADS / 64)};
}
bool geometry(int log_n, int variant, Geometry &g) {
    if (log_n == 16 && variant == 10) g = geometry_of<16, 10>();
    else if (log_n == 14 && variant == 3) g = geometry_of<14, 3>();
    else if (log_n == 14 && variant == 4) g = geometry_of<14, 4>();
    else if (log_n == 15 && variant == 3) g = geometry_of<15, 3>();
    else if (log_n == 15 && variant == 4) g = geometry_of<15, 4>();
    else if (log_n == 17 && variant == 3) g = geometry_of<17, 3>();
    else if (log_n == 17 && variant == 4) g = geometry_of<17, 4>();
    else return false;
    return true;
}

}  // namespace

extern "C" {

// One launch of `count` limbs x `batch` polynomials on plan (log_n, variant); fp[y] != 0: limb y runs on the FP64 back end.
// part / parts: the whole launch (0 / 1) or one of its two limb-range halves (0 or 1 / 2).
// Out: info[0] = polynomials per workgroup of the contiguous pass (0: the rule does not engage, nothing else is written),
//      info[1] = first limb of the part, info[2] = its limb count, info[3] = blocks of the strided grid (x * y * z), info[4] = strided tiles per
//      limb, info[5] = blocks of the contiguous grid, info[6] = integer limbs of the part;
//      s_limbs [info[2]]: the contiguous pass's limb list (order S), relative to the SELECTION's first limb;
//      dec [(info[3] + margin) x 4]: per block of the strided pass (valid, limb relative to the selection, polynomial, tile).
// Returns 0, -1 for a plan without a geometry here, -2 when `cap` blocks do not hold the grid and the margin.
int emu_ntt_order(int log_n, int variant, uint32_t batch, uint32_t count, const uint8_t *fp, int int_head, uint32_t part, uint32_t parts,
                  uint32_t margin, uint32_t cap, uint32_t *info, uint8_t *s_limbs, uint32_t *dec) {
    Geometry g;
    if (!geometry(log_n, variant, g)) return -1;
    info[0] = 0;
    if (count > 128) return 0;
    const uint32_t zper = zloop_zper(batch, (size_t)g.tiles_c * count, g.waves_c, 8);
    ZloopMap m;
    if (!zper || !zloop_fill(m, count, fp, batch, zper, g.tiles_c)) return 0;
    uint32_t lo = 0, hi = count;
    if (parts == 2) {
        lo = part ? pass_order_half(count) : 0;
        hi = part ? count : pass_order_half(count);
        m = zloop_sub(m, lo, hi, batch);
    }
    const PassOrder o = pass_order_reverse(m, g.tiles_s, int_head != 0);
    uint32_t gx, gy, gz;
    pass_order_grid(o, batch, gx, gy, gz);
    const uint32_t blocks = gx * gy * gz;
    info[0] = zper;
    info[1] = lo;
    info[2] = hi - lo;
    info[3] = blocks;
    info[4] = g.tiles_s;
    info[5] = zloop_blocks(m, batch);
    info[6] = m.n_int;
    if (m.n_int + m.n_fp != hi - lo) return -3;
    for (uint32_t i = 0; i < hi - lo; i++) s_limbs[i] = (uint8_t)(m.limb[i] + lo);
    if ((size_t)blocks + margin > cap) return -2;
    for (uint32_t b = 0; b < blocks + margin; b++) {
        uint32_t y = 0xffffffffu, z = 0xffffffffu, tile = 0xffffffffu;
        // block b of the dispatch order: x fastest, then y, then z (the margin: further z planes)
        const bool ok = pass_order_decode(o, batch, b % gx, (b / gx) % gy, b / (gx * gy), y, z, tile);
        dec[4 * (size_t)b] = ok ? 1u : 0u;
        dec[4 * (size_t)b + 1] = ok ? y + lo : y;
        dec[4 * (size_t)b + 2] = z;
        dec[4 * (size_t)b + 3] = tile;
    }
    return 0;
}

}
