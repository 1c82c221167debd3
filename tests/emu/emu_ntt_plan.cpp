// emu_ntt_plan.cpp -- TEST-ONLY: which plan a launch takes (phantom-fhe_amd/csrc/pha_ntt_core.h: resolve_plan, the very function the
// launchers call behind choose_plan) and the geometry of that plan's two grids, compiled for the host.  tests/test_emu_ntt_plan.py holds
// the expected values: the kernel traces recorded in profiles/ntt_plan_switch_kernels.md.
#include <cstddef>
#include <cstdint>
#include "../../phantom-fhe_amd/csrc/pha_ntt_core.h"

using namespace pha;

namespace {

// out[0..3]: strided pass tiles per limb, threads; contiguous pass tiles per limb, threads
template <class P1, class P2>
void geometry_of(int log_n, uint32_t *out) {
    out[0] = (uint32_t)((1u << log_n) >> P1::LOGTILE);
    out[1] = (uint32_t)P1::THREADS;
    out[2] = (uint32_t)((1u << log_n) >> P2::LOGTILE);
    out[3] = (uint32_t)P2::THREADS;
}
template <int LOGN>
bool geometry_at(int variant, uint32_t *out) {
#define PLAN(V) case V: geometry_of<typename NttPlan<LOGN, V>::P1, typename NttPlan<LOGN, V>::P2>(LOGN, out); return true;
    switch (variant) {
        PLAN(0) PLAN(1) PLAN(2) PLAN(3) PLAN(4)
    }
    if constexpr (LOGN >= 14 && LOGN <= 16) {
        switch (variant) { PLAN(5) }
    }
    if constexpr (LOGN == 16) {
        switch (variant) { PLAN(8) PLAN(10) PLAN(12) }
    }
#undef PLAN
    return false;
}
bool geometry(const ResolvedPlan &r, uint32_t *out) {
    if (r.whole) {   // one workgroup per limb and polynomial, no strided pass
        out[0] = out[1] = 0;
        out[2] = 1;
        out[3] = r.whole == 12 ? WholePlan12::THREADS : r.whole == 13 ? WholePlan13::THREADS : WholePlan14::THREADS;
        return r.whole == r.log_n && r.whole >= 12 && r.whole <= 14;
    }
    switch (r.log_n) {
        case 12: return geometry_at<12>(r.variant, out);
        case 13: return geometry_at<13>(r.variant, out);
        case 14: return geometry_at<14>(r.variant, out);
        case 15: return geometry_at<15>(r.variant, out);
        case 16: return geometry_at<16>(r.variant, out);
        case 17: return geometry_at<17>(r.variant, out);
    }
    return false;
}

}  // namespace

extern "C" {

// The plan of a launch of `limbs` limbs x `batch` polynomials at N = 2^log_n.  flags: bit 0 first_pass_only, bit 1 second_pass_only,
// bit 2 the experiments library's rules, bit 3 (experiments) workgroups are placed round-robin on the XCDs.
// out[0] = NttPlan variant, out[1] = whole (0 / 12 / 13 / 14), out[2] = zfast, out[3] = one launch (bit 0: taken, bit 1: asked for),
// out[4..7] = the geometry above.
// Returns 0, or -1 when NttPlan has no such (degree, variant).
int emu_ntt_plan(int log_n, uint32_t limbs, uint32_t batch, int flags, int variant_bits, uint64_t whole14_min, uint64_t one_launch_min_tiles,
                 uint32_t *out) {
    PlanShape p{};
    p.log_n = log_n;
    p.limbs = limbs;
    p.batch = batch;
    p.first_pass_only = (flags & 1) != 0;
    p.second_pass_only = (flags & 2) != 0;
    p.variant_bits = variant_bits;
    p.experiments = (flags & 4) != 0;
    p.xcd_round_robin = (flags & 8) != 0;
    p.whole14_min = (size_t)whole14_min;
    p.one_launch_min_tiles = (size_t)one_launch_min_tiles;
    const ResolvedPlan r = resolve_plan(p);
    out[0] = (uint32_t)r.variant;
    out[1] = (uint32_t)r.whole;
    out[2] = r.zfast ? 1u : 0u;
    out[3] = (r.one_launch ? 1u : 0u) | (r.one_launch_asked ? 2u : 0u);
    return geometry(r, out + 4) ? 0 : -1;
}

int emu_ntt_default_variant() { return kDefaultVariant; }

// The twiddle-resident contiguous pass of a two-pass launch on plan (log_n, variant), by the rule plan_zloop (pha_ntt.hip) calls:
// zloop_variant and zloop_plan.  fp[y] != 0 where limb y runs on the FP64 back end.  out[0] = polynomials per workgroup (0: the launch
// takes the plan's own contiguous pass), out[1] = blocks of the 1-D grid.
int emu_ntt_plan_zloop(int log_n, int variant, uint32_t limbs, uint32_t batch, const uint8_t *fp, uint32_t *out) {
    out[0] = out[1] = 0;
    if (zloop_variant(variant) < 0) return 0;
    ResolvedPlan r{log_n, zloop_variant(variant), 0, false, false, false};
    uint32_t g[4];
    if (!geometry(r, g)) return -1;
    ZloopMap m;
    if (!zloop_plan(m, limbs, fp, batch, g[2], g[3] / 64, kZloopMinBatch)) return 0;
    out[0] = m.zper;
    out[1] = zloop_blocks(m, batch);
    return 0;
}

}
