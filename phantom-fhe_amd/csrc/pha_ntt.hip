// pha_ntt.hip -- NTT kernels and launchers (gfx950).
//
// One templated kernel per (pass configuration, direction, epilogue); the thread program is
// pha_ntt_core.h.  The 17 launchers of include/ntt.cuh:157-226 that the hot path uses collapse to
// two drivers (forward / inverse) parameterised by a limb selector (start, special-prime remap,
// excluded range: src/ntt/fntt_2d.cu:434-437, src/ntt/ntt_modup.cu:422) and an epilogue
// (canonicalise / fused mod-down / scale), instead of 25 hand-copied kernels.
#include "../../include/phantom_amd.h"
#include "pha_internal.h"
#include "pha_experiments.h"
#include "pha_ntt_core.h"

#include <atomic>
#include <type_traits>

namespace pha {

// Kernel selection.  The product library holds ONE plan per degree and launch size (constants below, chosen from the r01 / r02
// sweeps); every other geometry that was built and measured (16 coefficients per thread, 512-thread contiguous passes, the
// one-workgroup N = 2^14 plan, both passes in one launch with the L2 hand-off, ...) lives behind -DPHA_EXPERIMENTS in the test-only
// library libphantom_amd_exp.so (csrc/pha_experiments.h: pha_set_tuning), because the extra instantiations alone cost ~30 us per
// key switch when they sat in the product code object.
// The rules that pick a plan for a launch shape, and the variant bits of the experiments build, are resolve_plan (pha_ntt_core.h).
// twiddle request schedule of the stand-alone passes (PassProgram's HOIST): every round requests its own (r04: all up front and one
// round ahead both measured slower, profiles/r04_experiments.md)
constexpr int kPassHoist = 0;
// Block order of the strided pass of a launch pair whose contiguous pass is ntt_zloop_kernel (PassOrder, pha_ntt_core.h; measured in
// profiles/ntt_pass_order.md).  A compile-time choice, no run-time knob: 0 = the plain grid (tile, limb, polynomial), poly-major;
// 1 = the reverse of the contiguous pass's order; 2 = 1, and a launch whose buffer is larger than the last-level cache goes as two
// launch pairs, one per half of its limbs.
#ifndef PHA_NTT_PASS_ORDER
#define PHA_NTT_PASS_ORDER 1
#endif
#ifndef PHA_NTT_ORDER_INT_HEAD
#define PHA_NTT_ORDER_INT_HEAD 1   // 1: the integer limbs stay at the head of the strided launch (pass_order_reverse); 0: the exact reverse, integer limbs last
#endif
#if defined(PHA_EXPERIMENTS)
std::atomic<int> g_ntt_variant{kDefaultVariant};
static inline int ntt_variant() { return g_ntt_variant.load(std::memory_order_relaxed); }
std::atomic<int> g_whole14_min{1 << 30};     // key 2: limb-polynomials per launch from which N = 2^14 takes the one-workgroup plan (r02: never faster)
std::atomic<int> g_fused_split{0};           // key 5: one pass per workgroup in the one-launch transform (r02: slower still)
std::atomic<int> g_fused_lag{2};             // key 3: lag (in units per XCD) between the two passes of the one-launch transform
std::atomic<int> g_fused_min_tiles{1 << 30}; // key 4: tiles per launch from which the two passes share one launch (r02: 7 % slower at every size)
extern std::atomic<int> g_bconv_split;       // pha_rns.hip (key 1)
#else
static constexpr int ntt_variant() { return kDefaultVariant; }
#endif

struct NttKArgs {
    const u64 *in;
    u64 *out;
    u64 *mid;                // buffer between the two passes (pass 1: in -> mid, pass 2: mid -> out)
    const u64x2 *tw;         // table base [prime][n] (forward or inverse)
    const DModulus *mod;     // [prime]
    const u64x2 *ninv;       // [prime]
    const u64x2 *w1ninv;     // [prime]
    const u64 *twf;          // FP64 path: table base [prime][n] of doubles W (forward or inverse)
    const u64x2 *ninvf, *w1ninvf;
    const FpInfo *fpinfo;    // [prime]; null = FP64 path off
    const u64 *scale;        // [limb] or null
    const u64 *scale_shoup;  // [limb] or null
    const u64 *aux;          // fuse_moddown: cx base
    const u64 *aux2;         // EPI_FWD_KSRESCALE: ct base; scale2 / scale2_shoup [limb]: PInv
    union {
        const u64 *scale2;
        const u64 *aux3;     // EPI_FWD_NEG_MULADD (which has no scale2): the plaintext's base, or null
    };
    const u64 *scale2_shoup;
    size_t aux2_stride;
    LimbSel sel;
    uint32_t log_n;
    uint32_t t1, t2;         // N = t1 * t2
    uint32_t reserved;       // unused, zero (make_args value-initialises the struct and nothing writes it).  It holds the place of a field
                             // nothing read: without these 4 bytes every later kernel argument moves by 8, the kernels' scalar loads regroup,
                             // 38 of the product's kernels change and 18 strided passes take 2 SGPRs more.  A change that alters these
                             // kernels anyway can drop it.
    uint32_t batch;          // polynomials per launch (blockIdx.z)
    size_t poly_stride, out_stride, aux_stride;
    size_t in_stride;        // elements between the polynomials of `in` (first pass; the second pass reads mid at poly_stride)
    bool first_pass_only;    // forward: the caller runs its own (fused) second pass
    bool second_pass_only;   // inverse: the contiguous pass was folded into the producer of `mid`
    bool first_pass_done;    // forward: the strided pass was folded into the producer of `mid` (modup_conv_s1_kernel)
    uint32_t excl_step, excl_limit, excl_mod;
    const u64 *pro_src;      // rescale prologue: every limb of polynomial z reads pro_src + z * pro_stride instead
    size_t pro_stride;
    // batched launches, polynomial-fastest order: a 1-D grid in which the `batch` polynomials of one (tile, limb) run back to
    // back on ONE XCD (block b -> XCD b % 8), so that the twiddle rows they share are fetched into that L2 once
    uint32_t zfast_tiles;    // 0 = plain 3-D grid (tile, limb, polynomial); else tiles per limb of the 1-D form
    uint32_t zfast_run;      // tiles of one polynomial that run back to back before the next polynomial's (a multiple of 8)
    bool pro_ckks;           // the prologue is CKKS round-and-reduce instead (PRO_CKKS kernels): pro_src holds doubles
    bool pro_small;          // the prologue is the sample lift instead (PRO_SMALL kernels, encryption): pro_src holds signed words |v| <= 2^16
    union {
        u64 pro_t;           // != 0 (not pro_small): the prologue is the BFV plain lift instead (PRO_LIFT kernels): pro_src holds words below pro_t
        u64 pro_k;           // pro_small: != 0: the lifted sample is multiplied by this factor (bgv's t), reduced per limb
    };
    union {
        size_t aux_pair_stride;  // EPI_INV_CANON_ADD: polynomial z adds aux + (z / 2) * aux_pair_stride + (z % 2) * aux_stride (acc of group z / 2)
        size_t aux3_stride;      // EPI_FWD_NEG_MULADD: polynomial z reads aux3 + z * aux3_stride (and aux, aux2 at z * aux_stride, z * aux2_stride, 0 = shared)
    };
    const u64 *h_primes;     // HOST copy of the context's primes (launchers only: which limbs run on the FP64 back end)
};
// (The encryption launches added no field behind h_primes: a longer NttKArgs moves the kernels' second argument, and every kernel of
//  this file then differs from its earlier build.  Their flag sits in the padding behind pro_ckks; their third operand, its stride and
//  the sample factor share the storage of fields no such launch reads -- the anonymous unions above.)
// The plain modulus of the BFV plain lift, 0 where the launch has none.  The HOST reads pro_t through this alone: under pro_small the
// word is the sample factor (bgv: t != 0), which must never select a PRO_LIFT kernel.  (The device reads k.pro_t once, in
// full_tile_args, for operands that only the PRO_LIFT kernels use; scale2 is read under EPI_FWD_KSRESCALE only, which pro_small excludes.)
static inline u64 lift_t(const NttKArgs &k) { return k.pro_small ? 0 : k.pro_t; }
static_assert(sizeof(NttKArgs) == 296,"NttKArgs is a kernel argument in front of another: its size is part of every kernel's code");

// Per-tile arguments of limb `twr` (absolute limb index in the buffer), tile `tile`.
template <bool FWD, int EPI, bool FOLD>
__device__ __forceinline__ void tile_args(const NttKArgs &k, uint32_t twr, uint32_t tile, PassArgs &a) {
    const uint32_t prime = twr >= k.sel.remap_from ? twr + k.sel.remap_add : twr;
    const size_t n = (size_t)1 << k.log_n;
    a.in = k.in + (size_t)twr * n;
    a.out = k.out + (size_t)twr * n;
    a.tw = k.tw + (size_t)prime * n;
    a.twd = nullptr;
    a.q = k.mod[prime].value;
    a.tile = tile;
    a.rho0 = k.t1;
    a.stride = k.t2;
    if (!FWD && FOLD) {
        a.ninv = k.ninv[prime];
        a.w1ninv = k.w1ninv[prime];
    }
    a.pro_reduce = false;
    a.pro_ratio1 = 0;
    a.fp = false;
    if (k.fpinfo) {  // primes below 2^50 take the FP64 butterflies (uniform per workgroup)
        const FpInfo fi = k.fpinfo[prime];
        if (fi.ok) {
            a.fp = true;
            a.fpm = FpMod{fi.q, fi.qinv, (fi.ok & 2) != 0, (fi.ok & 4) != 0};
            a.twd = k.twf + (size_t)prime * n;
            if (!FWD && FOLD) {
                a.ninv = k.ninvf[prime];
                a.w1ninv = k.w1ninvf[prime];
            }
        }
    }
    if (EPI == EPI_INV_SCALE || EPI == EPI_FWD_MODDOWN || EPI == EPI_FWD_MODDOWN_ADD || EPI == EPI_FWD_KSRESCALE) {
        a.scale.x = k.scale[twr];
        a.scale.y = k.scale_shoup[twr];
    }
    a.aux = (EPI == EPI_FWD_MODDOWN || EPI == EPI_FWD_MODDOWN_ADD || EPI == EPI_FWD_KSRESCALE || EPI == EPI_INV_CANON_ADD) ? k.aux + (size_t)twr * n : nullptr;
    if (EPI == EPI_FWD_KSRESCALE) {
        a.scale2.x = k.scale2[twr];
        a.scale2.y = k.scale2_shoup[twr];
        a.aux2 = k.aux2 + (size_t)twr * n;
    }
    if (muladd_epilogue(EPI)) {   // the factors and the plaintext are indexed by buffer limb, like out
        a.aux = k.aux + (size_t)twr * n;
        a.aux2 = k.aux2 + (size_t)twr * n;
        a.aux3 = k.aux3 ? k.aux3 + (size_t)twr * n : nullptr;
        a.ratio0 = k.mod[prime].ratio0;
        a.ratio1 = k.mod[prime].ratio1;
    }
}

// polynomial z skips its own digit: the limbs [excl_start + z*step, min(that + len, limit))  (ntt_modup.cu:422).  The one statement of
// the rule, for the kernels and for the host (launch_fused counts the units a launch transforms with it).
PHA_HD bool limb_excluded(const NttKArgs &k, uint32_t twr, uint32_t z) {
    const uint32_t zd = k.excl_mod ? z % k.excl_mod : z;
    const uint32_t es = k.sel.excl_start + zd * k.excl_step;
    uint32_t ee = es + (k.sel.excl_end - k.sel.excl_start);
    ee = ee < k.excl_limit ? ee : k.excl_limit;
    return twr >= es && twr < ee;
}

// Arguments of tile `tile` of limb `twr` of polynomial `z`, with the batch offsets and the rescale prologue.
template <class C, bool FWD, int EPI, bool FOLD>
__device__ __forceinline__ void full_tile_args(const NttKArgs &k, uint32_t twr, uint32_t z, uint32_t tile, PassArgs &a) {
    tile_args<FWD, EPI, FOLD>(k, twr, tile, a);
    if (k.batch > 1) {  // same limbs of several polynomials in one launch
        a.in += (size_t)z * k.in_stride;
        a.out += (size_t)z * k.out_stride;
        if (EPI == EPI_FWD_MODDOWN || EPI == EPI_FWD_MODDOWN_ADD || EPI == EPI_FWD_KSRESCALE) a.aux += (size_t)z * k.aux_stride;
        if (EPI == EPI_FWD_KSRESCALE) a.aux2 += (size_t)z * k.aux2_stride;
    }
    if (EPI == EPI_INV_CANON_ADD) a.aux += (size_t)(z >> 1) * k.aux_pair_stride + (size_t)(z & 1) * k.aux_stride;
    if (muladd_epilogue(EPI)) {   // (the strides as the caller gave them: 0 shares an operand between the polynomials)
        a.aux += (size_t)z * k.aux_stride;
        a.aux2 += (size_t)z * k.aux2_stride;
        if (a.aux3) a.aux3 += (size_t)z * k.aux3_stride;
    }
    if (FWD && (C::STRIDED || C::WHOLE) && k.pro_src) {  // rescale prologue: transform (the last limb of polynomial z) mod this prime
        const uint32_t prime = twr >= k.sel.remap_from ? twr + k.sel.remap_add : twr;
        a.in = k.pro_src + (size_t)z * k.pro_stride;
        a.pro_reduce = true;
        a.pro_ratio1 = k.mod[prime].ratio1;
        a.pro_half = bfv_lift_threshold(k.pro_t);   // (read by the PRO_LIFT kernels only; under pro_small the word is pro_k and these two are dead)
        a.pro_inc = bfv_lift_increment(a.q, k.pro_t);
        a.pro_k = k.pro_k;   // (read by the PRO_SMALL kernels only, as the Barrett ratio; plain loads, so that the other kernels drop them)
        a.ratio0 = k.mod[prime].ratio0;
        a.ratio1 = a.pro_ratio1;
    }
}

// One pass over one tile, one specialised body per butterfly back end (PHA_WITH_FP_KNOWN).
// COH: the pass reads what other workgroups of this launch wrote (one-launch transform).
// ONLY: 0 = both back ends (a.fp decides), 2 = the caller knows the limb runs on the integer back end (one body: fewer registers).
template <class C, bool FWD, int EPI, bool FOLD, int HOIST, bool COH, int ONLY = 0, int PRO = PRO_NONE>
__device__ __forceinline__ void exec_pass(const PassArgs &a, u64 *lds, int tid) {
    u64 reg[C::EPT];
    u64x2 twreg[C::TW_TOTAL];
    using Prog = PassProgram<C, FWD, EPI, FOLD, HOIST, COH, PRO>;
    auto pass = [&](const PassArgs &pa) __attribute__((always_inline)) {
        Prog::load_twiddles(pa, tid, twreg);
        Prog::template run_pass<SEG_PLAIN, false>(pa, lds, tid, reg, twreg);
    };
    PHA_WITH_FP_KNOWN(a, ONLY != 2 && a.fp, pass);
}

// ---- r04: the contiguous pass of BATCHED forward launches with the twiddles resident in registers ------------------------------
// A tile of the contiguous pass (whole rows of limb j) needs the same twiddles for every polynomial of the batch.  ntt_pass_kernel
// fetches them once per (tile, polynomial) -- 26 loads per thread with their address arithmetic, from the L2 when the
// polynomial-fastest block order has kept the rows there.  Here one workgroup owns tile t of limb j for `zper` polynomials in a
// row: on the FP64 back end it requests ALL rounds' twiddles once (8 bytes per entry: two registers each) and then walks its
// polynomials -- 26 loads, their address arithmetic and their waits leave the loop, which is what an issue-bound pass is short of
// (720 limbs at N = 2^16: 300 -> 274 us per step with 4 polynomials per workgroup).  Integer-back-end limbs (60-bit primes: 16-byte twiddle pairs would need 100+ registers) take the plain pass, one
// (tile, polynomial) per workgroup, at the head of the same grid.
// Work map of one launch: ZloopMap (pha_ntt_core.h): a 1-D grid, the integer-back-end limbs FIRST (their tiles are the longest: one
// polynomial per workgroup, so that they run side by side from the start), then the FP64 limbs with zper polynomials per workgroup.
template <class C, bool FWD, int EPI, bool FOLD>
__global__ __launch_bounds__(C::THREADS) void ntt_zloop_kernel(const NttKArgs k, const ZloopMap m) {
    static_assert(!C::WHOLE, "the batched form exists for the passes of the two-pass plans");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *lds = reinterpret_cast<u64 *>(smem);
    __builtin_amdgcn_s_setprio(3);
    const int tid = threadIdx.x;
    uint32_t b = blockIdx.x;
    PassArgs a;
    if (b < m.int_blocks) {   // (uniform) integer back end: the plain pass on one (tile, limb, polynomial)
        const uint32_t tile = b % m.tiles, rest = b / m.tiles, z = rest % k.batch, twr = k.sel.start + m.limb[rest / k.batch];
        if (limb_excluded(k, twr, z)) return;    // (uniform) the mod-up's rule: digit z does not transform its own limbs
        full_tile_args<C, FWD, EPI, FOLD>(k, twr, z, tile, a);
        exec_pass<C, FWD, EPI, FOLD, 0, false, 2>(a, lds, tid);   // (integer body only: the map put no FP64 limb here)
        return;
    }
    b -= m.int_blocks;
    const uint32_t tile = b % m.tiles, rest = b / m.tiles, zgroups = (k.batch + m.zper - 1) / m.zper;
    const uint32_t twr = k.sel.start + m.limb[m.n_int + rest / zgroups];
    const uint32_t z0 = (rest % zgroups) * m.zper, z1 = (z0 + m.zper < k.batch) ? z0 + m.zper : k.batch;
    full_tile_args<C, FWD, EPI, FOLD>(k, twr, z0, tile, a);
    using Prog = PassProgram<C, FWD, EPI, FOLD, 1, false>;   // HOIST 1: every round's twiddles before the loop
    a.fp = true;
    u64x2 twreg[C::TW_TOTAL];
    Prog::load_twiddles(a, tid, twreg);
    // Polynomial z + 1's coefficients are requested before polynomial z is transformed (a second register set: 126 registers, still
    // four wavefronts per SIMD): with the twiddles out of the loop those 8 loads are the only ones inside it, so no wait for anything
    // else drains them early.  Forward step +-0, inverse step 285 -> 272 us (its contiguous pass is the transform's first).
    u64 regA[C::EPT], regB[C::EPT];
    auto args_of = [&](uint32_t z) __attribute__((always_inline)) {
        PassArgs b = a;
        const size_t dz = (size_t)(z - z0);
        b.in += dz * k.in_stride;
        b.out += dz * k.out_stride;
        if (EPI == EPI_FWD_MODDOWN || EPI == EPI_FWD_MODDOWN_ADD || EPI == EPI_FWD_KSRESCALE) b.aux += dz * k.aux_stride;
        if (EPI == EPI_FWD_KSRESCALE) b.aux2 += dz * k.aux2_stride;
        return b;
    };
    auto transform = [&](const PassArgs &b, u64 *reg) __attribute__((always_inline)) {
        Prog::template run_pass<SEG_PREFETCHED, true>(b, lds, tid, reg, twreg);   // (tail hand-over: the next polynomial's first round writes the same LDS words)
    };
    auto next = [&](uint32_t z) __attribute__((always_inline)) {   // (uniform) first polynomial >= z that transforms this limb (mod-up: a digit skips its own)
        while (z < z1 && limb_excluded(k, twr, z)) z++;
        return z;
    };
    uint32_t z = next(z0);
    if (z >= z1) return;
    Prog::prefetch(args_of(z), tid, regA);
    __builtin_amdgcn_s_setprio(0);
    for (;;) {
        uint32_t zn = next(z + 1);
        if (zn < z1) Prog::prefetch(args_of(zn), tid, regB);
        transform(args_of(z), regA);
        if (zn >= z1) break;
        z = zn;
        zn = next(z + 1);
        if (zn < z1) Prog::prefetch(args_of(zn), tid, regA);
        transform(args_of(z), regB);
        if (zn >= z1) break;
        z = zn;
    }
}

// (r04: asking the compiler for a minimum occupancy per pass, amdgpu_waves_per_eu / a second __launch_bounds__ argument, never
//  beat its own choice: profiles/r04_experiments.md)
template <class C, bool FWD, int EPI, bool FOLD, int HOIST, int PRO = PRO_NONE>
__global__ __launch_bounds__(C::THREADS) void ntt_pass_kernel(const NttKArgs k, const PassOrder o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *lds = reinterpret_cast<u64 *>(smem);

    __builtin_amdgcn_s_setprio(3);   // until the first round's global loads are issued (PassProgram::run)
    uint32_t tile = blockIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (k.zfast_tiles) {
        // block b = ((chunk * batch) + z) * run + i: the `run` adjacent (tile, limb) groups of a chunk for polynomial 0, then the same
        // groups for polynomial 1, ...; run is a multiple of 8, so group i of every polynomial lands on XCD i % 8
        const uint32_t b = blockIdx.x, per_chunk = k.zfast_run * k.batch, chunk = b / per_chunk, rem = b - chunk * per_chunk;
        z = rem / k.zfast_run;
        const uint32_t group = chunk * k.zfast_run + (rem - z * k.zfast_run);
        if (group >= k.zfast_tiles * k.sel.count) return;
        tile = group % k.zfast_tiles;
        y = group / k.zfast_tiles;
    }
#if PHA_NTT_PASS_ORDER
    else if (o.tiles) {   // (uniform) the strided pass of a pair whose contiguous pass is ntt_zloop_kernel: the reverse of that kernel's order
        if (!pass_order_decode(o, k.batch, blockIdx.x, blockIdx.y, blockIdx.z, y, z, tile)) return;
    }
#endif
    const uint32_t twr = k.sel.start + y;  // limb in the buffer (uniform)
    if (limb_excluded(k, twr, z)) return;
    PassArgs a;
    full_tile_args<C, FWD, EPI, FOLD>(k, twr, z, tile, a);
    exec_pass<C, FWD, EPI, FOLD, HOIST, false, 0, PRO>(a, lds, threadIdx.x);
}

// A kernel whose dynamic LDS request can exceed the default limit of 64 KiB: raise the limit to `bytes` once per kernel and device
// (`raised`: the kernel's own flag word, one bit per device).
static void raise_lds_limit(const void *kernel, size_t bytes, std::atomic<uint64_t> &raised) {
    if (bytes <= 64 * 1024) return;
    int dev = 0;
    PHA_HIP(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (raised.load(std::memory_order_acquire) & bit) return;
    PHA_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    raised.fetch_or(bit, std::memory_order_release);
}

template <class C, bool FWD, int EPI, bool FOLD, int PRO = PRO_NONE>
static void launch_pass(const NttKArgs &k, hipStream_t s, const PassOrder *order = nullptr) {
    const size_t n = (size_t)1 << k.log_n;
    const size_t lds_bytes = (size_t)C::LDS_WORDS * sizeof(u64);
    const unsigned tiles_per_limb = (unsigned)(n >> C::LOGTILE);
    dim3 grid(tiles_per_limb, k.sel.count, k.batch);
    NttKArgs kk = k;
    kk.zfast_tiles = 0;   // (k.zfast_tiles is only the caller's request flag)
    if (!C::STRIDED && !C::WHOLE && k.zfast_tiles) {
        kk.zfast_tiles = tiles_per_limb;
        kk.zfast_run = 8;
        const unsigned groups = tiles_per_limb * k.sel.count;
        grid = dim3(((groups + kk.zfast_run - 1) / kk.zfast_run) * kk.zfast_run * k.batch, 1, 1);
    }
    PassOrder o{};
    if (order && !kk.zfast_tiles) {   // the caller's block order (the strided pass of a pair with ntt_zloop_kernel)
        o = *order;
        pass_order_grid(o, k.batch, grid.x, grid.y, grid.z);
    }
    // (requesting all rounds' twiddles up front, HOIST 1, was measured again in r02 for the small launches of mod-down and
    //  rescale: no gain at any size)
    static std::atomic<uint64_t> raised{0};
    raise_lds_limit(reinterpret_cast<const void *>(&ntt_pass_kernel<C, FWD, EPI, FOLD, kPassHoist, PRO>), lds_bytes, raised);
    // (r03: a two-tiles-per-wavefront, software-pipelined form of the one-wavefront contiguous pass for small launches was
    //  measured and dropped -- half as many wavefronts with twice the work each lose more latency hiding than the overlap of
    //  one tile's stores with the next tile's butterflies gains: 45 limbs 17.3 -> 19.2 us, 32 limbs 15.0 -> 16.5 us)
    hipLaunchKernelGGL((ntt_pass_kernel<C, FWD, EPI, FOLD, kPassHoist, PRO>), grid, dim3(C::THREADS), lds_bytes, s, kk, o);
    check_launch();
}

#if defined(PHA_EXPERIMENTS)
}  // namespace pha
#include "pha_ntt_onelaunch.h"
namespace pha {
constexpr bool kExperiments = true;
#else
constexpr bool kExperiments = false;
#endif

// ---- run-time choices -> template arguments ---------------------------------------------------------------------------------------
template <int E> using EpiC = std::integral_constant<int, E>;
template <int P> using ProC = std::integral_constant<int, P>;
// the epilogue of a transform's last pass: f(EpiC<...>) with the forward (FWD) or the inverse epilogue `epi` names; anything else is
// the canonical one
template <bool FWD, class F>
static void dispatch_epi(int epi, F &&f) {
    if constexpr (FWD) {
        if (epi == EPI_FWD_MODDOWN) f(EpiC<EPI_FWD_MODDOWN>{});
        else if (epi == EPI_FWD_MODDOWN_ADD) f(EpiC<EPI_FWD_MODDOWN_ADD>{});
        else if (epi == EPI_FWD_KSRESCALE) f(EpiC<EPI_FWD_KSRESCALE>{});
        else f(EpiC<EPI_FWD_CANON>{});
    } else {
        if (epi == EPI_INV_SCALE) f(EpiC<EPI_INV_SCALE>{});
        else if (epi == EPI_INV_CANON_ADD) f(EpiC<EPI_INV_CANON_ADD>{});
        else f(EpiC<EPI_INV_CANON>{});
    }
}
// the load prologue of a forward transform's first pass: the BFV plain lift (a plaintext's words lifted as they are loaded) where
// k.pro_t asks for it, the CKKS round-and-reduce (double coefficients rounded and reduced as they are loaded) where k.pro_ckks does.
// ntt_forward admits either with the canonical epilogue only.
template <class F>
static void dispatch_pro(const NttKArgs &k, F &&f) {
    if (k.pro_ckks) f(ProC<PRO_CKKS>{});
    else if (lift_t(k)) f(ProC<PRO_LIFT>{});
    else f(ProC<PRO_NONE>{});
}

// the inverse transform's last pass (the strided one, or the whole transform) with the epilogue the caller asked for
template <class P>
static void launch_inverse_last(const NttKArgs &k, int epi, hipStream_t s, const PassOrder *order = nullptr) {
    dispatch_epi<false>(epi, [&](auto e) { launch_pass<P, false, e(), true>(k, s, order); });
}

// N = 4096 / 8192 as ONE pass (the transform fits a tile): T1 = 1, T2 = N
template <class W, bool FWD>
static void launch_whole(NttKArgs k, int epi, hipStream_t s) {
    k.t1 = 1;
    k.t2 = W::T;
    k.mid = k.out;
    if constexpr (FWD) {
        if (k.pro_small) {   // encryption: the sample lift with the canonical or a mul-add epilogue, prologue and epilogue in one kernel
            if constexpr (W::LOGT <= 13) {   // (the product's one-workgroup plans; ntt_transform sends N = 2^14 through two passes)
                if (epi == EPI_FWD_MULADD) return launch_pass<W, true, EPI_FWD_MULADD, false, PRO_SMALL>(k, s);
                if (epi == EPI_FWD_NEG_MULADD) return launch_pass<W, true, EPI_FWD_NEG_MULADD, false, PRO_SMALL>(k, s);
                return launch_pass<W, true, EPI_FWD_CANON, false, PRO_SMALL>(k, s);
            } else {
                throw std::logic_error("ntt_forward: the sample lift has no one-workgroup form at this degree");
            }
        }
        dispatch_epi<true>(epi, [&](auto e) {
            if constexpr (e() == EPI_FWD_CANON) dispatch_pro(k, [&](auto p) { launch_pass<W, true, EPI_FWD_CANON, false, p()>(k, s); });
            else launch_pass<W, true, e(), false>(k, s);
        });
    } else {
        launch_inverse_last<W>(k, epi, s);
    }
}

// the batched, twiddle-resident passes (ntt_zloop_kernel): plain launches of >= 8 polynomials that fill the device
// several times over (the headline step, the batched key switch's 2 B-polynomial transforms); zper polynomials per workgroup, chosen so
// that the launch still holds >= 3 generations of wavefronts
// the launcher rule: does this launch take ntt_zloop_kernel for its contiguous pass, and with which work map
template <class C>
static bool plan_zloop(const NttKArgs &k, ZloopMap &m) {
    if (k.pro_src || k.sel.count > 128) return false;
    // which limbs of the selection run on the FP64 back end (the others: runs of consecutive limbs through the plain kernel)
    uint8_t fp[128];
    for (uint32_t y = 0; y < k.sel.count; y++) {
        const uint32_t twr = k.sel.start + y, prime = twr >= k.sel.remap_from ? twr + k.sel.remap_add : twr;
        fp[y] = k.fpinfo != nullptr && (k.h_primes[prime] >> 50) == 0;
    }
    return zloop_plan(m, k.sel.count, fp, k.batch, (uint32_t)(((size_t)1 << k.log_n) >> C::LOGTILE), C::THREADS / 64, kZloopMinBatch);
}
template <class C, bool FWD, int EPI, bool FOLD>
static void launch_zloop(const NttKArgs &k, const ZloopMap &m, hipStream_t s) {
    NttKArgs kk = k;
    kk.zfast_tiles = 0;
    const size_t lds_bytes = (size_t)C::LDS_WORDS * sizeof(u64);
    hipLaunchKernelGGL((ntt_zloop_kernel<C, FWD, EPI, FOLD>), dim3(zloop_blocks(m, k.batch)), dim3(C::THREADS), lds_bytes, s, kk, m);
    check_launch();
}
template <class C>
static void launch_zloop_forward(const NttKArgs &k, const ZloopMap &m, int epi, hipStream_t s) {
    dispatch_epi<true>(epi, [&](auto e) { launch_zloop<C, true, e(), false>(k, m, s); });
}

constexpr size_t kLastLevelCacheBytes = (size_t)256 << 20;   // Infinity Cache of the MI355X
// limbs [lo, lo + cnt) of the selection of k
static NttKArgs limb_range(const NttKArgs &k, uint32_t lo, uint32_t cnt) {
    NttKArgs h = k;
    h.sel.start = k.sel.start + lo;
    h.sel.count = cnt;
    return h;
}
// how many limb ranges the pair is issued in (order 2: two, for a selection whose words exceed the cache)
static uint32_t order_parts(const NttKArgs &k) {
    const size_t bytes = ((size_t)k.sel.count * k.batch << k.log_n) * sizeof(u64);
    return PHA_NTT_PASS_ORDER == 2 && k.sel.count >= 2 && bytes > kLastLevelCacheBytes ? 2u : 1u;
}

// The launch pairs of a batched transform whose contiguous pass is ntt_zloop_kernel with map `m`: pair(limbs [lo, lo + cnt) of the
// selection, their map, the block order of their strided pass -- null: the plain grid) once per limb range.  The strided pass ends
// where the contiguous pass begins, and the next transform of the buffer starts where this one ended; the caller states only which
// of the two launches goes first.
template <class F>
static void for_each_order_part(const NttKArgs &k, const ZloopMap &m, int strided_logtile, F &&pair) {
    if (PHA_NTT_PASS_ORDER == 0) return pair(0u, k.sel.count, m, (const PassOrder *)nullptr);
    const uint32_t parts = order_parts(k), cut = pass_order_half(k.sel.count);
    for (uint32_t h = 0; h < parts; h++) {
        const uint32_t lo = h * cut, hi = parts == 1 ? k.sel.count : h ? k.sel.count : cut;
        const ZloopMap mh = parts == 1 ? m : zloop_sub(m, lo, hi, k.batch);
        const PassOrder o = pass_order_reverse(mh, (uint32_t)(((size_t)1 << k.log_n) >> strided_logtile), PHA_NTT_ORDER_INT_HEAD != 0);
        pair(lo, hi - lo, mh, &o);
    }
}

constexpr int kIpPlan = 3;    // NttPlan variant whose contiguous pass carries the inner product (3: 8 coefficients per thread; 5: 4)
// the two-pass form: pass 1 runs in -> mid with the input stride; pass 2 reads mid and writes out with the output stride
template <int LOGN, int VARIANT>
struct TwoPass {
    using P1 = typename NttPlan<LOGN, VARIANT>::P1;
    using P2 = typename NttPlan<LOGN, VARIANT>::P2;
    // batched launches of the product's plans take the twiddle-resident contiguous pass (with the twiddles out of the loop there is
    // nothing to form on the fly: plan 4 runs plan 3's)
    static constexpr bool ZLOOP = zloop_variant(VARIANT) >= 0;
    using Z2 = typename NttPlan<LOGN, ZLOOP ? zloop_variant(VARIANT) : VARIANT>::P2;
    // both passes in one launch (experiments): the geometries ntt_fused_kernel is built for
    static constexpr bool ONE_LAUNCH = kExperiments && P1::THREADS == 512 && P1::LOGTILE == 12 && P2::THREADS == 64;
    NttKArgs k1, k2;
    explicit TwoPass(NttKArgs k) {
        k.t1 = P1::T;
        k.t2 = P2::T;
        k1 = k2 = k;
        k1.out = k.mid;
        k1.out_stride = k.poly_stride;
        k2.in = k.mid;
        k2.in_stride = k.poly_stride;
    }
};

template <int LOGN, int VARIANT>
static void forward_impl(const NttKArgs &k_in, int epi, hipStream_t s, Context *fused) {
    using T = TwoPass<LOGN, VARIANT>;
    using P1 = typename T::P1;
    using P2 = typename T::P2;
    T t(k_in);
    const NttKArgs &k1 = t.k1;
    NttKArgs &k = t.k2;
    k.pro_src = nullptr;   // the rescale prologue belongs to the first pass
    // the only producer that folds the strided pass away (modup_conv_s1_kernel) writes the 64 x 1024 split of NttPlan<16, 10>: a
    // plan choice that disagrees with it would transform garbage silently (the inverse's second_pass_only has the same guard)
    if (k.first_pass_done && !(LOGN == 16 && VARIANT == 10 && P1::LOGT == 6))
        throw std::logic_error("ntt_forward: first_pass_done needs the 64 x 1024 plan the fused conversion wrote");
    if (k.pro_small) {
        // encryption: the sample lift is the load of the strided pass, the canonical or a mul-add epilogue the store of the contiguous
        // one; both plain passes, on ONE plan per degree (ntt_transform resolves these launches to plan 3), so that the library holds
        // one pair of new kernels per degree
        if constexpr (VARIANT == 3) {
            launch_pass<P1, true, EPI_NONE, false, PRO_SMALL>(k1, s);
            if (epi == EPI_FWD_MULADD) return launch_pass<P2, true, EPI_FWD_MULADD, false>(k, s);
            if (epi == EPI_FWD_NEG_MULADD) return launch_pass<P2, true, EPI_FWD_NEG_MULADD, false>(k, s);
            return launch_pass<P2, true, EPI_FWD_CANON, false>(k, s);
        } else {
            throw std::logic_error("ntt_forward: the sample lift runs on plan 3");
        }
    }
#if defined(PHA_EXPERIMENTS)
    if constexpr (T::ONE_LAUNCH) {
        if (fused && epi != EPI_FWD_KSRESCALE && !k.first_pass_done && !lift_t(k) && !k.pro_ckks && !k.pro_small) {   // both passes in one launch
            bool done = false;
            dispatch_epi<true>(epi, [&](auto e) {
                if constexpr (e() != EPI_FWD_KSRESCALE) done = launch_fused<P1, P2, true, e(), false>(*fused, k1, k, s);
            });
            if (done) return;
        }
    }
#endif
    // (the strided pass in the batched form measured SLOWER -- 720 limbs 282 -> 302 us: its twiddles are few and shared by a tile's columns,
    //  and a 512-thread workgroup that walks several polynomials keeps its barrier schedule for all of them)
    auto strided = [&](const NttKArgs &ka, const PassOrder *order) {
        dispatch_pro(ka, [&](auto p) { launch_pass<P1, true, EPI_NONE, false, p()>(ka, s, order); });
    };
    if constexpr (T::ZLOOP) {
        using Z2 = typename T::Z2;
        ZloopMap m;
        if (!k.first_pass_only && plan_zloop<Z2>(k, m)) {
            if (k.first_pass_done) return launch_zloop_forward<Z2>(k, m, epi, s);
            return for_each_order_part(k, m, P1::LOGTILE, [&](uint32_t lo, uint32_t cnt, const ZloopMap &mh, const PassOrder *o) {
                strided(limb_range(k1, lo, cnt), o);
                launch_zloop_forward<Z2>(limb_range(k, lo, cnt), mh, epi, s);
            });
        }
    }
    if (!k.first_pass_done) strided(k1, nullptr);
    if (k.first_pass_only) return;
    dispatch_epi<true>(epi, [&](auto e) { launch_pass<P2, true, e(), false>(k, s); });
}

template <int LOGN, int VARIANT>
static void inverse_impl(const NttKArgs &k_in, int epi, hipStream_t s, Context *fused) {
    using T = TwoPass<LOGN, VARIANT>;
    using P1 = typename T::P1;
    using P2 = typename T::P2;
    T t(k_in);
    const NttKArgs &k1 = t.k1, &k = t.k2;
#if defined(PHA_EXPERIMENTS)
    if constexpr (T::ONE_LAUNCH) {
        if (fused && epi != EPI_INV_CANON_ADD) {
            bool done = false;
            dispatch_epi<false>(epi, [&](auto e) {
                if constexpr (e() != EPI_INV_CANON_ADD) done = launch_fused<P1, P2, false, e(), true>(*fused, k1, k, s);
            });
            if (done) return;
        }
    }
#endif
    if (k.second_pass_only) {   // mid already holds the contiguous pass's output (T1 x T2 of this plan: resolve_plan keeps the split of plan 3)
        // the producer (modup_ip_kernel) ran the contiguous pass of the fused mod-up's plan: this strided pass must complete THAT split
        using IpPlan = NttPlan<LOGN, (LOGN >= 14 && LOGN <= 16) ? kIpPlan : 3>;
        if (P1::LOGT + IpPlan::P2::LOGT != LOGN)
            throw std::logic_error("second_pass_only: the chosen plan's strided pass does not complete the fused mod-up's contiguous pass");
        return launch_inverse_last<P1>(k, epi, s);
    }
    if constexpr (T::ZLOOP) {   // batched launches: the contiguous pass with the twiddles resident (ntt_zloop_kernel)
        using Z2 = typename T::Z2;
        ZloopMap m;
        if (plan_zloop<Z2>(k1, m))
            return for_each_order_part(k, m, P1::LOGTILE, [&](uint32_t lo, uint32_t cnt, const ZloopMap &mh, const PassOrder *o) {
                launch_zloop<Z2, false, EPI_NONE, false>(limb_range(k1, lo, cnt), mh, s);
                launch_inverse_last<P1>(limb_range(k, lo, cnt), epi, s, o);
            });
    }
    launch_pass<P2, false, EPI_NONE, false>(k1, s);
    launch_inverse_last<P1>(k, epi, s);
}

static NttKArgs make_args(Context &c, const u64 *in, u64 *mid, u64 *out, const LimbSel &sel, const NttExtra &x,
                          bool fwd) {
    NttKArgs k{};
    k.in = in;
    k.mid = mid;
    k.out = out;
    k.tw = fwd ? c.d_tw.p : c.d_itw.p;
    k.mod = c.d_mod.p;
    k.ninv = c.d_ninv.p;
    k.w1ninv = c.d_w1ninv.p;
    const bool use_fp = !(ntt_variant() & 8);
    k.twf = fwd ? c.d_twf.p : c.d_itwf.p;
    k.ninvf = c.d_ninvf.p;
    k.w1ninvf = c.d_w1ninvf.p;
    k.fpinfo = use_fp ? c.d_fpinfo.p : nullptr;
    k.scale = x.scale;
    k.scale_shoup = x.scale_shoup;
    k.aux = x.aux;
    k.aux2 = x.aux2;
    k.scale2 = x.scale2;
    k.scale2_shoup = x.scale2_shoup;
    k.aux2_stride = x.aux2_stride ? x.aux2_stride : x.poly_stride;
    k.sel = sel;
    k.log_n = c.log_n;
    k.h_primes = c.primes.data();
    k.batch = x.batch ? x.batch : 1;
    k.poly_stride = x.poly_stride;
    k.in_stride = x.in_stride ? x.in_stride : x.poly_stride;
    k.first_pass_only = fwd && x.first_pass_only;
    k.second_pass_only = !fwd && x.second_pass_only;
    k.first_pass_done = fwd && x.first_pass_done;
    k.out_stride = x.out_stride ? x.out_stride : x.poly_stride;
    k.aux_stride = x.aux_stride ? x.aux_stride : x.poly_stride;
    k.excl_step = x.excl_step;
    k.excl_limit = x.excl_limit;
    k.excl_mod = x.excl_mod;
    k.pro_src = fwd ? x.pro_src : nullptr;
    k.pro_stride = x.pro_stride;
    k.pro_t = fwd && x.pro_src ? x.pro_lift_t : 0;
    k.pro_ckks = fwd && x.pro_src && x.pro_ckks;
    k.aux_pair_stride = x.aux_pair_stride;
    k.pro_small = fwd && x.pro_src && x.pro_small;
    if (k.pro_small) {   // encryption: the fields these launches share with others (see NttKArgs), and the strides as they are given
        k.pro_k = x.pro_small_k;
        k.aux3 = x.aux3;
        k.aux_stride = x.muladd_stride[0];
        k.aux2_stride = x.muladd_stride[1];
        k.aux3_stride = x.muladd_stride[2];
    }
    return k;
}

static void check_sel(Context &c, const LimbSel &sel) {
    if (sel.count == 0) return;
    const uint32_t last = sel.start + sel.count - 1;
    const uint32_t prime_last = last >= sel.remap_from ? last + sel.remap_add : last;
    if (prime_last >= c.rows) throw std::invalid_argument("modulus index out of range of the NTT tables");
}


}  // namespace pha
#include "pha_modup_ip.h"
namespace pha {

// the plan of a launch: resolve_plan (pha_ntt_core.h) on this context's degree and this library's tuning state
static ResolvedPlan choose_plan(Context &c, const LimbSel &sel, const NttExtra &x) {
    PlanShape p{};
    p.log_n = (int)c.log_n;
    p.limbs = sel.count;
    p.batch = x.batch;
    p.first_pass_only = x.first_pass_only;
    p.second_pass_only = x.second_pass_only;
    p.variant_bits = ntt_variant();
#if defined(PHA_EXPERIMENTS)
    p.experiments = true;
    p.whole14_min = (size_t)g_whole14_min.load(std::memory_order_relaxed);
    p.one_launch_min_tiles = (size_t)g_fused_min_tiles.load(std::memory_order_relaxed);
    p.xcd_round_robin = c.xcd_placement_round_robin();
#endif
    return resolve_plan(p);
}

// The one list of the plans each library instantiates: f(LOGN, VARIANT) as std::integral_constants, VARIANT = kWholePlan for the
// one-workgroup plan of that degree.  The product: the one-workgroup plans of N = 4096 / 8192, plan 3 from N = 8192, plans 4 from
// N = 2^14, 5 at 2^14 .. 2^16, 10 at 2^16; the experiments library: plans 0 .. 4 of every degree, 5 at 2^14 .. 2^16, 8 / 10 / 12 at
// 2^16, and the one-workgroup plan of N = 2^14 too.  (The extra instantiations alone cost ~30 us per key switch when they sat in the
// product code object: DESIGN.md section 7.)
constexpr int kWholePlan = -1;
template <int LOGN> struct WholePlanOf;
template <> struct WholePlanOf<12> { using type = WholePlan12; };
template <> struct WholePlanOf<13> { using type = WholePlan13; };
template <> struct WholePlanOf<14> { using type = WholePlan14; };
template <int V> using VarC = std::integral_constant<int, V>;
template <int LOGN, class F>
static bool dispatch_variant(const ResolvedPlan &r, F &&f) {
    const std::integral_constant<int, LOGN> logn{};
    if (r.whole) {
        if constexpr (LOGN == 12 || LOGN == 13 || (kExperiments && LOGN == 14)) {
            if (r.whole == LOGN) return f(logn, VarC<kWholePlan>{}), true;
        }
        return false;
    }
    switch (r.variant) {
        case 0: if constexpr (kExperiments && LOGN >= 12) return f(logn, VarC<0>{}), true; break;
        case 1: if constexpr (kExperiments && LOGN >= 12) return f(logn, VarC<1>{}), true; break;
        case 2: if constexpr (kExperiments && LOGN >= 12) return f(logn, VarC<2>{}), true; break;
        case 3: if constexpr (kExperiments || LOGN >= 13) return f(logn, VarC<3>{}), true; break;
        case 4: if constexpr (kExperiments || LOGN >= 14) return f(logn, VarC<4>{}), true; break;
        case 5: if constexpr (LOGN >= 14 && LOGN <= 16) return f(logn, VarC<5>{}), true; break;
        case 8: if constexpr (kExperiments && LOGN == 16) return f(logn, VarC<8>{}), true; break;
        case 10: if constexpr (LOGN == 16) return f(logn, VarC<10>{}), true; break;
        case 12: if constexpr (kExperiments && LOGN == 16) return f(logn, VarC<12>{}), true; break;
    }
    return false;
}
template <class F>
static void dispatch_plan(const ResolvedPlan &r, F &&f) {
    bool found = false;
    switch (r.log_n) {
        case 12: found = dispatch_variant<12>(r, f); break;
        case 13: found = dispatch_variant<13>(r, f); break;
        case 14: found = dispatch_variant<14>(r, f); break;
        case 15: found = dispatch_variant<15>(r, f); break;
        case 16: found = dispatch_variant<16>(r, f); break;
        case 17: found = dispatch_variant<17>(r, f); break;
        default: throw std::invalid_argument("unsupported polynomial degree");
    }
    if (!found) throw std::logic_error("ntt: this library does not build the plan the launch resolved to");
}

template <bool FWD>
static void ntt_transform(Context &c, const u64 *in, u64 *mid, u64 *out, const LimbSel &sel, int epi, const NttExtra &x, hipStream_t s) {
    if (sel.count == 0) return;
    check_sel(c, sel);
    NttKArgs k = make_args(c, in, mid, out, sel, x, FWD);
    if ((lift_t(k) || k.pro_ckks) && (epi != EPI_FWD_CANON || x.first_pass_done || (lift_t(k) && k.pro_ckks)))
        throw std::logic_error("ntt_forward: the plain lift and the CKKS round-and-reduce go with the plain forward transform only, one at a time");
    if (muladd_epilogue(epi) && !(FWD && k.pro_small)) throw std::logic_error("ntt_forward: the mul-add epilogues go with the sample lift");
    if (k.pro_small && (x.pro_lift_t || x.pro_ckks || x.scale2 || x.aux_pair_stride || x.first_pass_done || x.first_pass_only || (epi != EPI_FWD_CANON && !muladd_epilogue(epi))))
        throw std::logic_error("ntt_forward: the sample lift goes with the canonical and the mul-add epilogues of the plain forward transform, alone");
    if (muladd_epilogue(epi) && !(x.aux && x.aux2)) throw std::logic_error("ntt_forward: the mul-add epilogues need both factors");
    ResolvedPlan r = choose_plan(c, sel, x);
    if (k.pro_small && r.whole > 13) r.whole = 0;
    if (k.pro_small && !r.whole) {   // a prologue takes the plain passes (as plan_zloop declines pro_src), here on plan 3 at every size
        r.variant = 3;
        r.zfast = r.one_launch = false;
    }
    k.zfast_tiles = r.zfast ? 1u : 0u;   // request: launch_pass turns it into the tile count of the contiguous pass
    dispatch_plan(r, [&](auto logn, auto variant) {
        if constexpr (variant() == kWholePlan) launch_whole<typename WholePlanOf<logn()>::type, FWD>(k, epi, s);
        else if constexpr (FWD) forward_impl<logn(), variant()>(k, epi, s, r.one_launch ? &c : nullptr);
        else inverse_impl<logn(), variant()>(k, epi, s, r.one_launch ? &c : nullptr);
    });
}
void ntt_forward(Context &c, const u64 *in, u64 *mid, u64 *out, const LimbSel &sel, int epi, const NttExtra &x, hipStream_t s) {
    ntt_transform<true>(c, in, mid, out, sel, epi, x, s);
}
void ntt_inverse(Context &c, const u64 *in, u64 *mid, u64 *out, const LimbSel &sel, int epi, const NttExtra &x, hipStream_t s) {
    ntt_transform<false>(c, in, mid, out, sel, epi, x, s);
}

bool modup_ntt_inner_prod(Context &c, u64 *digits, const LimbSel &sel, const NttExtra &x, uint32_t beta, const ModupIpArgs &ip,
                          hipStream_t s) {
    if (c.log_n < 14 || c.log_n > 17 || beta < 1 || beta > 4 || sel.count == 0) return false;   // (N <= 8192 takes the one-launch plans)
    if (choose_plan(c, sel, x).whole) return false;
    check_sel(c, sel);
    NttExtra x1 = x;
    x1.first_pass_only = true;
    ntt_forward(c, digits, digits, digits, sel, EPI_FWD_CANON, x1, s);   // strided pass of every digit, in place
    const NttKArgs k = make_args(c, digits, digits, digits, sel, x, true);
    switch (c.log_n) {   // (the contiguous pass that carries the inner product is plan kIpPlan's at every launch size)
        case 14: launch_modup_ip<14>(k, beta, ip, s); break;
        case 15: launch_modup_ip<15>(k, beta, ip, s); break;
        case 16: launch_modup_ip<16>(k, beta, ip, s); break;
        default: launch_modup_ip<17>(k, beta, ip, s); break;
    }
    return true;
}

}  // namespace pha
#include "pha_modup_conv.h"

using namespace pha;

extern "C" {

int pha_nwt_2d_radix8_forward_inplace(pha_context_t ctx, uint64_t *inout, size_t cms, size_t start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout);
    ntt_forward(ctx->c, inout, inout, inout, plain_sel(start, cms), EPI_FWD_CANON, NttExtra{}, as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_forward_inplace_include_special_mod(pha_context_t ctx, uint64_t *inout, size_t cms,
                                                          size_t start, size_t size_QP, size_t size_P,
                                                          void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout);
    if (size_P > cms) throw std::invalid_argument("size_P exceeds coeff_modulus_size");
    ntt_forward(ctx->c, inout, inout, inout, special_sel(start, cms, size_QP, size_P), EPI_FWD_CANON, NttExtra{},
                as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_forward_inplace_include_special_mod_exclude_range(pha_context_t ctx, uint64_t *inout,
                                                                        size_t cms, size_t start, size_t size_QP,
                                                                        size_t size_P, size_t ex_start,
                                                                        size_t ex_end, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout);
    if (size_P > cms) throw std::invalid_argument("size_P exceeds coeff_modulus_size");
    LimbSel sel = special_sel(start, cms, size_QP, size_P);
    sel.excl_start = (uint32_t)ex_start;
    sel.excl_end = (uint32_t)ex_end;
    ntt_forward(ctx->c, inout, inout, inout, sel, EPI_FWD_CANON, NttExtra{}, as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_forward_inplace_fuse_moddown(pha_context_t ctx, uint64_t *ct, const uint64_t *cx,
                                                   const uint64_t *pinv, const uint64_t *pinv_shoup,
                                                   uint64_t *delta, size_t cms, size_t start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(cx); need(pinv); need(pinv_shoup); need(delta);
    NttExtra x;
    x.scale = pinv;
    x.scale_shoup = pinv_shoup;
    x.aux = cx;
    // pass 1 in place on delta; pass 2 reads delta, fuses (cx - NTT(delta)) * PInv and writes ct
    // (ntt_moddown.cu:106-261).  ct may alias cx: every thread reads cx[i] before it writes ct[i].
    ntt_forward(ctx->c, delta, delta, ct, plain_sel(start, cms), EPI_FWD_MODDOWN, x, as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_backward_inplace(pha_context_t ctx, uint64_t *inout, size_t cms, size_t start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout);
    ntt_inverse(ctx->c, inout, inout, inout, plain_sel(start, cms), EPI_INV_CANON, NttExtra{}, as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_backward(pha_context_t ctx, uint64_t *out, const uint64_t *in, size_t cms, size_t start,
                               void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(out); need(in);
    ntt_inverse(ctx->c, in, out, out, plain_sel(start, cms), EPI_INV_CANON, NttExtra{}, as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_backward_scale(pha_context_t ctx, uint64_t *out, const uint64_t *in, size_t cms,
                                     size_t start, const uint64_t *scale, const uint64_t *scale_shoup,
                                     void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(out); need(in); need(scale); need(scale_shoup);
    NttExtra x;
    x.scale = scale;
    x.scale_shoup = scale_shoup;
    ntt_inverse(ctx->c, in, out, out, plain_sel(start, cms), EPI_INV_SCALE, x, as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_backward_inplace_scale(pha_context_t ctx, uint64_t *inout, size_t cms, size_t start,
                                             const uint64_t *scale, const uint64_t *scale_shoup, void *stream) {
    return pha_nwt_2d_radix8_backward_scale(ctx, inout, inout, cms, start, scale, scale_shoup, stream);
}

int pha_nwt_2d_radix8_backward_inplace_include_special_mod(pha_context_t ctx, uint64_t *inout, size_t cms,
                                                           size_t start, size_t size_QP, size_t size_P,
                                                           void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout);
    if (size_P > cms) throw std::invalid_argument("size_P exceeds coeff_modulus_size");
    ntt_inverse(ctx->c, inout, inout, inout, special_sel(start, cms, size_QP, size_P), EPI_INV_CANON, NttExtra{},
                as_stream(stream));
    PHA_API_END
}

// BEHZ base Bsk = B u {m_sk} (src/evaluate.cu:434,528).  The reference keeps the tables of Bsk u {m_tilde} in their own
// DNTTTable and sends the last data limb (m_sk) to its last row (fntt_2d.cu:226, intt_2d.cu:334); here those primes
// are auxiliary rows of the context's one table set, so the selector is a plain offset.
static LimbSel temp_mod_sel(Context &c, size_t cms, size_t start, size_t total) {
    Behz &b = c.behz();
    if (start != 0 || cms != b.size_bsk || total != (size_t)b.size_bsk + 1)
        throw std::invalid_argument("include_temp_mod transforms a whole Bsk buffer: coeff_modulus_size = |Bsk|, total = |Bsk| + 1");
    LimbSel s = plain_sel(0, cms);
    s.remap_from = 0;
    s.remap_add = b.aux0;
    return s;
}

int pha_nwt_2d_radix8_forward_inplace_include_temp_mod(pha_context_t ctx, uint64_t *inout, size_t cms, size_t start,
                                                       size_t total_modulus_size, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout);
    ntt_forward(ctx->c, inout, inout, inout, temp_mod_sel(ctx->c, cms, start, total_modulus_size), EPI_FWD_CANON, NttExtra{},
                as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_backward_inplace_include_temp_mod_scale(pha_context_t ctx, uint64_t *inout, size_t cms,
                                                              size_t start, size_t total_modulus_size,
                                                              const uint64_t *scale, const uint64_t *scale_shoup,
                                                              void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout); need(scale); need(scale_shoup);
    NttExtra x;
    x.scale = scale;
    x.scale_shoup = scale_shoup;
    ntt_inverse(ctx->c, inout, inout, inout, temp_mod_sel(ctx->c, cms, start, total_modulus_size), EPI_INV_SCALE, x,
                as_stream(stream));
    PHA_API_END
}

// out[limb] = NTT modulo q_{modulus_index} of in[limb] for the limbs [start, start + cms): the reference lifts a
// plaintext (coefficients below t < q) into one RNS limb at a time this way (ntt_keyswitch_old.cu:225-265, callers
// evaluate.cu:1152,1210,1321).  Inputs are reduced modulo the prime as they are loaded (the reference leaves
// that reduction commented out, :47-49: same results for its inputs below q).
int pha_nwt_2d_radix8_forward_modup_fuse(pha_context_t ctx, uint64_t *out, const uint64_t *in, size_t modulus_index,
                                         size_t cms, size_t start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(out); need(in);
    Context &c = ctx->c;
    if (modulus_index >= c.size_qp) throw std::invalid_argument("modulus_index out of range");
    if (cms == 0) return 0;
    if (cms > 65535) throw std::invalid_argument("coeff_modulus_size out of range");
    // ONE launch pair for all limbs: limb start + z is "polynomial" z of a batch of one-limb polynomials that sit n
    // coefficients apart, all of them transformed with table row modulus_index
    LimbSel sel = plain_sel(start, 1);
    sel.remap_from = (uint32_t)start;
    sel.remap_add = (uint32_t)modulus_index - (uint32_t)start;
    NttExtra x;
    x.batch = (uint32_t)cms;
    x.poly_stride = c.n;
    x.pro_src = in + start * c.n;
    x.pro_stride = c.n;
    ntt_forward(c, out, out, out, sel, EPI_FWD_CANON, x, as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_forward_inplace_batched(pha_context_t ctx, uint64_t *inout, size_t cms, size_t start,
                                              size_t batch, size_t poly_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout);
    if (batch == 0 || batch > 65535) throw std::invalid_argument("batch out of range");
    NttExtra x;
    x.batch = (uint32_t)batch;
    x.poly_stride = poly_stride;
    ntt_forward(ctx->c, inout, inout, inout, plain_sel(start, cms), EPI_FWD_CANON, x, as_stream(stream));
    PHA_API_END
}

int pha_nwt_2d_radix8_backward_inplace_batched(pha_context_t ctx, uint64_t *inout, size_t cms, size_t start,
                                               size_t batch, size_t poly_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(inout);
    if (batch == 0 || batch > 65535) throw std::invalid_argument("batch out of range");
    NttExtra x;
    x.batch = (uint32_t)batch;
    x.poly_stride = poly_stride;
    ntt_inverse(ctx->c, inout, inout, inout, plain_sel(start, cms), EPI_INV_CANON, x, as_stream(stream));
    PHA_API_END
}

#if defined(PHA_EXPERIMENTS)
int pha_set_tuning(int key, int value) {
    PHA_API_BEGIN
    if (key == 0) {
        if (value < 0 || value > 32767 || (value & 6)) throw std::invalid_argument("unknown NTT variant");
        g_ntt_variant.store(value);
    } else if (key == 1) {
        g_bconv_split.store(value ? 1 : 0);
    } else if (key == 2) {
        if (value < 1) throw std::invalid_argument("threshold must be positive");
        g_whole14_min.store(value);
    } else if (key == 3) {
        if (value < 0 || value > 64) throw std::invalid_argument("lag out of range");
        g_fused_lag.store(value);
    } else if (key == 5) {
        g_fused_split.store(value ? 1 : 0);
    } else if (key == 4) {
        if (value < 1) throw std::invalid_argument("threshold must be positive");
        g_fused_min_tiles.store(value);
    } else {
        throw std::invalid_argument("unknown tuning key");
    }
    PHA_API_END
}
#endif  // PHA_EXPERIMENTS

}  // extern "C"
