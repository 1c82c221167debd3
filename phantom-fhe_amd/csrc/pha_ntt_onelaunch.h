// pha_ntt_onelaunch.h -- TEST-ONLY (-DPHA_EXPERIMENTS): both passes of a transform in one launch.  A part of pha_ntt.hip's translation
// unit, included there behind NttKArgs, exec_pass and full_tile_args, which it uses; forward_impl / inverse_impl call launch_fused.
#pragma once

namespace pha {

// ---- both passes in ONE launch, the intermediate handed over through the XCD's own L2 -------------------------------
// (r02; profiles/HISTORY.md has the memory-side experiment behind it: the two access patterns at 720 limbs take
// 286 us as two launches and 211 us in this form, because the intermediate never crosses the fabric a second time.)
// Placement: the workgroups of a 1-D grid are dealt to the 8 XCDs round-robin, so all workgroups with the same
// b % 8 (a "class") share one XCD -- XCD (b + r) % 8 with r = 0 for plain launches and some other constant under
// hipGraph replay.  Only the sharing matters here and it is checked in every launch: the first workgroup of a class
// records its XCC_ID, every other one compares and traps on a difference (the context also runs a census launch and
// keeps the two-launch form if the rule does not hold on the device).  A "unit" is one limb of one polynomial;
// unit u belongs to class u % 8, whose workgroups visit its units in order: workgroup (slot s, tile t) of a class first
// runs the transform's first pass on tile t of the unit of slot s, then the second pass on tile t of the unit of slot
// s - lag, whose tiles were all started lag * tiles_per_unit workgroups earlier in this class and have normally been
// written by then.  Hand-off protocol (every participant of a unit is on one XCD, whose L2 is the only cache level they
// share):
//   producer: plain stores (written through, the line stays in this XCD's L2), s_waitcnt vmcnt(0), workgroup barrier,
//             one non-returning atomic add on the unit's counter (executes in this L2);
//   consumer: one lane polls the counter with a returning atomic OR 0 (never answered by the CU's L1) until all tiles
//             have arrived, workgroup barrier, then reads the intermediate with agent-scope loads (`sc1`: miss the L1,
//             answered by the L2) -- PassProgram's COH flag.
// The counter array cleans itself: every consumer counts itself in right after its poll has succeeded, and the one that
// finds all the others counted puts the unit's two words back to zero (nobody polls them any more); that workgroup also
// counts the finished unit at agent scope, and the one that finishes the launch's last unit clears the 8 class words
// (every workgroup that has work looked at its class word before its own unit could finish).  So a launch never
// allocates or clears anything from the host, which keeps it capturable.
// Dispatch order is ascending block index, so a waiting workgroup only ever waits for workgroups that are already
// resident or finished (the same assumption every decoupled look-back scan makes); the poll is bounded and traps.
constexpr int kFusedMinWaves = 6;   // three 512-thread workgroups per CU
struct FusedArgs {
    uint32_t *cls;         // [8] XCC_ID + 1 of each workgroup class (0 = not recorded yet); [8] = units finished
    uint32_t *flags;       // [units][2]: tiles of the unit's first pass that have been written, consumers that have seen that
    uint32_t units, slots, tpl, lag, count;   // count = limbs per polynomial (unit = z * count + y)
    uint32_t active_units; // units that are not excluded
    uint32_t split;        // 1: a workgroup runs ONE pass (even positions of a class: first pass, odd: second pass of the lagged unit)
};
__device__ __forceinline__ void l2_arrive(uint32_t *p) {
    asm volatile("global_atomic_add %0, %1, off" ::"v"(p), "v"(1u) : "memory");
}
__device__ __forceinline__ uint32_t l2_fetch_or(uint32_t *p, uint32_t v) {
    uint32_t r;
    asm volatile("global_atomic_or %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(p), "v"(v) : "memory");
    return r;
}
__device__ __forceinline__ uint32_t l2_fetch_add(uint32_t *p, uint32_t v) {
    uint32_t r;
    asm volatile("global_atomic_add %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(p), "v"(v) : "memory");
    return r;
}
__device__ __forceinline__ void l2_store(uint32_t *p, uint32_t v) {
    asm volatile("global_atomic_swap %0, %1, off" ::"v"(p), "v"(v) : "memory");
}

// run configuration C on 4096-coefficient tile `tile` with the 512 threads of the workgroup: a 512-thread configuration
// directly, a one-wavefront configuration (512-coefficient tiles) as eight independent wavefronts
template <class C, bool FWD, int EPI, bool FOLD, bool COH>
__device__ __forceinline__ void fused_run_tile(const NttKArgs &k, uint32_t twr, uint32_t z, uint32_t tile, u64 *lds) {
    static_assert(C::THREADS == 512 || C::THREADS == 64, "the one-launch transform runs 512-thread workgroups");
    PassArgs a;
    if constexpr (C::THREADS == 512) {
        full_tile_args<C, FWD, EPI, FOLD>(k, twr, z, tile, a);
        exec_pass<C, FWD, EPI, FOLD, 0, COH>(a, lds, threadIdx.x);
    } else {
        const uint32_t wave = threadIdx.x >> 6;
        full_tile_args<C, FWD, EPI, FOLD>(k, twr, z, tile * 8 + wave, a);
        exec_pass<C, FWD, EPI, FOLD, 0, COH>(a, lds + (size_t)wave * C::LDS_WORDS, threadIdx.x & 63);
    }
}

template <class PS, class PC, bool FWD, int EPI, bool FOLD>   // PS: strided pass (512 threads), PC: contiguous pass
__global__ __launch_bounds__(512, kFusedMinWaves) void ntt_fused_kernel(const NttKArgs kA, const NttKArgs kB, const FusedArgs f) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *lds = reinterpret_cast<u64 *>(smem);
    const uint32_t b = blockIdx.x, xcd = b & 7u, within = b >> 3;
    // split form: the positions of a class alternate between first-pass and second-pass workgroups, so that a workgroup
    // lives for one pass only and the second pass's wavefronts are not tied to a first pass's barrier schedule
    const uint32_t role = f.split ? (within & 1u) : 2u, idx = f.split ? (within >> 1) : within;
    const uint32_t tile = idx % f.tpl, slot = idx / f.tpl;
    const uint32_t uA = slot * 8 + xcd;
    const bool has_a = role != 1u && slot < f.slots && uA < f.units && !limb_excluded(kA, kA.sel.start + uA % f.count, uA / f.count);
    const uint32_t uB = (slot - f.lag) * 8 + xcd;   // (wraps when slot < lag: has_b is false then)
    const bool has_b = role != 0u && slot >= f.lag && uB < f.units && !limb_excluded(kB, kB.sel.start + uB % f.count, uB / f.count);
    if (!has_a && !has_b) return;   // (and never touches the class words: see the clean-up rule above)
    uint32_t cls_seen = 0, cls_mine = 0;
    if (threadIdx.x == 0) {   // class check, part 1 (the answer is looked at after the first pass)
        uint32_t id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
        cls_mine = (id & 7u) + 1;
        uint32_t expected = 0;
        __hip_atomic_compare_exchange_strong(f.cls + xcd, &expected, cls_mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cls_seen = expected;
    }
    if (has_a) {
        const uint32_t z = uA / f.count, twr = kA.sel.start + uA % f.count;
        if (FWD) fused_run_tile<PS, true, EPI_NONE, false, false>(kA, twr, z, tile, lds);
        else fused_run_tile<PC, false, EPI_NONE, false, false>(kA, twr, z, tile, lds);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this workgroup's stores have reached the L2
        __syncthreads();
        if (threadIdx.x == 0) l2_arrive(f.flags + 2 * (size_t)uA);
    }
    if (threadIdx.x == 0 && cls_seen != 0 && cls_seen != cls_mine) {   // class check, part 2
        __builtin_trap();   // two workgroups of one class on different XCDs: the hand-off below would not be coherent
    }
    if (!has_b) return;
    const uint32_t z = uB / f.count, twr = kB.sel.start + uB % f.count;
    uint32_t *flag = f.flags + 2 * (size_t)uB;
    // wait until every tile of the unit's first pass has been written.  One lane polls for the workgroup -- or, when the
    // second pass is the barrier-free contiguous one, one lane per wavefront, so that no wavefront waits for another's poll
    constexpr bool kWaveConsumer = FWD && PC::THREADS == 64;
    const bool poller = kWaveConsumer && f.split ? (threadIdx.x & 63) == 0 : threadIdx.x == 0;
    if (poller) {
        uint32_t spins = 0;
        while (l2_fetch_or(flag, 0u) < f.tpl) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > (1u << 24)) __builtin_trap();   // never hang the device on a broken assumption
        }
    }
    if (!(kWaveConsumer && f.split)) __syncthreads();   // also: pass A no longer uses the LDS
    if (FWD) fused_run_tile<PC, true, EPI, false, true>(kB, twr, z, tile, lds);
    else fused_run_tile<PS, false, EPI, FOLD, true>(kB, twr, z, tile, lds);
    // every wavefront of this workgroup has seen the unit complete: count the workgroup in; the last one of the unit puts
    // the unit's words back to zero (nobody polls them any more)
    __syncthreads();
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(flag + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == f.tpl - 1) {
        l2_store(flag, 0u);
        l2_store(flag + 1, 0u);
        if (__hip_atomic_fetch_add(f.cls + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == f.active_units - 1) {
            for (int i = 0; i < 9; i++) __hip_atomic_store(f.cls + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <class PS, class PC, bool FWD, int EPI, bool FOLD>
static bool launch_fused(Context &c, const NttKArgs &kA_in, const NttKArgs &kB_in, hipStream_t s) {
    static_assert(PS::THREADS == 512 && PS::LOGTILE == 12, "strided pass: one 4096-coefficient tile per 512-thread workgroup");
    NttKArgs kA = kA_in, kB = kB_in;
    const size_t n = (size_t)1 << kA.log_n;
    kA.zfast_tiles = kB.zfast_tiles = 0;   // (the request flag of the two-launch form means nothing here)
    FusedArgs f{};
    f.count = kA.sel.count;
    f.units = kA.sel.count * kA.batch;
    f.slots = (f.units + 7) / 8;
    f.tpl = (uint32_t)(n >> 12);
    f.lag = (uint32_t)g_fused_lag.load(std::memory_order_relaxed);
    f.cls = c.ntt_flags(s, f.units);
    if (!f.cls) return false;   // no counter arena for this stream: the caller takes the two launches
    f.flags = f.cls + 16;
    f.active_units = 0;
    for (uint32_t z = 0; z < kA.batch; z++)   // the limbs of the selection that polynomial z transforms
        for (uint32_t y = 0; y < kA.sel.count; y++) f.active_units += limb_excluded(kA, kA.sel.start + y, z) ? 0u : 1u;
    if (f.active_units == 0) return true;
    const size_t lds_a = (size_t)PS::LDS_WORDS * sizeof(u64);
    const size_t lds_b = (size_t)PC::LDS_WORDS * sizeof(u64) * (PC::THREADS == 64 ? 8 : 1);
    const size_t lds_bytes = lds_a > lds_b ? lds_a : lds_b;
    f.split = g_fused_split.load(std::memory_order_relaxed) ? 1u : 0u;
    const unsigned blocks = (f.slots + f.lag) * f.tpl * 8 * (f.split ? 2u : 1u);
    hipLaunchKernelGGL((ntt_fused_kernel<PS, PC, FWD, EPI, FOLD>), dim3(blocks), dim3(512), lds_bytes, s, kA, kB, f);
    check_launch();
    return true;
}

}  // namespace pha
