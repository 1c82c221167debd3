// pha_modup_ip.h -- the key inner product as the epilogue of the mod-up's contiguous pass (r03).  A part of pha_ntt.hip's translation
// unit, included there behind NttKArgs, full_tile_args, limb_excluded and check_launch, which it uses; modup_ntt_inner_prod calls
// launch_modup_ip.
#pragma once

namespace pha {

// keyswitch_inplace runs, per digit b, the forward NTT of the converted limbs and then key_switch_inner_prod over all digits
// (src/rns_bconv.cu:530-627, src/eval_key_switch.cu:14-92): the transformed digits (beta x (l + alpha) limbs) are written and read
// back once, and the digit's own limbs are copied verbatim first.  Here ONE wavefront owns a 512-coefficient tile of limb j for
// ALL digits: it runs the contiguous pass on digit 0's tile, multiplies the outputs -- still in registers -- by the two key words,
// does the same for digit 1, ... and stores only the two sums.  A digit's own limb is not transformed at all: its NTT-form value
// is the input c2 itself, read where it lies (so the conversion need not copy it).  Per key switch at C3 that removes 67.5 MiB of
// transformed-digit stores, 90 MiB of digit loads, the 45 MiB own-limb copy and one launch.
// Accumulation: limbs on the FP64 back end add centred residues as doubles (fp_mulmod of the lazy transform output with the key
// word as a double: |sum| <= beta (q/2 + 1)); integer limbs add Barrett-reduced products modulo q.  Both equal
// (sum_b x_b k_b) mod q, the value the 128-bit accumulate + Barrett of inner_prod_kernel stores.
template <class C, int BETA, bool FP>
__device__ __forceinline__ void modup_ip_body(const NttKArgs &k, const ModupIpArgs &ip, uint32_t twr, uint32_t prime, uint32_t tile,
                                              u64 *lds, int tid) {
    constexpr int RL = C::NR - 1, r = C::r(RL), K = 1 << r, G = C::EPT >> r;
    static_assert(C::LOGT - C::s0(RL) - r == 0, "the last round holds runs of K consecutive coefficients");
    using Prog = PassProgram<C, true, EPI_NONE, false, 0, false>;
    const size_t n = (size_t)1 << k.log_n;
    const DModulus m = k.mod[prime];
    const u64 q = m.value;
    FpMod fm{};
    u64 accb[C::EPT], acca[C::EPT];      // FP: doubles (bit patterns); integer: residues
#pragma unroll
    for (int i = 0; i < C::EPT; i++) accb[i] = acca[i] = FP ? as_u64(0.0) : 0;
    size_t g0[G];                        // first coefficient of each run inside the limb
#pragma unroll
    for (int gi = 0; gi < G; gi++) {
        int v, hi, lo;
        decode_group<C, RL>(tid + C::THREADS * gi, v, hi, lo);
        g0[gi] = ((size_t)tile * C::V + v) * C::T + ((size_t)hi << r);
    }
    // (r03 A/B: the unrolled digit loop overlaps consecutive digits, needs 210 VGPRs = two wavefronts per SIMD, and is 3 % slower per
    //  key switch than the rolled one at 164 VGPRs = three)
#pragma unroll 1
    for (int b = 0; b < BETA; b++) {
        PassArgs a;
        full_tile_args<C, true, EPI_NONE, false>(k, twr, (uint32_t)b, tile, a);
        a.fp = FP;
        fm = a.fpm;
        u64 reg[C::EPT];
        if (ip.own && limb_excluded(k, twr, (uint32_t)b)) {   // (uniform) digit b's own limb: the NTT-form input itself
#pragma unroll
            for (int gi = 0; gi < G; gi++)
#pragma unroll
                for (int kk = 0; kk < K; kk += 2) {
                    const u64x2 w = *reinterpret_cast<const u64x2 *>(ip.own + (size_t)twr * n + g0[gi] + kk);
                    reg[gi * K + kk] = FP ? as_u64(fp_from_canon(w.x)) : w.x;
                    reg[gi * K + kk + 1] = FP ? as_u64(fp_from_canon(w.y)) : w.y;
                }
        } else {
            u64x2 twreg[C::TW_TOTAL];
            Prog::load_twiddles(a, tid, twreg);
            Prog::template run_pass<SEG_KEEP, true>(a, lds, tid, reg, twreg);   // (tail hand-over: the next digit reuses the LDS words)
            if (!FP) {
#pragma unroll
                for (int i = 0; i < C::EPT; i++) reg[i] = csub(csub(csub(reg[i], q << 2), q << 1), q);
            }
        }
        const u64 *key = ip.evks[b];
#pragma unroll
        for (int gi = 0; gi < G; gi++)
#pragma unroll
            for (int kk = 0; kk < K; kk += 2) {
                const size_t id = (size_t)prime * n + g0[gi] + kk;
                const u64x2 kb = *reinterpret_cast<const u64x2 *>(key + id);
                const u64x2 ka = *reinterpret_cast<const u64x2 *>(key + id + ip.qp_n);
                const int i0 = gi * K + kk;
                if (FP) {
                    // r04: the lazy outputs of the last round are below M q (M from the pass's compile-time schedule; 2.13 for the
                    // 8-8-4 rounds), so a LIGHT product is below q (0.5 + 0.375 M) and BETA of them stay exact integers below 8 q:
                    // 6 instead of 9 operations per product where that holds (every plan at beta <= 3, all but N = 2^14 at beta = 4)
                    constexpr double mlast = Prog::fp_sched().after[C::NR - 1];
                    constexpr bool light = (0.5 + 0.375 * (mlast > 1.0 ? mlast : 1.0)) * BETA < 7.5;
                    const double x0 = as_f64(reg[i0]), x1 = as_f64(reg[i0 + 1]);
                    auto prod = [&](double x, u64 kw) __attribute__((always_inline)) {
                        return light ? fp_mulmod_light(x, fp_from_canon(kw), fm) : fp_mulmod(x, fp_from_canon(kw), fm);
                    };
                    accb[i0] = as_u64(as_f64(accb[i0]) + prod(x0, kb.x));
                    accb[i0 + 1] = as_u64(as_f64(accb[i0 + 1]) + prod(x1, kb.y));
                    acca[i0] = as_u64(as_f64(acca[i0]) + prod(x0, ka.x));
                    acca[i0 + 1] = as_u64(as_f64(acca[i0 + 1]) + prod(x1, ka.y));
                } else {
                    // (128-bit accumulators with one Barrett at the end, as inner_prod_kernel has them, cost 32 more VGPRs across the
                    //  transforms: 256+ registers, one wavefront per SIMD; measured r03)
                    accb[i0] = add_mod(accb[i0], mul_mod(reg[i0], kb.x, m), q);
                    accb[i0 + 1] = add_mod(accb[i0 + 1], mul_mod(reg[i0 + 1], kb.y, m), q);
                    acca[i0] = add_mod(acca[i0], mul_mod(reg[i0], ka.x, m), q);
                    acca[i0 + 1] = add_mod(acca[i0 + 1], mul_mod(reg[i0 + 1], ka.y, m), q);
                }
            }
    }
    const bool fix = twr == ip.fix_limb;   // (uniform) pha_keyswitch_rescale: ct_last + cx_last * P^-1
    // (uniform) this limb goes back to coefficient form next: run the inverse transform's contiguous pass here (ModupIpArgs::inv_from)
    const bool inv = ip.inv_from != 0xffffffffu && (twr >= ip.inv_from || twr == ip.inv_lead);
#pragma unroll
    for (int gi = 0; gi < G; gi++)
#pragma unroll
        for (int kk = 0; kk < K; kk += 2) {
            const int i0 = gi * K + kk;
            u64x2 rb, ra;
            if (FP) {
                rb = u64x2{fp_to_canon(as_f64(accb[i0]), fm), fp_to_canon(as_f64(accb[i0 + 1]), fm)};
                ra = u64x2{fp_to_canon(as_f64(acca[i0]), fm), fp_to_canon(as_f64(acca[i0 + 1]), fm)};
            } else {
                rb = u64x2{accb[i0], accb[i0 + 1]};
                ra = u64x2{acca[i0], acca[i0 + 1]};
            }
            const size_t id = (size_t)twr * n + g0[gi] + kk;
            if (fix) {
                const u64x2 c0 = *reinterpret_cast<const u64x2 *>(ip.fix_ct + id);
                const u64x2 c1 = *reinterpret_cast<const u64x2 *>(ip.fix_ct + ip.fix_ct_stride + id);
                rb.x = add_mod(c0.x, shoup(rb.x, ip.fix_cst, q), q);
                rb.y = add_mod(c0.y, shoup(rb.y, ip.fix_cst, q), q);
                ra.x = add_mod(c1.x, shoup(ra.x, ip.fix_cst, q), q);
                ra.y = add_mod(c1.y, shoup(ra.y, ip.fix_cst, q), q);
            }
            if (inv) {   // canonical residues, in the layout the inverse pass's first round loads
                accb[i0] = rb.x; accb[i0 + 1] = rb.y;
                acca[i0] = ra.x; acca[i0 + 1] = ra.y;
            } else {
                *reinterpret_cast<u64x2 *>(ip.cx + id) = rb;
                *reinterpret_cast<u64x2 *>(ip.cx + ip.qlp_n + id) = ra;
            }
        }
    if (!inv) return;
    // nwt_2d_radix8_backward's first pass (intt_2d.cu:9-104) on the rows this wavefront owns, from registers: the pass stores what the
    // stand-alone launch would (lazy integers / centred doubles) and the caller launches the strided pass alone
    using InvProg = PassProgram<C, false, EPI_NONE, false, 0, false>;
    NttKArgs ki = k;
    ki.tw = ip.itw;
    ki.twf = ip.itwf;
    ki.in = ki.out = ip.cx;
    ki.batch = 2;
    ki.in_stride = ki.out_stride = ip.qlp_n;
    ki.pro_src = nullptr;
    auto inverse_rows = [&](u64 *r, uint32_t z) __attribute__((always_inline)) {
        PassArgs ai;
        full_tile_args<C, false, EPI_NONE, false>(ki, twr, z, tile, ai);
        ai.fp = FP;
        u64x2 twreg[C::TW_TOTAL];
        InvProg::template run_pass<SEG_PREFETCHED, true>(ai, lds, tid, r, twreg);   // (tail hand-over: the second sum reuses the LDS words)
    };
    inverse_rows(accb, 0);
    inverse_rows(acca, 1);
}

// Limb order: blockIdx.y walks the special (P) limbs first -- 60-bit primes on the integer back end, the longest wavefronts of
// the launch -- then the data limbs, so that the long poles start at once and the FP64 limbs fill in behind them.
template <class C, int BETA>
__global__ __launch_bounds__(C::THREADS) void modup_ip_kernel(const NttKArgs k, const ModupIpArgs ip) {
    static_assert(C::WAVE_LOCAL && !C::STRIDED && !C::WHOLE, "the fused inner product rides on the one-wavefront contiguous pass");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *lds = reinterpret_cast<u64 *>(smem);
    const uint32_t tile = blockIdx.x;
    const uint32_t n_special = k.sel.remap_from <= k.sel.start + k.sel.count ? k.sel.start + k.sel.count - k.sel.remap_from : 0;
    const uint32_t y = blockIdx.y < n_special ? k.sel.count - n_special + blockIdx.y : blockIdx.y - n_special;
    const uint32_t twr = k.sel.start + y;
    const uint32_t prime = twr >= k.sel.remap_from ? twr + k.sel.remap_add : twr;
    const bool fp = k.fpinfo && k.fpinfo[prime].ok;   // uniform
    if (fp) modup_ip_body<C, BETA, true>(k, ip, twr, prime, tile, lds, threadIdx.x);
    else modup_ip_body<C, BETA, false>(k, ip, twr, prime, tile, lds, threadIdx.x);
}

template <int LOGN>
static void launch_modup_ip(NttKArgs k, uint32_t beta, const ModupIpArgs &ip, hipStream_t s) {
    constexpr int V = (LOGN >= 14 && LOGN <= 16) ? kIpPlan : 3;
    using P1 = typename NttPlan<LOGN, V>::P1;
    using P2 = typename NttPlan<LOGN, V>::P2;
    k.t1 = P1::T;
    k.t2 = P2::T;
    k.in = k.mid;                 // the contiguous pass reads what the strided pass left in the digits
    k.in_stride = k.poly_stride;
    k.pro_src = nullptr;
    k.zfast_tiles = 0;
    const dim3 grid((unsigned)(((size_t)1 << LOGN) >> P2::LOGTILE), k.sel.count, 1), block(P2::THREADS);
    const size_t lds_bytes = (size_t)P2::LDS_WORDS * sizeof(u64);
    switch (beta) {
        case 1: hipLaunchKernelGGL((modup_ip_kernel<P2, 1>), grid, block, lds_bytes, s, k, ip); break;
        case 2: hipLaunchKernelGGL((modup_ip_kernel<P2, 2>), grid, block, lds_bytes, s, k, ip); break;
        case 3: hipLaunchKernelGGL((modup_ip_kernel<P2, 3>), grid, block, lds_bytes, s, k, ip); break;
        default: hipLaunchKernelGGL((modup_ip_kernel<P2, 4>), grid, block, lds_bytes, s, k, ip); break;
    }
    check_launch();
}

}  // namespace pha
