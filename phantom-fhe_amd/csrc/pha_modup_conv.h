// pha_modup_conv.h -- the mod-up's base conversion fused with the strided pass of the forward transform (r05).  A part
// of pha_ntt.hip's translation unit, included there behind NttKArgs, make_args, choose_plan and raise_lds_limit, which it uses.
#pragma once

namespace pha {

// bconv_kernel (pha_rns.hip) writes beta x (l + alpha - alpha_b) converted limbs in coefficient form and the strided pass of the
// forward transform reads them back: 67.5 + 67.5 MiB per key switch at C3, plus a launch.  Here the conversion is the LOAD of that
// pass: a workgroup owns a strided-pass tile (T1 rows x V adjacent columns) of ONE digit polynomial, each thread reads the digit's
// <= 16 scaled input residues of ITS coefficients once (the first round's register layout: EPT coefficients per thread, so the
// inputs are EPT x isz words = 30 registers per coefficient as 30-bit halves -- hence four coefficients per thread and radix-4
// rounds, where the stand-alone pass has eight and radix-8), and then walks the digit's output limbs: convert (the carry-free
// 30 / 30 MAC against the LDS-staged Montgomery rows, REDC: the arithmetic of bconv_kernel, the same canonical residues), run
// the pass from registers (PassProgram::run_prefetched), store the pass's output where the contiguous pass expects it.
// Per output limb everything uniform (modulus, REDC constant, destination limb, table row, FP64 constants) comes from an LDS record
// staged once per workgroup, so the loop has no dependent scalar-memory round trip.
// LOGTILE 8: one wavefront per workgroup (64 rows x 4 columns: 32-byte runs, no workgroup barrier); 10: 64 x 16 (128-byte runs,
// 256 threads); 11: 64 x 32.
struct ConvLimbRec {      // 56 bytes; one per output limb of the digit
    u64 p, oninv;
    double fq, fqinv;
    uint32_t jo, prime, fpok, pad;
    u64 ratio1;           // floor(2^64 / p): the rescale form reduces c_last modulo this limb's prime (barrett64)
};
constexpr int kMcsMaxOut = 64;
__device__ __forceinline__ uint32_t uni32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ u64 uni64(u64 x) { return ((u64)uni32((uint32_t)(x >> 32)) << 32) | uni32((uint32_t)x); }

// The geometry below is the one kept out of the 12 that r05 measured (profiles/r05_experiments.md §2: batched HomMul + relinearize +
// rescale, us per op at B = 8 / 32; separate kernels 279.5 / 275.0): every round's twiddles requested before the conversion, all four
// coefficients converted side by side (a matrix row is read from LDS once), 8 of the 15 input limbs in registers (226 registers, two
// 256-thread workgroups per CU with 76 KB of LDS each): 275.1 / 275.2.  The losers (10 limbs in registers 290 / 286; 7: 322;
// per-round twiddles 284; 64 x 4 tiles 365; 64 x 8 295; 64 x 32 292; one wavefront per SIMD 339; staggered workgroups, raised
// priority for the rounds: no gain) are in that log, not in this source.
constexpr int kMcsWaves = 2;      // wavefronts per SIMD the register allocation aims at (the inputs alone are 120 registers)
constexpr int kMcsRegLimbs = 8;   // input limbs held in registers; the rest of the digit's inputs in LDS
constexpr int kRescRegLimbs = 15;   // r06: the rescale form has no copy loop and fewer live pointers (174 registers with 8 limbs in registers): all 15 inputs fit, no LDS input reads (B = 8: 256.6 -> 251.6 us per op, B = 32: 254.0 -> 252.0)
constexpr int kDownRegLimbs = 8;    // the plain mod-down form spills at 12 (76 bytes of scratch) and 15 (260 bytes: 280 instead of 230 us per key switch)
constexpr int mcs_reg_limbs(int form) { return form == 1 ? kRescRegLimbs : form == 2 ? kDownRegLimbs : kMcsRegLimbs; }
constexpr int kMcsLogTile = 10;   // 64 rows x 16 columns: 128-byte runs, 256 threads
// RESC (r06): the same kernel as the load of the forward transform that ends key switch + rescale (pha_keyswitch_rescale_batched): the
// conversion is bconv_rescale_kernel's (pha_rns.hip) -- inputs = the P limbs of cx in coefficient form (x phat_i^-1), ONE converter
// (P -> Ql with P^-1 in its rows) whose LAST row belongs to the last data limb: c_last = t_last - convert(last row) mod q_last once per
// coefficient, then v_j = convert(row j) + (c_last mod q_j) for j < Ql - 1 goes straight into the strided pass's registers.  The
// 2 x (Ql - 1) limbs of v are then never written and read back in coefficient form (92 MB per ciphertext at C3) and one launch goes.
// FORM 2 (r06): the plain mod-down form -- the same without the last-limb fold: every row of the P -> Ql converter is an output limb (the CKKS
// mod-down of a batched key switch WITHOUT rescale; the transform's contiguous pass then carries the (cx - NTT delta) P^-1 epilogue)
template <class C, int ISZ_PAD, int FORM = 0>
__global__ __launch_bounds__(C::THREADS) __attribute__((amdgpu_waves_per_eu(kMcsWaves, kMcsWaves)))
void modup_conv_s1_kernel(const NttKArgs k, const ModupConvArgs m) {
    constexpr bool RESC = FORM == 1;
    static_assert(C::STRIDED && C::EPT == 4 && C::NR == 3 && C::r(0) == 2, "radix-4 strided pass, four coefficients per thread");
    constexpr int K = 4, LOGD = C::LOGT - 2;
    using Prog = PassProgram<C, true, EPI_NONE, false, 1, false>;   // HOIST 1: a limb's twiddles are requested before its conversion
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *lds = reinterpret_cast<u64 *>(smem);                                                  // the pass's tile
    uint2 *s_rows = reinterpret_cast<uint2 *>(smem + (size_t)C::LDS_WORDS * sizeof(u64));      // [max_osz][kBcRowPad]
    ConvLimbRec *s_rec = reinterpret_cast<ConvLimbRec *>(s_rows + m.max_osz * kBcRowPad);      // [max_osz]
    const int tid = threadIdx.x;
    const uint32_t z = blockIdx.z, tile = blockIdx.x;
    const uint32_t ci = z % m.beta, grp = z / m.beta;
    const BConvDev &d = m.convs[ci];
    const uint32_t n = 1u << k.log_n, isz = d.isz, osz = d.osz, pitch = d.row_pad;
    const bool r90 = uni32(d.r90) != 0;
    for (uint32_t e = tid; e < osz * kBcRowPad; e += C::THREADS) {
        const uint32_t j = e / kBcRowPad, i = e % kBcRowPad;
        s_rows[e] = i < pitch ? reinterpret_cast<const uint2 *>(d.mat30)[j * pitch + i] : uint2{0u, 0u};
    }
    for (uint32_t j = tid; j < osz; j += C::THREADS) {
        ConvLimbRec r;
        r.jo = j + (j >= d.pad_start ? d.pad_len : 0);                                   // limb of the [Ql | P] digit buffer
        r.prime = r.jo >= k.sel.remap_from ? r.jo + k.sel.remap_add : r.jo;              // its row of the QP tables (= d.oprime[j])
        r.p = k.mod[r.prime].value;
        r.oninv = d.oninv[j];
        r.fpok = 0; r.fq = 0.0; r.fqinv = 0.0; r.pad = 0;
        r.ratio1 = k.mod[r.prime].ratio1;
        if (k.fpinfo) {
            const FpInfo fi = k.fpinfo[r.prime];
            r.fpok = fi.ok; r.fq = fi.q; r.fqinv = fi.qinv;
        }
        s_rec[j] = r;
    }
    // this thread's coefficients: the first round's layout (round_load<C, 0>): rows lo + (kk << LOGD) of column tile * V + v
    int v, hi, lo;
    decode_group<C, 0>(tid, v, hi, lo);
    uint32_t off[K];
#pragma unroll
    for (int kk = 0; kk < K; kk++) off[kk] = (uint32_t)(lo + (kk << LOGD)) * k.t2 + tile * C::V + (uint32_t)v;
    const u64 *src = m.src + (size_t)grp * m.src_group_stride + (size_t)d.src_limb * n;
    u64 *dig = k.out + (size_t)z * k.poly_stride;
    // the first RL input limbs live in registers (8 per limb: four coefficients x two 30-bit halves), the others in LDS, [limb][kk][thread]
    // as (lo, hi) pairs: conflict-free 8-byte reads.  All in registers is 120 + the pass's ~130: spills at two wavefronts per SIMD.
    constexpr int RL = mcs_reg_limbs(FORM) < ISZ_PAD ? mcs_reg_limbs(FORM) : ISZ_PAD;
    uint2 *s_in = reinterpret_cast<uint2 *>(s_rec + m.max_osz);                                // [ISZ_PAD - RL][K][THREADS]
    u32 ylo[RL][K], yhi[RL][K];
#pragma unroll
    for (int i = 0; i < ISZ_PAD; i++)
#pragma unroll
        for (int kk = 0; kk < K; kk++) {
            const u64 y = i < (int)isz ? src[(size_t)i * n + off[kk]] : 0;
            if (i < RL) {
                ylo[i][kk] = (u32)y & 0x3fffffffu;
                yhi[i][kk] = (u32)(y >> 30);
            } else {
                s_in[((i - RL) * K + kk) * C::THREADS + tid] = uint2{(u32)y & 0x3fffffffu, (u32)(y >> 30)};
            }
        }
    if (d.copy_own && m.own) {   // modup_copy_partQl_kernel rns_bconv.cu:522-528
        const u64 *own = m.own + (size_t)grp * m.own_group_stride + (size_t)d.src_limb * n;
        for (uint32_t i = 0; i < isz; i++)
#pragma unroll
            for (int kk = 0; kk < K; kk++) dig[(size_t)(d.src_limb + i) * n + off[kk]] = own[(size_t)i * n + off[kk]];
    }
    __syncthreads();
    // out[kk] = REDC(sum_i y_i[kk] * row_e[i]) for the thread's four coefficients: sum_i y_i qhat_i mod p, canonical (the arithmetic of
    // bconv_kernel, SPLIT 30 / 30, Montgomery rows; all four coefficients side by side, so a matrix row is read from LDS once)
    auto convert4 = [&](uint32_t e, u64 p, u64 oninv, u64 *out) __attribute__((always_inline)) {
        const uint2 *row = s_rows + e * kBcRowPad;
        u64 ll[K], lh[K], hl[K], hh[K];
#pragma unroll
        for (int kk = 0; kk < K; kk++) ll[kk] = lh[kk] = hl[kk] = hh[kk] = 0;
#pragma unroll
        for (int i = 0; i < ISZ_PAD; i++) {
            const uint2 mm = row[i];
#pragma unroll
            for (int kk = 0; kk < K; kk++) {
                u32 y0, y1;
                if (i < RL) {
                    y0 = ylo[i < RL ? i : 0][kk];
                    y1 = yhi[i < RL ? i : 0][kk];
                } else {
                    const uint2 yy = s_in[((i - RL) * K + kk) * C::THREADS + threadIdx.x];
                    y0 = yy.x;
                    y1 = yy.y;
                }
                ll[kk] = (u64)y0 * mm.x + ll[kk];
                lh[kk] = (u64)y0 * mm.y + lh[kk];
                hl[kk] = (u64)y1 * mm.x + hl[kk];
                hh[kk] = (u64)y1 * mm.y + hh[kk];
            }
        }
        if (r90) {   // (uniform) rows carry 2^90: word-wise REDC from the accumulators (pha_arith.h)
            const u32 p0 = (u32)p & 0x3fffffffu, p1 = (u32)(p >> 30);
#pragma unroll
            for (int kk = 0; kk < K; kk++) out[kk] = mont_redc90_split(ll[kk], lh[kk], hl[kk], hh[kk], p, p0, p1, (u32)oninv);
            return;
        }
#pragma unroll
        for (int kk = 0; kk < K; kk++) {
            const u64 mid = lh[kk] + hl[kk], mid_c = mid < lh[kk] ? 1 : 0;
            u64 rl = ll[kk], rh = 0;
            const u64 t1 = mid << 30;
            rl += t1;
            rh += (rl < t1) + (mid >> 34) + (mid_c << 30);
            const u64 t2 = hh[kk] << 60;
            rl += t2;
            rh += (rl < t2) + (hh[kk] >> 4);
            out[kk] = mont_redc128(rl, rh, p, oninv);
        }
    };
    u64 c_last[K];                       // RESC: t_last - dP_last mod q_last of the thread's four coefficients
    uint32_t n_out = osz;
    if (RESC) {
        n_out = osz - 1;                 // the converter's last row is the last data limb's
        const ConvLimbRec rl = s_rec[n_out];
        const u64 ql_ = uni64(rl.p);
        u64 dl[K];
        convert4(n_out, ql_, uni64(rl.oninv), dl);
        const u64 *last = m.resc_last + (size_t)grp * m.src_group_stride;
#pragma unroll
        for (int kk = 0; kk < K; kk++) c_last[kk] = sub_mod(last[off[kk]], dl[kk], ql_);
    }
#pragma unroll 1
    for (uint32_t e = 0; e < n_out; e++) {
        const ConvLimbRec rc = s_rec[e];
        const u64 p = uni64(rc.p), oninv = uni64(rc.oninv);
        const uint32_t jo = uni32(rc.jo), prime = uni32(rc.prime), fpok = uni32(rc.fpok);
        PassArgs a;
        a.in = nullptr;
        a.out = dig + (size_t)jo * n;
        a.tw = k.tw + (size_t)prime * n;
        a.twd = k.twf + (size_t)prime * n;
        a.q = p;
        a.tile = tile;
        a.rho0 = k.t1;
        a.stride = k.t2;
        a.aux = a.aux2 = nullptr;
        a.pro_reduce = false;
        a.pro_ratio1 = 0;
        a.fp = fpok != 0;
        a.fpm = FpMod{as_f64(uni64(as_u64(rc.fq))), as_f64(uni64(as_u64(rc.fqinv))), (fpok & 2) != 0, (fpok & 4) != 0};
        u64 reg[K];
        u64x2 twreg[C::TW_TOTAL];
        // the pass's LDS / global offsets are functions of the thread index alone: recomputed per limb (a few dozen scalar-like
        // vector instructions against ~2500) instead of living in ~40 registers next to the 120 of the inputs
        int tid_e = threadIdx.x;
        asm volatile("" : "+v"(tid_e));
        auto limb = [&](const PassArgs &pa) __attribute__((always_inline)) {
            const int tid = tid_e;
            Prog::load_twiddles(pa, tid, twreg);
            convert4(e, p, oninv, reg);
            if (RESC) {   // v_j = dP_j + (c_last mod q_j)   (bconv_rescale_kernel; divide_and_round_reduce_q_last_kernel rns.cu:1128-1139)
                const u64 ratio1 = uni64(rc.ratio1);
#pragma unroll
                for (int kk = 0; kk < K; kk++) reg[kk] = add_mod(reg[kk], barrett64(c_last[kk], p, ratio1), p);
            }
            Prog::template run_pass<SEG_PREFETCHED, true>(pa, lds, tid, reg, twreg);   // (tail hand-over: the next limb's first round writes the same LDS words)
        };
        PHA_WITH_FP_KNOWN(a, a.fp, limb);   // (uniform) one specialised body per butterfly back end, as exec_pass has them
    }
}

// workgroups from which a mod-up takes the fused form.  The test-only library: every N = 2^16 mod-up, so that the key-switch parity
// tests reach it with ONE ciphertext (tests/test_gpu_ntt_variants.py)
#if defined(PHA_EXPERIMENTS)
constexpr size_t kMcsMinWorkgroups = 1;
#else
constexpr size_t kMcsMinWorkgroups = 1024;
#endif
// one launch of the kernel for ISZ_PAD input limbs in FORM
template <class C, int ISZ_PAD, int FORM>
static void launch_modup_conv(const NttKArgs &k, const ModupConvArgs &m, dim3 grid, hipStream_t s) {
    auto lds_for = [&](uint32_t max_osz) {
        constexpr int rl = mcs_reg_limbs(FORM), in_lds = ISZ_PAD > rl ? ISZ_PAD - rl : 0;
        return (size_t)C::LDS_WORDS * sizeof(u64) + (size_t)max_osz * kBcRowPad * sizeof(uint2) + (size_t)max_osz * sizeof(ConvLimbRec) +
               (size_t)in_lds * 4 * C::THREADS * sizeof(uint2);
    };
    // the request grows with the level's output-limb count (176 B per limb of max_osz), so the limit is raised ONCE per kernel and
    // device to the WORST case (kMcsMaxOut output limbs), not to the first call's size (a later, larger level would
    // otherwise ask for more than the recorded limit)
    const size_t lds_bytes = lds_for(m.max_osz), lds_worst = lds_for(kMcsMaxOut);
    static_assert(kMcsMaxOut <= 64, "worst-case LDS request must stay inside the CU's 160 KiB");
    if (lds_worst > 160 * 1024) throw std::logic_error("modup_conv_strided: worst-case LDS request exceeds the CU");
    static std::atomic<uint64_t> raised{0};
    raise_lds_limit(reinterpret_cast<const void *>(&modup_conv_s1_kernel<C, ISZ_PAD, FORM>), lds_worst, raised);
    hipLaunchKernelGGL((modup_conv_s1_kernel<C, ISZ_PAD, FORM>), grid, dim3(C::THREADS), lds_bytes, s, k, m);
    check_launch();
}

bool modup_conv_strided(Context &c, u64 *digits, const LimbSel &sel, const NttExtra &x, const ModupConvArgs &m, hipStream_t s) {
    // the fused pass replaces the strided pass of NttPlan<16, 10> (64 rows x 1024-point rows): N = 2^16 launches that take that plan
    if (c.log_n != 16 || !m.mont_split || m.max_isz > 16 || m.max_osz > (uint32_t)kMcsMaxOut || sel.count == 0 || sel.start != 0) return false;
    NttExtra xd = x;
    xd.first_pass_done = true;
    const ResolvedPlan r = choose_plan(c, sel, xd);
    if (r.whole || r.one_launch_asked || r.variant != 10) return false;
    using P1 = NttPlan<16, 10>::P1;
    using P2 = NttPlan<16, 10>::P2;
    using C = PassCfg<6, true, 2, 2, 2, 4, false, kMcsLogTile>;    // = NttPlan<16, 13>::P1 (the CPU replay runs that plan)
    static_assert(C::LOGT == P1::LOGT, "the fused pass is the strided pass of the plan whose contiguous pass follows");
    static_assert(std::is_same<C, NttPlan<16, 13>::P1>::value, "NttPlan<16, 13> names this pass");
    check_sel(c, sel);
    NttKArgs k = make_args(c, digits, digits, digits, sel, x, true);
    k.t1 = P1::T;
    k.t2 = P2::T;
    const dim3 grid((unsigned)(c.n >> C::LOGTILE), 1, k.batch);
    // a workgroup walks all output limbs of its tile (45 at the top level: ~200 us), so the form only pays when the launch fills the
    // device several times over: two workgroups per CU are resident, four generations of them = batches of >= 6 ciphertexts at
    // beta = 3 (measured: equal to the separate kernels at B = 32, 1.5 % ahead at B = 8; a single ciphertext would wait ~200 us for
    // 192 workgroups where the separate kernels take 67)
    if ((size_t)grid.x * grid.z < kMcsMinWorkgroups) return false;
    // rescale form: one converter, its last row is the last data limb's (and yields no output limb); plain mod-down form: one
    // converter, every row an output limb
    if (m.resc_last && (m.beta != 1 || sel.count + 1 != m.max_osz)) throw std::logic_error("modup_conv_strided: rescale form needs the P -> Ql converter of this level");
    if (!m.resc_last && m.moddown && (m.beta != 1 || sel.count != m.max_osz)) throw std::logic_error("modup_conv_strided: mod-down form needs the P -> Ql converter of this level");
    if (m.max_isz <= 8) return false;
    auto form = [&](auto f) {
        if (m.max_isz == 15) launch_modup_conv<C, 15, f()>(k, m, grid, s);
        else launch_modup_conv<C, 16, f()>(k, m, grid, s);
    };
    if (m.resc_last) form(std::integral_constant<int, 1>{});
    else if (m.moddown) form(std::integral_constant<int, 2>{});
    else form(std::integral_constant<int, 0>{});
    return true;
}

}  // namespace pha
