// pha_rns.hip -- fast base conversion, hybrid key-switch (mod-up / inner product / mod-down),
// CKKS rescale and Galois permutations on gfx950.
//
// Reference: src/rns_bconv.cu (bconv_mult / bconv_matmul / modup / moddown), src/eval_key_switch.cu,
// src/rns.cu:1082-1184, src/galois.cu.  Differences in HOW (results are bit-identical):
//   * base conversion is one kernel: a thread owns one coefficient, keeps the (scaled) input
//     residues of the digit in registers and walks the output primes, so inputs are read once per
//     output group instead of once per output prime, the q-hat matrix and the output modulus are
//     wave-uniform scalar loads, and stores are coalesced along the coefficient axis (the
//     reference maps adjacent threads to different output limbs);
//   * the q-hat^-1 scaling (bconv phase 1) is fused into the load (no temp round trip);
//   * limb index = blockIdx.y everywhere (no tid / N);
//   * mod-down and rescale reuse the forward NTT's fused epilogue (cx - NTT(delta)) * c.
// A conversion launch is one BConvCall (pha_internal.h) filled by name: bconv_call() fills the converter's part from a BConv or,
// for the mod-up digits, from the Tool; launch_bconv() turns it into the kernel's BConvLaunch and picks the instantiation with
// with_isz_pad, as the fused rescale conversion does.  The mod-down's P -> Ql step is p_to_ql_delta().
#include "../../include/phantom_amd.h"
#include "pha_internal.h"
#include <algorithm>
#include <atomic>

#include "pha_ntt_core.h"

namespace pha {

void launch_add(Context &c, const u64 *a, const u64 *b, u64 *r, size_t limbs, size_t mod_start, hipStream_t s);

// carry-free split-accumulator MAC in base conversion (experiments library: pha_set_tuning key 1 switches it off)
#if defined(PHA_EXPERIMENTS)
std::atomic<int> g_bconv_split{1};
static inline bool bconv_split_on() { return g_bconv_split.load(std::memory_order_relaxed) != 0; }
#else
static constexpr bool bconv_split_on() { return true; }
#endif

constexpr int kBcThreads = 256;
constexpr int kBcMaxOutPerBlock = 32;  // output primes per workgroup (upper bound; the launch balances the groups)

struct BConvLaunch {
    const BConvDev *convs;       // device array
    uint32_t conv_step;          // converter of polynomial z = convs[z * conv_step]
    u64 *dst;                    // polynomial z: dst + z * dst_stride
    const u64 *src;              // polynomial z: src + z * src_stride (+ src_limb * n)
    const u64 *own;              // copy_own source (the NTT-form input of mod-up), same for every z
    size_t dst_stride, src_stride;
    const DModulus *mod;
    uint32_t n;
    uint32_t out_per_block;      // output primes per workgroup (<= kBcMaxOutPerBlock)
    // batches of ciphertexts (mod-up): polynomial z = (ciphertext z / conv_count, digit z % conv_count);
    // conv_count = 0: every z has its own converter index z (one ciphertext) or shares converter 0 (conv_step 0)
    uint32_t conv_count;
    size_t src_group_stride, own_group_stride;  // per ciphertext
    // optional epilogue (BFV mod-down, moddown_kernel rns_bconv.cu:680-689 + add_to_ct_kernel :763-769 fused into the conversion):
    // instead of storing delta_j the kernel stores epi_dst_j (+)= (epi_cx_j - delta_j) * epi_cst_j; null epi_cx = off
    const u64 *epi_cx;
    u64 *epi_dst;
    const u64x2 *epi_cst;        // [limb] constant with its Shoup quotient (P^-1 mod q_j)
    size_t epi_cx_stride, epi_dst_stride;
    uint32_t epi_acc;
    // optional bConv_HPS correction (BConvEpilogue::hps_inv / hps_alpha)
    const double *hps_inv;
    const u64 *hps_alpha;
};
struct BConvWho {
    uint32_t ci, grp;
};
__device__ __forceinline__ BConvWho bconv_who(const BConvLaunch &L) {
    const uint32_t z = blockIdx.z;
    return L.conv_count ? BConvWho{z % L.conv_count, z / L.conv_count} : BConvWho{z, 0u};
}

// bconv_mult (+) bconv_matmul (src/rns_bconv.cu:22-60,109-170; padded variant :455-485).
// SPLIT: carry-free MAC -- inputs are cut at bit SY and matrix entries at bit SM, the four partial
// products accumulate in plain 64-bit registers with one v_mad_u64_u32 each and are recombined once per
// output.  (SY, SM) = (30, 30): primes <= 60 bits, isz <= 16 (products < 2^60, 16 of them).  (30, 31) / (31, 30): isz <= 32,
// residues up to 60 bits on one side and up to 62 on the other (products < 2^61, recombined every 8 terms) -- the Q -> Bsk,
// Q -> R and back conversions of the BFV multiply, whose auxiliary primes are 61 bits wide (BConv::split_kind).
template <int ISZ_PAD, bool SCALE_IN, bool SPLIT, int SY = 30, int SM = 30>
__global__ __launch_bounds__(kBcThreads) void bconv_kernel(const BConvLaunch L) {
    constexpr int ROWPAD = ISZ_PAD > kBcRowPad ? 32 : kBcRowPad;
    const BConvWho who = bconv_who(L);
    const BConvDev &d = L.convs[who.ci * L.conv_step];
    const uint32_t coeff = blockIdx.x * kBcThreads + threadIdx.x;
    const uint32_t n = L.n;
    const u64 *src = L.src + (size_t)blockIdx.z * L.src_stride + (size_t)who.grp * L.src_group_stride + (size_t)d.src_limb * n;
    const u64 *own = L.own + (size_t)who.grp * L.own_group_stride;
    u64 *dst = L.dst + (size_t)blockIdx.z * L.dst_stride;
    const uint32_t isz = d.isz, osz = d.osz;
    const uint32_t j0 = blockIdx.y * L.out_per_block;
    const uint32_t j1 = min(j0 + L.out_per_block, osz);
    const bool mont = SPLIT && d.oninv != nullptr;
    const bool r90 = mont && SY == 30 && SM == 30 && d.r90 != 0;   // (uniform) word-wise REDC from the split accumulators
    // Everything the output loop needs per output prime goes through LDS once per workgroup: the matrix rows (SPLIT:
    // out_per_block x 16 entries of two dwords, read back as broadcast ds_read_b64) and the prime's constants and
    // destination limb.  (r02: the loop used to fetch oprime[j] and then mod[oprime[j]] from global memory for every
    // output -- two dependent vector loads per iteration, which made the kernel latency-bound at 2.3x its VALU time.)
    __shared__ uint2 s_rows[kBcMaxOutPerBlock * ROWPAD];
    __shared__ u64 s_p[kBcMaxOutPerBlock], s_c0[kBcMaxOutPerBlock], s_c1[kBcMaxOutPerBlock];
    __shared__ uint32_t s_jo[kBcMaxOutPerBlock];
    __shared__ u64x2 s_e[kBcMaxOutPerBlock];
    if (SPLIT) {
        // the converter's own row pitch may be smaller than this instantiation's (a short last digit next to full ones)
        const uint32_t pitch = d.row_pad;
        for (uint32_t e = threadIdx.x; e < L.out_per_block * ROWPAD; e += kBcThreads) {
            const uint32_t j = j0 + e / ROWPAD, i = e % ROWPAD;
            s_rows[e] = (j < osz && i < pitch) ? reinterpret_cast<const uint2 *>(d.mat30)[j * pitch + i] : uint2{0u, 0u};
        }
    }
    if (threadIdx.x < L.out_per_block && j0 + threadIdx.x < osz) {
        const uint32_t j = j0 + threadIdx.x;
        const DModulus m = L.mod[d.oprime[j]];
        s_p[threadIdx.x] = m.value;
        s_c0[threadIdx.x] = mont ? d.oninv[j] : m.ratio0;   // Montgomery: -p^-1 mod 2^64; Barrett: floor(2^128 / p)
        // r06 (2^90 rows): the 30-bit halves of p ride in the Barrett word the Montgomery branch does not use
        s_c1[threadIdx.x] = r90 ? ((m.value >> 30) << 32) | (m.value & 0x3fffffffu) : m.ratio1;
        const uint32_t jo = j + (j >= d.pad_start ? d.pad_len : 0);
        s_jo[threadIdx.x] = jo;
        if (L.epi_cx) s_e[threadIdx.x] = L.epi_cst[jo];
    }
    __syncthreads();
    if (j0 >= osz) return;  // (after the barrier) nothing to produce for this group
    u64 y[ISZ_PAD];
    u32 ylo[ISZ_PAD], yhi[ISZ_PAD];  // SPLIT: 30-bit halves, cut once per input
    double hps_frac = 0.0;           // bConv_HPS: sum_i y_i / q_i in the reference's order (hps_fix_kernel)
#pragma unroll
    for (int i = 0; i < ISZ_PAD; i++) {
        y[i] = 0;
        if (i < (int)isz) {
            u64 x = src[(size_t)i * n + coeff];
            if (SCALE_IN) x = shoup(x, d.hat_inv[i], L.mod[d.iprime[i]].value);
            y[i] = x;
            if (L.hps_inv) hps_frac = __builtin_fma((double)x, L.hps_inv[i], hps_frac);
        }
        ylo[i] = (u32)y[i] & ((1u << SY) - 1);
        yhi[i] = (u32)(y[i] >> SY);
    }
    if (d.copy_own && L.own && blockIdx.y == 0) {  // modup_copy_partQl_kernel rns_bconv.cu:522-528 (null own: the caller reads c2 itself)
        for (uint32_t i = 0; i < isz; i++)
            dst[(size_t)(d.src_limb + i) * n + coeff] = own[(size_t)(d.src_limb + i) * n + coeff];
    }
    const uint32_t count = j1 - j0;
    const u64 *hps_row = L.hps_inv ? L.hps_alpha + (size_t)llround(hps_frac) * osz + j0 : nullptr;
    for (uint32_t e = 0; e < count; e++) {
        u64 lo = 0, hi = 0, r = 0;
        bool reduced = false;
        if (SPLIT) {
            // rows are zero-padded to ROWPAD entries, and y[i] = 0 beyond isz: no per-term branch
            const uint2 *row = s_rows + e * ROWPAD;
            if (SY == 30 && SM == 30) {
                u64 ll = 0, lh = 0, hl = 0, hh = 0;
#pragma unroll
                for (int i = 0; i < ISZ_PAD; i++) {
                    const u32 y0 = ylo[i], y1 = yhi[i];
                    const uint2 mm = row[i];
                    const u32 m0 = mm.x, m1 = mm.y;
                    ll = (u64)y0 * m0 + ll;
                    lh = (u64)y0 * m1 + lh;
                    hl = (u64)y1 * m0 + hl;
                    hh = (u64)y1 * m1 + hh;
                }
                if (r90) {   // rows carry 2^90: three 30-bit REDC steps on the accumulators as they stand
                    const u64 pp = s_c1[e];
                    r = mont_redc90_split(ll, lh, hl, hh, s_p[e], (u32)pp, (u32)(pp >> 32), (u32)s_c0[e]);
                    reduced = true;
                } else {
                    // value = ll + (lh + hl) * 2^30 + hh * 2^60   (mid < 2^65: keep its carry)
                    const u64 mid = lh + hl;
                    const u64 mid_c = mid < lh ? 1 : 0;
                    lo = ll;
                    hi = 0;
                    const u64 t1 = mid << 30;
                    lo += t1;
                    hi += (lo < t1) + (mid >> 34) + (mid_c << 30);
                    const u64 t2 = hh << 60;
                    lo += t2;
                    hi += (lo < t2) + (hh >> 4);
                }
            } else {
                // halves of up to 30 / 31 bits: partial products below 2^61, so the four sums are folded into the 128-bit
                // total every 8 terms: value += ll + lh * 2^SM + hl * 2^SY + hh * 2^(SY + SM)
                lo = 0;
                hi = 0;
#pragma unroll
                for (int base = 0; base < ISZ_PAD; base += 8) {
                    u64 ll = 0, lh = 0, hl = 0, hh = 0;
#pragma unroll
                    for (int i = base; i < base + 8 && i < ISZ_PAD; i++) {
                        const u32 y0 = ylo[i], y1 = yhi[i];
                        const uint2 mm = row[i];
                        const u32 m0 = mm.x, m1 = mm.y;
                        ll = (u64)y0 * m0 + ll;
                        lh = (u64)y0 * m1 + lh;
                        hl = (u64)y1 * m0 + hl;
                        hh = (u64)y1 * m1 + hh;
                    }
                    lo += ll;
                    hi += lo < ll;
                    u64 t = lh << SM;
                    lo += t;
                    hi += (lo < t) + (lh >> (64 - SM));
                    t = hl << SY;
                    lo += t;
                    hi += (lo < t) + (hl >> (64 - SY));
                    t = hh << (SY + SM);
                    lo += t;
                    hi += (lo < t) + (hh >> (64 - SY - SM));
                }
            }
        } else {
            const u64 *row = d.mat + (size_t)(j0 + e) * isz;
            lo = 0;
            hi = 0;
#pragma unroll
            for (int i = 0; i < ISZ_PAD; i++)
                if (i < (int)isz) mac128(y[i], row[i], lo, hi);
        }
        // SPLIT rows are in Montgomery form when the converter has oninv (uniform): sum_i y_i * (qhat_i 2^64) < 16 * 2^60 * p
        // = 2^64 p, and REDC brings it to sum_i y_i * qhat_i mod p with a third of Barrett-128's multiplies
        const u64 p = s_p[e];
        if (reduced) {}
        else if (mont) r = mont_redc128(lo, hi, p, s_c0[e]);
        else r = barrett128(lo, hi, DModulus{p, s_c0[e], s_c1[e]});
        if (hps_row) r = sub_mod(r, hps_row[e], p);
        const size_t id = (size_t)s_jo[e] * n + coeff;
        if (L.epi_cx) {
            const u64 t = sub_mod(L.epi_cx[(size_t)blockIdx.z * L.epi_cx_stride + id], r, p);
            u64 o = shoup(t, s_e[e], p);
            u64 *out = L.epi_dst + (size_t)blockIdx.z * L.epi_dst_stride + id;
            if (L.epi_acc) o = add_mod(*out, o, p);
            *out = o;
        } else {
            dst[id] = r;
        }
    }
}

// generic fallback for very wide input bases (isz > 16): inputs are re-read per output prime
template <bool SCALE_IN>
__global__ __launch_bounds__(kBcThreads) void bconv_wide_kernel(const BConvLaunch L) {
    const BConvWho who = bconv_who(L);
    const BConvDev &d = L.convs[who.ci * L.conv_step];
    const uint32_t coeff = blockIdx.x * kBcThreads + threadIdx.x;
    const uint32_t n = L.n;
    const u64 *src = L.src + (size_t)blockIdx.z * L.src_stride + (size_t)who.grp * L.src_group_stride + (size_t)d.src_limb * n;
    const u64 *own = L.own + (size_t)who.grp * L.own_group_stride;
    u64 *dst = L.dst + (size_t)blockIdx.z * L.dst_stride;
    if (d.copy_own && L.own && blockIdx.y == 0) {
        for (uint32_t i = 0; i < d.isz; i++)
            dst[(size_t)(d.src_limb + i) * n + coeff] = own[(size_t)(d.src_limb + i) * n + coeff];
    }
    const uint32_t j0 = blockIdx.y * L.out_per_block;
    const uint32_t j1 = min(j0 + L.out_per_block, d.osz);
    for (uint32_t j = j0; j < j1; j++) {
        const DModulus m = L.mod[d.oprime[j]];
        const u64 *row = d.mat + (size_t)j * d.isz;
        u64 lo = 0, hi = 0;
        for (uint32_t i = 0; i < d.isz; i++) {
            u64 x = src[(size_t)i * n + coeff];
            if (SCALE_IN) x = shoup(x, d.hat_inv[i], L.mod[d.iprime[i]].value);
            mac128(x, row[i], lo, hi);
        }
        const uint32_t jo = j + (j >= d.pad_start ? d.pad_len : 0);
        dst[(size_t)jo * n + coeff] = barrett128(lo, hi, m);
    }
}

// Output groups (blockIdx.y) of a conversion launch: up to 32 outputs per workgroup (the inputs are loaded and scaled once per
// group: config 4's 30-output mod-down in one group, +4 % on that job) when that still leaves four workgroups per CU, 24 otherwise
// (a single polynomial at N = 2^15); balanced: 45 outputs -> 2 groups of 23
static uint32_t bconv_groups(const Context &c, uint32_t osz, uint32_t polys) {
    const uint32_t few = (osz + kBcMaxOutPerBlock - 1) / kBcMaxOutPerBlock;
    const uint32_t cap = (c.n / kBcThreads) * few * polys >= 1024 ? kBcMaxOutPerBlock : 24;
    return (osz + cap - 1) / cap;
}

// the instantiation with P register-resident inputs: the 30 / 30 cuts (or no split), and the wide cuts of kinds 2 and 3
template <int P>
static void launch_bconv_kernel(bool scale_in, bool split, dim3 grid, dim3 block, hipStream_t s, const BConvLaunch &L) {
    if (scale_in && split) hipLaunchKernelGGL((bconv_kernel<P, true, true>), grid, block, 0, s, L);
    else if (scale_in) hipLaunchKernelGGL((bconv_kernel<P, true, false>), grid, block, 0, s, L);
    else if (split) hipLaunchKernelGGL((bconv_kernel<P, false, true>), grid, block, 0, s, L);
    else hipLaunchKernelGGL((bconv_kernel<P, false, false>), grid, block, 0, s, L);
}
template <int P, int SY, int SM>
static void launch_bconv_kernel_cut(bool scale_in, dim3 grid, dim3 block, hipStream_t s, const BConvLaunch &L) {
    if (scale_in) hipLaunchKernelGGL((bconv_kernel<P, true, true, SY, SM>), grid, block, 0, s, L);
    else hipLaunchKernelGGL((bconv_kernel<P, false, true, SY, SM>), grid, block, 0, s, L);
}
// (BConvCall: pha_internal.h)
void launch_bconv(Context &c, const BConvCall &k, hipStream_t s) {
    BConvLaunch L{};
    if (k.epi) {
        if (k.max_isz > 32) throw std::logic_error("the fused conversion epilogues need the register-resident converter");
        L.epi_cx = k.epi->cx; L.epi_dst = k.epi->dst; L.epi_cst = k.epi->cst;
        L.epi_cx_stride = k.epi->cx_stride; L.epi_dst_stride = k.epi->dst_stride; L.epi_acc = k.epi->accumulate ? 1 : 0;
        L.hps_inv = k.epi->hps_inv; L.hps_alpha = k.epi->hps_alpha;
    }
    L.conv_count = k.conv_count; L.src_group_stride = k.group_stride;
    L.own_group_stride = k.own_group_stride ? k.own_group_stride : k.group_stride;
    L.convs = k.convs; L.conv_step = k.conv_step; L.dst = k.dst; L.src = k.src; L.own = k.own;
    L.dst_stride = k.dst_stride; L.src_stride = k.src_stride; L.mod = c.d_mod.p; L.n = (uint32_t)c.n;
    const uint32_t groups = bconv_groups(c, k.max_osz, k.polys);
    L.out_per_block = (k.max_osz + groups - 1) / groups;
    const dim3 grid((unsigned)(c.n / kBcThreads), groups, k.polys), block(kBcThreads);
    // the 30 / 30 split accumulators hold at most 16 terms; wider bases or wider primes take the 30 / 31 cuts (16 or 32 inputs in
    // registers) or the 128-bit accumulate, and more than 32 inputs the kernel that re-reads them
    bool resident;
    if (k.split_kind == 2 && bconv_split_on()) {
        resident = with_isz_pad<16, 32>(k.max_isz, [&](auto P) { launch_bconv_kernel_cut<decltype(P)::value, 30, 31>(k.scale_in, grid, block, s, L); });
    } else if (k.split_kind == 3 && bconv_split_on()) {
        resident = with_isz_pad<16, 32>(k.max_isz, [&](auto P) { launch_bconv_kernel_cut<decltype(P)::value, 31, 30>(k.scale_in, grid, block, s, L); });
    } else {
        const bool split = k.split_kind == 1 && k.max_isz <= 16 && bconv_split_on();
        resident = with_isz_pad<2, 32>(k.max_isz, [&](auto P) { launch_bconv_kernel<decltype(P)::value>(k.scale_in, split, grid, block, s, L); });
    }
    if (!resident) {
        if (k.scale_in) hipLaunchKernelGGL((bconv_wide_kernel<true>), grid, block, 0, s, L);
        else hipLaunchKernelGGL((bconv_wide_kernel<false>), grid, block, 0, s, L);
    }
    check_launch();
}

// ---- pha_keyswitch_rescale: the P -> Ql conversion of mod-down with the rescale's last-limb work folded in ----------------
// Per coefficient (one thread), with y_i the P residues of cx in coefficient form, already scaled by phat_i^-1 (the inverse
// transform's epilogue did that) and M' the converter whose rows carry P^-1 (Tool::p_to_ql_pinv):
//   dP_j   = sum_i y_i M'_ij mod q_j            = delta_j * P^-1        (moddown_from_NTT rns_bconv.cu:776-828 up to its NTT)
//   c_last = t_last - dP_last mod q_last          t_last = iNTT(ct_last + cx_last P^-1): coefficient form of the key-switched
//                                                 ciphertext's last limb (rns.cu:1171 after rns_bconv.cu:763-769)
//   v_j    = dP_j + (c_last mod q_j) mod q_j      j < Ql - 1
// One forward transform of v then gives out_j = (ct_j + cx_j P^-1 - NTT(v)_j) q_last^-1 (EPI_FWD_KSRESCALE), bit for bit what
// keyswitch_inplace followed by divide_and_round_q_last_ntt stores (NTT is linear; every stored value is canonical).
struct BConvRescaleLaunch {
    const BConvDev *conv;        // P -> Ql with P^-1 folded into the rows (Montgomery form)
    u64 *dst;                    // v: polynomial z at dst + z * dst_stride, [Ql - 1][N]
    const u64 *cx;               // polynomial z at cx + z * cx_stride: [QlP][N], limb Ql - 1 = t_last, limbs >= Ql = y
    size_t dst_stride, cx_stride;
    const DModulus *mod;
    uint32_t n, ql, out_per_block;
};
template <int ISZ_PAD>
__global__ __launch_bounds__(kBcThreads) void bconv_rescale_kernel(const BConvRescaleLaunch L) {
    const BConvDev &d = *L.conv;
    const uint32_t coeff = blockIdx.x * kBcThreads + threadIdx.x;
    const uint32_t n = L.n, nl = L.ql - 1;
    const u64 *cx = L.cx + (size_t)blockIdx.z * L.cx_stride;
    const u64 *src = cx + (size_t)L.ql * n;
    u64 *dst = L.dst + (size_t)blockIdx.z * L.dst_stride;
    const uint32_t j0 = blockIdx.y * L.out_per_block;
    const uint32_t j1 = min(j0 + L.out_per_block, nl);
    // rows / constants of this group's outputs, plus (slot out_per_block) those of the last data limb
    __shared__ uint2 s_rows[(kBcMaxOutPerBlock + 1) * kBcRowPad];
    __shared__ u64 s_p[kBcMaxOutPerBlock + 1], s_c0[kBcMaxOutPerBlock + 1], s_c1[kBcMaxOutPerBlock + 1];
    __shared__ uint2 s_pp[kBcMaxOutPerBlock + 1];   // r06: the 30-bit halves of p (mont_redc90_split)
    const bool r90 = d.r90 != 0;                    // (uniform) the rows carry 2^90
    for (uint32_t e = threadIdx.x; e < (L.out_per_block + 1) * kBcRowPad; e += kBcThreads) {
        const uint32_t slot = e / kBcRowPad, i = e % kBcRowPad;
        const uint32_t j = slot == L.out_per_block ? nl : j0 + slot;
        s_rows[e] = j <= nl ? reinterpret_cast<const uint2 *>(d.mat30)[j * kBcRowPad + i] : uint2{0u, 0u};
    }
    if (threadIdx.x <= L.out_per_block) {
        const uint32_t j = threadIdx.x == L.out_per_block ? nl : j0 + threadIdx.x;
        if (j <= nl) {
            const DModulus m = L.mod[d.oprime[j]];
            s_p[threadIdx.x] = m.value;
            s_c0[threadIdx.x] = d.oninv[j];
            s_c1[threadIdx.x] = m.ratio1;
            s_pp[threadIdx.x] = uint2{(uint32_t)(m.value & 0x3fffffffu), (uint32_t)(m.value >> 30)};
        }
    }
    __syncthreads();
    if (j0 >= nl) return;
    u32 ylo[ISZ_PAD], yhi[ISZ_PAD];
#pragma unroll
    for (int i = 0; i < ISZ_PAD; i++) {
        const u64 y = i < (int)d.isz ? src[(size_t)i * n + coeff] : 0;
        ylo[i] = (u32)y & 0x3fffffffu;
        yhi[i] = (u32)(y >> 30);
    }
    auto convert = [&](uint32_t slot) -> u64 {   // sum_i y_i * row_i, reduced (REDC) modulo the slot's prime
        const uint2 *row = s_rows + slot * kBcRowPad;
        u64 ll = 0, lh = 0, hl = 0, hh = 0;
#pragma unroll
        for (int i = 0; i < ISZ_PAD; i++) {
            const uint2 mm = row[i];
            ll = (u64)ylo[i] * mm.x + ll;
            lh = (u64)ylo[i] * mm.y + lh;
            hl = (u64)yhi[i] * mm.x + hl;
            hh = (u64)yhi[i] * mm.y + hh;
        }
        if (r90) {
            const uint2 pp = s_pp[slot];
            return mont_redc90_split(ll, lh, hl, hh, s_p[slot], pp.x, pp.y, (u32)s_c0[slot]);
        }
        const u64 mid = lh + hl, mid_c = mid < lh ? 1 : 0;
        u64 lo = ll, hi = 0;
        const u64 t1 = mid << 30;
        lo += t1;
        hi += (lo < t1) + (mid >> 34) + (mid_c << 30);
        const u64 t2 = hh << 60;
        lo += t2;
        hi += (lo < t2) + (hh >> 4);
        return mont_redc128(lo, hi, s_p[slot], s_c0[slot]);
    };
    const u64 q_last = s_p[L.out_per_block];
    const u64 c_last = sub_mod(cx[(size_t)nl * n + coeff], convert(L.out_per_block), q_last);
    const uint32_t count = j1 - j0;
    for (uint32_t e = 0; e < count; e++) {
        const u64 p = s_p[e];
        const u64 r = barrett64(c_last, p, s_c1[e]);   // divide_and_round_reduce_q_last_kernel rns.cu:1128-1139
        dst[(size_t)(j0 + e) * n + coeff] = add_mod(convert(e), r, p);
    }
}

// ---- alpha == 1 fast paths (rns_bconv.cu:432-453, :691-707) -------------------------------------
struct SinglePArgs {
    u64 *dst;
    const u64 *src_raw, *src_normal;
    const DModulus *mod;
    const uint32_t *qlp_prime;
    uint32_t in_limb, n;
};
// out limb = blockIdx.y over [0, count): dst[j] = (j == in_limb) ? src_raw : reduce(src_normal)
__global__ __launch_bounds__(256) void single_p_kernel(const SinglePArgs k) {
    const uint32_t j = blockIdx.y;
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    u64 v;
    if (j == k.in_limb) {
        v = k.src_raw[coeff];
    } else {
        const DModulus mo = k.mod[k.qlp_prime[j]];
        const u64 ip = k.mod[k.qlp_prime[k.in_limb]].value;
        v = k.src_normal[coeff];
        if (ip > mo.value) v = barrett64(v, mo.value, mo.ratio1);
    }
    k.dst[(size_t)j * k.n + coeff] = v;
}

// ---- key-switch inner product (eval_key_switch.cu:14-69) ----------------------------------------
struct InnerArgs {
    u64 *cx;
    const u64 *t_mod_up;
    const u64 *const *evks;
    const DModulus *mod;
    const uint32_t *qlp_prime;
    uint32_t n, beta;
    size_t qlp_n, qp_n;
    // pha_keyswitch_rescale: limb fix_limb of cx (the last data limb) receives ct_last + cx_last * P^-1 instead of cx_last
    // (its inverse transform is the first half of c_last; rns.cu:1171 after rns_bconv.cu:763-769); 0xffffffff = off
    uint32_t fix_limb;
    u64x2 fix_cst;           // P^-1 mod q_last
    const u64 *fix_ct;       // ct [2][Ql][N] of the (first) ciphertext
    size_t fix_ct_stride;    // Ql * N
    const FpInfo *fpinfo;    // [prime]: limbs below 2^50 form their sums in FP64 (batched kernel, r04)
    // r06 (batched kernel, NTT-form schemes): digit i's own limbs [i * alpha, min((i + 1) * alpha, ql)) are read from c2 where they lie
    // (own + b * own_stride) instead of from a verbatim copy inside t_mod_up, which the mod-up then does not make (modup's
    // own_in_place): 2 x 22.5 MiB per ciphertext at C3 that only moved data.  null = the copy is there (pha_modup's callers).
    const u64 *own;
    size_t own_stride;
    uint32_t alpha, ql;
};
__device__ __forceinline__ void inner_fix(const InnerArgs &k, uint32_t nid, const DModulus &m, size_t coeff, uint32_t b,
                                          u64x2 &r0, u64x2 &r1) {
    if (nid != k.fix_limb) return;   // uniform per workgroup
    const u64 *ct0 = k.fix_ct + (size_t)(2 * b) * k.fix_ct_stride + (size_t)nid * k.n + coeff;
    const u64x2 c0 = *reinterpret_cast<const u64x2 *>(ct0), c1 = *reinterpret_cast<const u64x2 *>(ct0 + k.fix_ct_stride);
    r0.x = add_mod(c0.x, shoup(r0.x, k.fix_cst, m.value), m.value);
    r0.y = add_mod(c0.y, shoup(r0.y, k.fix_cst, m.value), m.value);
    r1.x = add_mod(c1.x, shoup(r1.x, k.fix_cst, m.value), m.value);
    r1.y = add_mod(c1.y, shoup(r1.y, k.fix_cst, m.value), m.value);
}
__global__ __launch_bounds__(256) void inner_prod_kernel(const InnerArgs k) {
    const uint32_t nid = blockIdx.y;          // limb in [Ql || P]
    const uint32_t twr = k.qlp_prime[nid];    // its row in the key (keys live at full QP width)
    const DModulus m = k.mod[twr];
    const size_t coeff = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t c2_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    KeyAcc acc;
    for (uint32_t i = 0; i < k.beta; i++) {
        const u64 *key = k.evks[i];
        const u64x2 v = *reinterpret_cast<const u64x2 *>(k.t_mod_up + (size_t)i * k.qlp_n + c2_id);
        acc.mac(v.x, v.y, *reinterpret_cast<const u64x2 *>(key + evk_id), *reinterpret_cast<const u64x2 *>(key + evk_id + k.qp_n));
    }
    u64x2 r0, r1;
    acc.reduce(m, r0, r1);
    inner_fix(k, nid, m, coeff, 0, r0, r1);
    *reinterpret_cast<u64x2 *>(k.cx + c2_id) = r0;
    *reinterpret_cast<u64x2 *>(k.cx + c2_id + k.qlp_n) = r1;
}

// Batch of ciphertexts against ONE key: the key limbs are read once and stay in registers while the kernel
// walks the ciphertexts (the inner product is HBM-bound and 2/3 of its bytes are the key).
// r06: the digits are read once and the sums written once, in a launch that moves 157 MB per ciphertext: nontemporal loads and
// stores (33.6 -> 32.0 us per op at B = 32; see EW_TENSOR_NT in pha_poly.hip).
template <int BETA>
__global__ __launch_bounds__(256) void inner_prod_batched_kernel(const InnerArgs k, uint32_t batch) {
    const uint32_t nid = blockIdx.y;
    const uint32_t twr = k.qlp_prime[nid];
    const DModulus m = k.mod[twr];
    const size_t coeff = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t c2_id = (size_t)nid * k.n + coeff;
    const size_t evk_id = (size_t)twr * k.n + coeff;
    u64x2 kb[BETA], ka[BETA];
#pragma unroll
    for (int i = 0; i < BETA; i++) {
        const u64 *key = k.evks[i];
        kb[i] = *reinterpret_cast<const u64x2 *>(key + evk_id);
        ka[i] = *reinterpret_cast<const u64x2 *>(key + evk_id + k.qp_n);
    }
    bool mine[BETA];   // (uniform) digit i holds this limb itself: its NTT form is c2's own
#pragma unroll
    for (int i = 0; i < BETA; i++) mine[i] = k.own != nullptr && nid < k.ql && nid >= (uint32_t)i * k.alpha && nid < ((uint32_t)i + 1) * k.alpha;
    if (k.fpinfo && k.fpinfo[twr].ok) {   // (uniform) r04: limbs below 2^50 -- every product an exact fp_mulmod_light (digits and key
        // words are canonical: a product is below 0.875 q, BETA <= 4 of them below 3.5 q), one fp_to_canon per sum: ~125 FP64
        // operations per ciphertext and thread where four 128-bit accumulators and four Barrett reductions take ~260
        const FpInfo fi = k.fpinfo[twr];
        const FpMod fm{fi.q, fi.qinv, false, false};
        double kbx[BETA], kby[BETA], kax[BETA], kay[BETA];
#pragma unroll
        for (int i = 0; i < BETA; i++) {
            kbx[i] = fp_from_canon(kb[i].x); kby[i] = fp_from_canon(kb[i].y);
            kax[i] = fp_from_canon(ka[i].x); kay[i] = fp_from_canon(ka[i].y);
        }
        for (uint32_t b = 0; b < batch; b++) {
            const u64 *mu = k.t_mod_up + (size_t)b * BETA * k.qlp_n + c2_id;
            const u64 *own = k.own + (size_t)b * k.own_stride + c2_id;
            u64 *cx = k.cx + (size_t)b * 2 * k.qlp_n + c2_id;
            double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
#pragma unroll
            for (int i = 0; i < BETA; i++) {
                const u64x2 v = gload2<true>(reinterpret_cast<const u64x2 *>(mine[i] ? own : mu + (size_t)i * k.qlp_n));
                const double vx = fp_from_canon(v.x), vy = fp_from_canon(v.y);
                a0 += fp_mulmod_light(vx, kbx[i], fm);
                a1 += fp_mulmod_light(vy, kby[i], fm);
                b0 += fp_mulmod_light(vx, kax[i], fm);
                b1 += fp_mulmod_light(vy, kay[i], fm);
            }
            u64x2 r0{fp_to_canon(a0, fm), fp_to_canon(a1, fm)};
            u64x2 r1{fp_to_canon(b0, fm), fp_to_canon(b1, fm)};
            inner_fix(k, nid, m, coeff, b, r0, r1);
            gstore2<true>(reinterpret_cast<u64x2 *>(cx), r0);
            gstore2<true>(reinterpret_cast<u64x2 *>(cx + k.qlp_n), r1);
        }
        return;
    }
    for (uint32_t b = 0; b < batch; b++) {
        const u64 *mu = k.t_mod_up + (size_t)b * BETA * k.qlp_n + c2_id;
        const u64 *own = k.own + (size_t)b * k.own_stride + c2_id;
        u64 *cx = k.cx + (size_t)b * 2 * k.qlp_n + c2_id;
        KeyAcc acc;
#pragma unroll
        for (int i = 0; i < BETA; i++) {
            const u64x2 v = gload2<true>(reinterpret_cast<const u64x2 *>(mine[i] ? own : mu + (size_t)i * k.qlp_n));
            acc.mac(v.x, v.y, kb[i], ka[i]);
        }
        u64x2 r0, r1;
        acc.reduce(m, r0, r1);
        inner_fix(k, nid, m, coeff, b, r0, r1);
        gstore2<true>(reinterpret_cast<u64x2 *>(cx), r0);
        gstore2<true>(reinterpret_cast<u64x2 *>(cx + k.qlp_n), r1);
    }
}


// ---- (cx - delta) * c element-wise: moddown_kernel rns_bconv.cu:680-689 and
//      divide_and_round_q_last_kernel rns.cu:1082-1108 (REDUCE_LAST) ---------------------------------
struct SubMulArgs {
    u64 *dst;
    const u64 *cx, *delta;
    const u64x2 *cst;  // per-limb constant (Shoup pair)
    const DModulus *mod;
    uint32_t n;
    // polynomial blockIdx.z of a batch: element strides (0 for a single polynomial)
    size_t dst_stride = 0, cx_stride = 0, delta_stride = 0;
    uint32_t accumulate = 0;   // dst += result (the add_to_ct_kernel of keyswitch_inplace, rns_bconv.cu:763-769, fused)
};
template <bool REDUCE_LAST>
__global__ __launch_bounds__(256) void sub_mul_kernel(const SubMulArgs k) {
    const uint32_t limb = blockIdx.y;
    const DModulus m = k.mod[limb];
    const u64x2 cst = k.cst[limb];
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const u64 *delta = k.delta + (size_t)blockIdx.z * k.delta_stride;
    const u64 *cx = k.cx + (size_t)blockIdx.z * k.cx_stride;
    u64 *dst = k.dst + (size_t)blockIdx.z * k.dst_stride;
    u64 d = REDUCE_LAST ? barrett64(delta[coeff], m.value, m.ratio1) : delta[(size_t)limb * k.n + coeff];
    const u64 t = sub_mod(cx[(size_t)limb * k.n + coeff], d, m.value);
    u64 r = shoup(t, cst, m.value);
    if (k.accumulate) r = add_mod(dst[(size_t)limb * k.n + coeff], r, m.value);
    dst[(size_t)limb * k.n + coeff] = r;
}

// ---- BGV (plain modulus t): base_P_to_t_conv (rns.cu:283) as one thread per coefficient, writing over
//      the first P limb it has just read; bgv_moddown_kernel rns_bconv.cu:636-652;
//      bgv_mod_t_divide_q_kernel rns.cu:1186-1208 ---------------------------------------------------
struct PToTArgs {
    u64 *cx_p;                 // P block of polynomial 0: [alpha][N]; limb 0 receives [.]_t
    size_t stride;             // elements between polynomials (blockIdx.y)
    const u64x2 *hat_inv;      // [alpha] phat_i^-1 mod p_i
    const uint32_t *iprime;    // [alpha] rows of the QP table
    const u64 *hat_mod_t;      // [alpha] phat_i mod t
    const DModulus *mod;
    DModulus t;
    uint32_t isz, n;
};
__global__ __launch_bounds__(256) void p_to_t_kernel(const PToTArgs k) {
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    u64 *p = k.cx_p + (size_t)blockIdx.y * k.stride + coeff;
    u64 lo = 0, hi = 0;
    for (uint32_t i = 0; i < k.isz; i++) {
        const u64 x = shoup(p[(size_t)i * k.n], k.hat_inv[i], k.mod[k.iprime[i]].value);
        mac128(x, k.hat_mod_t[i], lo, hi);
    }
    p[0] = barrett128(lo, hi, k.t);
}

struct BgvDownArgs {
    u64 *dst;
    const u64 *cx, *delta, *cp_t;
    const u64x2 *p_mod_q, *pinv;
    const DModulus *mod;
    u64x2 pinv_t;
    u64 t;
    uint32_t n;
    size_t dst_stride = 0, cx_stride = 0, delta_stride = 0;   // polynomial blockIdx.z of a batch (cp_t moves with cx)
};
__global__ __launch_bounds__(256) void bgv_moddown_kernel(const BgvDownArgs k) {
    const uint32_t limb = blockIdx.y;
    const u64 q = k.mod[limb].value;
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const size_t id = (size_t)limb * k.n + coeff;
    const size_t z = blockIdx.z;
    const u64 u = shoup(k.cp_t[z * k.cx_stride + coeff], k.pinv_t, k.t);
    const u64 corr = shoup(u, k.p_mod_q[limb], q);
    const u64 d = add_mod(sub_mod(k.cx[z * k.cx_stride + id], k.delta[z * k.delta_stride + id], q), corr, q);
    k.dst[z * k.dst_stride + id] = shoup(d, k.pinv[limb], q);
}

struct BgvSwitchArgs {
    u64 *dst;
    const u64 *src;            // polynomial 0: [ql][N] in coefficient form
    const u64x2 *q_last_mod_q, *inv_q_last;
    const DModulus *mod;
    u64x2 inv_q_last_t;
    DModulus t;
    uint32_t n, nl;
    size_t src_stride, dst_stride;
};
__global__ __launch_bounds__(256) void bgv_switch_kernel(const BgvSwitchArgs k) {
    const uint32_t limb = blockIdx.y;
    const DModulus m = k.mod[limb];
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const u64 *in = k.src + (size_t)blockIdx.z * k.src_stride;
    const u64 last = in[(size_t)k.nl * k.n + coeff];
    const u64 delta = barrett64(last, m.value, m.ratio1);
    const u64 last_t = barrett64(last, k.t.value, k.t.ratio1);
    const u64 u = shoup(last_t, k.inv_q_last_t, k.t.value);
    const u64 corr = shoup(u, k.q_last_mod_q[limb], m.value);
    const u64 d = add_mod(sub_mod(in[(size_t)limb * k.n + coeff], delta, m.value), corr, m.value);
    k.dst[(size_t)blockIdx.z * k.dst_stride + (size_t)limb * k.n + coeff] = shoup(d, k.inv_q_last[limb], m.value);
}

// ---- pha_keyswitch_mod_switch: BGV key switch + mod_switch_to_next in one.  The mod-down's forward transform, the add to ct and
//      the switch's inverse transform cancel (iNTT(ct + NTT(w)) = iNTT(ct) + w, word for word: every stored word is the canonical
//      residue), so ct is folded into the extended-base sums in NTT form and ONE kernel does the work of p_to_t_kernel,
//      bgv_moddown_kernel and bgv_switch_kernel in coefficient form. ------------------------------------------------------------
struct BgvFoldArgs {
    u64 *cx;                   // [polys][QlP][N], NTT form: limbs j < Ql receive cx_j + (P mod q_j) * ct_j
    const u64 *ct;             // [polys][Ql][N], only read
    const u64x2 *p_mod_q;
    const DModulus *mod;
    uint32_t n;
    size_t cx_stride, ct_stride;
};
// two coefficients per thread (16-byte loads and stores); limb = blockIdx.y, polynomial = blockIdx.z
__global__ __launch_bounds__(256) void bgv_fold_ct_kernel(const BgvFoldArgs k) {
    const uint32_t limb = blockIdx.y;
    const u64 q = k.mod[limb].value;
    const u64x2 p = k.p_mod_q[limb];
    const size_t id = (size_t)limb * k.n + ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    u64x2 *cx = reinterpret_cast<u64x2 *>(k.cx + (size_t)blockIdx.z * k.cx_stride + id);
    const u64x2 a = *reinterpret_cast<const u64x2 *>(k.ct + (size_t)blockIdx.z * k.ct_stride + id);
    u64x2 v = *cx;
    v.x = add_mod(v.x, shoup(a.x, p, q), q);
    v.y = add_mod(v.y, shoup(a.y, p, q), q);
    *cx = v;
}

struct BgvDownSwitchArgs {
    u64 *dst;                  // [polys][Ql-1][N], coefficient form
    const u64 *cx;             // [polys][QlP][N], coefficient form (ct folded in)
    const u64 *delta;          // [polys][Ql][N]: the P -> Ql conversion of cx's P limbs
    size_t dst_stride, cx_stride, delta_stride;
    const u64x2 *hat_inv;      // the constants of p_to_t_kernel, bgv_moddown_kernel and bgv_switch_kernel
    const uint32_t *iprime;
    const u64 *hat_mod_t;
    const u64x2 *p_mod_q, *pinv, *q_last_mod_q, *inv_q_last;
    const DModulus *mod;
    DModulus t;
    u64x2 pinv_t, inv_q_last_t;
    uint32_t n, ql, alpha, per_group;   // output limbs [blockIdx.y * per_group, +per_group) of [0, ql - 1)
};
// bgv_moddown_kernel's word of one limb: (cx - delta + u (P mod q)) P^-1 mod q
__device__ __forceinline__ u64 bgv_down_word(const BgvDownSwitchArgs &k, uint32_t limb, u64 q, u64 cx, u64 delta, u64 u) {
    const u64 corr = shoup(u, k.p_mod_q[limb], q);
    return shoup(add_mod(sub_mod(cx, delta, q), corr, q), k.pinv[limb], q);
}
// two coefficients per thread, polynomial = blockIdx.z; a thread walks the output limbs of its group, so the alpha + 2 reads
// behind u, v_last and u' are made once per group
__global__ __launch_bounds__(256) void bgv_down_switch_kernel(const BgvDownSwitchArgs k) {
    const size_t coeff = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    const u64 *cx = k.cx + (size_t)blockIdx.z * k.cx_stride + coeff;
    const u64 *delta = k.delta + (size_t)blockIdx.z * k.delta_stride + coeff;
    u64 *dst = k.dst + (size_t)blockIdx.z * k.dst_stride + coeff;
    const uint32_t nl = k.ql - 1;
    // [cx_P]_t (base_P_to_t_conv) and u = [cx_P]_t P^-1 mod t
    u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    for (uint32_t i = 0; i < k.alpha; i++) {
        const u64 p = k.mod[k.iprime[i]].value;
        const u64x2 h = k.hat_inv[i];
        const u64x2 x = *reinterpret_cast<const u64x2 *>(cx + (size_t)(k.ql + i) * k.n);
        mac128(shoup(x.x, h, p), k.hat_mod_t[i], lo0, hi0);
        mac128(shoup(x.y, h, p), k.hat_mod_t[i], lo1, hi1);
    }
    const u64 tv = k.t.value;
    const u64 u0 = shoup(barrett128(lo0, hi0, k.t), k.pinv_t, tv), u1 = shoup(barrett128(lo1, hi1, k.t), k.pinv_t, tv);
    // the last limb of ct + keyswitch(c2) in coefficient form, and u' = (v_last mod t) q_last^-1 mod t
    const u64 q_last = k.mod[nl].value;
    const u64x2 cl = *reinterpret_cast<const u64x2 *>(cx + (size_t)nl * k.n);
    const u64x2 dl = *reinterpret_cast<const u64x2 *>(delta + (size_t)nl * k.n);
    const u64 last0 = bgv_down_word(k, nl, q_last, cl.x, dl.x, u0), last1 = bgv_down_word(k, nl, q_last, cl.y, dl.y, u1);
    const u64 s0 = shoup(barrett64(last0, tv, k.t.ratio1), k.inv_q_last_t, tv);
    const u64 s1 = shoup(barrett64(last1, tv, k.t.ratio1), k.inv_q_last_t, tv);
    const uint32_t j0 = blockIdx.y * k.per_group, j1 = min(j0 + k.per_group, nl);
    for (uint32_t j = j0; j < j1; j++) {
        const DModulus m = k.mod[j];
        const u64 q = m.value;
        const u64x2 c = *reinterpret_cast<const u64x2 *>(cx + (size_t)j * k.n);
        const u64x2 d = *reinterpret_cast<const u64x2 *>(delta + (size_t)j * k.n);
        const u64x2 qlm = k.q_last_mod_q[j], iql = k.inv_q_last[j];
        const u64 w0 = bgv_down_word(k, j, q, c.x, d.x, u0), w1 = bgv_down_word(k, j, q, c.y, d.y, u1);
        u64x2 r;
        r.x = shoup(add_mod(sub_mod(w0, barrett64(last0, q, m.ratio1), q), shoup(s0, qlm, q), q), iql, q);
        r.y = shoup(add_mod(sub_mod(w1, barrett64(last1, q, m.ratio1), q), shoup(s1, qlm, q), q), iql, q);
        *reinterpret_cast<u64x2 *>(dst + (size_t)j * k.n) = r;
    }
}

// ---- key-switching key generation, arithmetic part (src/secretkey.cu:232-341): per digit d and limb j of QP
//      b = -(a*s + u) [multiply_and_add_negate_rns_poly polymath.cu:234-251], and on the digit's own limbs
//      b += P * new_key [multiply_temp_mod_and_add_rns_poly polymath.cu:318-338]; the key is (b, a). ----
struct KeyGenArgs {
    u64 *const *evk;        // device array [dnum] of keys [2][QP][N]
    const u64 *sk;          // [QP][N] NTT form
    const u64 *new_key;     // [Q][N] NTT form
    const u64 *a, *u;       // [dnum][QP][N]: uniform part, noise in NTT form
    const u64x2 *p_mod_q;   // [Q]
    const DModulus *mod;
    uint32_t n, size_qp, alpha;
};
__global__ __launch_bounds__(256) void kswitch_key_kernel(const KeyGenArgs k) {
    const uint32_t limb = blockIdx.y, d = blockIdx.z;
    const DModulus m = k.mod[limb];
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const size_t id = (size_t)limb * k.n + coeff, did = (size_t)d * k.size_qp * k.n + id;
    const u64 a = k.a[did];
    u64 b = neg_mod(add_mod(mul_mod(a, k.sk[id], m), k.u[did], m.value), m.value);
    if (limb >= d * k.alpha && limb < (d + 1) * k.alpha)
        b = add_mod(b, shoup(k.new_key[id], k.p_mod_q[limb], m.value), m.value);
    u64 *key = k.evk[d];
    key[id] = b;
    key[(size_t)k.size_qp * k.n + id] = a;
}
__global__ __launch_bounds__(256) void scale_by_t_kernel(u64 *e, const DModulus *mod, u64 t, uint32_t n, size_t stride) {
    const DModulus m = mod[blockIdx.y];
    const size_t id = (size_t)blockIdx.z * stride + (size_t)blockIdx.y * n + blockIdx.x * 256 + threadIdx.x;
    e[id] = mul_mod(e[id], barrett64(t, m.value, m.ratio1), m);
}

// ---- Galois (src/galois.cu:11-39) ----------------------------------------------------------------
// elt^-1 mod 2n for an odd elt (Newton: x <- x (2 - elt x) doubles the correct low bits)
static uint32_t inv_mod_2n(uint32_t elt, size_t n) {
    uint32_t x = elt;                      // correct to 3 bits: elt^2 = 1 mod 8
    for (int i = 0; i < 5; i++) x *= 2 - elt * x;
    return x & (uint32_t)(2 * n - 1);
}
__global__ __launch_bounds__(256) void galois_ntt_kernel(u64 *dst, const u64 *src, const uint32_t *table, uint32_t n) {
    const uint32_t limb = blockIdx.y;
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    dst[(size_t)limb * n + coeff] = src[(size_t)limb * n + table[coeff]];
}
// blockIdx.z = polynomial of a batch (stride = gridDim.y limbs)
__global__ __launch_bounds__(256) void galois_coeff_kernel(u64 *dst, const u64 *src, const DModulus *mod,
                                                           uint32_t mod_start, uint32_t elt_inv, uint32_t n) {
    const uint32_t limb = blockIdx.z * gridDim.y + blockIdx.y;
    const u64 q = mod[mod_start + blockIdx.y].value;
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    // index_raw = c * galois_elt mod 2n sends coefficient c to position index_raw mod n, negated when index_raw >= n
    // (include/galois.cuh:115-130).  As a gather (contiguous stores): position `coeff` comes from c = coeff * elt^-1 mod 2n, from
    // c - n and negated when c >= n; `elt_inv` = elt^-1 mod 2n (inv_mod_2n below)
    const uint32_t c = (uint32_t)(((u64)coeff * elt_inv) & (2 * (u64)n - 1));
    u64 v = src[(size_t)limb * n + (c & (n - 1))];
    if (c >= n) v = neg_mod(v, q);
    dst[(size_t)limb * n + coeff] = v;
}

void launch_galois_coeff(Context &c, u64 *dst, const u64 *src, uint32_t galois_elt, size_t cms, size_t mod_start, size_t polys,
                         hipStream_t s) {
    hipLaunchKernelGGL(galois_coeff_kernel, dim3((unsigned)(c.n / 256), (unsigned)cms, (unsigned)polys), dim3(256), 0, s, dst, src,
                       c.d_mod.p, (uint32_t)mod_start, inv_mod_2n(galois_elt, c.n), (uint32_t)c.n);
    check_launch();
}

// Galois automorphism of a batch of size-2 ciphertexts laid out for the key switch that follows it (rotate_internal /
// apply_galois_inplace, src/evaluate.cu:1567-1624): polynomial 0 goes to dst_ct[b][0], dst_ct[b][1] is zeroed and polynomial 1
// goes to the dense key-switch operand dst_c2[b] -- one kernel instead of permutation + memset + two strided copies.
// blockIdx.z = 2 b + p.  `table` != null: NTT-domain gather; null: coefficient-domain scatter with sign (galois.cu:11-39).
// (`elt` is the element for the table form and its inverse mod 2n for the coefficient form: see the gather below.)
// `add` != null: the automorphism is applied to src + add (mod q), add being polynomial p of ciphertext b at add + (b * add_ct_polys
// + p) * Ql * N -- the sum ct + keyswitch(c2) of a relinearization that was never stored (pha_relinearize_rotate_batched).
__global__ __launch_bounds__(256) void galois_split_kernel(u64 *dst_ct, u64 *dst_c2, const u64 *src, const uint32_t *table,
                                                           const DModulus *mod, uint32_t elt, uint32_t n, uint32_t ql,
                                                           const u64 *add, uint32_t add_ct_polys) {
    const uint32_t limb = blockIdx.y, b = blockIdx.z >> 1, p = blockIdx.z & 1;
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const u64 *in = src + ((size_t)(2 * b + p) * ql + limb) * n;
    const u64 *in2 = add ? add + ((size_t)(add_ct_polys * b + p) * ql + limb) * n : nullptr;
    u64 *out = p ? dst_c2 + ((size_t)b * ql + limb) * n : dst_ct + ((size_t)(2 * b) * ql + limb) * n;
    if (!p) dst_ct[((size_t)(2 * b + 1) * ql + limb) * n + coeff] = 0;
    const u64 q = mod[limb].value;
    if (table) {
        const uint32_t from = table[coeff];
        u64 v = in[from];
        if (in2) v = add_mod(v, in2[from], q);
        out[coeff] = v;
    } else {
        // X -> X^elt sends coefficient c to position c elt mod n with the sign of (c elt mod 2n) >= n (galois.cu:11-39).  Written
        // as a gather: output `coeff` comes from c = coeff elt^-1 mod 2n (c >= n: from c - n, negated), so the stores of a
        // wavefront are one contiguous run and the scattered side is the loads, which the limb's 256-512 KB in L2 absorb;
        // `elt` holds elt^-1 mod 2n here (the launcher inverts it)
        const uint32_t c = (uint32_t)(((u64)coeff * elt) & (2 * (u64)n - 1));
        const uint32_t from = c & (n - 1);
        u64 v = in[from];
        if (in2) v = add_mod(v, in2[from], q);
        if (c >= n) v = neg_mod(v, q);
        out[coeff] = v;
    }
}


// ------------------------------------------------------------------------------------------------
// drivers
// ------------------------------------------------------------------------------------------------
// fused_ip may be passed to modup (pha_internal.h) only for the shapes that have a fused form
static bool fusable_ip(Context &c, Tool &t) { return t.alpha > 1 && c.log_n >= 14 && c.log_n <= 17 && t.beta <= 4; }
// r06: batched key switches of the NTT-form schemes leave the digits' own limbs where they are (modup's own_in_place + InnerArgs::own):
// the batched inner product kernel is the one that knows how to read them from c2
static bool own_in_place_ok(const Tool &t, int scheme, uint32_t batch) {
    return (scheme == PHA_SCHEME_CKKS || scheme == PHA_SCHEME_BGV) && batch > 1 && t.alpha > 1 && t.beta <= 4;
}
// (described with its declaration in pha_internal.h)
void modup(Context &c, Tool &t, u64 *dst, const u64 *cks, int scheme, u64 *t_cks, hipStream_t s, uint32_t batch, size_t cks_stride,
           const ModupIpArgs *fused_ip, bool own_in_place) {
    const size_t n = c.n;
    const uint32_t ql = t.size_ql, qlp = t.size_qlp, alpha = t.alpha;
    const bool ntt_dom = ntt_domain_scheme(scheme);
    if (!cks_stride) cks_stride = (size_t)ql * n;
    if (ntt_dom) {
        NttExtra x;
        x.batch = batch;
        x.poly_stride = (size_t)ql * n;
        x.in_stride = cks_stride;
        if (alpha == 1) {
            ntt_inverse(c, cks, t_cks, t_cks, plain_sel(0, ql), EPI_INV_CANON, x, s);
        } else {
            // iNTT fused with x partQlHatInv (bconv phase 1), :558-559
            x.scale = t.part_hat_inv.p;
            x.scale_shoup = t.part_hat_inv_shoup.p;
            ntt_inverse(c, cks, t_cks, t_cks, plain_sel(0, ql), EPI_INV_SCALE, x, s);
        }
    }
    if (alpha == 1) {
        for (uint32_t g = 0; g < batch; g++)
            for (uint32_t b = 0; b < t.beta; b++) {
                const size_t off = (size_t)g * ql * n + (size_t)b * n, off_c = (size_t)g * cks_stride + (size_t)b * n;
                u64 *out = dst + ((size_t)g * t.beta + b) * qlp * n;
                SinglePArgs k{out, cks + off_c, ntt_dom ? t_cks + off : cks + off_c, c.d_mod.p, t.d_qlp_prime.p, b, (uint32_t)n};
                hipLaunchKernelGGL(single_p_kernel, dim3((unsigned)(n / 256), qlp), dim3(256), 0, s, k);
                check_launch();
            }
    }
    LimbSel sel = special_sel(0, qlp, c.size_qp, c.size_p);
    NttExtra x;
    x.batch = t.beta * batch;
    x.poly_stride = (size_t)qlp * n;
    if (ntt_dom) {  // digit z % beta skips [d*alpha, min((d+1)*alpha, ql))
        sel.excl_start = 0;
        sel.excl_end = alpha;
        x.excl_step = alpha;
        x.excl_limit = ql;
        x.excl_mod = batch > 1 ? t.beta : 0;
    }
    if (alpha > 1) {
        // own limbs are copied verbatim by the same kernel (modup_copy_partQl_kernel :522-528);
        // BFV still needs the q-hat^-1 scaling (bconv_mult_kernel :603-607), ckks/bgv got it in the iNTT
        // r05: NTT-form input, N = 2^16, the separate (batched) inner product: the conversion is the load of the forward
        // transform's strided pass (modup_conv_strided, pha_ntt.hip); the transform then runs its contiguous pass only
        if (ntt_dom && !fused_ip) {
            const ModupConvArgs mc{t.d_digit_convs.p, t.beta, t_cks, (size_t)ql * n, own_in_place ? nullptr : cks, cks_stride, alpha, t.modup_max_osz, t.modup_mont30};
            if (modup_conv_strided(c, dst, sel, x, mc, s)) {
                x.first_pass_done = true;
                ntt_forward(c, dst, dst, dst, sel, EPI_FWD_CANON, x, s);
                return;
            }
        }
        // (coefficient-form input: the conversion reads c2 itself, at its own stride; NTT form: the dense t_cks, and c2 only
        //  for the verbatim copy of the digit's own limbs)
        // (fused inner product, NTT-form input: the own limbs are read from c2 by the fused pass, no copy)
        BConvCall k = bconv_call(t);
        k.polys = t.beta * batch; k.dst = dst; k.dst_stride = (size_t)qlp * n;
        k.src = ntt_dom ? t_cks : cks; k.scale_in = !ntt_dom;   // (every digit of a ciphertext reads the same polynomial: no src_stride)
        k.own = ((fused_ip || own_in_place) && ntt_dom) ? nullptr : cks;
        k.conv_count = batch > 1 ? t.beta : 0; k.group_stride = ntt_dom ? (size_t)ql * n : cks_stride; k.own_group_stride = cks_stride;
        launch_bconv(c, k, s);
    }
    if (fused_ip) {
        ModupIpArgs ip = *fused_ip;
        ip.own = ntt_dom ? cks : nullptr;
        if (!modup_ntt_inner_prod(c, dst, sel, x, t.beta, ip, s)) throw std::logic_error("fused inner product requested for a shape without one");
        return;
    }
    ntt_forward(c, dst, dst, dst, sel, EPI_FWD_CANON, x, s);
}

// The fused-rescale fix-up fields of InnerArgs / ModupIpArgs (pha_keyswitch_rescale): the last data limb of cx receives
// ct_last + cx_last * P^-1; fix_ct = null: off
template <class Args>
static void set_last_limb_fix(Context &c, Tool &t, const u64 *fix_ct, Args &k) {
    k.fix_limb = 0xffffffffu;
    if (!fix_ct) return;
    const u64 pinv_last = t.h_pinv[t.size_ql - 1];   // P^-1 mod q_last (bigPInv_mod_q rns.cu:110-123)
    k.fix_limb = t.size_ql - 1;
    k.fix_cst = u64x2{pinv_last, h_shoup(pinv_last, c.primes[t.size_ql - 1])};
    k.fix_ct = fix_ct;
    k.fix_ct_stride = (size_t)t.size_ql * c.n;
}

// phantom::key_switch_inner_prod eval_key_switch.cu:71-92
// fix_ct != null (pha_keyswitch_rescale): cx's last data limb receives ct_last + cx_last * P^-1 (see InnerArgs)
static void inner_prod(Context &c, Tool &t, u64 *cx, const u64 *t_mod_up, const u64 *const *rlk, hipStream_t s, uint32_t batch = 1,
                       const u64 *fix_ct = nullptr, const u64 *own = nullptr, size_t own_stride = 0) {
    InnerArgs k{};
    k.cx = cx; k.t_mod_up = t_mod_up; k.evks = rlk; k.mod = c.d_mod.p; k.qlp_prime = t.d_qlp_prime.p;
    k.n = (uint32_t)c.n; k.beta = t.beta; k.qlp_n = (size_t)t.size_qlp * c.n; k.qp_n = (size_t)c.size_qp * c.n;
    set_last_limb_fix(c, t, fix_ct, k);
    k.fpinfo = c.d_fpinfo.p;
    if (own && !(batch > 1 && t.beta <= 4)) throw std::logic_error("inner_prod: own limbs in place need the batched kernel");
    k.own = own; k.own_stride = own_stride; k.alpha = t.alpha; k.ql = t.size_ql;
    const dim3 grid((unsigned)(c.n / 512), t.size_qlp), block(256);
    if (batch > 1 && t.beta <= 4) {  // key limbs stay in registers across the ciphertexts
        with_beta<4>(t.beta, [&](auto B) { hipLaunchKernelGGL(inner_prod_batched_kernel<decltype(B)::value>, grid, block, 0, s, k, batch); });
        check_launch();
        return;
    }
    for (uint32_t b = 0; b < batch; b++) {
        hipLaunchKernelGGL(inner_prod_kernel, grid, block, 0, s, k);
        check_launch();
        k.t_mod_up += (size_t)t.beta * k.qlp_n;
        k.cx += 2 * k.qlp_n;
        if (k.fix_ct) k.fix_ct += 2 * k.fix_ct_stride;
    }
}

// mod-up + inner product of B ciphertexts, c2 at c2 + b * c2_stride: k.cx from c2 (pha_internal.h: the hybrid key switch).  ONE
// ciphertext takes the fused form where the shape has one, everything else the two steps; a batch of an NTT-form scheme leaves the
// digits' own limbs where they are (modup's own_in_place) and its inner product reads them from c2 (InnerArgs::own).  fix_ct as in
// inner_prod.
// fold_inverse (ckks forms): the fused kernel also runs the contiguous pass of the mod-down's inverse transform on the special limbs
// (and on the last data limb when fix_ct is given, the fused rescale); returns true when it did -- the caller then launches that
// inverse with NttExtra::second_pass_only.
static bool modup_inner_prod(Context &c, Tool &t, const KsScratch &k, const u64 *c2, size_t c2_stride, const u64 *const *keys, int scheme,
                             uint32_t B, hipStream_t s, const u64 *fix_ct = nullptr, bool fold_inverse = false) {
    if (B == 1 && fusable_ip(c, t)) {
        ModupIpArgs ip{};
        ip.cx = k.cx; ip.evks = keys; ip.qlp_n = (size_t)t.size_qlp * c.n; ip.qp_n = (size_t)c.size_qp * c.n;
        set_last_limb_fix(c, t, fix_ct, ip);
        if (fold_inverse) {
            ip.inv_from = t.size_ql;
            ip.inv_lead = fix_ct ? t.size_ql - 1 : 0xffffffffu;
            ip.itw = c.d_itw.p;
            ip.itwf = c.d_itwf.p;
        }
        modup(c, t, k.t_mod_up, c2, scheme, k.tmp, s, 1, 0, &ip);
        return ip.inv_from != 0xffffffffu;
    }
    const bool in_place = own_in_place_ok(t, scheme, B);
    modup(c, t, k.t_mod_up, c2, scheme, k.tmp, s, B, c2_stride, nullptr, in_place);
    inner_prod(c, t, k.cx, k.t_mod_up, keys, s, B, fix_ct, in_place ? c2 : nullptr, c2_stride);
    return false;
}

// The mod-down's P -> Ql step on `polys` coefficient-form polynomials cx + z * cx_stride ([Ql || P] limbs): delta [polys][Ql][N].
// alpha = 1 is a copy with a reduction (rns_bconv.cu:691-707), anything else the conversion; epi rides on the conversion only.
static void p_to_ql_delta(Context &c, Tool &t, u64 *delta, const u64 *cx, size_t cx_stride, uint32_t polys, bool scale_in,
                          const BConvEpilogue *epi, hipStream_t s) {
    const size_t n = c.n, d_stride = (size_t)t.size_ql * n;
    if (t.alpha == 1) {
        for (uint32_t z = 0; z < polys; z++) {
            SinglePArgs k{delta + z * d_stride, nullptr, cx + z * cx_stride + d_stride, c.d_mod.p, t.d_qlp_prime.p, t.size_ql, (uint32_t)n};
            hipLaunchKernelGGL(single_p_kernel, dim3((unsigned)(n / 256), t.size_ql), dim3(256), 0, s, k);
            check_launch();
        }
        return;
    }
    BConvCall k = bconv_call(t.p_to_ql);
    k.polys = polys; k.dst = delta; k.dst_stride = d_stride; k.src = cx; k.src_stride = cx_stride;
    k.scale_in = scale_in; k.epi = epi;
    launch_bconv(c, k, s);
}

// (described with its declaration in pha_internal.h)
void moddown_from_ntt(Context &c, Tool &t, u64 *ct, size_t ct_stride, u64 *cx, size_t cx_stride, uint32_t polys, int scheme,
                      bool accumulate, u64 *delta, hipStream_t s, bool folded, bool coeff_input) {
    const size_t n = c.n;
    const uint32_t ql = t.size_ql, qlp = t.size_qlp;
    NttExtra xb;
    xb.batch = polys;
    xb.poly_stride = cx_stride;
    // ckks, alpha > 1: bconv phase 1 (x phat_i^-1 mod p_i, bconv_mult_kernel rns_bconv.cu:22-33) rides on the
    // inverse NTT's last round, exactly as mod-up does (:558-559); the conversion then skips its own scaling
    const bool prescaled = scheme == PHA_SCHEME_CKKS && t.alpha > 1;
    if (folded && scheme != PHA_SCHEME_CKKS) throw std::logic_error("folded inverse pass outside the ckks mod-down");
    xb.second_pass_only = folded;
    if (prescaled) {
        xb.scale = t.p_hat_inv_by_limb.p;
        xb.scale_shoup = t.p_hat_inv_by_limb_shoup.p;
        ntt_inverse(c, cx, cx, cx, special_sel(ql, c.size_p, c.size_qp, c.size_p), EPI_INV_SCALE, xb, s);
    } else if (scheme == PHA_SCHEME_CKKS)
        ntt_inverse(c, cx, cx, cx, special_sel(ql, c.size_p, c.size_qp, c.size_p), EPI_INV_CANON, xb, s);
    else if (scheme == PHA_SCHEME_BFV && coeff_input)
        ;   // (rns_bconv.cu:722-730 transforms ckks and bgv only)
    else if (scheme == PHA_SCHEME_BFV || scheme == PHA_SCHEME_BGV)
        ntt_inverse(c, cx, cx, cx, special_sel(0, qlp, c.size_qp, c.size_p), EPI_INV_CANON, xb, s);
    else
        throw std::invalid_argument("unsupported scheme");
    if (coeff_input && scheme != PHA_SCHEME_BFV) throw std::logic_error("coefficient-form mod-down input outside bfv");
    if (scheme == PHA_SCHEME_BGV && !t.bgv_ready)
        throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
    const size_t d_stride = (size_t)ql * n;
    bool bfv_epilogue_fused = false, ckks_conv_fused = false;
    // r06, CKKS batches at N = 2^16 with the prescaled inputs: the P -> Ql conversion is the LOAD of the forward transform's strided
    // pass (mod-down form of modup_conv_s1_kernel, pha_ntt.hip): delta is never written in coefficient form
    if (prescaled && polys > 1 && t.p_to_ql.mont30()) {
        NttExtra xf;
        xf.batch = polys;
        xf.poly_stride = d_stride;
        ModupConvArgs mc{t.p_to_ql.dev.p, 1, cx, cx_stride, nullptr, 0, t.alpha, ql, true, nullptr};
        mc.moddown = true;
        ckks_conv_fused = modup_conv_strided(c, delta, plain_sel(0, ql), xf, mc, s);
    }
    if (!ckks_conv_fused) {
        // BFV: (cx - delta) * P^-1 (+ add_to_ct) rides on the conversion's output loop, delta is never stored -- for the
        // register-resident converter (1 < alpha <= 32); a wider P takes the conversion into delta and the element-wise kernel below
        const BConvEpilogue e{cx, ct, t.pinv2.p, cx_stride, ct_stride, accumulate};
        bfv_epilogue_fused = scheme == PHA_SCHEME_BFV && t.alpha > 1 && t.alpha <= 32;
        p_to_ql_delta(c, t, delta, cx, cx_stride, polys, !prescaled, bfv_epilogue_fused ? &e : nullptr, s);
    }
    if (scheme == PHA_SCHEME_BGV) {
        // [cx_P]_t lands in the first P limb of each polynomial, then the t-corrected division and the NTT
        PToTArgs pk{cx + (size_t)ql * n, cx_stride, t.p_to_ql.hat_inv.p, t.p_to_ql.d_iprime.p, t.p_hat_mod_t.p,
                    c.d_mod.p, t.t_mod, t.alpha, (uint32_t)n};
        hipLaunchKernelGGL(p_to_t_kernel, dim3((unsigned)(n / 256), polys), dim3(256), 0, s, pk);
        check_launch();
        {   // every polynomial in one launch
            BgvDownArgs k{accumulate ? delta : ct, cx, delta, cx + (size_t)ql * n, t.p_mod_q2.p, t.pinv2.p, c.d_mod.p,
                          t.pinv_mod_t, t.t_mod.value, (uint32_t)n};
            k.dst_stride = accumulate ? d_stride : ct_stride;
            k.cx_stride = cx_stride;
            k.delta_stride = d_stride;
            hipLaunchKernelGGL(bgv_moddown_kernel, dim3((unsigned)(n / 256), ql, polys), dim3(256), 0, s, k);
            check_launch();
        }
        NttExtra x;
        x.batch = polys;
        x.poly_stride = accumulate ? d_stride : ct_stride;
        u64 *buf = accumulate ? delta : ct;
        ntt_forward(c, buf, buf, buf, plain_sel(0, ql), EPI_FWD_CANON, x, s);
        if (accumulate)
            for (uint32_t z = 0; z < polys; z++)
                launch_add(c, ct + z * ct_stride, delta + z * d_stride, ct + z * ct_stride, ql, 0, s);
    } else if (scheme == PHA_SCHEME_CKKS) {
        NttExtra x;  // NTT(delta) fused with (cx - .) * P^-1 (ntt_moddown.cu:106-261)
        x.scale = t.pinv.p;
        x.scale_shoup = t.pinv_shoup.p;
        x.aux = cx;
        x.batch = polys;
        x.poly_stride = d_stride;
        x.out_stride = ct_stride;
        x.aux_stride = cx_stride;
        x.first_pass_done = ckks_conv_fused;   // the conversion already ran as the load of this transform's strided pass
        ntt_forward(c, delta, delta, ct, plain_sel(0, ql), accumulate ? EPI_FWD_MODDOWN_ADD : EPI_FWD_MODDOWN, x, s);
    } else if (!bfv_epilogue_fused) {
        // BFV, alpha = 1 or alpha > 32 (moddown_kernel rns_bconv.cu:680-689): every polynomial in ONE launch,
        // ct (+)= (cx - delta) * P^-1 (for 1 < alpha <= 32 this already happened inside the base conversion above)
        SubMulArgs k{ct, cx, delta, t.pinv2.p, c.d_mod.p, (uint32_t)n};
        k.dst_stride = ct_stride;
        k.cx_stride = cx_stride;
        k.delta_stride = d_stride;
        k.accumulate = accumulate ? 1 : 0;
        hipLaunchKernelGGL(sub_mul_kernel<false>, dim3((unsigned)(n / 256), ql, polys), dim3(256), 0, s, k);
        check_launch();
    }
}

// keyswitch_inplace eval_key_switch.cu:95-182 on B ciphertexts: dst [B][2][Ql][N] (+)= keyswitch(c2 + b * c2_stride); accumulate adds
// to what dst holds (ct += ..., the add fused into the mod-down's epilogue).  dst and k.cx are uniformly strided over the 2 B polynomials.
static void keyswitch(Context &c, Tool &t, const KsScratch &k, u64 *dst, bool accumulate, const u64 *c2, size_t c2_stride,
                      const u64 *const *keys, int scheme, uint32_t B, hipStream_t s) {
    const bool folded = modup_inner_prod(c, t, k, c2, c2_stride, keys, scheme, B, s, nullptr, scheme == PHA_SCHEME_CKKS && B == 1);
    moddown_from_ntt(c, t, dst, (size_t)t.size_ql * c.n, k.cx, (size_t)t.size_qlp * c.n, 2 * B, scheme, accumulate, k.tmp, s, folded);
}

// DRNSTool::divide_and_round_q_last_ntt rns.cu:1160-1184 on `polys` polynomials src [polys][Ql][N] -> dst [polys][Ql-1][N]
static void rescale_ntt(Context &c, Tool &t, u64 *src, uint32_t polys, u64 *dst, hipStream_t s) {
    const size_t n = c.n, size_Ql = t.size_ql, nl = size_Ql - 1;
    // all polynomials of the ciphertext in one launch each (blockIdx.z = polynomial)
    NttExtra xi;
    xi.batch = polys;
    xi.poly_stride = size_Ql * n;
    ntt_inverse(c, src, src, src, plain_sel(nl, 1), EPI_INV_CANON, xi, s);  // ci[last] -> coefficients (rns.cu:1171)
    // NTT(ci[last] mod qj) fused with (ci[j] - .) * q_last^-1 (rns.cu:1173-1182): the reduction modulo qj
    // (divide_and_round_reduce_q_last_kernel) happens as the first pass loads ci[last]; dst doubles as the
    // buffer between the two passes
    NttExtra x;
    x.scale = t.inv_q_last.p;
    x.scale_shoup = t.inv_q_last_shoup.p;
    x.aux = src;
    x.batch = polys;
    x.poly_stride = nl * n;
    x.out_stride = nl * n;
    x.aux_stride = size_Ql * n;
    x.pro_src = src + nl * n;
    x.pro_stride = size_Ql * n;
    ntt_forward(c, dst, dst, dst, plain_sel(0, nl), EPI_FWD_MODDOWN, x, s);
}

// Key switch + CKKS rescale in one (build-defined fusion; equals keyswitch_inplace eval_key_switch.cu:95-182 followed by
// divide_and_round_q_last_ntt rns.cu:1160-1184 bit for bit): dst [B][2][Ql-1][N] = rescale(ct + keyswitch(c2)).
// Against the two calls it drops the mod-down's forward transform over 2 x Ql limbs and the rescale's separate last-limb inverse
// (their work rides on one inverse over the P limbs + the last data limb and ONE forward over 2 x (Ql - 1) limbs), and ct is
// never written.
static bool keyswitch_rescale_fusable(const Tool &t) {
    // bconv_rescale_kernel hard-codes the 16-row padding and the 30 / 30 cuts of converter kind 1 (Montgomery entries)
    return t.alpha > 1 && t.alpha <= (uint32_t)kBcRowPad && t.split_ok && t.p_to_ql_pinv.mont30() && t.size_ql >= 2;
}
static void keyswitch_rescale(Context &c, Tool &t, const u64 *ct, const u64 *c2, const u64 *const *rlk, u64 *dst, uint32_t B,
                              const KsScratch &k, hipStream_t s) {
    const size_t n = c.n, ql = t.size_ql, ql_n = ql * n, qlp_n = (size_t)t.size_qlp * n, nl = ql - 1;
    u64 *tmp = k.tmp, *cx = k.cx;
    // cx_last <- ct_last + cx_last * P^-1; folded: the inverse transform's contiguous pass already ran inside the fused mod-up
    const bool folded = modup_inner_prod(c, t, k, c2, ql_n, rlk, PHA_SCHEME_CKKS, B, s, ct, B == 1);
    {   // coefficient form of the P limbs (x phat_i^-1, bconv phase 1) and of the last data limb, both polynomials, one launch pair
        NttExtra xb;
        xb.batch = 2 * B;
        xb.poly_stride = qlp_n;
        xb.scale = t.p_hat_inv_by_limb.p;
        xb.scale_shoup = t.p_hat_inv_by_limb_shoup.p;
        xb.second_pass_only = folded;
        ntt_inverse(c, cx, cx, cx, special_sel(nl, c.size_p + 1, c.size_qp, c.size_p), EPI_INV_SCALE, xb, s);
    }
    NttExtra x;   // out_j = (ct_j + cx_j P^-1 - NTT(v)_j) q_last^-1
    x.scale = t.inv_q_last.p;
    x.scale_shoup = t.inv_q_last_shoup.p;
    x.scale2 = t.pinv.p;
    x.scale2_shoup = t.pinv_shoup.p;
    x.aux = cx;
    x.aux2 = ct;
    x.batch = 2 * B;
    x.poly_stride = ql_n;
    x.out_stride = nl * n;
    x.aux_stride = qlp_n;
    x.aux2_stride = ql_n;
    // r06, batches at N = 2^16: the conversion (+ last-limb fold) is the LOAD of that transform's strided pass (modup_conv_s1_kernel's
    // rescale form, pha_ntt.hip): v is never written in coefficient form
    if (B > 1) {
        const ModupConvArgs mc{t.p_to_ql_pinv.dev.p, 1, cx, qlp_n, nullptr, 0, t.alpha, (uint32_t)ql, true, cx + nl * n};
        x.first_pass_done = modup_conv_strided(c, tmp, plain_sel(0, nl), x, mc, s);
    }
    if (!x.first_pass_done) {   // v_j = delta_j P^-1 + (c_last mod q_j)
        BConvRescaleLaunch L{};
        L.conv = t.p_to_ql_pinv.dev.p; L.dst = tmp; L.cx = cx; L.dst_stride = ql_n; L.cx_stride = qlp_n;
        L.mod = c.d_mod.p; L.n = (uint32_t)n; L.ql = (uint32_t)ql;
        const uint32_t groups = bconv_groups(c, (uint32_t)nl, 2 * (uint32_t)B);
        L.out_per_block = ((uint32_t)nl + groups - 1) / groups;
        const dim3 grid((unsigned)(n / kBcThreads), groups, 2 * B), block(kBcThreads);
        // (keyswitch_rescale_fusable: alpha <= 16)
        if (!with_isz_pad<2, 16>(t.alpha, [&](auto P) { hipLaunchKernelGGL(bconv_rescale_kernel<decltype(P)::value>, grid, block, 0, s, L); }))
            throw std::logic_error("fused key switch + rescale for a special base without one");
        check_launch();
    }
    ntt_forward(c, tmp, tmp, dst, plain_sel(0, nl), EPI_FWD_KSRESCALE, x, s);
}

// Key switch + BGV mod_switch_to_next in one (build-defined fusion; equals keyswitch_inplace eval_key_switch.cu:95-182 under bgv
// followed by mod_t_and_divide_q_last_ntt rns.cu:1186-1236 bit for bit): dst [B][2][Ql-1][N] = mod_switch(ct + keyswitch(c2)).
// A sibling of moddown_from_ntt's bgv branch, not a mode of it.  Both the t-corrected mod-down and the switch work in coefficient
// form, so the forward transform of 2 x Ql limbs, the add to ct and the inverse transform of the same limbs between them cancel:
// ct rides into the one inverse transform as cx_j + (P mod q_j) ct_j (the division by P that follows gives it back), which leaves
// 4 Ql + 2 alpha - 2 limb transforms per ciphertext after the inner product where the two calls run 8 Ql + 2 alpha - 2, two
// element-wise passes for five, and no copy of ct.  Only generic pieces: every tool shape takes this path.
static void keyswitch_mod_switch(Context &c, Tool &t, const u64 *ct, const u64 *c2, const u64 *const *rlk, u64 *dst, uint32_t B,
                                 const KsScratch &k, hipStream_t s) {
    const size_t n = c.n, ql = t.size_ql, ql_n = ql * n, qlp_n = (size_t)t.size_qlp * n, nl = ql - 1;
    const uint32_t polys = 2 * B;
    u64 *cx = k.cx, *delta = k.tmp;
    modup_inner_prod(c, t, k, c2, ql_n, rlk, PHA_SCHEME_BGV, B, s);
    {
        const BgvFoldArgs f{cx, ct, t.p_mod_q2.p, c.d_mod.p, (uint32_t)n, qlp_n, ql_n};
        hipLaunchKernelGGL(bgv_fold_ct_kernel, dim3((unsigned)(n / 512), (unsigned)ql, polys), dim3(256), 0, s, f);
        check_launch();
    }
    NttExtra xb;
    xb.batch = polys;
    xb.poly_stride = qlp_n;
    ntt_inverse(c, cx, cx, cx, special_sel(0, t.size_qlp, c.size_qp, c.size_p), EPI_INV_CANON, xb, s);
    p_to_ql_delta(c, t, delta, cx, qlp_n, polys, true, nullptr, s);   // as the bgv mod-down
    BgvDownSwitchArgs a{};
    a.dst = dst; a.cx = cx; a.delta = delta; a.dst_stride = nl * n; a.cx_stride = qlp_n; a.delta_stride = ql_n;
    a.hat_inv = t.p_to_ql.hat_inv.p; a.iprime = t.p_to_ql.d_iprime.p; a.hat_mod_t = t.p_hat_mod_t.p;
    a.p_mod_q = t.p_mod_q2.p; a.pinv = t.pinv2.p; a.q_last_mod_q = t.q_last_mod_q2.p; a.inv_q_last = t.inv_q_last2.p;
    a.mod = c.d_mod.p; a.t = t.t_mod; a.pinv_t = t.pinv_mod_t; a.inv_q_last_t = t.inv_q_last_mod_t;
    a.n = (uint32_t)n; a.ql = (uint32_t)ql; a.alpha = t.alpha;
    // a group re-reads alpha + 2 shared limbs for its outputs' 2 each: at least 8 outputs per group, and more than that only
    // while two workgroups per CU remain
    const size_t col_blocks = (n / 512) * polys;
    size_t groups = std::max<size_t>(1, std::min<size_t>((nl + 7) / 8, (2 * (size_t)c.num_cus + col_blocks - 1) / col_blocks));
    a.per_group = (uint32_t)((nl + groups - 1) / groups);
    groups = (nl + a.per_group - 1) / a.per_group;
    hipLaunchKernelGGL(bgv_down_switch_kernel, dim3((unsigned)(n / 512), (unsigned)groups, polys), dim3(256), 0, s, a);
    check_launch();
    NttExtra xo;
    xo.batch = polys;
    xo.poly_stride = nl * n;
    ntt_forward(c, dst, dst, dst, plain_sel(0, nl), EPI_FWD_CANON, xo, s);
}

void check_level(Context &c, size_t size_Ql, bool need_p) {
    if (size_Ql < 1 || size_Ql > c.size_q) throw std::invalid_argument("size_Ql out of range");
    if (need_p && c.size_p == 0) throw std::invalid_argument("context has no special modulus");
}

}  // namespace pha

using namespace pha;

extern "C" {

int pha_bconv_P_to_Ql(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(dst); need(src);
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    Tool &t = c.tool((uint32_t)size_Ql);
    BConvCall k = bconv_call(t.p_to_ql);
    k.dst = dst;
    k.src = src - (size_t)size_Ql * c.n;   // src is the bare [P][N] block: the converter's src_limb offset (Ql) must not be applied
    launch_bconv(c, k, as_stream(stream));
    PHA_API_END
}

int pha_modup(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *cks, int scheme, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(dst); need(cks);
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    Tool &t = c.tool((uint32_t)size_Ql);
    strict_operand(c, "modup input", cks, rows_plain(0, size_Ql), 1, 0, as_stream(stream));
    u64 *t_cks = c.scratch(stream, size_Ql * c.n);
    modup(c, t, dst, cks, scheme, t_cks, as_stream(stream));
    PHA_API_END
}

int pha_key_switch_inner_prod(pha_context_t ctx, size_t size_Ql, uint64_t *p_cx, const uint64_t *p_t_mod_up,
                              const uint64_t *const *rlk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(p_cx); need(p_t_mod_up); need(rlk);
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    {
        Tool &ts = c.tool((uint32_t)size_Ql);
        strict_operand(c, "key_switch_inner_prod t_mod_up", p_t_mod_up, rows_qlp(ts.size_ql, c.size_q, c.size_p), ts.beta,
                       (size_t)ts.size_qlp * c.n, as_stream(stream));
        strict_keys(c, "key_switch_inner_prod key", rlk, ts.beta, (uint32_t)size_Ql, as_stream(stream));
    }
    inner_prod(c, c.tool((uint32_t)size_Ql), p_cx, p_t_mod_up, rlk, as_stream(stream));
    PHA_API_END
}

int pha_moddown_from_NTT(pha_context_t ctx, size_t size_Ql, uint64_t *ct_i, uint64_t *cx_i, int scheme,
                         void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct_i); need(cx_i);
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    Tool &t = c.tool((uint32_t)size_Ql);
    strict_operand(c, "mod-down input", cx_i, rows_qlp(t.size_ql, c.size_q, c.size_p), 1, 0, as_stream(stream));
    u64 *delta = c.scratch(stream, size_Ql * c.n);
    moddown_from_ntt(c, t, ct_i, 0, cx_i, 0, 1, scheme, false, delta, as_stream(stream));
    PHA_API_END
}

// DRNSTool::moddown rns_bconv.cu:712-761.  Against moddown_from_NTT (:776-828): bfv input is in coefficient form already; ckks
// and bgv take the same steps (the reference's separate forward transform of delta + moddown_kernel :748-757 stores the same
// canonical words as the fused epilogue; its alpha = 1 route through bConv_BEHZ :733 / :746 stores what the single-prime kernel
// does: y = x for a one-prime base, then x mod q_j).
int pha_moddown(pha_context_t ctx, size_t size_Ql, uint64_t *ct_i, uint64_t *cx_i, int scheme, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct_i); need(cx_i);
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    Tool &t = c.tool((uint32_t)size_Ql);
    strict_operand(c, "mod-down input", cx_i, rows_qlp(t.size_ql, c.size_q, c.size_p), 1, 0, as_stream(stream));
    u64 *delta = c.scratch(stream, size_Ql * c.n);
    moddown_from_ntt(c, t, ct_i, 0, cx_i, 0, 1, scheme, false, delta, as_stream(stream), false, scheme == PHA_SCHEME_BFV);
    PHA_API_END
}

// the batch limits of the batched key-switch entries: blockIdx.z carries beta * batch digit polynomials and 2 * batch polynomials
static void check_ks_batch(const Tool &t, size_t batch) {
    if (batch > 1024 || (size_t)t.beta * batch > 65535 || 2 * batch > 65535) throw std::invalid_argument("batch out of range");
}
// strict mode: the operands of a key switch of B ciphertexts, ct [B][2][Ql][N], c2 [B][Ql][N] and the keys
static void strict_ks_operands(Context &c, Tool &t, const u64 *ct, const u64 *c2, const u64 *const *keys, uint32_t B, hipStream_t s) {
    const size_t ql_n = (size_t)t.size_ql * c.n;
    strict_operand(c, "keyswitch ct", ct, rows_plain(0, t.size_ql), 2 * B, ql_n, s);
    strict_operand(c, "keyswitch c2", c2, rows_plain(0, t.size_ql), B, ql_n, s);
    strict_keys(c, "keyswitch key", keys, t.beta, t.size_ql, s);
}

int pha_keyswitch_inplace_batched(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint64_t *c2, size_t batch,
                                  const uint64_t *const *rlk, int scheme, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(c2); need(rlk);
    if (batch == 0) return 0;
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    Tool &t = c.tool((uint32_t)size_Ql);
    check_ks_batch(t, batch);
    hipStream_t s = as_stream(stream);
    const uint32_t B = (uint32_t)batch;
    strict_ks_operands(c, t, ct, c2, rlk, B, s);
    const KsScratch k(c.scratch(stream, KsScratch::words(c, t, B)), c, t, B);
    keyswitch(c, t, k, ct, true, c2, size_Ql * c.n, rlk, scheme, B, s);
    PHA_API_END
}

int pha_keyswitch_inplace(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint64_t *c2,
                          const uint64_t *const *rlk, int scheme, void *stream) {
    return pha_keyswitch_inplace_batched(ctx, size_Ql, ct, c2, 1, rlk, scheme, stream);
}

int pha_keyswitch_rescale_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, const uint64_t *c2, size_t batch,
                                  const uint64_t *const *rlk, uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(c2); need(rlk); need(dst);
    if (batch == 0) return 0;
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    if (size_Ql < 2) throw std::invalid_argument("cannot rescale the last remaining modulus");
    Tool &t = c.tool((uint32_t)size_Ql);
    check_ks_batch(t, batch);
    hipStream_t s = as_stream(stream);
    const uint32_t B = (uint32_t)batch;
    strict_ks_operands(c, t, ct, c2, rlk, B, s);
    const size_t n = c.n, ql_n = size_Ql * n;
    if (overlaps(dst, B * 2 * (size_Ql - 1) * n, ct, B * 2 * ql_n) || overlaps(dst, B * 2 * (size_Ql - 1) * n, c2, B * ql_n))
        throw std::invalid_argument("dst must not overlap ct or c2");
    const size_t words = KsScratch::words(c, t, B);
    if (keyswitch_rescale_fusable(t)) {
        keyswitch_rescale(c, t, ct, c2, rlk, dst, B, KsScratch(c.scratch(stream, words), c, t, B), s);
    } else {   // alpha = 1, wide primes, wide P: the two reference steps on a copy of ct [B][2][Ql][N], kept after the key switch's scratch
        u64 *base = c.scratch(stream, words + B * 2 * ql_n), *work = base + words;
        PHA_HIP(hipMemcpyAsync(work, ct, B * 2 * ql_n * sizeof(u64), hipMemcpyDeviceToDevice, s));
        keyswitch(c, t, KsScratch(base, c, t, B), work, true, c2, ql_n, rlk, PHA_SCHEME_CKKS, B, s);
        rescale_ntt(c, t, work, 2 * B, dst, s);
    }
    PHA_API_END
}

int pha_keyswitch_rescale(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, const uint64_t *c2,
                          const uint64_t *const *rlk, uint64_t *dst, void *stream) {
    return pha_keyswitch_rescale_batched(ctx, size_Ql, ct, c2, 1, rlk, dst, stream);
}

int pha_keyswitch_mod_switch_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, const uint64_t *c2, size_t batch,
                                     const uint64_t *const *rlk, uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct); need(c2); need(rlk); need(dst);
    if (batch == 0) return 0;
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    if (size_Ql < 2) throw std::invalid_argument("cannot switch down the last remaining modulus");
    Tool &t = c.tool((uint32_t)size_Ql);
    if (!t.bgv_ready) throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
    check_ks_batch(t, batch);
    hipStream_t s = as_stream(stream);
    const uint32_t B = (uint32_t)batch;
    const size_t n = c.n, ql_n = size_Ql * n;
    if (overlaps(dst, B * 2 * (size_Ql - 1) * n, ct, B * 2 * ql_n) || overlaps(dst, B * 2 * (size_Ql - 1) * n, c2, B * ql_n))
        throw std::invalid_argument("dst must not overlap ct or c2");
    strict_ks_operands(c, t, ct, c2, rlk, B, s);
    keyswitch_mod_switch(c, t, ct, c2, rlk, dst, B, KsScratch(c.scratch(stream, KsScratch::words(c, t, B)), c, t, B), s);
    PHA_API_END
}

int pha_keyswitch_mod_switch(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, const uint64_t *c2,
                             const uint64_t *const *rlk, uint64_t *dst, void *stream) {
    return pha_keyswitch_mod_switch_batched(ctx, size_Ql, ct, c2, 1, rlk, dst, stream);
}

// BASELINE config 4 as one call (build-defined composition of relinearize_inplace src/evaluate.cu:1028-1077 and
// apply_galois_inplace :1567-1624 over a batch): out [B][2][Ql][N] = rotate_elt(relinearize(ct3 [B][3][Ql][N])).
// Against the host composition of the two batched key switches it makes no copies at all: the first key switch reads c2 in
// place (strided) and stores only keyswitch(c2); the Galois kernel forms ct + keyswitch(c2) as it permutes, writing the
// operands of the second key switch straight into `out`, which that key switch then completes in place.
int pha_relinearize_rotate_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct3, size_t batch,
                                   const uint64_t *const *rlk, const uint64_t *const *glk, uint32_t galois_elt, int scheme,
                                   uint64_t *out, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(ct3); need(rlk); need(glk); need(out);
    if (batch == 0) return 0;
    Context &c = ctx->c;
    check_level(c, size_Ql, true);
    check_galois_elt(c, galois_elt);
    Tool &t = c.tool((uint32_t)size_Ql);
    const bool ntt_dom = ntt_domain_scheme(scheme);
    if (scheme == PHA_SCHEME_BGV && !t.bgv_ready) throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
    hipStream_t s = as_stream(stream);
    const size_t n = c.n, ql_n = size_Ql * n, qlp_n = (size_t)t.size_qlp * n;
    if (overlaps(out, batch * 2 * ql_n, ct3, batch * 3 * ql_n)) throw std::invalid_argument("out must not overlap ct3");
    // ciphertexts per set of launches: the mod-up digits of a set (beta x (l + alpha) limbs each) should stay within the MALL
    // (measured at N = 2^15 / 30 + 15 limbs: 8 per set 233 us per ciphertext, all 64 at once 268, one by one 334).
    // chunk = 0 also spreads the sets over two internal streams, half a set each: the short kernels of one set fill the tails of
    // the other's (same process, alternating: 6045-6086 against 5909-5920 ciphertexts/s; four streams or two full sets: no better).
    const bool auto_chunk = chunk == 0;
    if (chunk == 0) chunk = std::max<size_t>(1, ((size_t)192 << 20) / ((size_t)t.beta * qlp_n * sizeof(u64)));
    chunk = std::min<size_t>(std::min<size_t>(chunk, batch), 1024);
    while ((size_t)t.beta * chunk > 65535 || 2 * chunk > 65535) chunk /= 2;
    const bool two_lanes = auto_chunk && chunk >= 2 && batch >= 2 * chunk;
    if (two_lanes) chunk /= 2;
    const uint32_t *tab = ntt_dom ? c.galois_table(galois_elt) : nullptr;
    const size_t C = chunk;
    const size_t ks_words = KsScratch::words(c, t, C), words = ks_words + C * 3 * ql_n;
    // one set of B <= C ciphertexts from b0 on stream ls, scratch base: the key switches' scratch for C | ks [C][2][Ql][N] | g1 [C][Ql][N]
    auto one_set = [&](hipStream_t ls, u64 *base, size_t b0) {
        const KsScratch k(base, c, t, C);
        u64 *ks = base + ks_words, *g1 = ks + C * 2 * ql_n;
        const uint32_t B = (uint32_t)std::min(C, batch - b0);
        const u64 *in = ct3 + b0 * 3 * ql_n;
        u64 *o = out + b0 * 2 * ql_n;
        // relinearize: ks = keyswitch(c2), c2 read where it lies (every third polynomial)
        keyswitch(c, t, k, ks, false, in + 2 * ql_n, 3 * ql_n, rlk, scheme, B, ls);
        // rotate: (galois(c0 + ks0), 0) and galois(c1 + ks1) in the layout of the second key switch (apply_galois_inplace)
        hipLaunchKernelGGL(galois_split_kernel, dim3((unsigned)(n / 256), (unsigned)size_Ql, 2 * B), dim3(256), 0, ls, o, g1, ks, tab,
                           c.d_mod.p, tab ? galois_elt : inv_mod_2n(galois_elt, n), (uint32_t)n, (uint32_t)size_Ql, in, 3u);
        check_launch();
        keyswitch(c, t, k, o, true, g1, ql_n, glk, scheme, B, ls);
    };
    if (!two_lanes) {
        u64 *base = c.scratch(stream, words);
        for (size_t b0 = 0; b0 < batch; b0 += C) one_set(s, base, b0);
    } else {
        std::lock_guard<std::mutex> lk(c.lanes.mu);
        c.lanes.ensure();
        u64 *base[2] = {c.scratch(c.lanes.s[0], words), c.scratch(c.lanes.s[1], words)};
        // (both lane arenas are reserved above, before the fork: nothing below allocates)
        PHA_HIP(hipEventRecord(c.lanes.fork, s));
        for (int l = 0; l < 2; l++) PHA_HIP(hipStreamWaitEvent(c.lanes.s[l], c.lanes.fork, 0));
        auto join = [&]() {   // whatever the lanes have been given so far is ordered before anything the caller enqueues on `stream` next
            for (int l = 0; l < 2; l++)
                if (hipEventRecord(c.lanes.join[l], c.lanes.s[l]) == hipSuccess) (void)hipStreamWaitEvent(s, c.lanes.join[l], 0);
        };
        try {
            size_t set = 0;
            for (size_t b0 = 0; b0 < batch; b0 += C, set++) one_set(c.lanes.s[set & 1], base[set & 1], b0);
        } catch (...) {   // a failed launch must not leave work in flight on the internal streams behind an error code
            join();
            throw;
        }
        for (int l = 0; l < 2; l++) {
            PHA_HIP(hipEventRecord(c.lanes.join[l], c.lanes.s[l]));
            PHA_HIP(hipStreamWaitEvent(s, c.lanes.join[l], 0));
        }
    }
    PHA_API_END
}

int pha_divide_and_round_q_last_ntt(pha_context_t ctx, size_t size_Ql, uint64_t *src, size_t cipher_size,
                                    uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(src); need(dst);
    Context &c = ctx->c;
    check_level(c, size_Ql, false);
    if (size_Ql < 2) throw std::invalid_argument("cannot rescale the last remaining modulus");
    Tool &t = c.tool((uint32_t)size_Ql);
    if (cipher_size == 0) return 0;
    if (cipher_size > 65535) throw std::invalid_argument("cipher_size out of range");
    rescale_ntt(c, t, src, (uint32_t)cipher_size, dst, as_stream(stream));
    PHA_API_END
}

int pha_generate_one_kswitch_key(pha_context_t ctx, const uint64_t *sk_ntt, const uint64_t *new_key_ntt,
                                 const uint64_t *a, uint64_t *e, uint64_t *const *evk, int scheme, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(sk_ntt); need(new_key_ntt); need(a); need(e); need(evk);
    Context &c = ctx->c;
    if (c.size_p == 0) throw std::invalid_argument("context has no special modulus");
    if (c.size_q % c.size_p) throw std::invalid_argument("#Q must be a multiple of special_modulus_size");
    ntt_domain_scheme(scheme);  // validates the scheme
    Tool &t = c.tool(c.size_q);
    hipStream_t s = as_stream(stream);
    const uint32_t dnum = c.size_q / c.size_p, n = (uint32_t)c.n;
    const size_t qp_n = (size_t)c.size_qp * n;
    if (scheme == PHA_SCHEME_BGV) {  // noise = t*e (secretkey.cu:268-273)
        if (!t.bgv_ready) throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
        hipLaunchKernelGGL(scale_by_t_kernel, dim3(n / 256, c.size_qp, dnum), dim3(256), 0, s, e, c.d_mod.p,
                           t.t_mod.value, n, qp_n);
        check_launch();
    }
    NttExtra x;  // e -> NTT form, every digit in one launch (secretkey.cu:275)
    x.batch = dnum;
    x.poly_stride = qp_n;
    ntt_forward(c, e, e, e, plain_sel(0, c.size_qp), EPI_FWD_CANON, x, s);
    KeyGenArgs k{evk, sk_ntt, new_key_ntt, a, e, t.p_mod_q2.p, c.d_mod.p, n, c.size_qp, c.size_p};
    hipLaunchKernelGGL(kswitch_key_kernel, dim3(n / 256, c.size_qp, dnum), dim3(256), 0, s, k);
    check_launch();
    PHA_API_END
}

int pha_mod_t_and_divide_q_last_ntt(pha_context_t ctx, size_t size_Ql, uint64_t *src, size_t cipher_size,
                                    uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(src); need(dst);
    Context &c = ctx->c;
    check_level(c, size_Ql, false);
    if (size_Ql < 2) throw std::invalid_argument("cannot switch down the last remaining modulus");
    Tool &t = c.tool((uint32_t)size_Ql);
    if (!t.bgv_ready) throw std::invalid_argument("bgv needs a plain modulus (pha_context_set_plain_modulus)");
    if (cipher_size == 0) return 0;
    if (cipher_size > 65535) throw std::invalid_argument("cipher_size out of range");
    hipStream_t s = as_stream(stream);
    const size_t n = c.n, nl = size_Ql - 1;
    NttExtra xi;
    xi.batch = (uint32_t)cipher_size;
    xi.poly_stride = size_Ql * n;
    ntt_inverse(c, src, src, src, plain_sel(0, size_Ql), EPI_INV_CANON, xi, s);  // rns.cu:1221
    BgvSwitchArgs k{dst, src, t.q_last_mod_q2.p, t.inv_q_last2.p, c.d_mod.p, t.inv_q_last_mod_t, t.t_mod,
                    (uint32_t)n, (uint32_t)nl, size_Ql * n, nl * n};
    hipLaunchKernelGGL(bgv_switch_kernel, dim3((unsigned)(n / 256), (unsigned)nl, (unsigned)cipher_size), dim3(256), 0,
                       s, k);
    check_launch();
    NttExtra xo;
    xo.batch = (uint32_t)cipher_size;
    xo.poly_stride = nl * n;
    ntt_forward(c, dst, dst, dst, plain_sel(0, nl), EPI_FWD_CANON, xo, s);  // rns.cu:1234
    PHA_API_END
}

int pha_divide_and_round_q_last(pha_context_t ctx, size_t size_Ql, const uint64_t *src, size_t cipher_size,
                                uint64_t *dst, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(src); need(dst);
    Context &c = ctx->c;
    check_level(c, size_Ql, false);
    if (size_Ql < 2) throw std::invalid_argument("cannot switch down the last remaining modulus");
    Tool &t = c.tool((uint32_t)size_Ql);
    const size_t n = c.n, nl = size_Ql - 1;
    if (cipher_size == 0) return 0;
    if (cipher_size > 65535) throw std::invalid_argument("cipher_size out of range");
    SubMulArgs k{dst, src, src + nl * n, t.inv_q_last2.p, c.d_mod.p, (uint32_t)n};   // every polynomial in one launch
    k.dst_stride = nl * n;
    k.cx_stride = size_Ql * n;
    k.delta_stride = size_Ql * n;
    hipLaunchKernelGGL(sub_mul_kernel<true>, dim3((unsigned)(n / 256), (unsigned)nl, (unsigned)cipher_size), dim3(256), 0,
                       as_stream(stream), k);
    check_launch();
    PHA_API_END
}

int pha_apply_galois_ntt(pha_context_t ctx, const uint64_t *src, uint64_t *dst, uint32_t galois_elt, size_t cms,
                         void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(src); need(dst);
    if (src == dst) throw std::invalid_argument("apply_galois_ntt cannot run in place");
    Context &c = ctx->c;
    const uint32_t *tab = c.galois_table(galois_elt);
    hipLaunchKernelGGL(galois_ntt_kernel, dim3((unsigned)(c.n / 256), (unsigned)cms), dim3(256), 0,
                       as_stream(stream), dst, src, tab, (uint32_t)c.n);
    check_launch();
    PHA_API_END
}

int pha_apply_galois_batched(pha_context_t ctx, const uint64_t *src, uint64_t *dst, uint32_t galois_elt, size_t cms,
                             size_t polys, int ntt_form, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(src); need(dst);
    if (src == dst) throw std::invalid_argument("apply_galois cannot run in place");
    Context &c = ctx->c;
    check_galois_elt(c, galois_elt);
    if (cms > c.size_qp) throw std::invalid_argument("modulus index out of range");
    if (polys == 0 || cms == 0) return 0;
    if (polys > 65535) throw std::invalid_argument("batch out of range");
    if (ntt_form) {   // the NTT-domain permutation does not depend on the modulus: the polynomials are just more limbs
        const uint32_t *tab = c.galois_table(galois_elt);
        for (size_t p0 = 0; p0 < polys * cms; p0 += 65535) {
            const size_t cnt = std::min<size_t>(65535, polys * cms - p0);
            hipLaunchKernelGGL(galois_ntt_kernel, dim3((unsigned)(c.n / 256), (unsigned)cnt), dim3(256), 0, as_stream(stream),
                               dst + p0 * c.n, src + p0 * c.n, tab, (uint32_t)c.n);
        }
    } else {
        launch_galois_coeff(c, dst, src, galois_elt, cms, 0, polys, as_stream(stream));
    }
    check_launch();
    PHA_API_END
}

int pha_apply_galois_for_keyswitch(pha_context_t ctx, const uint64_t *src, uint64_t *dst_ct, uint64_t *dst_c2,
                                   uint32_t galois_elt, size_t size_Ql, size_t batch, int ntt_form, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(src); need(dst_ct); need(dst_c2);
    if (src == dst_ct || src == dst_c2) throw std::invalid_argument("apply_galois cannot run in place");
    Context &c = ctx->c;
    check_galois_elt(c, galois_elt);
    if (size_Ql == 0 || size_Ql > c.size_q) throw std::invalid_argument("size_Ql out of range");
    if (batch == 0) return 0;
    if (2 * batch > 65535) throw std::invalid_argument("batch out of range");
    const uint32_t *tab = ntt_form ? c.galois_table(galois_elt) : nullptr;
    hipLaunchKernelGGL(galois_split_kernel, dim3((unsigned)(c.n / 256), (unsigned)size_Ql, (unsigned)(2 * batch)), dim3(256), 0,
                       as_stream(stream), dst_ct, dst_c2, src, tab, c.d_mod.p, tab ? galois_elt : inv_mod_2n(galois_elt, c.n), (uint32_t)c.n,
                       (uint32_t)size_Ql, (const u64 *)nullptr, 0u);
    check_launch();
    PHA_API_END
}

int pha_apply_galois(pha_context_t ctx, const uint64_t *src, uint64_t *dst, uint32_t galois_elt, size_t cms,
                     size_t mod_start, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(src); need(dst);
    if (src == dst) throw std::invalid_argument("apply_galois cannot run in place");
    Context &c = ctx->c;
    check_galois_elt(c, galois_elt);
    if (mod_start + cms > c.size_qp) throw std::invalid_argument("modulus index out of range");
    launch_galois_coeff(c, dst, src, galois_elt, cms, mod_start, 1, as_stream(stream));
    PHA_API_END
}

}  // extern "C"
