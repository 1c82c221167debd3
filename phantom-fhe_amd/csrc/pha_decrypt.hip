// pha_decrypt.hip -- decryption on raw buffers: the device work of PhantomSecretKey::ckks_decrypt / bgv_decrypt / bfv_decrypt
// (src/secretkey.cu:533-691), DRNSTool::hps_decrypt_scale_and_round (src/rns.cu:1519-1689) and DRNSTool::decrypt_mod_t, for BATCHES
// of ciphertexts.  The per-thread programs, their bounds and the one deviation from the reference are in pha_decrypt.h; the tables in
// pha_rns_tables.h (decrypt_round_tables / decrypt_mod_t_tables); DESIGN.md section 4.11.
//
// Phase kernel: dst (b) = c0 (b) + sum_{i = 1 .. k - 1} c_i (b) (.) s^i over NTT-form operands, one (limb, adjacent coefficient pair)
// per thread and a group of up to kPhaseGroup = 4 ciphertexts per workgroup row (blockIdx.z): the words of s^i are loaded once per
// thread and stay in registers across the group.  Ciphertext words are read once: 16-byte nontemporal loads, as the two streaming
// kernels of the key switch; the secret key is re-read by every group and keeps the default policy, as does the result, which the
// next kernel (inverse transform, decode) reads right away.  Per output word the kernel moves k + (k - 1) / G + 1 words (k ciphertext
// words, the key's share, the store) against 4 (k - 1) + 2 of the reference's composition (a copy: 2; k - 1 launches reading c_i, s^i
// and the sum and writing it: 4 each) -- derived, not measured.
#include "../../include/phantom_amd.h"
#include "pha_decrypt.h"
#include "pha_internal.h"
#include "pha_ntt_core.h"

#include <algorithm>

namespace pha {

constexpr int kDecThreads = 256;
static_assert(kPhaseBatchMax == (size_t)kPhaseGroup * 65535, "pha_layout.h: a group per workgroup row, the row in blockIdx.z");
constexpr int kModTPolys = 16;         // polynomials per conversion launch: their factors travel in the kernel arguments

struct PhaseArgs {
    const u64 *c0;        // polynomial 0 of ciphertext 0; null: dropped (bfv adds it behind the inverse transform)
    const u64 *c1;        // polynomial 1 of ciphertext 0; polynomial i >= 1 of ciphertext b at c1 + b * ct_stride + (i - 1) * L * N
    const u64 *sk;        // s^i at sk + (i - 1) * sk_stride
    u64 *dst;
    const DModulus *mod;
    const FpInfo *fpinfo;
    uint32_t n, limbs, k, batch;
    size_t ct_stride, sk_stride, dst_stride;
};

struct PhaseSrc {
    const u64 *c0, *c1, *sk;   // at this thread's words
    size_t ln, ct_stride, sk_stride;
    __device__ __forceinline__ u64x2 c(int g, uint32_t i) const {
        const u64 *p = i == 0 ? c0 + g * ct_stride : c1 + g * ct_stride + (size_t)(i - 1) * ln;
        return gload2<true>(reinterpret_cast<const u64x2 *>(p));
    }
    __device__ __forceinline__ u64x2 s(uint32_t i) const { return *reinterpret_cast<const u64x2 *>(sk + (size_t)(i - 1) * sk_stride); }
};

template <int G, int K>
__device__ __forceinline__ void phase_group(const PhaseArgs &k, PhaseSrc &src, uint32_t limb, const DModulus &m, u64 *dst) {
    u64x2 r[G];
    PlainSumNoProbe probe;
    const FpInfo fi = k.fpinfo[limb];
    if (fi.ok) phase_fp<G, K>(src, k.k, k.c0 != nullptr, FpMod{fi.q, fi.qinv, false, false}, modulus_bits(m.value), r, probe);   // (uniform)
    else phase_int<G, K>(src, k.k, k.c0 != nullptr, m, r, probe);
#pragma unroll
    for (int g = 0; g < G; g++) gstore2<false>(reinterpret_cast<u64x2 *>(dst + g * k.dst_stride), r[g]);
}

// K = 2, 3: the ciphertext size as a constant; 0: the run-time loop
template <int K>
__global__ __launch_bounds__(kDecThreads) void phase_kernel(const PhaseArgs k) {
    const uint32_t limb = blockIdx.y;
    const DModulus m = k.mod[limb];
    const size_t b0 = (size_t)blockIdx.z * kPhaseGroup;
    const uint32_t ng = k.batch - b0 < (size_t)kPhaseGroup ? (uint32_t)(k.batch - b0) : (uint32_t)kPhaseGroup;   // (uniform) the last group may be short
    const size_t idx = (size_t)limb * k.n + ((size_t)blockIdx.x * kDecThreads + threadIdx.x) * 2;
    const size_t at = b0 * k.ct_stride + idx;
    PhaseSrc src{k.c0 ? k.c0 + at : nullptr, k.c1 + at, k.sk + idx, (size_t)k.limbs * k.n, k.ct_stride, k.sk_stride};
    u64 *dst = k.dst + b0 * k.dst_stride + idx;
    switch (ng) {
        case 4: phase_group<4, K>(k, src, limb, m, dst); break;
        case 3: phase_group<3, K>(k, src, limb, m, dst); break;
        case 2: phase_group<2, K>(k, src, limb, m, dst); break;
        default: phase_group<1, K>(k, src, limb, m, dst); break;
    }
}

// launch only: the callers have validated.  c0 == null drops it
static void launch_phase(Context &c, size_t size_Ql, const u64 *c0, const u64 *c1, size_t cipher_size, size_t batch, size_t ct_stride,
                         const u64 *sk, u64 *dst, size_t dst_stride, hipStream_t s) {
    const PhaseArgs k{c0, c1, sk, dst, c.d_mod.p, c.d_fpinfo.p, (uint32_t)c.n, (uint32_t)size_Ql, (uint32_t)cipher_size, (uint32_t)batch,
                      ct_stride, (size_t)c.size_qp * c.n, dst_stride};
    const dim3 grid((unsigned)(c.n / (kDecThreads * 2)), (unsigned)size_Ql, (unsigned)((batch + kPhaseGroup - 1) / kPhaseGroup)), block(kDecThreads);
    if (cipher_size == 2) hipLaunchKernelGGL(phase_kernel<2>, grid, block, 0, s, k);
    else if (cipher_size == 3) hipLaunchKernelGGL(phase_kernel<3>, grid, block, 0, s, k);
    else hipLaunchKernelGGL(phase_kernel<0>, grid, block, 0, s, k);
    check_launch();
}

// NTT form (bgv, ckks): the phase kernel, one batched inverse transform.  Coefficient form (bfv): the three steps below
void phase_to_coeff(Context &c, size_t size_Ql, bool ntt_form, const CtBatch &chunk, u64 *work, size_t wst, hipStream_t s) {
    const size_t ln = size_Ql * c.n, km1 = chunk.cipher_size - 1, B = chunk.batch, ct_stride = chunk.ct_stride;
    const LimbSel sel = plain_sel(0, size_Ql);
    NttExtra x;
    x.batch = (uint32_t)B;
    x.poly_stride = wst;
    if (ntt_form) {
        launch_phase(c, size_Ql, chunk.ct, chunk.ct + ln, chunk.cipher_size, B, ct_stride, chunk.sk_powers, work, wst, s);
        return ntt_inverse(c, work, work, work, sel, EPI_INV_CANON, x, s);
    }
    // 1. c1 .. c_{k-1} of every ciphertext forward, out of place into the work buffer [B][k - 1][L][N]
    NttExtra f;
    f.poly_stride = ln;
    if (km1 == 1 || B == 1) {   // one polynomial per ciphertext, or one ciphertext: the polynomials are evenly spaced
        f.batch = (uint32_t)(B * km1);
        f.in_stride = km1 == 1 ? ct_stride : ln;
        ntt_forward(c, chunk.ct + ln, work, work, sel, EPI_FWD_CANON, f, s);
    } else {
        f.batch = (uint32_t)km1;
        f.in_stride = ln;
        for (size_t g = 0; g < B; g++) ntt_forward(c, chunk.ct + g * ct_stride + ln, work + g * wst, work + g * wst, sel, EPI_FWD_CANON, f, s);
    }
    // 2. the phase without c0; result b takes the place of its own c1 in the work buffer (a thread reads its words before it writes)
    launch_phase(c, size_Ql, nullptr, work, chunk.cipher_size, B, wst, chunk.sk_powers, work, wst, s);
    // 3. back to coefficient form in place, c0 (b) added in the final store
    x.aux = chunk.ct;
    x.aux_stride = ct_stride ? ct_stride : wst;   // (B == 1 with stride 0: unused)
    x.aux_pair_stride = 2 * ct_stride;            // polynomial z adds c0 of ciphertext z: (z / 2) * 2 stride + (z % 2) * stride
    ntt_inverse(c, work, work, work, sel, EPI_INV_CANON_ADD, x, s);
}

// ---- the two tails: one coefficient per thread, the polynomial is blockIdx.y ----------------------------------------------------
struct LimbSrc {
    const u64 *p;   // this thread's coefficient in limb 0
    size_t n;
    __device__ __forceinline__ u64 operator()(uint32_t i) const { return gload<true>(p + (size_t)i * n); }   // read once
};

struct ScaleRoundArgs {
    u64 *dst;
    const u64 *src;
    const double *frac;
    const u64 *itab;
    DModulus t;
    uint32_t n, limbs;
    int h;
    size_t src_stride, dst_stride;
};
__global__ __launch_bounds__(kDecThreads) void scale_round_kernel(const ScaleRoundArgs k) {
    const size_t coeff = (size_t)blockIdx.x * kDecThreads + threadIdx.x, z = blockIdx.y;
    LimbSrc src{k.src + z * k.src_stride + coeff, k.n};
    k.dst[z * k.dst_stride + coeff] = decrypt_scale_round(src, k.limbs, k.h, k.frac, k.itab, k.t);
}

struct ModTArgs {
    u64 *dst;
    const u64 *src;
    const u64x2 *hat_inv;
    const u64 *mat, *q;
    u64 q_mod_t;
    DModulus t;
    uint32_t n, limbs;
    size_t src_stride, dst_stride;
    u64 factor[kModTPolys];   // inverse correction factor of polynomial z, mod t
};
__global__ __launch_bounds__(kDecThreads) void mod_t_kernel(const ModTArgs k) {
    const size_t coeff = (size_t)blockIdx.x * kDecThreads + threadIdx.x, z = blockIdx.y;
    LimbSrc src{k.src + z * k.src_stride + coeff, k.n};
    k.dst[z * k.dst_stride + coeff] = decrypt_mod_t_convert(src, k.limbs, k.hat_inv, k.mat, k.q, k.q_mod_t, k.t, k.factor[z]);
}

DecryptLevel &Context::decrypt_level(uint32_t size_ql) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = decrypt_tables.find(size_ql);
    if (it != decrypt_tables.end()) return *it->second;
    check_rns_level(size_ql, size_q);
    need_plain_modulus(shape(*this));
    if (size_ql > kDecryptMaxLimbs) throw std::invalid_argument("decryption to a plain modulus takes levels of at most 64 limbs");
    PHA_HIP(hipSetDevice(device));
    auto d = std::make_unique<DecryptLevel>();
    d->size = size_ql;
    d->t_mod = h_modulus(plain_t);
    const DecryptRoundTables r = decrypt_round_tables(primes, size_ql, plain_t);
    d->h = r.h;
    d->frac.upload(r.frac);
    d->itab.upload(r.itab);
    const DecryptModTTables m = decrypt_mod_t_tables(primes, size_ql, plain_t);
    d->hat_inv.upload(m.hat_inv);
    d->mat.upload(m.mat);
    d->q.upload(std::vector<u64>(primes.begin(), primes.begin() + size_ql));
    d->q_mod_t = m.q_mod_t;
    return *(decrypt_tables[size_ql] = std::move(d));
}

static void launch_scale_round(Context &c, DecryptLevel &d, u64 *dst, size_t dst_stride, const u64 *src, size_t src_stride, size_t polys,
                               hipStream_t s) {
    const ScaleRoundArgs k{dst, src, d.frac.p, d.itab.p, d.t_mod, (uint32_t)c.n, d.size, d.h, src_stride, dst_stride};
    hipLaunchKernelGGL(scale_round_kernel, dim3((unsigned)(c.n / kDecThreads), (unsigned)polys), dim3(kDecThreads), 0, s, k);
    check_launch();
}
// inv_factors: `polys` words below t, or null: all 1
static void launch_mod_t(Context &c, DecryptLevel &d, u64 *dst, size_t dst_stride, const u64 *src, size_t src_stride, size_t polys,
                         const u64 *inv_factors, hipStream_t s) {
    for (size_t p0 = 0; p0 < polys; p0 += kModTPolys) {
        const size_t P = std::min<size_t>(kModTPolys, polys - p0);
        ModTArgs k{dst + p0 * dst_stride, src + p0 * src_stride, d.hat_inv.p, d.mat.p, d.q.p, d.q_mod_t, d.t_mod, (uint32_t)c.n, d.size,
                   src_stride, dst_stride, {}};
        for (size_t z = 0; z < (size_t)kModTPolys; z++) k.factor[z] = inv_factors && z < P ? inv_factors[p0 + z] : 1;
        hipLaunchKernelGGL(mod_t_kernel, dim3((unsigned)(c.n / kDecThreads), (unsigned)P), dim3(kDecThreads), 0, s, k);
        check_launch();
    }
}

// strict mode of the entries over a CtBatch (what they refuse: check_decrypt / check_noise_budget of pha_layout.h)
void decrypt_strict(Context &c, const char *entry, size_t size_Ql, const CtBatch &b, hipStream_t s) {
    if (!strict_mode()) return;
    const std::string ct_name = std::string(entry) + " ct", sk_name = std::string(entry) + " sk_powers";
    for (size_t i = 0; i < b.batch; i++)
        strict_operand(c, ct_name.c_str(), b.ct + i * b.ct_stride, rows_plain(0, size_Ql), (uint32_t)b.cipher_size, size_Ql * c.n, s);
    strict_operand(c, sk_name.c_str(), b.sk_powers, rows_plain(0, size_Ql), (uint32_t)(b.cipher_size - 1), (size_t)c.size_qp * c.n, s);
}

// the inverse correction factors of a batch, mod t: every factor is validated before anything is launched
static std::vector<u64> invert_factors(Context &c, const uint64_t *factors, size_t batch) {
    std::vector<u64> inv;
    if (!factors) return inv;
    inv.resize(batch);
    for (size_t b = 0; b < batch; b++) {
        const u64 f = factors[b] % c.plain_t;
        u64 a = f, m = c.plain_t;
        while (m) { const u64 r = a % m; a = m; m = r; }
        if (a != 1) throw std::logic_error("invalid correction factor");   // bgv_decrypt, src/secretkey.cu:683-685
        inv[b] = factors[b] == 1 ? 1 : h_invmod(f, c.plain_t);
    }
    return inv;
}

// the two entries that decrypt to a plain modulus: the phase front end per chunk, then the bgv tail (factors may be null) or the bfv tail
static void decrypt_to_plain(Context &c, bool bfv, size_t size_Ql, const CtBatch &b, const uint64_t *factors, u64 *dst, size_t dst_stride,
                             size_t chunk, void *stream) {
    check_decrypt(shape(c), size_Ql, b, dst, dst_stride, c.n, false, true);
    const std::vector<u64> inv = invert_factors(c, factors, b.batch);
    if (b.batch == 0) return;
    hipStream_t s = as_stream(stream);
    decrypt_strict(c, bfv ? "bfv_decrypt" : "bgv_decrypt", size_Ql, b, s);
    DecryptLevel &d = c.decrypt_level((uint32_t)size_Ql);
    const PhaseChunk pc = phase_chunk(!bfv, b.cipher_size, size_Ql * c.n, b.batch, chunk, kDecryptChunk);
    u64 *work = c.scratch_outer(stream, pc.C * pc.wst);
    for (size_t b0 = 0; b0 < b.batch; b0 += pc.C) {
        const size_t B = std::min(pc.C, b.batch - b0);
        phase_to_coeff(c, size_Ql, !bfv, CtBatch{b.ct + b0 * b.ct_stride, b.cipher_size, B, b.ct_stride, b.sk_powers, b.n_powers}, work, pc.wst, s);
        if (bfv) launch_scale_round(c, d, dst + b0 * dst_stride, dst_stride, work, pc.wst, B, s);   // floor(t x / Q + 1/2) mod t
        else launch_mod_t(c, d, dst + b0 * dst_stride, dst_stride, work, pc.wst, B, inv.empty() ? nullptr : inv.data() + b0, s);
    }
}

// the two DRNSTool launchers on ONE polynomial: what they refuse, strict mode, the level's tables
static DecryptLevel &one_polynomial(Context &c, const char *src_name, size_t size_Ql, const u64 *dst, const u64 *src, hipStream_t s) {
    need(dst); need(src);
    check_rns_level(size_Ql, c.size_q);
    DecryptLevel &d = c.decrypt_level((uint32_t)size_Ql);
    if (overlaps(dst, c.n, src, size_Ql * c.n)) throw std::invalid_argument("dst must not overlap src");
    strict_operand(c, src_name, src, rows_plain(0, size_Ql), 1, 0, s);
    return d;
}

}  // namespace pha

using namespace pha;

extern "C" {

int pha_secret_key_powers(pha_context_t ctx, const uint64_t *sk_ntt, size_t max_power, uint64_t *out, void *stream) {
    PHA_CTX_BEGIN(ctx)   // compute_secret_key_array src/secretkey.cu:196-230
    need(sk_ntt); need(out);
    Context &c = ctx->c;
    if (max_power < 1 || max_power > 65535) throw std::invalid_argument("max_power out of range");
    const size_t words = (size_t)c.size_qp * c.n;
    if (overlaps(out, max_power * words, sk_ntt, words) && out != sk_ntt) throw std::invalid_argument("out must not overlap sk_ntt");
    hipStream_t s = as_stream(stream);
    strict_operand(c, "secret_key_powers sk_ntt", sk_ntt, rows_plain(0, c.size_qp), 1, 0, s);
    if (out != sk_ntt) PHA_HIP(hipMemcpyAsync(out, sk_ntt, words * sizeof(u64), hipMemcpyDeviceToDevice, s));
    for (size_t p = 1; p < max_power; p++) rc(pha_multiply_rns_poly(ctx, out + (p - 1) * words, out, out + p * words, c.size_qp, 0, stream));
    PHA_API_END
}

int pha_decrypt_phase_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t cipher_size, size_t batch, size_t ct_stride,
                              const uint64_t *sk_powers, size_t n_powers, uint64_t *dst, size_t dst_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    const size_t ln = size_Ql * c.n;
    const CtBatch b{ct, cipher_size, batch, ct_stride, sk_powers, n_powers};
    check_decrypt(shape(c), size_Ql, b, dst, dst_stride, ln, true, false);
    if (batch == 0) return 0;
    hipStream_t s = as_stream(stream);
    decrypt_strict(c, "decrypt_phase", size_Ql, b, s);
    launch_phase(c, size_Ql, ct, ct + ln, cipher_size, batch, ct_stride, sk_powers, dst, dst_stride, s);
    PHA_API_END
}

int pha_bgv_decrypt_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t cipher_size, size_t batch, size_t ct_stride,
                            const uint64_t *sk_powers, size_t n_powers, const uint64_t *correction_factors, uint64_t *dst,
                            size_t dst_stride, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    decrypt_to_plain(ctx->c, false, size_Ql, CtBatch{ct, cipher_size, batch, ct_stride, sk_powers, n_powers}, correction_factors, dst, dst_stride, chunk, stream);
    PHA_API_END
}

int pha_bfv_decrypt_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t cipher_size, size_t batch, size_t ct_stride,
                            const uint64_t *sk_powers, size_t n_powers, uint64_t *dst, size_t dst_stride, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    decrypt_to_plain(ctx->c, true, size_Ql, CtBatch{ct, cipher_size, batch, ct_stride, sk_powers, n_powers}, nullptr, dst, dst_stride, chunk, stream);
    PHA_API_END
}

int pha_hps_decrypt_scale_and_round(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)   // DRNSTool::hps_decrypt_scale_and_round src/rns.cu:1519-1689, the one form of pha_decrypt.h
    hipStream_t s = as_stream(stream);
    launch_scale_round(ctx->c, one_polynomial(ctx->c, "hps_decrypt_scale_and_round src", size_Ql, dst, src, s), dst, 0, src, 0, 1, s);
    PHA_API_END
}

int pha_decrypt_mod_t(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream) {
    PHA_CTX_BEGIN(ctx)   // DRNSTool::decrypt_mod_t: base_q_to_t_conv_.exact_convert_array
    hipStream_t s = as_stream(stream);
    launch_mod_t(ctx->c, one_polynomial(ctx->c, "decrypt_mod_t src", size_Ql, dst, src, s), dst, 0, src, 0, 1, nullptr, s);
    PHA_API_END
}

}  // extern "C"
