// pha_prng.hip -- seeded samplers and key generation on raw buffers: the device work of src/prng.cu (sample_ternary_poly,
// sample_error_poly, sample_uniform_poly) and of the call sequences of PhantomSecretKey that use it (gen_secretkey,
// generate_one_kswitch_key / gen_relinkey / create_galois_keys, src/secretkey.cu:297-460).  The per-thread arithmetic is in
// pha_prng.h; DESIGN.md section 4.14.  Seeds are DEVICE pointers to 64 bytes each; nothing here draws entropy but pha_random_bytes.
//
// Two kernels.  prng_small_kernel (ternary / noise): one generator block per coefficient, written either as ONE signed word (the [N]
// form pha_encrypt_*_batched take) or as the canonical residue of every limb of the reference's [cms][N] layout -- the reference
// recomputes the block per limb, the words are the same.  prng_uniform_kernel: one thread per group of eight coefficients of one row
// (pha_prng.h prng_uniform_group), four 16-byte stores.  blockIdx.z = the polynomial of a batch.
#include "../../include/phantom_amd.h"
#include "pha_prng.h"
#include "pha_internal.h"
#include "pha_ntt_core.h"   // EPI_FWD_CANON

#include <algorithm>
#include <cstring>
#include <random>

namespace pha {

constexpr int kPrngThreads = 256;
static_assert(kPrngGroupWords == 8, "check_degree() of pha_layout.h refuses a degree below one generator block");

// polynomial z: seed at seeds + z * seed_stride bytes, output at out + z * out_stride words.  cms == 0: [N] signed words;
// else [cms][N] canonical residues modulo mod[mod_start + y]
struct PrngSmallArgs {
    u64 *out;
    const uint8_t *seeds;
    const DModulus *mod;
    size_t out_stride, seed_stride;
    uint32_t n, cms, mod_start;
};
template <bool TERNARY>
__global__ __launch_bounds__(kPrngThreads) void prng_small_kernel(const PrngSmallArgs k) {
    const uint32_t i = blockIdx.x * kPrngThreads + threadIdx.x, z = blockIdx.z;
    if (i >= k.n) return;
    const PrngKey key = prng_load_key(k.seeds + (size_t)z * k.seed_stride);
    const PrngBlock b = prng_block(key, i);
    const int v = TERNARY ? prng_ternary_value(b.w[0]) : prng_error_value(b.w[0], b.w[1]);
    u64 *out = k.out + (size_t)z * k.out_stride + i;
    if (k.cms == 0) {
        *out = prng_signed_word(v);
        return;
    }
    for (uint32_t y = 0; y < k.cms; y++) out[(size_t)y * k.n] = prng_residue(v, k.mod[k.mod_start + y].value);
}

// row y of the [rows][N] output uses prime-table row y + row0 for y < l, size_q + (y - l) above (the encoder's row convention; the
// reference layout is l = rows, row0 = mod_start_idx).  The nonce uses the row's POSITION y
struct PrngUniformArgs {
    u64 *out;
    const uint8_t *seeds;
    const DModulus *mod;
    size_t out_stride, seed_stride;
    uint32_t n, rows, l, row0, size_q;
};
__global__ __launch_bounds__(kPrngThreads) void prng_uniform_kernel(const PrngUniformArgs k) {
    const uint32_t j = blockIdx.x * kPrngThreads + threadIdx.x, y = blockIdx.y, z = blockIdx.z, groups = k.n / kPrngGroupWords;
    if (j >= groups) return;
    const DModulus m = k.mod[y < k.l ? k.row0 + y : k.size_q + (y - k.l)];
    const PrngKey key = prng_load_key(k.seeds + (size_t)z * k.seed_stride);
    u64 w[kPrngGroupWords];
    prng_uniform_group(key, (u64)y * groups + j, (u64)k.n * k.rows, m.value, m.ratio1, w);
    u64x2 *out = reinterpret_cast<u64x2 *>(k.out + (size_t)z * k.out_stride + (size_t)y * k.n + (size_t)j * kPrngGroupWords);
#pragma unroll
    for (int h = 0; h < kPrngGroupWords / 2; h++) out[h] = u64x2{w[2 * h], w[2 * h + 1]};
}

// c0 of component b = (key b / dnum, digit d = b % dnum) += P * new_key on the digit's own limbs [d alpha, (d + 1) alpha)
// (generate_one_kswitch_key src/secretkey.cu:318-338, the last term of kswitch_key_kernel)
struct KeyAddArgs {
    u64 *evk;
    const u64 *new_keys;
    const u64x2 *p_mod_q;
    const DModulus *mod;
    size_t evk_stride, new_key_stride;
    uint32_t n, alpha, dnum;
};
__global__ __launch_bounds__(kPrngThreads) void kswitch_add_new_key_kernel(const KeyAddArgs k) {
    const uint32_t b = blockIdx.z, d = b % k.dnum, limb = d * k.alpha + blockIdx.y;
    const u64 q = k.mod[limb].value;
    const size_t at = (size_t)limb * k.n + blockIdx.x * kPrngThreads + threadIdx.x;
    u64 *p = k.evk + (size_t)b * k.evk_stride + at;
    *p = add_mod(*p, shoup(k.new_keys[(size_t)(b / k.dnum) * k.new_key_stride + at], k.p_mod_q[limb], q), q);
}

// ---- launchers (launch only: the callers have validated) ---------------------------------------------------------------------------
static void launch_small(Context &c, bool ternary, u64 *out, size_t out_stride, const uint8_t *seeds, size_t seed_stride, size_t count,
                         uint32_t cms, uint32_t mod_start, hipStream_t s) {
    const PrngSmallArgs k{out, seeds, c.d_mod.p, out_stride, seed_stride, (uint32_t)c.n, cms, mod_start};
    const dim3 grid((unsigned)((c.n + kPrngThreads - 1) / kPrngThreads), 1, (unsigned)count), block(kPrngThreads);
    if (ternary) hipLaunchKernelGGL(prng_small_kernel<true>, grid, block, 0, s, k);
    else hipLaunchKernelGGL(prng_small_kernel<false>, grid, block, 0, s, k);
    check_launch();
}
static void launch_uniform(Context &c, u64 *out, size_t out_stride, const uint8_t *seeds, size_t seed_stride, size_t count, uint32_t l,
                           uint32_t special, uint32_t row0, hipStream_t s) {
    const PrngUniformArgs k{out, seeds, c.d_mod.p, out_stride, seed_stride, (uint32_t)c.n, l + special, l, row0, c.size_q};
    const size_t groups = c.n / kPrngGroupWords;
    hipLaunchKernelGGL(prng_uniform_kernel, dim3((unsigned)((groups + kPrngThreads - 1) / kPrngThreads), l + special, (unsigned)count),
                       dim3(kPrngThreads), 0, s, k);
    check_launch();
}

// ---- what the entries refuse: check_sample_ref, check_sample_batch, check_kswitch of pha_layout.h --------------------------------------
static void sample_ref(pha_context_t ctx, bool ternary, uint64_t *out, const uint8_t *seed, size_t cms, size_t mod_start, void *stream) {
    Context &c = ctx->c;
    check_sample_ref(shape(c), out, seed, cms, mod_start, ternary ? 0 : kNoiseMinPrime);
    launch_small(c, ternary, out, 0, seed, 0, 1, (uint32_t)cms, (uint32_t)mod_start, as_stream(stream));
}
static void sample_signed(pha_context_t ctx, bool ternary, const uint8_t *seeds, size_t count, uint64_t *out, size_t out_stride, void *stream) {
    Context &c = ctx->c;
    check_sample_batch(shape(c), false, 0, false, seeds, count, out, out_stride);
    if (count == 0) return;
    launch_small(c, ternary, out, out_stride, seeds, kPrngSeedBytes, count, 0, 0, as_stream(stream));
}

}  // namespace pha

using namespace pha;

extern "C" {

int pha_random_bytes(unsigned char *host_buf, size_t count) {
    PHA_API_BEGIN
    if (!host_buf && count) throw std::invalid_argument("null host pointer");
    std::random_device rd;   // random_bytes of src/prng.cu: the one place that draws entropy
    for (size_t i = 0; i < count; i += sizeof(uint32_t)) {
        const uint32_t v = rd();
        std::memcpy(host_buf + i, &v, std::min(sizeof(v), count - i));
    }
    PHA_API_END
}

int pha_sample_ternary_poly(pha_context_t ctx, uint64_t *out, const uint8_t *seed, size_t coeff_mod_size, size_t mod_start_idx, void *stream) {
    PHA_CTX_BEGIN(ctx)
    sample_ref(ctx, true, out, seed, coeff_mod_size, mod_start_idx, stream);
    PHA_API_END
}

int pha_sample_error_poly(pha_context_t ctx, uint64_t *out, const uint8_t *seed, size_t coeff_mod_size, size_t mod_start_idx, void *stream) {
    PHA_CTX_BEGIN(ctx)
    sample_ref(ctx, false, out, seed, coeff_mod_size, mod_start_idx, stream);
    PHA_API_END
}

int pha_sample_uniform_poly(pha_context_t ctx, uint64_t *out, const uint8_t *seed, size_t coeff_mod_size, size_t mod_start_idx, void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    check_sample_ref(shape(c), out, seed, coeff_mod_size, mod_start_idx, 0);
    launch_uniform(c, out, 0, seed, 0, 1, (uint32_t)coeff_mod_size, 0, (uint32_t)mod_start_idx, as_stream(stream));
    PHA_API_END
}

int pha_sample_ternary_signed_batched(pha_context_t ctx, const uint8_t *seeds, size_t count, uint64_t *out, size_t out_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    sample_signed(ctx, true, seeds, count, out, out_stride, stream);
    PHA_API_END
}

int pha_sample_error_signed_batched(pha_context_t ctx, const uint8_t *seeds, size_t count, uint64_t *out, size_t out_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    sample_signed(ctx, false, seeds, count, out, out_stride, stream);
    PHA_API_END
}

int pha_sample_uniform_batched(pha_context_t ctx, size_t size_Ql, int with_special, const uint8_t *seeds, size_t count, uint64_t *out,
                               size_t out_stride, void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    check_sample_batch(shape(c), true, size_Ql, with_special != 0, seeds, count, out, out_stride);
    const uint32_t special = with_special ? c.size_p : 0u;
    if (count == 0) return 0;
    launch_uniform(c, out, out_stride, seeds, kPrngSeedBytes, count, (uint32_t)size_Ql, special, 0, as_stream(stream));
    PHA_API_END
}

int pha_secret_key_generate(pha_context_t ctx, const uint8_t *seed, uint64_t *sk_ntt, void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    sample_ref(ctx, true, sk_ntt, seed, c.size_qp, 0, stream);   // gen_secretkey: the ternary sample over all QP limbs ...
    ntt_forward(c, sk_ntt, sk_ntt, sk_ntt, plain_sel(0, c.size_qp), EPI_FWD_CANON, NttExtra{}, as_stream(stream));   // ... transformed in place
    PHA_API_END
}

int pha_generate_kswitch_keys_seeded(pha_context_t ctx, const uint64_t *sk_ntt, const uint64_t *new_keys_ntt, size_t n_keys,
                                     size_t new_key_stride, const uint8_t *seeds, uint64_t *evk, size_t evk_stride, int scheme,
                                     void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    const size_t dnum = check_kswitch(shape(c), sk_ntt, new_keys_ntt, n_keys, new_key_stride, seeds, evk, evk_stride, scheme,
                                      [&] { return c.tool(c.size_q).bgv_ready; });
    const size_t n = c.n, qp_n = (size_t)c.size_qp * n, count = n_keys * dnum;
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    // component b = (key, digit): seeds + 128 b = the uniform seed, then the noise seed
    u64 *e = c.scratch_outer(stream, count * n);
    launch_uniform(c, evk + qp_n, evk_stride, seeds, 2 * kPrngSeedBytes, count, c.size_q, c.size_p, 0, s);          // a, where c1 lies
    launch_small(c, false, e, n, seeds + kPrngSeedBytes, 2 * kPrngSeedBytes, count, 0, 0, s);                       // e, [N] signed words
    rc(pha_encrypt_zero_symmetric_batched(ctx, c.size_q, 1, sk_ntt, e, n, evk, count > 1 ? evk_stride : 2 * qp_n, count, scheme, 1,
                                          stream));                                                                  // c0 = -(a s + NTT(k e))
    const KeyAddArgs k{evk, new_keys_ntt, c.tool(c.size_q).p_mod_q2.p, c.d_mod.p, evk_stride, new_key_stride, (uint32_t)n, c.size_p, (uint32_t)dnum};
    hipLaunchKernelGGL(kswitch_add_new_key_kernel, dim3((unsigned)(n / kPrngThreads), c.size_p, (unsigned)count), dim3(kPrngThreads), 0, s, k);
    check_launch();
    PHA_API_END
}

}  // extern "C"
