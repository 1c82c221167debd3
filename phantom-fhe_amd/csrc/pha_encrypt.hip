// pha_encrypt.hip -- encryption on raw buffers: the device work of PhantomSecretKey::encrypt_zero_symmetric / gen_publickey /
// encrypt_symmetric and PhantomPublicKey::encrypt_zero_asymmetric / encrypt_asymmetric (src/secretkey.cu:11-192, 232-295, 382-395,
// 463-531) for BATCHES of ciphertexts, with caller-supplied randomness (as pha_generate_one_kswitch_key takes it).  The per-thread
// arithmetic and its bounds are in pha_encrypt.h; DESIGN.md section 4.12.
//
// NTT form (ckks, bgv): ONE forward transform per ciphertext is the whole symmetric encryption.  Its load lifts the shared [N] signed
// noise words modulo each limb's prime (PRO_SMALL, times t under bgv), its store forms -(a (.) s + NTT(k e)) + plain from the
// ciphertext's own c1, the key limb and the NTT-form plaintext (EPI_FWD_NEG_MULADD): no intermediate is written.  Global words per
// word of c0: a, s, plain and the store = 4 on the one-pass plans (N <= 8192 from 64 limb-polynomials, N = 4096 always) plus the N
// shared sample words; 6 on the two-pass plans (the intermediate is written and read once).  The loop of existing entries
// (forward transform of the [L][N] noise residues it is handed, multiply_and_add_negate, add) costs 10 / 12 -- derived, not measured.
// The asymmetric form uses the same two pieces: NTT(u) once per ciphertext (PRO_SMALL, canonical store), two fused transforms
// c_j = pk_j (.) NTT(u) + NTT(k e_j) over rows [0, l) u P (EPI_FWD_MULADD), the batched mod-down of the key switch over 2 * chunk
// polynomials, the plaintext step.
// Coefficient form (bfv): element-wise products, batched inverse transforms, the noise added from the [N] samples, the scaling-variant
// plaintext -- small kernels per chunk, nothing fused (the [L][N] residue form of a sample is still never written).
#include "../../include/phantom_amd.h"
#include "pha_encrypt.h"
#include "pha_internal.h"
#include "pha_ntt_core.h"

#include <algorithm>

namespace pha {

constexpr int kEncThreads = 256;
constexpr size_t kEncChunk = 8;          // ciphertexts per set of launches of the asymmetric entry (work buffer: chunk * (5 l + 3 alpha) * N words)
constexpr size_t kEncPlainChunk = 64;    // bgv, symmetric: plaintexts lifted per launch (work buffer: chunk * l * N words)

// a ciphertext polynomial of `l` data rows, then `special` special rows: the prime-table row of buffer row y
struct EncRows {
    uint32_t l, special, size_q;
    __host__ __device__ uint32_t rows() const { return l + special; }
    __host__ __device__ uint32_t prime(uint32_t y) const { return y < l ? y : size_q + (y - l); }
};

// polynomial z of the launch.  pair == 0: dst + z * dst_stride = (a + z * a_stride) (.) key;
// pair == 1: z = 2 b + j: dst + z * dst_stride = (a + b * a_stride) (.) (key + j * key_half).  key rows are prime-table rows.
struct EncMulArgs {
    u64 *dst;
    const u64 *a, *key;
    const DModulus *mod;
    size_t dst_stride, a_stride, key_half;
    EncRows rows;
    uint32_t n, pair;
};
__global__ __launch_bounds__(kEncThreads) void enc_mul_kernel(const EncMulArgs k) {
    const uint32_t y = blockIdx.y, z = blockIdx.z, prime = k.rows.prime(y);
    const size_t i = (size_t)blockIdx.x * kEncThreads + threadIdx.x, at = (size_t)y * k.n + i;
    const u64 *a = k.a + (size_t)(k.pair ? z >> 1 : z) * k.a_stride;
    const u64 *key = k.key + (k.pair ? (size_t)(z & 1) * k.key_half : 0) + (size_t)prime * k.n;
    k.dst[(size_t)z * k.dst_stride + at] = mul_mod(a[at], key[i], k.mod[prime]);
}

// dst + z * dst_stride = +-(that + [v]) with v the signed samples at e + z * e_stride (pair == 0) or e + b * e_stride + j * N (z = 2 b + j)
struct EncNoiseArgs {
    u64 *dst;
    const u64 *e;
    const DModulus *mod;
    size_t dst_stride, e_stride;
    EncRows rows;
    uint32_t n, pair;
};
template <bool NEG>
__global__ __launch_bounds__(kEncThreads) void enc_noise_kernel(const EncNoiseArgs k) {
    const uint32_t y = blockIdx.y, z = blockIdx.z;
    const u64 q = k.mod[k.rows.prime(y)].value;
    const size_t i = (size_t)blockIdx.x * kEncThreads + threadIdx.x;
    const u64 *e = k.pair ? k.e + (size_t)(z >> 1) * k.e_stride + (size_t)(z & 1) * k.n : k.e + (size_t)z * k.e_stride;
    u64 *p = k.dst + (size_t)z * k.dst_stride + (size_t)y * k.n + i;
    const u64 r = add_mod(*p, small_lift(e[i], q), q);
    *p = NEG ? neg_mod(r, q) : r;
}

// c0 (b) += plain (b): [l][N] NTT-form words (mode 0), or the scaling variant of [N] words below t (mode 1:
// multiply_add_plain_with_scaling_variant, the arithmetic of bfv_add_timesQ_overt_kernel)
struct EncPlainArgs {
    u64 *ct;
    const u64 *plain;
    const DModulus *mod;
    const u64 *t_inv, *t_inv_shoup;   // mode 1: [l] t^-1 mod q_i
    u64x2 neg_ql_mod_t;
    u64 t;
    size_t ct_stride, plain_stride;
    uint32_t n, mode;
};
__global__ __launch_bounds__(kEncThreads) void enc_plain_kernel(const EncPlainArgs k) {
    const uint32_t y = blockIdx.y, z = blockIdx.z;
    const u64 q = k.mod[y].value;
    const size_t i = (size_t)blockIdx.x * kEncThreads + threadIdx.x;
    u64 *p = k.ct + (size_t)z * k.ct_stride + (size_t)y * k.n + i;
    const u64 *pl = k.plain + (size_t)z * k.plain_stride;
    u64 v;
    if (k.mode == 0) v = pl[(size_t)y * k.n + i];
    else v = shoup(shoup(pl[i], k.neg_ql_mod_t, k.t), u64x2{k.t_inv[y], k.t_inv_shoup[y]}, q);
    *p = add_mod(*p, v, q);
}

// strict mode: sample words whose magnitude exceeds 2^16
struct SampleCountArgs {
    const u64 *data;
    unsigned long long *count;
    size_t stride;
};
__global__ __launch_bounds__(kEncThreads) void sample_count_kernel(const SampleCountArgs k) {
    const size_t i = (size_t)blockIdx.x * kEncThreads + threadIdx.x;
    const bool bad = small_magnitude(k.data[(size_t)blockIdx.y * k.stride + i]) > kSmallSampleMax;
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(k.count, (unsigned long long)__popcll(m));
}
// `polys` runs of `words` sample words (a multiple of N), `stride` apart
static void strict_samples(Context &c, const char *what, const u64 *data, size_t words, size_t polys, size_t stride, hipStream_t s) {
    if (!strict_mode() || !data || polys == 0) return;
    unsigned long long *d_count = nullptr, host = 0;
    PHA_HIP(hipMalloc(&d_count, sizeof(unsigned long long)));   // (a debugging path, like the other strict counts)
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        const SampleCountArgs k{data, d_count, stride};
        hipLaunchKernelGGL(sample_count_kernel, dim3((unsigned)(words / kEncThreads), (unsigned)polys), dim3(kEncThreads), 0, s, k);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host, d_count, sizeof(host), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_count);
    PHA_HIP(e);
    if (host)
        throw std::invalid_argument(std::string("PHA_STRICT: ") + what + " holds " + std::to_string(host) +
                                    " word(s) of magnitude above 2^16 (a sample is a signed 64-bit word, |v| <= 2^16; include/phantom_amd.h)");
}

// ---- launchers (launch only: the callers have validated) ---------------------------------------------------------------------------
static void launch_mul(Context &c, const EncRows &r, u64 *dst, size_t dst_stride, const u64 *a, size_t a_stride, const u64 *key, bool pair,
                       size_t polys, hipStream_t s) {
    const EncMulArgs k{dst, a, key, c.d_mod.p, dst_stride, a_stride, (size_t)c.size_qp * c.n, r, (uint32_t)c.n, pair ? 1u : 0u};
    hipLaunchKernelGGL(enc_mul_kernel, dim3((unsigned)(c.n / kEncThreads), r.rows(), (unsigned)polys), dim3(kEncThreads), 0, s, k);
    check_launch();
}
static void launch_noise(Context &c, const EncRows &r, u64 *dst, size_t dst_stride, const u64 *e, size_t e_stride, bool pair, bool negate,
                         size_t polys, hipStream_t s) {
    const EncNoiseArgs k{dst, e, c.d_mod.p, dst_stride, e_stride, r, (uint32_t)c.n, pair ? 1u : 0u};
    const dim3 grid((unsigned)(c.n / kEncThreads), r.rows(), (unsigned)polys), block(kEncThreads);
    if (negate) hipLaunchKernelGGL(enc_noise_kernel<true>, grid, block, 0, s, k);
    else hipLaunchKernelGGL(enc_noise_kernel<false>, grid, block, 0, s, k);
    check_launch();
}
// c0 (b) += the plaintext, b < B.  ntt_plain: plain (b) is [l][N] in NTT form; else the bfv scaling variant of [N] words below t
static void launch_plain(Context &c, size_t l, u64 *ct, size_t ct_stride, const u64 *plain, size_t plain_stride, bool ntt_plain, size_t B,
                         hipStream_t s) {
    EncPlainArgs k{ct, plain, c.d_mod.p, nullptr, nullptr, u64x2{0, 0}, 0, ct_stride, plain_stride, (uint32_t)c.n, ntt_plain ? 0u : 1u};
    if (!ntt_plain) {
        Tool &t = c.tool((uint32_t)l);
        k.t_inv = t.t_inv_mod_q.p;
        k.t_inv_shoup = t.t_inv_mod_q_shoup.p;
        k.neg_ql_mod_t = t.neg_ql_mod_t;
        k.t = c.plain_t;
    }
    hipLaunchKernelGGL(enc_plain_kernel, dim3((unsigned)(c.n / kEncThreads), (unsigned)l, (unsigned)B), dim3(kEncThreads), 0, s, k);
    check_launch();
}
// the two row ranges of a [rows][N] polynomial: f(selection, words to add to a prime-row-indexed operand so that buffer row y finds its prime's row)
template <class F>
static void for_row_ranges(Context &c, const EncRows &r, F &&f) {
    f(plain_sel(0, r.l), (size_t)0);
    if (r.special) f(special_sel(r.l, r.special, c.size_qp, c.size_p), (size_t)(c.size_q - r.l) * c.n);
}
// B polynomials `stride` apart, [rows][N] each, forward from signed samples (canonical store) or backward in place
static void transform_samples(Context &c, const EncRows &r, const u64 *src, size_t src_stride, u64 *dst, size_t stride, size_t B, hipStream_t s) {
    for_row_ranges(c, r, [&](const LimbSel &sel, size_t) {
        NttExtra x;
        x.batch = (uint32_t)B;
        x.poly_stride = stride;
        x.pro_src = src;
        x.pro_stride = src_stride;
        x.pro_small = true;
        ntt_forward(c, dst, dst, dst, sel, EPI_FWD_CANON, x, s);
    });
}
static void inverse_polys(Context &c, const EncRows &r, u64 *p, size_t stride, size_t polys, hipStream_t s) {
    for_row_ranges(c, r, [&](const LimbSel &sel, size_t) {
        NttExtra x;
        x.batch = (uint32_t)polys;
        x.poly_stride = stride;
        ntt_inverse(c, p, p, p, sel, EPI_INV_CANON, x, s);
    });
}
// the fused transform: out (z) = +-(f0 (z) (.) f1 (z) + NTT(k e (z))) [+ p (z)] over the rows of r; `by_prime` names the factor (0 / 1)
// whose rows are prime-table rows (the key, the public key) instead of buffer rows
struct FusedOperands {
    const u64 *f[2];
    size_t f_stride[2];
    int by_prime;
    const u64 *p;
    size_t p_stride;
};
static void launch_fused(Context &c, const EncRows &r, int epi, const u64 *e, size_t e_stride, u64 k_factor, const FusedOperands &o, u64 *out,
                         size_t out_stride, size_t B, hipStream_t s) {
    for_row_ranges(c, r, [&](const LimbSel &sel, size_t prime_shift) {
        NttExtra x;
        x.batch = (uint32_t)B;
        x.poly_stride = out_stride;
        x.pro_src = e;
        x.pro_stride = e_stride;
        x.pro_small = true;
        x.pro_small_k = k_factor;
        x.aux = o.f[0] + (o.by_prime == 0 ? prime_shift : 0);
        x.aux2 = o.f[1] + (o.by_prime == 1 ? prime_shift : 0);
        x.aux3 = o.p;
        x.muladd_stride[0] = o.f_stride[0];
        x.muladd_stride[1] = o.f_stride[1];
        x.muladd_stride[2] = o.p_stride;
        ntt_forward(c, out, out, out, sel, epi, x, s);
    });
}

// strict mode: the uniform words found in c1's place, over the rows of r
static void strict_a(Context &c, const char *what, const EncRows &r, const u64 *ct, size_t ct_stride, size_t count, hipStream_t s) {
    const RowMap rows = r.special ? rows_qlp(r.l, c.size_q, c.size_p) : rows_plain(0, r.l);
    strict_operand(c, what, ct + (size_t)r.rows() * c.n, rows, (uint32_t)count, ct_stride, s);
}
static void strict_key(Context &c, const char *what, const EncRows &r, const u64 *key, uint32_t polys, hipStream_t s) {
    strict_operand(c, what, key, rows_plain(0, r.l), polys, (size_t)c.size_qp * c.n, s);
    if (r.special) strict_operand(c, what, key + (size_t)c.size_q * c.n, rows_plain(c.size_q, c.size_p), polys, (size_t)c.size_qp * c.n, s);
}
static void strict_plaintext(Context &c, const char *what, int scheme, size_t l, const u64 *plain, size_t plain_stride, size_t count, hipStream_t s) {
    const size_t polys = count > 1 && plain_stride == 0 ? 1 : count;
    if (scheme == PHA_SCHEME_CKKS) strict_operand(c, what, plain, rows_plain(0, l), (uint32_t)polys, plain_stride, s);
    else strict_plain(c, what, plain, c.plain_t, polys, plain_stride, s);
}

// bgv: NTT(m mod q_i) of `polys` plaintexts of [N] words below t into work [polys][l][N] (pha_bgv_lift_plain for a chunk: every limb
// reduces the same N words modulo its own prime on load)
static void lift_plain(Context &c, size_t size_Ql, const u64 *plain, size_t plain_stride, u64 *work, size_t polys, hipStream_t s) {
    NttExtra x;
    x.batch = (uint32_t)polys;
    x.poly_stride = size_Ql * c.n;
    x.pro_src = plain;
    x.pro_stride = plain_stride;
    ntt_forward(c, work, work, work, plain_sel(0, size_Ql), EPI_FWD_CANON, x, s);
}

// the zero encryption of B ciphertexts over the rows of r, in place of ct (c1 holds a): NTT form with the optional NTT-form plaintext
// fused, or coefficient form
static void zero_symmetric(Context &c, const EncRows &r, const u64 *sk, const u64 *e, size_t e_stride, u64 *ct, size_t ct_stride, size_t B,
                           int scheme, bool ntt_form, const u64 *plain_ntt, size_t plain_stride, hipStream_t s) {
    const size_t rn = (size_t)r.rows() * c.n;
    const size_t cs = B > 1 ? ct_stride : 2 * rn;
    if (ntt_form) {
        const FusedOperands o{{ct + rn, sk}, {cs, 0}, 1, plain_ntt, plain_stride};
        return launch_fused(c, r, EPI_FWD_NEG_MULADD, e, e_stride, scheme == PHA_SCHEME_BGV ? c.plain_t : 0, o, ct, cs, B, s);
    }
    launch_mul(c, r, ct, cs, ct + rn, cs, sk, false, B, s);                    // c0 = a (.) s
    if (cs == 2 * rn && 2 * B <= kMaxCount) inverse_polys(c, r, ct, rn, 2 * B, s);   // c0, c1 of every ciphertext lie in a row
    else {
        inverse_polys(c, r, ct, cs, B, s);
        inverse_polys(c, r, ct + rn, cs, B, s);
    }
    launch_noise(c, r, ct, cs, e, e_stride, false, true, B, s);               // c0 = -(c0 + e)
}

}  // namespace pha

using namespace pha;

extern "C" {

int pha_encrypt_zero_symmetric_batched(pha_context_t ctx, size_t size_Ql, int with_special, const uint64_t *sk_ntt, const uint64_t *e,
                                       size_t e_stride, uint64_t *ct, size_t ct_stride, size_t count, int scheme, int ntt_form,
                                       void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    check_encrypt(shape(c), size_Ql, with_special != 0, false, scheme, sk_ntt, nullptr, 0, e, e_stride, nullptr, 0, 0, ct, ct_stride, count);
    const EncRows r{(uint32_t)size_Ql, with_special ? c.size_p : 0u, c.size_q};
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    strict_key(c, "encrypt_zero_symmetric sk", r, sk_ntt, 1, s);
    strict_a(c, "encrypt_zero_symmetric a", r, ct, ct_stride, count, s);
    strict_samples(c, "encrypt_zero_symmetric samples", e, c.n, count, e_stride, s);
    zero_symmetric(c, r, sk_ntt, e, e_stride, ct, ct_stride, count, scheme, ntt_form != 0, nullptr, 0, s);
    PHA_API_END
}

int pha_public_key_generate(pha_context_t ctx, const uint64_t *sk_ntt, const uint64_t *e, uint64_t *pk, int scheme, void *stream) {
    if (!ctx) return pha_encrypt_zero_symmetric_batched(ctx, 0, 1, sk_ntt, e, 0, pk, 0, 1, scheme, 1, stream);
    return pha_encrypt_zero_symmetric_batched(ctx, ctx->c.size_q, 1, sk_ntt, e, 0, pk, 0, 1, scheme, 1, stream);   // gen_publickey: the key level, NTT form
}

int pha_encrypt_symmetric_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *sk_ntt, const uint64_t *e, size_t e_stride,
                                  const uint64_t *plain, size_t plain_stride, uint64_t *ct, size_t ct_stride, size_t count, int scheme,
                                  void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    const size_t ln = size_Ql * c.n, pw = scheme == PHA_SCHEME_CKKS ? ln : c.n;
    check_encrypt(shape(c), size_Ql, false, false, scheme, sk_ntt, nullptr, 0, e, e_stride, plain, pw, plain_stride, ct, ct_stride, count);
    const EncRows r{(uint32_t)size_Ql, 0u, c.size_q};
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    strict_key(c, "encrypt_symmetric sk", r, sk_ntt, 1, s);
    strict_a(c, "encrypt_symmetric a", r, ct, ct_stride, count, s);
    strict_plaintext(c, "encrypt_symmetric plain", scheme, size_Ql, plain, plain_stride, count, s);
    strict_samples(c, "encrypt_symmetric samples", e, c.n, count, e_stride, s);
    if (scheme == PHA_SCHEME_CKKS) {          // c0 += plain, in the transform's store
        zero_symmetric(c, r, sk_ntt, e, e_stride, ct, ct_stride, count, scheme, true, plain, plain_stride, s);
    } else if (scheme == PHA_SCHEME_BGV) {    // c0 += NTT(m mod q_i): the plaintexts of a chunk are transformed into the work buffer first
        const bool shared = count > 1 && plain_stride == 0;
        const size_t C = shared ? count : std::min(kEncPlainChunk, count);
        u64 *work = c.scratch_outer(stream, (shared ? 1 : C) * ln);
        for (size_t b0 = 0; b0 < count; b0 += C) {
            const size_t B = std::min(C, count - b0);
            if (b0 == 0 || !shared) lift_plain(c, size_Ql, plain + b0 * plain_stride, plain_stride, work, shared ? 1 : B, s);
            zero_symmetric(c, r, sk_ntt, e + b0 * e_stride, e_stride, ct + b0 * ct_stride, ct_stride, B, scheme, true, work, shared ? 0 : ln, s);
        }
    } else {                                  // bfv: coefficient form, then multiply_add_plain_with_scaling_variant
        zero_symmetric(c, r, sk_ntt, e, e_stride, ct, ct_stride, count, scheme, false, nullptr, 0, s);
        launch_plain(c, size_Ql, ct, ct_stride, plain, plain_stride, false, count, s);
    }
    PHA_API_END
}

int pha_encrypt_asymmetric_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *pk, const uint64_t *u, size_t u_stride,
                                   const uint64_t *e, size_t e_stride, const uint64_t *plain, size_t plain_stride, uint64_t *ct,
                                   size_t ct_stride, size_t count, int scheme, size_t chunk, void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    const EncRows r{(uint32_t)size_Ql, c.size_p, c.size_q};
    const size_t n = c.n, ln = size_Ql * n, rn = (size_t)r.rows() * n, pw = scheme == PHA_SCHEME_CKKS ? ln : n;
    check_encrypt(shape(c), size_Ql, true, true, scheme, pk, u, u_stride, e, e_stride, plain, pw, plain_stride, ct, ct_stride, count);
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    strict_key(c, "encrypt_asymmetric pk", r, pk, 2, s);
    strict_plaintext(c, "encrypt_asymmetric plain", scheme, size_Ql, plain, plain_stride, count, s);
    strict_samples(c, "encrypt_asymmetric samples", u, n, count, u_stride, s);
    strict_samples(c, "encrypt_asymmetric samples", e, 2 * n, count, e_stride, s);
    Tool &t = c.tool((uint32_t)size_Ql);
    const bool ntt_form = scheme != PHA_SCHEME_BFV, bgv = scheme == PHA_SCHEME_BGV, shared = count > 1 && plain_stride == 0;
    const size_t C = std::min<size_t>(std::min(chunk ? chunk : kEncChunk, count), 32767);
    // the work buffer: NTT(u) [C][rows][N] | c_0, c_1 over Q_l u P [C][2][rows][N] | the mod-down's delta [2 C][l][N] | bgv: NTT(m) [C][l][N]
    const size_t pl_words = bgv ? (shared ? 1 : C) * ln : 0;
    u64 *unt = c.scratch_outer(stream, C * (3 * rn + 2 * ln) + pl_words), *cx = unt + C * rn, *delta = cx + C * 2 * rn, *pl = delta + C * 2 * ln;
    const size_t qp_n = (size_t)c.size_qp * n;
    for (size_t b0 = 0; b0 < count; b0 += C) {
        const size_t B = std::min(C, count - b0);
        const u64 *eb = e + b0 * e_stride;
        u64 *cb = ct + b0 * ct_stride;
        transform_samples(c, r, u + b0 * u_stride, u_stride, unt, rn, B, s);                       // NTT(u), k = 1 in every scheme
        if (ntt_form) {   // c_j = pk_j (.) NTT(u) + NTT(k e_j), one fused transform per j
            for (int j = 0; j < 2; j++) {
                const FusedOperands o{{pk + j * qp_n, unt}, {0, rn}, 0, nullptr, 0};
                launch_fused(c, r, EPI_FWD_MULADD, eb + j * n, e_stride, bgv ? c.plain_t : 0, o, cx + j * rn, 2 * rn, B, s);
            }
        } else {          // c_j = iNTT(pk_j (.) NTT(u)) + e_j
            launch_mul(c, r, cx, rn, unt, rn, pk, true, 2 * B, s);
            inverse_polys(c, r, cx, rn, 2 * B, s);
            launch_noise(c, r, cx, rn, eb, e_stride, true, false, 2 * B, s);
        }
        // DRNSTool::moddown of both polynomials of every ciphertext of the chunk
        if (B == 1 || ct_stride == 2 * ln) {
            moddown_from_ntt(c, t, cb, ln, cx, rn, (uint32_t)(2 * B), scheme, false, delta, s, false, !ntt_form);
        } else {
            for (int j = 0; j < 2; j++)
                moddown_from_ntt(c, t, cb + j * ln, ct_stride, cx + j * rn, 2 * rn, (uint32_t)B, scheme, false, delta, s, false, !ntt_form);
        }
        // the plaintext step of encrypt_asymmetric on c0
        const u64 *pb = plain + b0 * plain_stride;
        const size_t cs = B > 1 ? ct_stride : 2 * ln;
        if (bgv) {
            if (b0 == 0 || !shared) lift_plain(c, size_Ql, pb, plain_stride, pl, shared ? 1 : B, s);
            launch_plain(c, size_Ql, cb, cs, pl, shared ? 0 : ln, true, B, s);
        } else {
            launch_plain(c, size_Ql, cb, cs, pb, plain_stride, ntt_form, B, s);
        }
    }
    PHA_API_END
}

}  // extern "C"
