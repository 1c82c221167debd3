// pha_noise.hip -- noise as a device-side quantity: the exact infinity norm of RNS polynomials and the invariant noise budget of
// BATCHES of ciphertexts (PhantomSecretKey::invariant_noise_budget, src/secretkey.cu:752-840, which composes on the host with
// multi-precision integers, one ciphertext per call behind a stream synchronise).  The per-thread programs and their bounds are in
// pha_noise.h, the tables in pha_rns_tables.h (noise_tables / noise_level_tables); DESIGN.md section 4.15.
//
// norm_kernel: one coefficient per thread.  The thread's column of L residues (times scalar mod q_i) lives in LDS laid out
// [limb][thread] -- L is a run-time value up to 64, and a dynamically indexed private array would go to scratch memory; consecutive
// lanes touch consecutive 8-byte words, so no access conflicts.  Garner turns the column into mixed-radix digits in place, the digits
// are compared with those of (Q - 1) / 2 and negated where above, and a tree over the workgroup's columns leaves the lexicographic
// maximum in column 0: ONE candidate [L] per workgroup goes to the work buffer.  The tables are indexed by loop counters only
// (wave-uniform).  finish_kernel: one workgroup per polynomial takes the maximum of the candidates, one thread converts the winner
// to binary (Horner, L-word arithmetic in LDS) and writes norm, bits and the budget.  No atomics: the result does not depend on the
// order in which workgroups run.
#include "../../include/phantom_amd.h"
#include "pha_internal.h"
#include "pha_noise.h"
#include "pha_ntt_core.h"

#include <algorithm>

namespace pha {

constexpr int kFinishThreads = 256;
// workgroup size of norm_kernel: L * threads * 8 bytes of LDS, at most 32 KiB
static uint32_t norm_threads(size_t size_Ql, size_t n) { return (uint32_t)std::min<size_t>(size_Ql > 32 ? 64 : 128, n); }

struct NormArgs {
    const u64 *src;
    u64 *cand;               // [count][workgroups per polynomial][L]
    const DModulus *mod;
    const u64x2 *inv;
    const u64 *lift, *half;
    uint32_t n, limbs, pitch, scaled;
    size_t src_stride;
    u64 scal[kNoiseMaxLimbs];   // scalar mod q_i (host-reduced: t can exceed a limb)
};

struct LdsCol {
    u64 *p;                  // this thread's word of limb 0
    uint32_t pitch;
    __device__ __forceinline__ u64 &operator()(uint32_t i) const { return p[(size_t)i * pitch]; }
};
struct ModOf {
    const DModulus *mod;
    __device__ __forceinline__ u64 operator()(uint32_t i) const { return mod[i].value; }
};
struct InvOf {
    const u64x2 *inv;
    uint32_t pitch;
    __device__ __forceinline__ u64x2 operator()(uint32_t i, uint32_t j) const { return inv[(size_t)i * pitch + j]; }
};
struct WordOf {
    const u64 *p;
    __device__ __forceinline__ u64 operator()(uint32_t i) const { return p[i]; }
};

__global__ __launch_bounds__(128) void norm_kernel(const NormArgs k) {
    extern __shared__ u64 noise_cols[];   // [L][threads]
    const uint32_t T = blockDim.x, tid = threadIdx.x, L = k.limbs;
    const size_t z = blockIdx.y;
    const u64 *src = k.src + z * k.src_stride + (size_t)blockIdx.x * T + tid;
    LdsCol col{noise_cols + tid, T};
    for (uint32_t i = 0; i < L; i++) {
        const u64 x = src[(size_t)i * k.n];
        col(i) = k.scaled ? mul_mod(x, k.scal[i], k.mod[i]) : x;
    }
    const ModOf q{k.mod};
    noise_garner(col, L, q, InvOf{k.inv, k.pitch}, WordOf{k.lift});
    noise_magnitude(col, L, q, WordOf{k.half});
    for (uint32_t s = T / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            const LdsCol other{noise_cols + tid + s, T};
            if (noise_greater(other, col, L))
                for (uint32_t i = 0; i < L; i++) col(i) = other(i);
        }
    }
    __syncthreads();
    u64 *cand = k.cand + (z * gridDim.x + blockIdx.x) * L;
    for (uint32_t i = tid; i < L; i += T) cand[i] = noise_cols[(size_t)i * T];
}

struct FinishArgs {
    const u64 *cand;
    const DModulus *mod;
    u64 *norm;               // [count][L], or null
    uint32_t *bits;          // [count], or null
    int32_t *budget;         // [count], or null
    uint32_t limbs, ncand;
    int q_bits;
};

__global__ __launch_bounds__(kFinishThreads) void finish_kernel(const FinishArgs k) {
    __shared__ uint32_t best[kFinishThreads];
    __shared__ u64 acc[kNoiseMaxLimbs];
    const uint32_t tid = threadIdx.x, L = k.limbs;
    const size_t z = blockIdx.x;
    const u64 *cand = k.cand + z * k.ncand * L;
    uint32_t b = tid < k.ncand ? tid : 0;
    for (uint32_t c = tid + kFinishThreads; c < k.ncand; c += kFinishThreads)
        if (noise_greater(WordOf{cand + (size_t)c * L}, WordOf{cand + (size_t)b * L}, L)) b = c;
    best[tid] = b;
    for (uint32_t s = kFinishThreads / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            const uint32_t o = best[tid + s], m = best[tid];
            if (noise_greater(WordOf{cand + (size_t)o * L}, WordOf{cand + (size_t)m * L}, L)) best[tid] = o;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    noise_horner(WordOf{cand + (size_t)best[0] * L}, L, ModOf{k.mod}, acc);
    const uint32_t nb = noise_bits(acc, L);
    if (k.norm)
        for (uint32_t w = 0; w < L; w++) k.norm[z * L + w] = acc[w];
    if (k.bits) k.bits[z] = nb;
    if (k.budget) k.budget[z] = noise_budget(k.q_bits, nb);
}

NoiseBase &Context::noise_base() {
    std::lock_guard<std::mutex> lk(mu);
    if (noise_tables) return *noise_tables;
    PHA_HIP(hipSetDevice(device));
    const NoiseTables t = pha::noise_tables(primes, std::min<uint32_t>(size_q, kNoiseMaxLimbs));
    auto b = std::make_unique<NoiseBase>();
    b->size = t.size;
    b->inv.upload(t.inv);
    b->lift.upload(t.lift);
    noise_tables = std::move(b);
    return *noise_tables;
}

NoiseLevel &Context::noise_level(uint32_t size_ql) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = noise_levels.find(size_ql);
    if (it != noise_levels.end()) return *it->second;
    PHA_HIP(hipSetDevice(device));
    const NoiseLevelTables t = noise_level_tables(primes, size_ql);
    auto d = std::make_unique<NoiseLevel>();
    d->size = size_ql;
    d->q_bits = t.q_bits;
    d->half.upload(t.half);
    return *(noise_levels[size_ql] = std::move(d));
}

static size_t norm_cand_words(Context &c, size_t size_Ql, size_t count) { return count * (c.n / norm_threads(size_Ql, c.n)) * size_Ql; }

// launch only: `count` <= 65535 polynomials [L][N] at src + z * src_stride -> norm / bits / budget (each may be null) at index z
static void launch_norm(Context &c, size_t size_Ql, const u64 *src, size_t count, size_t src_stride, u64 scalar, u64 *cand, u64 *norm,
                        uint32_t *bits, int32_t *budget, hipStream_t s) {
    NoiseBase &base = c.noise_base();
    NoiseLevel &lvl = c.noise_level((uint32_t)size_Ql);
    const uint32_t T = norm_threads(size_Ql, c.n), per_poly = (uint32_t)(c.n / T);
    NormArgs k{src, cand, c.d_mod.p, base.inv.p, base.lift.p, lvl.half.p, (uint32_t)c.n, (uint32_t)size_Ql, base.size, scalar != 1, src_stride, {}};
    for (size_t i = 0; i < size_Ql; i++) k.scal[i] = scalar % c.primes[i];
    hipLaunchKernelGGL(norm_kernel, dim3(per_poly, (unsigned)count), dim3(T), size_Ql * T * sizeof(u64), s, k);
    check_launch();
    const FinishArgs f{cand, c.d_mod.p, norm, bits, budget, (uint32_t)size_Ql, per_poly, lvl.q_bits};
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)count), dim3(kFinishThreads), 0, s, f);
    check_launch();
}

}  // namespace pha

using namespace pha;

extern "C" {

int pha_poly_infty_norm_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *src, size_t count, size_t src_stride,
                                uint64_t scalar, uint64_t *norm, uint32_t *bits, void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    check_poly_norm(shape(c), size_Ql, src, count, src_stride, norm, bits, kNoiseMaxLimbs);
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    if (strict_mode())
        for (size_t z0 = 0; z0 < count; z0 += 65535)
            strict_operand(c, "poly_infty_norm src", src + z0 * src_stride, rows_plain(0, size_Ql), (uint32_t)std::min<size_t>(65535, count - z0),
                           src_stride, s);
    const size_t C = std::min<size_t>(count, 65535);
    u64 *cand = c.scratch_outer(stream, norm_cand_words(c, size_Ql, C));
    for (size_t z0 = 0; z0 < count; z0 += C)
        launch_norm(c, size_Ql, src + z0 * src_stride, std::min(C, count - z0), src_stride, scalar, cand, norm ? norm + z0 * size_Ql : nullptr,
                    bits + z0, nullptr, s);
    PHA_API_END
}

int pha_invariant_noise_budget_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t cipher_size, size_t batch, size_t ct_stride,
                                       const uint64_t *sk_powers, size_t n_powers, int scheme, int32_t *budget, uint64_t *norm, size_t chunk,
                                       void *stream) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    const CtBatch b{ct, cipher_size, batch, ct_stride, sk_powers, n_powers};
    const bool ntt_form = check_noise_budget(shape(c), size_Ql, b, scheme, budget, norm, kNoiseMaxLimbs);
    if (batch == 0) return 0;
    hipStream_t s = as_stream(stream);
    decrypt_strict(c, "noise_budget", size_Ql, b, s);
    const PhaseChunk pc = phase_chunk(ntt_form, cipher_size, size_Ql * c.n, batch, chunk, kDecryptChunk);
    u64 *work = c.scratch_outer(stream, pc.C * pc.wst + norm_cand_words(c, size_Ql, pc.C)), *cand = work + pc.C * pc.wst;
    const u64 scalar = scheme == PHA_SCHEME_BFV ? c.plain_t : 1;   // invariant_noise_budget multiplies by t under bfv only
    for (size_t b0 = 0; b0 < batch; b0 += pc.C) {
        const size_t B = std::min(pc.C, batch - b0);
        phase_to_coeff(c, size_Ql, ntt_form, CtBatch{ct + b0 * ct_stride, cipher_size, B, ct_stride, sk_powers, n_powers}, work, pc.wst, s);
        launch_norm(c, size_Ql, work, B, pc.wst, scalar, cand, norm ? norm + b0 * size_Ql : nullptr, nullptr, budget + b0, s);
    }
    PHA_API_END
}

}  // extern "C"
