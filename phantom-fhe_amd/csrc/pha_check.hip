// pha_check.hip -- the canonical-operand precondition of include/phantom_amd.h made checkable (r06; VERDICT r05 "weak" 2).
//
// The reference's Barrett-128 kernels accept lazy or unreduced operand words (src/polymath.cu:463-496 multiplies an unreduced
// c0 + c1; include/uintmodmath.cuh:96-136 reduces any 128-bit value).  This library computes limbs below 2^50 in FP64
// (pha_arith.h: fp_from_canon is exact only for words below 2^52), so a word >= its modulus there can give a wrong residue with no
// error.  Two remedies, neither on the hot path:
//   * pha_check_canonical / pha_check_canonical_keys count the words of a buffer that are >= their limb's modulus;
//   * strict mode (PHA_STRICT=1 in the environment when the library is loaded, or pha_set_strict(1)): the entry points that
//     include/phantom_amd.h lists at pha_set_strict (dyadic, tensor, mod-up / inner product / mod-down, key switch, hoisting, BFV
//     multiply) count first and fail with status -1 (invalid_argument, naming the operand) instead of computing.  Strict mode synchronises the stream per checked operand: a debugging aid, not for capture or timing.
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "../../include/phantom_amd.h"
#include "pha_internal.h"

namespace pha {

struct CanonArgs {
    const u64 *data;             // [polys][limbs][N] with poly_stride, or nullptr when ptrs is set
    const u64 *const *ptrs;      // device array of key pointers, each [2][size_QP][N]
    const DModulus *mod;
    unsigned long long *count;
    RowMap rows;                 // data limb y (relative to `data`) -> table row
    uint32_t n;
    uint32_t key_gap_from, key_gap_add;   // keys: limbs >= key_gap_from sit key_gap_add limbs further (the special rows of a full-width key)
    size_t poly_stride, key_half;         // key_half: words between the two halves of one key (size_QP * N)
};

__global__ __launch_bounds__(256) void canon_count_kernel(const CanonArgs k) {
    const uint32_t y = blockIdx.y, z = blockIdx.z, coeff = blockIdx.x * 256 + threadIdx.x;
    uint32_t limb = y;
    uint32_t row = y < k.rows.tail_from ? k.rows.row0 + y : k.rows.tail_row0 + (y - k.rows.tail_from);
    const u64 *base;
    if (k.ptrs) {
        if (limb >= k.key_gap_from) limb += k.key_gap_add;
        row = limb;                                   // a key limb IS its table row (keys live at full QP width)
        base = k.ptrs[z >> 1] + (size_t)(z & 1) * k.key_half;
    } else {
        base = k.data + (size_t)z * k.poly_stride;
    }
    const u64 q = k.mod[row].value;
    const bool bad = base[(size_t)limb * k.n + coeff] >= q;
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(k.count, (unsigned long long)__popcll(m));
}

// words of `polys` raw plaintexts ([N] words each, plain_stride apart) that are not below t
struct PlainCountArgs {
    const u64 *data;
    unsigned long long *count;
    u64 t;
    uint32_t n;
    size_t stride;
};
__global__ __launch_bounds__(256) void plain_count_kernel(const PlainCountArgs k) {
    const uint32_t coeff = blockIdx.x * 256 + threadIdx.x;
    const bool bad = k.data[(size_t)blockIdx.y * k.stride + coeff] >= k.t;
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(k.count, (unsigned long long)__popcll(m));
}

static std::atomic<int> g_strict{-1};   // -1: not read yet
bool strict_mode() {
    int v = g_strict.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = std::getenv("PHA_STRICT");
        v = (e && e[0] == '1') ? 1 : 0;
        g_strict.store(v, std::memory_order_relaxed);
    }
    return v == 1;
}

static u64 run_count(Context &c, CanonArgs k, uint32_t limbs, uint32_t polys, hipStream_t s) {
    if (limbs == 0 || polys == 0) return 0;
    if (polys > 65535) throw std::invalid_argument("batch out of range");
    // one 8-byte counter per call: the check is a debugging path, an allocation per call is what it costs
    unsigned long long *d_count = nullptr;
    PHA_HIP(hipMalloc(&d_count, sizeof(unsigned long long)));
    unsigned long long host = 0;
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        k.count = d_count;
        k.mod = c.d_mod.p;
        k.n = (uint32_t)c.n;
        hipLaunchKernelGGL(canon_count_kernel, dim3((unsigned)(c.n / 256), limbs, polys), dim3(256), 0, s, k);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host, d_count, sizeof(host), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_count);
    PHA_HIP(e);
    return host;
}

u64 count_noncanonical(Context &c, const u64 *data, const RowMap &rows, uint32_t polys, size_t poly_stride, hipStream_t s) {
    for (uint32_t y = 0; y < rows.count; y++) {
        const uint32_t row = y < rows.tail_from ? rows.row0 + y : rows.tail_row0 + (y - rows.tail_from);
        if (row >= c.rows) throw std::invalid_argument("modulus index out of range");
    }
    CanonArgs k{};
    k.data = data;
    k.rows = rows;
    k.poly_stride = poly_stride;
    return run_count(c, k, rows.count, polys, s);
}

// the key limbs a key switch at level size_Ql reads: rows [0, size_Ql) and the special rows [size_Q, size_QP) of both halves
u64 count_noncanonical_keys(Context &c, const u64 *const *keys, uint32_t n_keys, uint32_t size_Ql, hipStream_t s) {
    if (size_Ql > c.size_q) throw std::invalid_argument("RNSBase is invalid");
    CanonArgs k{};
    k.ptrs = keys;
    k.rows = rows_plain(0, size_Ql + c.size_p);
    k.key_gap_from = size_Ql;
    k.key_gap_add = c.size_q - size_Ql;
    k.key_half = (size_t)c.size_qp * c.n;
    return run_count(c, k, size_Ql + c.size_p, 2 * n_keys, s);
}

void strict_operand(Context &c, const char *what, const u64 *data, const RowMap &rows, uint32_t polys, size_t poly_stride,
                    hipStream_t s) {
    if (!strict_mode() || !data) return;
    const u64 bad = count_noncanonical(c, data, rows, polys, poly_stride, s);
    if (bad)
        throw std::invalid_argument(std::string("PHA_STRICT: ") + what + " holds " + std::to_string(bad) +
                                    " word(s) >= their limb's modulus (operands must be canonical; include/phantom_amd.h)");
}
void strict_plain(Context &c, const char *what, const u64 *data, u64 t, size_t polys, size_t stride, hipStream_t s) {
    if (!strict_mode() || !data) return;
    unsigned long long *d_count = nullptr, host = 0;
    PHA_HIP(hipMalloc(&d_count, sizeof(unsigned long long)));   // (a debugging path, like run_count)
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s);
    for (size_t p0 = 0; p0 < polys && e == hipSuccess; p0 += 65535) {
        const PlainCountArgs k{data + p0 * stride, d_count, t, (uint32_t)c.n, stride};
        hipLaunchKernelGGL(plain_count_kernel, dim3((unsigned)(c.n / 256), (unsigned)std::min<size_t>(65535, polys - p0)), dim3(256), 0, s, k);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host, d_count, sizeof(host), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_count);
    PHA_HIP(e);
    if (host)
        throw std::invalid_argument(std::string("PHA_STRICT: ") + what + " holds " + std::to_string(host) +
                                    " word(s) >= the plain modulus (a bfv plaintext's words are below t; include/phantom_amd.h)");
}
void strict_sum_operand(Context &c, const char *what, const SumOperand &op, size_t cms, size_t terms, size_t batch, bool raw, hipStream_t s) {
    if (!strict_mode() || !op.p) return;
    auto run = [&](const u64 *base, size_t polys, size_t stride) {
        if (raw) strict_plain(c, what, base, c.plain_t, polys, stride, s);
        else strict_operand(c, what, base, rows_plain(0, cms), (uint32_t)polys, stride, s);
    };
    if (raw) op.strict_runs(terms, batch, run, SIZE_MAX);   // strict_plain cuts a group's terms into counts itself and reports their sum
    else op.strict_runs(terms, batch, run);
}
void strict_keys(Context &c, const char *what, const u64 *const *keys, uint32_t n_keys, uint32_t size_Ql, hipStream_t s) {
    if (!strict_mode() || !keys) return;
    const u64 bad = count_noncanonical_keys(c, keys, n_keys, size_Ql, s);
    if (bad)
        throw std::invalid_argument(std::string("PHA_STRICT: ") + what + " holds " + std::to_string(bad) +
                                    " word(s) >= their limb's modulus (operands must be canonical; include/phantom_amd.h)");
}

}  // namespace pha

using namespace pha;

extern "C" {

int pha_set_strict(int on) {
    strict_mode();   // settle the environment's value first, so that the return value is the state before this call
    return g_strict.exchange(on ? 1 : 0, std::memory_order_relaxed);
}

int pha_check_canonical(pha_context_t ctx, const uint64_t *data, size_t coeff_modulus_size, size_t start_modulus_idx,
                        size_t size_P_tail, size_t polys, size_t poly_stride, uint64_t *bad_words, void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!data || !bad_words) throw std::invalid_argument("null pointer");
    Context &c = ctx->c;
    if (size_P_tail > coeff_modulus_size) throw std::invalid_argument("size_P exceeds coeff_modulus_size");
    RowMap rows = rows_plain(start_modulus_idx, coeff_modulus_size);
    if (size_P_tail) {   // the twr_idx2 remap of src/ntt/fntt_2d.cu:434-437: the last size_P limbs are the special rows
        rows.tail_from = (uint32_t)(coeff_modulus_size - size_P_tail);
        rows.tail_row0 = (uint32_t)(c.size_qp - size_P_tail);
    }
    *bad_words = count_noncanonical(c, data, rows, (uint32_t)polys, poly_stride, as_stream(stream));
    PHA_API_END
}

int pha_check_canonical_keys(pha_context_t ctx, size_t size_Ql, const uint64_t *const *keys, size_t n_keys, uint64_t *bad_words,
                             void *stream) {
    PHA_CTX_BEGIN(ctx)
    if (!keys || !bad_words) throw std::invalid_argument("null pointer");
    if (n_keys > 32767) throw std::invalid_argument("batch out of range");
    *bad_words = count_noncanonical_keys(ctx->c, keys, (uint32_t)n_keys, (uint32_t)size_Ql, as_stream(stream));
    PHA_API_END
}

}  // extern "C"
