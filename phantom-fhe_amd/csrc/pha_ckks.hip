// pha_ckks.hip -- the CKKS encoder on the device (src/ckks.cu, src/fft.cu, src/rns_base.cu:49-253): the special FFT over complex
// doubles in both directions for a batch of messages, round-and-reduce into RNS limbs, CRT composition back into doubles, and the
// batched encode / decode entries built from them.  The arithmetic is pha_ckks_fft.h (host/device; tests/emu/emu_ckks_fft.cpp
// compiles it on the host); DESIGN.md section 4.10 has the kernels and their bounds.
//
// The special FFT of n = 2^log_n points takes at most two passes over global memory.  A pass is fft_pass_kernel: a workgroup loads
// a tile of up to 2^13 points into LDS (128 KiB of the CU's 160), runs the pass's stages there, three at a time in registers, and
// stores the tile.  n <= 2^13 is ONE pass with one workgroup per message.  Larger n splits into a contiguous pass (tiles of 2^12
// consecutive points: the stages whose pairs are 1 .. 2^11 apart) and a strided pass (tiles of n / 2^12 rows x 2^24 / n adjacent
// columns: the stages whose pairs are 2^12 and more apart); the inverse transform (encode) runs the contiguous pass first, the
// forward one (decode) the strided pass first.  The bit-reversal permutations of the reference's separate launches are the gather
// of the first load (encode: value i sits at point brev(i), the rest is zero) and the scatter of the last store (decode); encode's
// scale / n is applied in the last store, which writes the coefficients as [re[0..n) | im[0..n)] = the [N] doubles round-and-reduce
// reads, and reduces max |coefficient| per message (wave reduction, then a vector atomic max on the bit pattern: non-negative
// doubles order like their bit patterns, and Inf / NaN compare largest, so they are refused with the too-large coefficients).
#include "../../include/phantom_amd.h"
#include "../../include/phantom_amd_bench.h"
#include "pha_ckks_fft.h"
#include "pha_internal.h"
#include "pha_ntt_core.h"

#include <atomic>
#include <cmath>
#include <complex>

using namespace pha;

struct pha_ckks_encoder {
    pha_context_t ctx = nullptr;
    uint32_t log_slots = 0, m = 0;   // n = 2^log_slots = N / 2 slots, m = 2 N roots
    std::vector<cplx> h_roots;       // [m]      e^{2 pi i k / m}
    std::vector<uint32_t> h_group;   // [n / 2]  5^k mod m
    DevBuf<cplx> roots;
    DevBuf<uint32_t> group;
};

namespace {

constexpr uint32_t kSingleLog = kFftSingleLog, kMaxLog = kFftMaxLog;   // the plan: pha_ckks_fft.h fft_pass_shape
constexpr int kFftThreads = 512;

enum { IN_INTERLEAVED = FFT_IN_INTERLEAVED, IN_GATHER = FFT_IN_GATHER, IN_SPLIT = FFT_IN_SPLIT };
enum { OUT_INTERLEAVED = FFT_OUT_INTERLEAVED, OUT_SPLIT = FFT_OUT_SPLIT, OUT_SCATTER = FFT_OUT_SCATTER };

// One pass over one tile of one message (pha_ckks_fft.h has the phases): load, the stages three at a time, store + max.
template <bool INV>
__global__ void __launch_bounds__(kFftThreads) fft_pass_kernel(const FftPass p) {
    extern __shared__ __align__(16) unsigned char fft_smem[];
    cplx *lds = reinterpret_cast<cplx *>(fft_smem);
    const uint32_t tile = blockIdx.x, msg = blockIdx.y;
    fft_load(p, lds, tile, msg, threadIdx.x, blockDim.x);
    __syncthreads();
    for (uint32_t done = 0; done < p.stages;) {
        done += fft_stage_phase<INV>(p, lds, tile, done, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    u64 mx = fft_store(p, lds, tile, msg, threadIdx.x, blockDim.x);
    if (p.maxbits) {   // uniform
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = (u64)__shfl_xor((unsigned long long)mx, off, 64);
            mx = mx > o ? mx : o;
        }
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(reinterpret_cast<unsigned long long *>(p.maxbits + msg), (unsigned long long)mx);
    }
}

// the LDS-resident single pass needs more dynamic LDS than the default limit of 64 KiB: raised once per kernel and device
template <bool INV>
void launch_fft_pass(const FftPass &p, uint32_t count, hipStream_t s) {
    static std::atomic<uint64_t> raised{0};
    const size_t bytes = sizeof(cplx) << p.log_tile;
    if (bytes > 64 * 1024) {
        int dev = 0;
        PHA_HIP(hipGetDevice(&dev));
        const uint64_t bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            PHA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&fft_pass_kernel<INV>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)bytes));
            raised.fetch_or(bit, std::memory_order_release);
        }
    }
    const uint32_t threads = p.log_tile >= 12 ? kFftThreads : p.log_tile >= 9 ? 256 : 64;
    hipLaunchKernelGGL(fft_pass_kernel<INV>, dim3(1u << (p.log_n - p.log_tile), count), dim3(threads), bytes, s, p);
    check_launch();
}

// What one transform reads and writes: `in` as in_mode says, `out` as out_mode says; `mid` (interleaved, may be `in` or `out` where
// those are interleaved too: every workgroup reads its whole tile before it writes it) carries a two-pass transform between the passes.
struct FftIo {
    const double *in;
    size_t in_stride;
    int in_mode;
    uint32_t values_size;
    double *mid;
    size_t mid_stride;
    double *out;
    size_t out_stride;
    int out_mode;
    double fix;
    u64 *maxbits;
};

void special_fft(const pha_ckks_encoder &e, bool inverse, uint32_t log_n, uint32_t count, const FftIo &io, hipStream_t s) {
    if (log_n < 1 || log_n > e.log_slots || log_n > kMaxLog) throw std::invalid_argument("log_n out of range");
    if (count == 0) return;
    if (count > 65535) throw std::invalid_argument("count out of range");
    FftPass p{};
    p.roots = e.roots.p; p.group = e.group.p; p.m = e.m;
    const uint32_t passes = fft_pass_count(log_n);
    for (uint32_t which = 0; which < passes; which++) {
        const bool first = which == 0, last = which + 1 == passes;
        fft_pass_shape(p, log_n, inverse, which);
        p.in = first ? io.in : io.mid; p.in_stride = first ? io.in_stride : io.mid_stride;
        p.in_mode = first ? io.in_mode : (int)IN_INTERLEAVED;
        p.values_size = io.values_size;
        p.out = last ? io.out : io.mid; p.out_stride = last ? io.out_stride : io.mid_stride;
        p.out_mode = last ? io.out_mode : (int)OUT_INTERLEAVED;
        p.fix = last ? io.fix : 0.0;
        p.maxbits = last ? io.maxbits : nullptr;
        if (inverse) launch_fft_pass<true>(p, count, s);
        else launch_fft_pass<false>(p, count, s);
    }
}

// ---- round and reduce (decompose_array, src/rns_base.cu:49-171) -------------------------------------------------------------------
// limb y of message z <- coefficient j of that message modulo the limb's prime; every limb reads the same N doubles.  split: the
// doubles are [re[0..n) | im[0..n)] (the encoder's own form); otherwise n interleaved complex numbers (the reference's argument).
template <bool WIDE>
__global__ void __launch_bounds__(256) ckks_decompose_kernel(u64 *dst, size_t dst_stride, const double *src, size_t src_stride, int split,
                                                             const DModulus *mod, uint32_t size_ql, uint32_t special_row0, uint32_t n_coeff) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (j >= n_coeff) return;
    const uint32_t half = n_coeff >> 1;
    const double *sp = src + (size_t)z * src_stride;
    const double x = split ? sp[j] : (j < half ? sp[2 * (size_t)j] : sp[2 * (size_t)(j - half) + 1]);
    const DModulus m = mod[y < size_ql ? y : special_row0 + (y - size_ql)];
    dst[(size_t)z * dst_stride + (size_t)y * n_coeff + j] = WIDE ? ckks_round_reduce_wide(x, m) : ckks_round_reduce64(x, m.value, m.ratio1);
}

void launch_decompose(Context &c, u64 *dst, size_t dst_stride, const double *src, size_t src_stride, bool split, uint32_t size_ql,
                      uint32_t limbs, uint32_t count, bool wide, hipStream_t s) {
    const dim3 grid((uint32_t)((c.n + 255) / 256), limbs, count);
    if (wide)
        hipLaunchKernelGGL(ckks_decompose_kernel<true>, grid, dim3(256), 0, s, dst, dst_stride, src, src_stride, (int)split, c.d_mod.p, size_ql,
                           c.size_q, (uint32_t)c.n);
    else
        hipLaunchKernelGGL(ckks_decompose_kernel<false>, grid, dim3(256), 0, s, dst, dst_stride, src, src_stride, (int)split, c.d_mod.p, size_ql,
                           c.size_q, (uint32_t)c.n);
    check_launch();
}

// ---- CRT composition into doubles (compose_array, src/rns_base.cu:173-253) -------------------------------------------------------
// One thread per coefficient.  x = sum_i [a_i * (Q/q_i)^-1]_{q_i} * (Q/q_i) mod Q over the integers, in `size` words kept in `acc`
// ([message][word][N]: consecutive threads touch consecutive addresses); then the double, word by word from the low word up with
// the factor 2^64 per word folded into the scale -- x itself below (Q + 1) / 2, the signed per-word differences against Q otherwise,
// in the reference kernel's comparison and order.
__global__ void __launch_bounds__(256) ckks_compose_kernel(double *dst, size_t dst_stride, int split, const u64 *src, size_t src_stride,
                                                           u64 *acc, uint32_t size, const DModulus *mod, const u64 *big_q, const u64 *punct,
                                                           const u64x2 *inv, const u64 *thresh, double inv_scale, uint32_t n_coeff) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y;
    if (j >= n_coeff) return;
    const u64 *sp = src + (size_t)z * src_stride + j;
    u64 *a = acc + (size_t)z * size * n_coeff + j;
    const size_t N = n_coeff;
    if (size == 1) {
        a[0] = sp[0];
    } else {
        for (uint32_t w = 0; w < size; w++) a[w * N] = 0;
        for (uint32_t i = 0; i < size; i++) {
            const u64 prod = shoup(sp[i * N], inv[i], mod[i].value);
            const u64 *pp = punct + (size_t)i * size;
            u64 carry = 0;
            for (uint32_t w = 0; w < size; w++) {   // acc += (Q / q_i) * prod; the word sum stays below 2^128
                u64 lo, hi;
                mul128(pp[w], prod, lo, hi);
                const u64 s1 = lo + a[w * N];
                const u64 s2 = s1 + carry;
                carry = hi + (s1 < lo) + (s2 < s1);
                a[w * N] = s2;
            }
            bool ge = carry != 0;   // both terms are below Q, so one subtraction of Q brings the sum back
            if (!ge) {
                ge = true;
                for (uint32_t w = size; w-- > 0;) {
                    const u64 av = a[w * N];
                    if (av != big_q[w]) { ge = av > big_q[w]; break; }
                }
            }
            if (ge) {
                u64 borrow = 0;
                for (uint32_t w = 0; w < size; w++) {
                    const u64 av = a[w * N], qv = big_q[w];
                    a[w * N] = av - qv - borrow;
                    borrow = (av < qv) || (av == qv && borrow);
                }
            }
        }
    }
    bool upper = true;   // x >= (Q + 1) / 2
    for (uint32_t w = size; w-- > 0;) {
        const u64 av = a[w * N];
        if (av != thresh[w]) { upper = av > thresh[w]; break; }
    }
    double res = 0.0, f = inv_scale;
    if (upper) {
        for (uint32_t w = 0; w < size; w++, f *= 18446744073709551616.0) {
            const u64 av = a[w * N], qv = big_q[w];
            if (av > qv) {
                const u64 diff = av - qv;
                res += diff ? (double)diff * f : 0.0;
            } else {
                const u64 diff = qv - av;
                res -= diff ? (double)diff * f : 0.0;
            }
        }
    } else {
        for (uint32_t w = 0; w < size; w++, f *= 18446744073709551616.0) {
            const u64 diff = a[w * N];
            res += diff ? (double)diff * f : 0.0;
        }
    }
    double *dp = dst + (size_t)z * dst_stride;
    const uint32_t half = n_coeff >> 1;
    if (split) dp[j] = res;
    else if (j < half) dp[2 * (size_t)j] = res;
    else dp[2 * (size_t)(j - half) + 1] = res;
}

void launch_compose(Context &c, CkksCompose &t, double *dst, size_t dst_stride, bool split, const u64 *src, size_t src_stride, u64 *acc,
                    uint32_t count, double inv_scale, hipStream_t s) {
    hipLaunchKernelGGL(ckks_compose_kernel, dim3((uint32_t)((c.n + 255) / 256), count), dim3(256), 0, s, dst, dst_stride, (int)split, src,
                       src_stride, acc, t.size, c.d_mod.p, t.big_q.p, t.punct.p, t.inv.p, t.thresh.p, inv_scale, (uint32_t)c.n);
    check_launch();
}

// pha_ckks_set_encode_path (phantom_amd_bench.h): -1 the rule below, 0 unfused, 1 fused
std::atomic<int> g_encode_path{-1};
// Round-and-reduce as the load prologue of the forward transform's first pass (PRO_CKKS) against the decompose kernel followed by the
// plain transform, per launch shape: the prologue measured faster at every shape timed (1, 8 and 128 messages over 3 and over 60
// limbs at N = 2^16: 1.02 x to 1.34 x, profiles/ckks_encoder.md), so every shape takes it.
bool fused_encode(size_t /*count*/, size_t /*limbs*/) {
    const int mode = g_encode_path.load(std::memory_order_relaxed);
    return mode < 0 || mode == 1;
}

void check_dst(const void *p, size_t stride, size_t count, size_t words, const char *what) {
    if (reinterpret_cast<uintptr_t>(p) & 15) throw std::invalid_argument("buffers must be 16-byte aligned");
    if (count > 1 && (stride & 1)) throw std::invalid_argument("strides must be even (16-byte loads)");
    if (count > 1 && stride < words) throw std::invalid_argument(what);
}

}  // namespace

// the big-integer tables of a level, built on the host on first use (as the auxiliary bases of the BFV multiply are)
CkksCompose &Context::ckks_compose(uint32_t size_ql) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = ckks_tables.find(size_ql);
    if (it != ckks_tables.end()) return *it->second;
    check_rns_level(size_ql, size_q);
    PHA_HIP(hipSetDevice(device));
    auto t = std::make_unique<CkksCompose>();
    t->size = size_ql;
    Big q{1};
    for (uint32_t i = 0; i < size_ql; i++) big_mul(q, primes[i]);
    t->bits = big_bits(q);
    std::vector<u64> punct((size_t)size_ql * size_ql, 0);
    std::vector<u64x2> inv(size_ql);
    for (uint32_t i = 0; i < size_ql; i++) {
        Big h = q;
        big_div(h, primes[i]);
        inv[i] = h_pair(h_invmod(big_mod(h, primes[i]), primes[i]), primes[i]);
        for (uint32_t w = 0; w < size_ql && w < h.size(); w++) punct[(size_t)i * size_ql + w] = h[w];
    }
    Big half = q;   // (Q + 1) / 2: Q is odd
    for (size_t w = 0; w < half.size(); w++) half[w] = (half[w] >> 1) | (w + 1 < half.size() ? half[w + 1] << 63 : 0);
    u64 carry = 1;
    for (size_t w = 0; w < half.size() && carry; w++) carry = ++half[w] == 0;
    q.resize(size_ql, 0);
    half.resize(size_ql, 0);
    t->big_q.upload(q);
    t->punct.upload(punct);
    t->inv.upload(inv);
    t->thresh.upload(half);
    return *(ckks_tables[size_ql] = std::move(t));
}

#define PHA_ENC_BEGIN(enc) \
    try {                  \
        if (!(enc)) throw std::invalid_argument("null encoder"); \
        pha::DeviceGuard device_guard__((enc)->ctx->c.device);

extern "C" {

int pha_ckks_encoder_create(pha_context_t ctx, pha_ckks_encoder_t *out) {
    PHA_CTX_BEGIN(ctx)
    if (!out) throw std::invalid_argument("null output pointer");
    Context &c = ctx->c;
    if (c.log_n < 3 || c.log_n - 1 > kMaxLog) throw std::invalid_argument("unsupported poly_modulus_degree for the CKKS encoder");
    auto e = std::make_unique<pha_ckks_encoder>();
    e->ctx = ctx;
    e->log_slots = c.log_n - 1;
    e->m = 2u << c.log_n;
    const uint32_t m = e->m, slots = 1u << e->log_slots;
    e->h_group.resize(slots >> 1);
    uint32_t pos = 1;
    for (auto &g : e->h_group) { g = pos; pos = (pos * 5u) & (m - 1); }
    // an eighth of the circle from polar(), the rest by the 8-fold symmetry (ComplexRoots, src/fft.cu:13-41)
    const double pi = 3.1415926535897932384626433832795028842;
    std::vector<cplx> eighth(m / 8 + 1);
    for (uint32_t i = 0; i <= m / 8; i++) {
        const std::complex<double> r = std::polar(1.0, 2 * pi * static_cast<double>(i) / static_cast<double>(m));
        eighth[i] = cplx{r.real(), r.imag()};
    }
    e->h_roots.resize(m);
    for (uint32_t i = 0; i < m; i++) {
        // fold i into the first eighth, remembering the mirrors taken on the way (each as the reference's get_root applies it)
        uint32_t k = i;
        bool conj_last = false, neg = false, neg_conj = false, mirror = false;
        if (k > 3 * (m / 4)) { conj_last = true; k = m - k; }
        else if (k > m / 2) { neg = true; k -= m / 2; }
        if (k > m / 4) { neg_conj = true; k = m / 2 - k; }   // (only reached with k <= m / 2)
        if (k > m / 8) { mirror = true; k = m / 4 - k; }
        cplx r = eighth[k];
        if (mirror) r = cplx{r.im, r.re};
        if (neg_conj) r = cplx{0.0 - r.re, 0.0 - (-r.im)};
        if (neg) r = cplx{0.0 - r.re, 0.0 - r.im};
        if (conj_last) r = cplx{r.re, -r.im};
        e->h_roots[i] = r;
    }
    e->roots.upload(e->h_roots);
    e->group.upload(e->h_group);
    *out = e.release();
    PHA_API_END
}

void pha_ckks_encoder_destroy(pha_ckks_encoder_t enc) { delete enc; }

int pha_ckks_set_encode_path(int mode) {
    PHA_API_BEGIN
    if (mode < -1 || mode > 1) throw std::invalid_argument("mode is -1 (the library's rule), 0 (decompose kernel) or 1 (load prologue)");
    g_encode_path.store(mode);
    PHA_API_END
}

int pha_ckks_encoder_tables(pha_ckks_encoder_t enc, double *roots_host, uint32_t *group_host) {
    PHA_ENC_BEGIN(enc)
    if (roots_host)
        for (size_t i = 0; i < enc->h_roots.size(); i++) { roots_host[2 * i] = enc->h_roots[i].re; roots_host[2 * i + 1] = enc->h_roots[i].im; }
    if (group_host) std::copy(enc->h_group.begin(), enc->h_group.end(), group_host);
    PHA_API_END
}

int pha_special_fft_backward(pha_ckks_encoder_t enc, double *inout, size_t log_n, double scalar, void *stream) {
    PHA_ENC_BEGIN(enc)
    need(inout);
    if (log_n > 64) throw std::invalid_argument("log_n out of range");
    const FftIo io{inout, 0, IN_INTERLEAVED, 0, inout, 0, inout, 0, OUT_INTERLEAVED, scalar, nullptr};
    special_fft(*enc, true, (uint32_t)log_n, 1, io, as_stream(stream));
    PHA_API_END
}

int pha_special_fft_forward(pha_ckks_encoder_t enc, double *inout, size_t log_n, void *stream) {
    PHA_ENC_BEGIN(enc)
    need(inout);
    if (log_n > 64) throw std::invalid_argument("log_n out of range");
    const FftIo io{inout, 0, IN_INTERLEAVED, 0, inout, 0, inout, 0, OUT_INTERLEAVED, 0.0, nullptr};
    special_fft(*enc, false, (uint32_t)log_n, 1, io, as_stream(stream));
    PHA_API_END
}

int pha_decompose_array(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const double *src, uint32_t max_coeff_bit_count, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(dst); need(src);
    Context &c = ctx->c;
    check_rns_level(size_Ql, c.size_q);
    launch_decompose(c, dst, 0, src, 0, false, (uint32_t)size_Ql, (uint32_t)size_Ql, 1, max_coeff_bit_count > 64, as_stream(stream));
    PHA_API_END
}

int pha_compose_array(pha_context_t ctx, size_t size_Ql, double *dst, const uint64_t *src, double inv_scale, void *stream) {
    PHA_CTX_BEGIN(ctx)
    need(dst); need(src);
    Context &c = ctx->c;
    check_rns_level(size_Ql, c.size_q);
    CkksCompose &t = c.ckks_compose((uint32_t)size_Ql);
    u64 *acc = c.scratch(stream, size_Ql * c.n);
    launch_compose(c, t, dst, 0, false, src, 0, acc, 1, inv_scale, as_stream(stream));
    PHA_API_END
}

int pha_ckks_encode_batched(pha_ckks_encoder_t enc, size_t size_Ql, int with_special, const double *values, size_t values_size,
                            size_t count, size_t values_stride, double scale, uint64_t *dst, size_t dst_stride, int *bit_counts_host_or_null,
                            void *stream) {
    PHA_ENC_BEGIN(enc)
    need(values); need(dst);
    Context &c = enc->ctx->c;
    check_rns_level(size_Ql, c.size_q);
    const size_t slots = (size_t)1 << enc->log_slots, limbs = size_Ql + (with_special ? c.size_p : 0);
    if (values_size == 0) throw std::invalid_argument("Input vector is empty");
    if (values_size > slots) throw std::invalid_argument("Input vector exceeds max slots");
    CkksCompose &t = c.ckks_compose((uint32_t)size_Ql);   // the level's modulus bit count
    if (!(scale > 0) || !std::isfinite(scale) || static_cast<int>(std::log2(scale)) + 1 >= t.bits)
        throw std::invalid_argument("scale out of bounds");
    if (count > 65535) throw std::invalid_argument("count out of range");
    if (count > 1 && values_stride < values_size) throw std::invalid_argument("values stride below values_size: the messages overlap");
    check_dst(dst, dst_stride, count, limbs * c.n, "dst stride below the encoded size: the plaintexts overlap");
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    // scratch: the coefficients [count][N] doubles, the hand-over of a two-pass transform [count][N], the maxima [count]
    const bool two_pass = enc->log_slots > kSingleLog;
    u64 *scratch = c.scratch_outer(stream, count * c.n * (two_pass ? 2 : 1) + count);
    double *coef = reinterpret_cast<double *>(scratch), *mid = coef + (two_pass ? count * c.n : 0);
    u64 *maxbits = scratch + count * c.n * (two_pass ? 2 : 1);
    PHA_HIP(hipMemsetAsync(maxbits, 0, count * sizeof(u64), s));
    const FftIo io{values, 2 * values_stride, IN_GATHER, (uint32_t)values_size, mid, c.n, coef, c.n, OUT_SPLIT,
                   scale / static_cast<double>(slots), maxbits};
    special_fft(*enc, true, enc->log_slots, (uint32_t)count, io, s);
    // the one host synchronisation of the call: the refusal and the choice of the decompose kernel need the maxima
    std::vector<u64> h_max(count);
    PHA_HIP(hipMemcpyAsync(h_max.data(), maxbits, count * sizeof(u64), hipMemcpyDeviceToHost, s));
    PHA_HIP(hipStreamSynchronize(s));
    int worst = 0;
    for (size_t i = 0; i < count; i++) {
        const int b = ckks_bit_count(h_max[i]);
        if (bit_counts_host_or_null) bit_counts_host_or_null[i] = b;
        worst = std::max(worst, b);
    }
    if (worst >= t.bits) throw std::invalid_argument("encoded values are too large");
    // coefficients that fit a word: every limb's first transform pass rounds and reduces the same [N] doubles as it loads them, and
    // the decomposed form is never written; wider ones go through the decompose kernel
    const bool fused = worst <= 64 && fused_encode(count, limbs);
    if (!fused) launch_decompose(c, dst, dst_stride, coef, c.n, true, (uint32_t)size_Ql, (uint32_t)limbs, (uint32_t)count, worst > 64, s);
    NttExtra x;
    x.batch = (uint32_t)count;
    x.poly_stride = count > 1 ? dst_stride : limbs * c.n;
    if (fused) {
        x.pro_src = reinterpret_cast<const u64 *>(coef);
        x.pro_stride = c.n;
        x.pro_ckks = true;
    }
    const LimbSel sel = with_special ? special_sel(0, limbs, c.size_qp, c.size_p) : plain_sel(0, limbs);
    ntt_forward(c, dst, dst, dst, sel, EPI_FWD_CANON, x, s);
    PHA_API_END
}

int pha_ckks_decode_batched(pha_ckks_encoder_t enc, size_t size_Ql, const uint64_t *plain, size_t count, size_t plain_stride, double scale,
                            double *values_out, size_t values_stride, void *stream) {
    PHA_ENC_BEGIN(enc)
    need(plain); need(values_out);
    Context &c = enc->ctx->c;
    check_rns_level(size_Ql, c.size_q);
    const size_t slots = (size_t)1 << enc->log_slots, ln = size_Ql * c.n;
    CkksCompose &t = c.ckks_compose((uint32_t)size_Ql);
    if (!(scale > 0) || !std::isfinite(scale) || static_cast<int>(std::log2(scale)) >= t.bits) throw std::invalid_argument("scale out of bounds");
    if (count > 65535) throw std::invalid_argument("count out of range");
    if (count > 1 && plain_stride < ln) throw std::invalid_argument("plain stride below L * N: the plaintexts overlap");
    if (count > 1 && values_stride < slots) throw std::invalid_argument("values stride below the slot count: the messages overlap");
    if (reinterpret_cast<uintptr_t>(plain) & 15) throw std::invalid_argument("buffers must be 16-byte aligned");
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    strict_operand(c, "ckks_decode plain", plain, rows_plain(0, size_Ql), (uint32_t)count, count > 1 ? plain_stride : 0, s);
    // scratch: a copy of the plaintexts [count][L][N] (taken back to coefficient form, then the composition's words), the
    // coefficients as doubles [count][N], the hand-over of a two-pass transform [count][N]
    const bool two_pass = enc->log_slots > kSingleLog;
    u64 *copy = c.scratch_outer(stream, count * ln * 2 + count * c.n * (two_pass ? 2 : 1));
    u64 *acc = copy + count * ln;
    double *coef = reinterpret_cast<double *>(acc + count * ln), *mid = coef + (two_pass ? count * c.n : 0);
    PHA_HIP(hipMemcpy2DAsync(copy, ln * sizeof(u64), plain, (count > 1 ? plain_stride : ln) * sizeof(u64), ln * sizeof(u64), count,
                             hipMemcpyDeviceToDevice, s));
    NttExtra x;
    x.batch = (uint32_t)count;
    x.poly_stride = ln;
    ntt_inverse(c, copy, copy, copy, plain_sel(0, size_Ql), EPI_INV_CANON, x, s);
    launch_compose(c, t, coef, c.n, true, copy, ln, acc, (uint32_t)count, 1.0 / scale, s);
    const FftIo io{coef, c.n, IN_SPLIT, 0, mid, c.n, values_out, 2 * values_stride, OUT_SCATTER, 0.0, nullptr};
    special_fft(*enc, false, enc->log_slots, (uint32_t)count, io, s);
    PHA_API_END
}

}  // extern "C"
