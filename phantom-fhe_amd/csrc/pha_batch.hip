// pha_batch.hip -- the BFV / BGV batch encoder on the device (PhantomBatchEncoder, src/batchencoder.cu): the negacyclic transform
// modulo the plain modulus t in both directions for a batch of messages (the reference's nwt_2d_radix8_{forward,backward}_inplace over
// gpu_plain_tables()), and the batched encode / decode entries built from it.  The arithmetic and the index math are pha_batch.h
// (host/device; tests/emu/emu_batch.cpp compiles it on the host); DESIGN.md section 4.13 has the kernels and their bounds.
//
// A transform takes at most two passes over global memory.  A pass is nwt_pass_kernel: a workgroup loads a tile of up to 2^14 words
// into LDS (128 KiB of the CU's 160), runs the pass's stages there, three at a time in registers, and stores the tile.  N <= 2^14 is
// ONE pass with one workgroup per message; larger N splits into a contiguous and a strided pass over tiles of 2^12 words (pha_batch.h
// nwt_pass_shape).  The reference's scatter / gather launches through matrix_reps_index_map are the gather of encode's first load and
// the scatter of decode's last store; both also exist with the permutation as a streaming kernel of its own, which large batches of
// a two-pass transform take (the rules: fused_encode / fused_decode below).  Nothing here touches pha_ntt.hip: the transform is over one modulus for the whole launch, and the
// encoder object owns its tables.
#include "../../include/phantom_amd.h"
#include "../../include/phantom_amd_bench.h"
#include "pha_batch.h"
#include "pha_internal.h"

#include <atomic>

using namespace pha;

struct pha_batch_encoder {
    pha_context_t ctx = nullptr;
    u64 t = 0;                         // the plain modulus the tables were built for
    uint32_t log_n = 0;
    std::vector<u64> h_index_map;      // [N] matrix_reps_index_map
    DevBuf<uint32_t> index_map, inv_map;   // [N] the map and its inverse permutation
    DevBuf<u64x2> tw, itw;             // [N] psi^brev(k), psi^-brev(k) (+Shoup)
    u64x2 ninv{};                      // N^-1 mod t (+Shoup)
};

namespace {

template <bool INV>
__global__ void __launch_bounds__(1024) nwt_pass_kernel(const NwtPass p) {
    extern __shared__ __align__(16) unsigned char nwt_smem[];
    u64 *lds = reinterpret_cast<u64 *>(nwt_smem);
    const uint32_t tile = blockIdx.x, msg = blockIdx.y;
    nwt_load(p, lds, tile, msg, threadIdx.x, blockDim.x);
    __syncthreads();
    for (uint32_t done = 0; done < p.stages;) {
        done += nwt_stage_phase<INV>(p, lds, tile, done, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    nwt_store<INV>(p, lds, tile, msg, threadIdx.x, blockDim.x);
}

__global__ void __launch_bounds__(256) batch_gather_kernel(u64 *out, size_t out_stride, const u64 *src, size_t src_stride,
                                                           const uint32_t *index_map, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, msg = blockIdx.y;
    if (i < n) batch_gather_word(out + (size_t)msg * out_stride, src + (size_t)msg * src_stride, index_map, i);
}

__global__ void __launch_bounds__(256) batch_permute_kernel(u64 *buf, size_t buf_stride, const u64 *values, size_t values_stride,
                                                            const uint32_t *perm, uint32_t values_size, u64 t, uint32_t n) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, msg = blockIdx.y;
    if (g < n) batch_permute_word(buf + (size_t)msg * buf_stride, values + (size_t)msg * values_stride, perm, values_size, t, g);
}

// strict mode: message words that are not below t after the sign rule
__global__ void __launch_bounds__(256) batch_values_count_kernel(const u64 *values, size_t stride, uint32_t values_size, u64 t,
                                                                 unsigned long long *count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, msg = blockIdx.y;
    const bool bad = i < values_size && batch_sign_rule(values[(size_t)msg * stride + i], t) >= t;
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (unsigned long long)__popcll(m));
}

// the LDS-resident single pass needs more dynamic LDS than the default limit of 64 KiB: raised once per kernel and device
template <bool INV>
void launch_nwt_pass(const NwtPass &p, uint32_t count, hipStream_t s) {
    static std::atomic<uint64_t> raised{0};
    const size_t bytes = sizeof(u64) << p.log_tile;
    if (bytes > 64 * 1024) {
        int dev = 0;
        PHA_HIP(hipGetDevice(&dev));
        const uint64_t bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            PHA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&nwt_pass_kernel<INV>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)bytes));
            raised.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(nwt_pass_kernel<INV>, dim3(1u << (p.log_n - p.log_tile), count), dim3(nwt_threads(p.log_tile)), bytes, s, p);
    check_launch();
}

// What one transform reads and writes: `in` as in_mode says, `out` as out_mode says (never NWT_OUT_LAZY); `mid` (may be `in` or `out`
// where those are plain: every workgroup reads its whole tile before it writes it) carries a two-pass transform between the passes.
struct NwtIo {
    const u64 *in;
    size_t in_stride;
    int in_mode;
    uint32_t values_size;
    u64 *mid;
    size_t mid_stride;
    u64 *out;
    size_t out_stride;
    int out_mode;
};

void nwt_transform(const pha_batch_encoder &e, bool inverse, uint32_t count, const NwtIo &io, hipStream_t s) {
    NwtPass p{};
    p.tw = inverse ? e.itw.p : e.tw.p; p.perm = e.inv_map.p; p.q = e.t; p.ninv = e.ninv;
    const uint32_t passes = nwt_pass_count(e.log_n);
    for (uint32_t which = 0; which < passes; which++) {
        const bool first = which == 0, last = which + 1 == passes;
        nwt_pass_shape(p, e.log_n, inverse, which);
        p.in = first ? io.in : io.mid; p.in_stride = first ? io.in_stride : io.mid_stride;
        p.in_mode = first ? io.in_mode : (int)NWT_IN_PLAIN;
        p.values_size = io.values_size;
        p.out = last ? io.out : io.mid; p.out_stride = last ? io.out_stride : io.mid_stride;
        p.out_mode = last ? io.out_mode : (int)NWT_OUT_LAZY;
        if (inverse) launch_nwt_pass<true>(p, count, s);
        else launch_nwt_pass<false>(p, count, s);
    }
}

// pha_batch_set_encode_path / pha_batch_set_decode_path (phantom_amd_bench.h): -1 the rules below, 0 the permutation as a kernel of
// its own, 1 the permutation inside the transform
std::atomic<int> g_encode_path{-1}, g_decode_path{-1};
// The rules restate the table of profiles/batch_encoder.md (N = 2^12, 2^15, 2^17; 1 to 64 messages; a 17-to-20-bit and a 59-bit t,
// which time alike).  A one-pass transform (N <= 2^14) keeps the permutation inside it at every count measured.  A two-pass transform
// does so while the batch is small (the call is then bound by its launches, and the fused form has one fewer); from 2^20 words per
// call on, the 8-byte accesses through the permutation cost the transform's workgroups, which hold 32 KiB of LDS each, more than they
// cost a streaming kernel of its own with every wave slot to hide them behind (at 2^20 words the two forms tie within 3 %, from 2^21
// on the kernel of its own is 1.1 x to 1.35 x faster).
constexpr size_t kPermuteKernelWords = (size_t)1 << 20;
bool permutation_inside(int mode, uint32_t log_n, size_t count) {
    if (mode >= 0) return mode == 1;
    return nwt_pass_count(log_n) == 1 || (count << log_n) < kPermuteKernelWords;
}
bool fused_encode(uint32_t log_n, size_t count) { return permutation_inside(g_encode_path.load(std::memory_order_relaxed), log_n, count); }
bool fused_decode(uint32_t log_n, size_t count) { return permutation_inside(g_decode_path.load(std::memory_order_relaxed), log_n, count); }

void strict_values(const char *what, const u64 *values, size_t stride, size_t values_size, size_t count, u64 t, hipStream_t s) {
    if (!strict_mode() || !values || values_size == 0 || count == 0) return;
    unsigned long long *d_count = nullptr, host = 0;
    PHA_HIP(hipMalloc(&d_count, sizeof(unsigned long long)));   // (a debugging path, like strict_plain)
    hipError_t err = hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s);
    if (err == hipSuccess) {
        const size_t msgs = stride ? count : 1;   // a shared message is counted once
        hipLaunchKernelGGL(batch_values_count_kernel, dim3((unsigned)((values_size + 255) / 256), (unsigned)msgs), dim3(256), 0, s, values,
                           stride, (uint32_t)values_size, t, d_count);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(&host, d_count, sizeof(host), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    (void)hipFree(d_count);
    PHA_HIP(err);
    if (host)
        throw std::invalid_argument(std::string("PHA_STRICT: ") + what + " holds " + std::to_string(host) +
                                    " word(s) >= the plain modulus after the sign rule (a message's words are below t, or the negative of "
                                    "such a word in two's complement; include/phantom_amd.h)");
}

void check_live(const pha_batch_encoder &e) {
    if (e.ctx->c.plain_t != e.t) throw std::invalid_argument("the context's plain modulus has changed since the encoder was created");
}

void check_batch(size_t count) {
    if (count > 65535) throw std::invalid_argument("count out of range");
}

}  // namespace

#define PHA_ENC_BEGIN(enc) \
    try {                  \
        if (!(enc)) throw std::invalid_argument("null encoder"); \
        pha::DeviceGuard device_guard__((enc)->ctx->c.device);

extern "C" {

int pha_batch_encoder_create(pha_context_t ctx, pha_batch_encoder_t *out) {
    PHA_CTX_BEGIN(ctx)
    if (!out) throw std::invalid_argument("null output pointer");
    Context &c = ctx->c;
    const u64 t = c.plain_t;
    if (t == 0) throw std::invalid_argument("the batch encoder needs a plain modulus (pha_context_set_plain_modulus)");
    if (c.log_n < 1 || c.log_n > kNwtMaxLog) throw std::invalid_argument("unsupported poly_modulus_degree for the batch encoder");
    const size_t n = c.n;
    if (!h_is_prime(t) || (t - 1) % (2 * n) != 0) throw std::invalid_argument("encryption parameters are not valid for batching");
    auto e = std::make_unique<pha_batch_encoder>();
    e->ctx = ctx;
    e->t = t;
    e->log_n = c.log_n;
    // the tables of gpu_plain_tables() (src/host/ntt.cu:11-56, slot 1 of the inverse table NOT folded with N^-1) ...
    const u64 psi = h_minimal_primitive_root(2 * n, t), ipsi = h_invmod(psi, t);
    std::vector<u64x2> tw(n), itw(n);
    u64 pw = 1, ipw = 1;
    for (size_t k = 0; k < n; k++) {   // slot brev(k) holds psi^k
        const uint32_t at = h_brev((uint32_t)k, (int)c.log_n);
        tw[at] = h_pair(pw, t);
        itw[at] = h_pair(ipw, t);
        pw = h_mulmod(pw, psi, t);
        ipw = h_mulmod(ipw, ipsi, t);
    }
    e->ninv = h_pair(h_invmod((u64)(n % t), t), t);
    // ... and of the encoder's constructor: the index map and its inverse permutation
    e->h_index_map.resize(n);
    batch_index_map(c.log_n, e->h_index_map.data());
    std::vector<uint32_t> map32(n), inv32(n);
    for (size_t i = 0; i < n; i++) {
        map32[i] = (uint32_t)e->h_index_map[i];
        inv32[map32[i]] = (uint32_t)i;
    }
    e->tw.upload(tw);
    e->itw.upload(itw);
    e->index_map.upload(map32);
    e->inv_map.upload(inv32);
    *out = e.release();
    PHA_API_END
}

void pha_batch_encoder_destroy(pha_batch_encoder_t enc) { delete enc; }

int pha_batch_set_encode_path(int mode) {
    PHA_API_BEGIN
    if (mode < -1 || mode > 1) throw std::invalid_argument("mode is -1 (the library's rule), 0 (permutation kernel) or 1 (gather in the first load)");
    g_encode_path.store(mode);
    PHA_API_END
}

int pha_batch_set_decode_path(int mode) {
    PHA_API_BEGIN
    if (mode < -1 || mode > 1) throw std::invalid_argument("mode is -1 (the library's rule), 0 (gather kernel) or 1 (scatter in the last store)");
    g_decode_path.store(mode);
    PHA_API_END
}

int pha_batch_encoder_index_map(pha_batch_encoder_t enc, uint64_t *index_map_host) {
    PHA_ENC_BEGIN(enc)
    if (!index_map_host) throw std::invalid_argument("null output pointer");
    std::copy(enc->h_index_map.begin(), enc->h_index_map.end(), index_map_host);
    PHA_API_END
}

int pha_plain_nwt_forward_inplace_batched(pha_batch_encoder_t enc, uint64_t *inout, size_t count, size_t stride, void *stream) {
    PHA_ENC_BEGIN(enc)
    check_live(*enc);
    need(inout);
    check_batch(count);
    const size_t n = enc->ctx->c.n;
    if (count > 1 && stride < n) throw std::invalid_argument("stride below N: the polynomials overlap");
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    strict_plain(enc->ctx->c, "plain_nwt_forward plain", inout, enc->t, count, count > 1 ? stride : n, s);
    const NwtIo io{inout, stride, NWT_IN_PLAIN, 0, inout, stride, inout, stride, NWT_OUT_CANON};
    nwt_transform(*enc, false, (uint32_t)count, io, s);
    PHA_API_END
}

int pha_plain_nwt_backward_inplace_batched(pha_batch_encoder_t enc, uint64_t *inout, size_t count, size_t stride, void *stream) {
    PHA_ENC_BEGIN(enc)
    check_live(*enc);
    need(inout);
    check_batch(count);
    const size_t n = enc->ctx->c.n;
    if (count > 1 && stride < n) throw std::invalid_argument("stride below N: the polynomials overlap");
    if (count == 0) return 0;
    hipStream_t s = as_stream(stream);
    strict_plain(enc->ctx->c, "plain_nwt_backward plain", inout, enc->t, count, count > 1 ? stride : n, s);
    const NwtIo io{inout, stride, NWT_IN_PLAIN, 0, inout, stride, inout, stride, NWT_OUT_CANON};
    nwt_transform(*enc, true, (uint32_t)count, io, s);
    PHA_API_END
}

int pha_batch_encode_batched(pha_batch_encoder_t enc, const uint64_t *values, size_t values_size, size_t count, size_t values_stride,
                             uint64_t *dst, size_t dst_stride, void *stream) {
    PHA_ENC_BEGIN(enc)
    check_live(*enc);
    Context &c = enc->ctx->c;
    const size_t n = c.n;
    if (values_size > n) throw std::logic_error("values_matrix size is too large");
    need(dst);
    if (values_size) need(values);
    check_batch(count);
    if (count > 1 && values_stride != 0 && values_stride < values_size)
        throw std::invalid_argument("values stride below values_size: the messages overlap");
    if (count > 1 && dst_stride < n) throw std::invalid_argument("dst stride below N: the plaintexts overlap");
    if (count == 0) return 0;
    if (values_size && overlaps(values, (count - 1) * values_stride + values_size, dst, (count - 1) * dst_stride + n))
        throw std::invalid_argument("dst overlaps values");
    hipStream_t s = as_stream(stream);
    strict_values("batch_encode values", values, count > 1 ? values_stride : 0, values_size, count, enc->t, s);
    // scratch [count][N]: the hand-over of a two-pass transform (lazy words: dst only ever receives canonical ones), and the permuted
    // messages where the permutation is a kernel of its own
    const bool two_pass = nwt_pass_count(enc->log_n) > 1, fused = fused_encode(enc->log_n, count);
    u64 *mid = (two_pass || !fused) ? c.scratch(stream, count * n) : dst;
    const u64 *src = values_size ? values : dst;   // (never read when values_size == 0)
    if (fused) {
        const NwtIo io{src, values_stride, NWT_IN_GATHER, (uint32_t)values_size, mid, n, dst, dst_stride, NWT_OUT_CANON};
        nwt_transform(*enc, true, (uint32_t)count, io, s);
    } else {
        hipLaunchKernelGGL(batch_permute_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)count), dim3(256), 0, s, mid, n, src,
                           count > 1 ? values_stride : 0, enc->inv_map.p, (uint32_t)values_size, enc->t, (uint32_t)n);
        check_launch();
        const NwtIo io{mid, n, NWT_IN_PLAIN, 0, mid, n, dst, dst_stride, NWT_OUT_CANON};
        nwt_transform(*enc, true, (uint32_t)count, io, s);
    }
    PHA_API_END
}

int pha_batch_decode_batched(pha_batch_encoder_t enc, const uint64_t *plain, size_t count, size_t plain_stride, uint64_t *values_out,
                             size_t values_stride, void *stream) {
    PHA_ENC_BEGIN(enc)
    check_live(*enc);
    Context &c = enc->ctx->c;
    const size_t n = c.n;
    need(plain); need(values_out);
    check_batch(count);
    if (count > 1 && plain_stride < n) throw std::invalid_argument("plain stride below N: the plaintexts overlap");
    if (count > 1 && values_stride < n) throw std::invalid_argument("values stride below N: the messages overlap");
    if (count == 0) return 0;
    if (overlaps(plain, (count - 1) * plain_stride + n, values_out, (count - 1) * values_stride + n))
        throw std::invalid_argument("values_out overlaps plain");
    hipStream_t s = as_stream(stream);
    strict_plain(c, "batch_decode plain", plain, enc->t, count, count > 1 ? plain_stride : n, s);
    const bool two_pass = nwt_pass_count(enc->log_n) > 1, fused = fused_decode(enc->log_n, count);
    // scratch: the hand-over of a two-pass transform, and the transform's output where the gather is a pass of its own, [count][N]
    u64 *mid = (two_pass || !fused) ? c.scratch(stream, count * n) : nullptr;
    if (fused) {
        const NwtIo io{plain, plain_stride, NWT_IN_PLAIN, 0, mid, n, values_out, values_stride, NWT_OUT_SCATTER};
        nwt_transform(*enc, false, (uint32_t)count, io, s);
    } else {
        const NwtIo io{plain, plain_stride, NWT_IN_PLAIN, 0, mid, n, mid, n, NWT_OUT_CANON};
        nwt_transform(*enc, false, (uint32_t)count, io, s);
        hipLaunchKernelGGL(batch_gather_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)count), dim3(256), 0, s, values_out, values_stride,
                           mid, n, enc->index_map.p, (uint32_t)n);
        check_launch();
    }
    PHA_API_END
}

}  // extern "C"
