// emu_ckks_fft.cpp -- TEST-ONLY: the arithmetic and the pass phases of the CKKS encoder (phantom-fhe_amd/csrc/pha_ckks_fft.h,
// host/device functions: the very source the kernels of pha_ckks.hip run) compiled for the host.  A workgroup's threads are played
// one after the other, phase by phase (a phase ends where the kernel has its barrier).  tests/test_emu_ckks_fft.py compares the
// results with the numpy restatement (tests/ckks_restatement.py), bit for bit.
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../phantom-fhe_amd/csrc/pha_ckks_fft.h"

using namespace pha;

extern "C" {

// which = 0: inverse (encode) butterfly a, b <- a + b, (a - b) * w; 1: forward (decode) a, b <- a + b * w, a - b * w
void emu_ckks_bfly(int which, double *a, double *b, const double *w) {
    cplx x{a[0], a[1]}, y{b[0], b[1]};
    if (which == 0) ckks_gs_bfly(x, y, cplx{w[0], w[1]});
    else ckks_ct_bfly(x, y, cplx{w[0], w[1]});
    a[0] = x.re; a[1] = x.im; b[0] = y.re; b[1] = y.im;
}

// out[log_pairs][t] = psi of butterfly t < n / 2 of the stage whose pairs are 2^log_pairs apart
void emu_ckks_psi_all(const uint32_t *group, uint32_t log_n, uint32_t m, uint32_t *out) {
    const uint32_t half = 1u << (log_n - 1);
    for (uint32_t lp = 0; lp < log_n; lp++)
        for (uint32_t t = 0; t < half; t++) out[(size_t)lp * half + t] = ckks_psi(group, log_n, lp, t >> lp, m);
}

uint32_t emu_ckks_brev(uint32_t x, uint32_t bits) { return ckks_brev(x, bits); }
double emu_ckks_round(double x) { return ckks_round(x); }
int emu_ckks_bit_count(uint64_t max_bits) { return ckks_bit_count(max_bits); }

// wide = 0: the one-word form (|round(x)| below 2^64); 1: mantissa and exponent.  ratio = floor(2^128 / q) as two words
void emu_ckks_round_reduce(int wide, const double *x, size_t count, uint64_t q, uint64_t ratio0, uint64_t ratio1, uint64_t *out) {
    const DModulus m{q, ratio0, ratio1};
    for (size_t i = 0; i < count; i++) out[i] = wide ? ckks_round_reduce_wide(x[i], m) : ckks_round_reduce64(x[i], q, ratio1);
}

// One whole transform of 2^log_n points through the kernels' plan and phases with `nthreads` threads per workgroup: in / out as
// the modes say, `mid` (2 * 2^log_n doubles) between the passes of a two-pass transform.  Returns the number of passes;
// *max_bits receives the max of the bit patterns of the stored |components| of the last pass.
uint32_t emu_ckks_fft(int inverse, uint32_t log_n, uint32_t m, const double *roots, const uint32_t *group, const double *in, int in_mode,
                      uint32_t values_size, double *mid, double *out, int out_mode, double fix, uint32_t nthreads, uint64_t *max_bits) {
    FftPass p{};
    p.roots = reinterpret_cast<const cplx *>(roots);
    p.group = group;
    p.m = m;
    u64 mx = 0;
    const u32 passes = fft_pass_count(log_n);
    for (u32 which = 0; which < passes; which++) {
        const bool first = which == 0, last = which + 1 == passes;
        fft_pass_shape(p, log_n, inverse != 0, which);
        p.in = first ? in : mid;
        p.in_mode = first ? in_mode : (int)FFT_IN_INTERLEAVED;
        p.values_size = values_size;
        p.out = last ? out : mid;
        p.out_mode = last ? out_mode : (int)FFT_OUT_INTERLEAVED;
        p.fix = last ? fix : 0.0;
        p.maxbits = last ? &mx : nullptr;
        std::vector<cplx> lds((size_t)1 << p.log_tile);
        for (u32 tile = 0; tile < (1u << (log_n - p.log_tile)); tile++) {
            for (u32 t = 0; t < nthreads; t++) fft_load(p, lds.data(), tile, 0, t, nthreads);
            for (u32 done = 0; done < p.stages;) {
                u32 r = 0;
                for (u32 t = 0; t < nthreads; t++)
                    r = inverse ? fft_stage_phase<true>(p, lds.data(), tile, done, t, nthreads)
                                : fft_stage_phase<false>(p, lds.data(), tile, done, t, nthreads);
                done += r;
            }
            for (u32 t = 0; t < nthreads; t++) {
                const u64 v = fft_store(p, lds.data(), tile, 0, t, nthreads);
                if (last && v > mx) mx = v;
            }
        }
    }
    if (max_bits) *max_bits = mx;
    return passes;
}

}  // extern "C"
