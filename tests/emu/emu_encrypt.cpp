// emu_encrypt.cpp -- TEST-ONLY: the per-thread programs of the encryption kernels compiled for the host: the PRO_SMALL lift and the
// two mul-add epilogues (phantom-fhe_amd/csrc/pha_encrypt.h, and apply_epilogue_muladd of pha_ntt_core.h, the very function the last
// round's store calls).  tests/test_emu_encrypt.py compares the words with Python integers and checks the magnitude of every FP64
// intermediate against the bound the header derives.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "../../phantom-fhe_amd/csrc/pha_ntt_core.h"

using namespace pha;

namespace {

struct MaxProbe {
    double mag[2] = {0.0, 0.0};   // |a b + x| and |r|, in the order muladd_fp probes them
    int at = 0;
    void f64(double x) {
        if (std::fabs(x) > mag[at & 1]) mag[at & 1] = std::fabs(x);
        at++;
    }
};

DModulus make_modulus(u64 q) {   // floor(2^128 / q) as two words (q is no power of two)
    const unsigned __int128 r = ~(unsigned __int128)0 / q;
    return DModulus{q, (u64)r, (u64)(r >> 64)};
}

}  // namespace

extern "C" {

uint64_t emu_small_sample_max() { return kSmallSampleMax; }
int emu_small_min_prime_bits() { return kSmallMinPrimeBits; }
int emu_muladd_bound(int which) { return which ? kMulAddOutBound : kMulAddSumBound; }

// the load prologue: w [count] signed words -> out [count] canonical residues of k v (k == 0: no factor); on an FP64 limb (fp != 0) outf
// receives what the pass's first round then holds (PassProgram::fp_after_global_load: fp_from_canon of the word)
void emu_small_lift(uint64_t q, uint64_t k, int fp, const uint64_t *w, size_t count, uint64_t *out, double *outf) {
    const DModulus m = make_modulus(q);
    const u64 kq = k ? barrett64(k, q, m.ratio1) : 0;   // as the prologue reduces PassArgs::pro_k once per workgroup (pha_ntt_core.h)
    for (size_t i = 0; i < count; i++) {
        out[i] = kq ? small_lift_scaled(w[i], kq, m) : small_lift(w[i], q);
        if (fp) outf[i] = fp_from_canon(out[i]);
    }
}

// the store epilogue on count coefficients: x [count] as the last round leaves them -- lazy integers below 8 q (fp == 0), or the bit
// patterns of the FP64 back end's lazy doubles (fp != 0); a, b the factors, p the plaintext (has_p != 0).  neg: EPI_FWD_NEG_MULADD.
// peak [2]: the largest |a b + x| and |result before fp_to_canon| of the FP64 program.
void emu_muladd(uint64_t q, int fp, int neg, int has_p, size_t count, const uint64_t *x, const uint64_t *a, const uint64_t *b,
                const uint64_t *p, uint64_t *out, double *peak) {
    const DModulus m = make_modulus(q);
    PassArgs args{};
    args.q = q;
    args.fp = fp != 0;
    args.fpm = make_fpmod(q);
    args.ratio0 = m.ratio0;
    args.ratio1 = m.ratio1;
    args.aux3 = has_p ? p : nullptr;
    MaxProbe probe;
    for (size_t i = 0; i < count; i++) {
        out[i] = neg ? apply_epilogue_muladd<EPI_FWD_NEG_MULADD>(x[i], args, a[i], b[i], has_p ? p[i] : 0)
                     : apply_epilogue_muladd<EPI_FWD_MULADD>(x[i], args, a[i], b[i], 0);
        if (fp) {   // the same function with a probe: the magnitudes
            const u64 r = neg ? muladd_fp<true>(as_f64(x[i]), a[i], b[i], has_p != 0, has_p ? p[i] : 0, args.fpm, probe)
                              : muladd_fp<false>(as_f64(x[i]), a[i], b[i], false, 0, args.fpm, probe);
            if (r != out[i]) out[i] = ~(u64)0;   // (cannot happen: one function)
        }
    }
    peak[0] = probe.mag[0];
    peak[1] = probe.mag[1];
}

}
