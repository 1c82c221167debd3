// emu_bfv_lift.cpp -- TEST-ONLY: the one-word centred lift of a BFV plaintext (phantom-fhe_amd/csrc/pha_bfv_lift.h, host/device
// functions: the very source the load prologue of the forward transform runs) compiled for the host.  tests/test_emu_bfv_lift.py
// compares the words with Python integers.
#include <cstddef>
#include <cstdint>
#include "../../phantom-fhe_amd/csrc/pha_bfv_lift.h"

using namespace pha;

extern "C" {

// out[i] = lift of w[i] into the limb of modulus q, plain modulus t, with the constants the launcher derives from (q, t)
void emu_bfv_lift(uint64_t q, uint64_t t, const uint64_t *w, size_t count, uint64_t *out) {
    const u64 half = bfv_lift_threshold(t), inc = bfv_lift_increment(q, t);
    for (size_t i = 0; i < count; i++) out[i] = bfv_lift_word(w[i], half, inc);
}

uint64_t emu_bfv_lift_threshold(uint64_t t) { return bfv_lift_threshold(t); }

}  // extern "C"
