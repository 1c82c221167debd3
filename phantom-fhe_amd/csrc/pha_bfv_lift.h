// pha_bfv_lift.h -- the one-word centred lift of a BFV plaintext into an RNS limb (multiply_plain_normal, evaluate.cu:1283-1285;
// abs_plain_rns_poly, polymath.cu:645-664): a word w below t stands for w when it is below (t + 1) / 2 and for w - t otherwise,
// and w - t modulo q is w + (q - t).  Host/device like pha_arith.h, so that tests/emu/emu_bfv_lift.cpp compiles the very source
// the load prologue of the forward transform runs (PassProgram PRO_LIFT, pha_ntt_core.h) -- test-only on the host.
// For w < t < q the result is below q: w < (t + 1) / 2 stays, and w + q - t < q.  The addition wraps like the element-wise kernel's
// (x_kernel X_ABS_PLAIN) for words that are not below t, so both forms agree on every input.
#pragma once
#include "pha_arith.h"

namespace pha {

PHA_HD u64 bfv_lift_threshold(u64 t) { return (t + 1) >> 1; }
PHA_HD u64 bfv_lift_increment(u64 q, u64 t) { return q - t; }
PHA_HD u64 bfv_lift_word(u64 w, u64 half, u64 inc) { return w >= half ? w + inc : w; }

}  // namespace pha
