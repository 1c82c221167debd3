/*
 * phantom_amd.h -- C ABI of the MI355X-native RNS polynomial-arithmetic core (libphantom_amd.so).
 *
 * The reference (encryptorion-lab/phantom-fhe) has no FFI layer: its boundary for this path is the
 * C++ launchers in include/ntt.cuh:157-226, the DRNSTool / DBaseConverter methods
 * (include/rns.cuh:156-205, include/rns_bconv.cuh:62-68) and phantom::key_switch_inner_prod /
 * keyswitch_inplace (include/evaluate.cuh:18-32).  Each entry point below replaces exactly one of
 * those and keeps its argument meaning; the only changes are (i) `const DNTTTable&` / `DRNSTool&`
 * become an opaque context handle plus the level (number of live data limbs), (ii) `cudaStream_t`
 * becomes `void*` (a hipStream_t; NULL = the legacy default stream), (iii) C++ exceptions become
 * an int status (0 = PHA_OK) with pha_last_error() carrying the what() text.
 *
 * All `uint64_t*` data arguments are DEVICE pointers owned by the caller, limb-major contiguous
 * `data[limb * N + coeff]`, values canonical in [0, q_limb).  No entry point
 * allocates caller-visible memory; scratch comes from a per-context, per-stream arena.
 * PRECONDITION on every operand word, including caller-supplied constants (keys, plaintext diagonals / weights, scale and P^-1
 * vectors): canonical, i.e. below its limb's modulus.  The reference's Barrett-128 kernels happen to tolerate lazy or unreduced
 * words (src/polymath.cu:463-496 multiplies an unreduced c0 + c1; include/uintmodmath.cuh:96-136 reduces any 128-bit value); this
 * library does not -- on limbs below 2^50 the dyadic, inner-product, hoisting and epilogue kernels compute in FP64 (exact only for
 * words below 2^52), so a non-canonical word there gives wrong residues WITHOUT an error.  Every word the library writes is
 * canonical, so chains of its own calls keep the precondition.  It is CHECKABLE (r06): pha_check_canonical / _keys count the
 * offending words of a buffer, and strict mode (PHA_STRICT=1 in the environment, or pha_set_strict) makes the entry points listed
 * at pha_set_strict count first and return status -1 naming the operand instead of computing.
 * Capturing calls into a hipGraph: warm the same call up once first (same level and batch: an arena grows on demand, and growth is
 * an allocation), and capture on an EXPLICIT stream -- the arenas behind NULL / hipStreamPerThread belong to the calling host thread
 * and are released when that thread exits, so a graph captured on them must not be replayed after the thread is gone.
 * Nothing here touches torch types.
 */
#ifndef PHANTOM_AMD_H
#define PHANTOM_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pha_context *pha_context_t;

enum { PHA_OK = 0, PHA_ERR_INVALID_ARGUMENT = -1, PHA_ERR_LOGIC = -2, PHA_ERR_RUNTIME = -3 };
/* scheme_type values of include/host/encryptionparams.h:19-27 */
enum { PHA_SCHEME_BFV = 1, PHA_SCHEME_CKKS = 2, PHA_SCHEME_BGV = 3 };

/* what() of the last failing call on this thread (std::invalid_argument / logic_error /
 * "HIP Runtime Error" -- mirrors include/cuda_wrapper.cuh:19-43). */
const char *pha_last_error(void);

/* ---- the canonical-operand precondition, checkable (csrc/pha_check.hip).  Both calls SYNCHRONISE the stream (they return a
 *      count): debugging and input validation, not the hot path, not inside a stream capture.
 * pha_check_canonical: data [polys][coeff_modulus_size][N] (polys spaced poly_stride words; 0 with polys = 1), limb i checked
 *   (data points at the FIRST checked limb) against table row start_modulus_idx + i -- or, for the last size_P_tail limbs of a [Q_l || P] buffer, against the special rows
 *   (the remap of nwt_2d_radix8_forward_inplace_include_special_mod, src/ntt/fntt_2d.cu:434-437); *bad_words = how many words are
 *   >= their modulus.
 * pha_check_canonical_keys: the limbs a key switch at level size_Ql READS of n_keys keys [2][size_QP][N] (rows 0 .. size_Ql - 1
 *   and the special rows), keys = DEVICE array of device pointers (PhantomRelinKey::public_keys_ptr()).
 * pha_set_strict(on): strict mode on / off for the process, returns the previous state.  Default: on iff PHA_STRICT=1 was in the
 *   environment when the library was first used.  In strict mode the dyadic, tensor, mod-up / inner-product / mod-down, key-switch,
 *   hoisting and BFV multiply entries check ct / c2 / t_mod_up / keys / weights / ct1 and ct2 before they compute (one
 *   synchronising pass per operand; among them pha_keyswitch_mod_switch, pha_keyswitch_mod_switch_batched,
 *   pha_inner_product_relin_mod_switch_batched, pha_hoisting_batched, pha_hoisting_weighted_batched, pha_hoisting_weighted_bsgs_batched, pha_decrypt_phase_batched, pha_bgv_decrypt_batched, pha_bfv_decrypt_batched, pha_poly_infty_norm_batched, pha_invariant_noise_budget_batched, pha_encrypt_zero_symmetric_batched,
 *   pha_public_key_generate, pha_encrypt_symmetric_batched and pha_encrypt_asymmetric_batched, which also count sample words of
 *   magnitude above 2^16; and the batch encoder's pha_batch_encode_batched, pha_batch_decode_batched,
 *   pha_plain_nwt_forward_inplace_batched and pha_plain_nwt_backward_inplace_batched, which count words that are not below the plain
 *   modulus) and fail with status -1 ("PHA_STRICT: <operand> holds k word(s) >= their limb's modulus"); results are unchanged otherwise. ---- */
int pha_check_canonical(pha_context_t ctx, const uint64_t *data, size_t coeff_modulus_size, size_t start_modulus_idx,
                        size_t size_P_tail, size_t polys, size_t poly_stride, uint64_t *bad_words, void *stream);
int pha_check_canonical_keys(pha_context_t ctx, size_t size_Ql, const uint64_t *const *keys, size_t n_keys, uint64_t *bad_words,
                             void *stream);
int pha_set_strict(int on);

/* ---- host precompute (replaces src/host/modulus.cu:82-111 CoeffModulus::Create and the
 *      hard-coded default table src/host/globals.cu:30-120) ---- */
int pha_coeff_modulus_create(uint64_t poly_modulus_degree, const int *bit_sizes, size_t count, uint64_t *out);

/* ---- context: replaces PhantomContext's hot-path state (src/context.cu:121-232): one DNTTTable for
 *      all QP primes (include/ntt.cuh:34-129) plus a DRNSTool per level (src/rns.cu:11-200), built
 *      lazily and cached.  primes_qp = [Q primes..., P primes...]; size_p = special_modulus_size. ---- */
int pha_context_create(pha_context_t *out, uint32_t log_n, const uint64_t *primes_qp, uint32_t size_qp,
                       uint32_t size_p, int device_id);
void pha_context_destroy(pha_context_t ctx);
/* EncryptionParameters::set_plain_modulus as seen by DRNSTool's constructor (argument `t`, src/rns.cu:11-26;
 * BGV constants :196-285).  0 = none.  Call before the first evaluation call: cached per-level tools are
 * dropped and rebuilt.  Errors: plain_modulus == 1 or >= 2^60 -> invalid_argument; not coprime with
 * the chain -> logic_error ("invalid rns bases", rns.cu:207-208,274-275). */
int pha_context_set_plain_modulus(pha_context_t ctx, uint64_t plain_modulus);
uint32_t pha_context_log_n(pha_context_t ctx);
uint32_t pha_context_size_qp(pha_context_t ctx);
uint32_t pha_context_size_p(pha_context_t ctx);
/* host copies of per-prime constants, for callers that mirror DNTTTable getters; rows 0 .. size_QP - 1 are the chain, the rows
 * after them the auxiliary BFV bases once they exist (first use of a BFV multiply entry or pha_tool_aux_sizes): Bsk then m_tilde
 * (root 0: no tables), R.  An index past the last row is status -1. */
int pha_context_prime_info(pha_context_t ctx, uint32_t prime_idx, uint64_t *value, uint64_t const_ratio[2],
                           uint64_t *root, uint64_t *n_inv);
/* download one twiddle row (host buffers of N words): which = 0 twiddle, 1 twiddle_shoup,
 * 2 itwiddle, 3 itwiddle_shoup -- same content as DNTTTable::twiddle()/itwiddle() rows
 * (itwiddle[1] carries N^-1 exactly like src/host/ntt.cu:53-55). */
int pha_context_download_twiddle(pha_context_t ctx, uint32_t prime_idx, int which, uint64_t *host_out);
/* level tool queries (DRNSTool): beta = number of key-switch digits at this level */
int pha_tool_beta(pha_context_t ctx, uint32_t size_ql, uint32_t *beta);

/* ---- NTT launchers (include/ntt.cuh:178-226).  Processed limbs are
 *      [start_modulus_idx, start_modulus_idx + coeff_modulus_size) of the buffer. ---- */
int pha_nwt_2d_radix8_forward_inplace(pha_context_t ctx, uint64_t *inout, size_t coeff_modulus_size,
                                      size_t start_modulus_idx, void *stream);
int pha_nwt_2d_radix8_forward_inplace_include_special_mod(pha_context_t ctx, uint64_t *inout,
                                                          size_t coeff_modulus_size, size_t start_modulus_idx,
                                                          size_t size_QP, size_t size_P, void *stream);
int pha_nwt_2d_radix8_forward_inplace_include_special_mod_exclude_range(
    pha_context_t ctx, uint64_t *inout, size_t coeff_modulus_size, size_t start_modulus_idx, size_t size_QP,
    size_t size_P, size_t excluded_range_start, size_t excluded_range_end, void *stream);
int pha_nwt_2d_radix8_forward_inplace_fuse_moddown(pha_context_t ctx, uint64_t *ct, const uint64_t *cx,
                                                   const uint64_t *bigPInv_mod_q,
                                                   const uint64_t *bigPInv_mod_q_shoup, uint64_t *delta,
                                                   size_t coeff_modulus_size, size_t start_modulus_idx,
                                                   void *stream);
int pha_nwt_2d_radix8_backward_inplace(pha_context_t ctx, uint64_t *inout, size_t coeff_modulus_size,
                                       size_t start_modulus_idx, void *stream);
int pha_nwt_2d_radix8_backward(pha_context_t ctx, uint64_t *out, const uint64_t *in, size_t coeff_modulus_size,
                               size_t start_modulus_idx, void *stream);
int pha_nwt_2d_radix8_backward_scale(pha_context_t ctx, uint64_t *out, const uint64_t *in,
                                     size_t coeff_modulus_size, size_t start_modulus_idx, const uint64_t *scale,
                                     const uint64_t *scale_shoup, void *stream);
int pha_nwt_2d_radix8_backward_inplace_scale(pha_context_t ctx, uint64_t *inout, size_t coeff_modulus_size,
                                             size_t start_modulus_idx, const uint64_t *scale,
                                             const uint64_t *scale_shoup, void *stream);
int pha_nwt_2d_radix8_backward_inplace_include_special_mod(pha_context_t ctx, uint64_t *inout,
                                                           size_t coeff_modulus_size, size_t start_modulus_idx,
                                                           size_t size_QP, size_t size_P, void *stream);

/* nwt_2d_radix8_forward_inplace_include_temp_mod (include/ntt.cuh:182-185, src/ntt/fntt_2d.cu:200-405,655-693) and
 * nwt_2d_radix8_backward_inplace_include_temp_mod_scale (include/ntt.cuh:222-226, src/ntt/intt_2d.cu:313-409,836-873):
 * transforms over the BEHZ base Bsk = B u {m_sk} (callers src/evaluate.cu:434,528).  The reference passes
 * rns_tool.gpu_Bsk_tables(); here the context owns those primes (pha_context_set_plain_modulus must have been
 * called), so coeff_modulus_size must be |Bsk|, start_modulus_idx 0 and total_modulus_size |Bsk| + 1. */
int pha_nwt_2d_radix8_forward_inplace_include_temp_mod(pha_context_t ctx, uint64_t *inout, size_t coeff_modulus_size,
                                                       size_t start_modulus_idx, size_t total_modulus_size,
                                                       void *stream);
int pha_nwt_2d_radix8_backward_inplace_include_temp_mod_scale(pha_context_t ctx, uint64_t *inout,
                                                              size_t coeff_modulus_size, size_t start_modulus_idx,
                                                              size_t total_modulus_size, const uint64_t *scale,
                                                              const uint64_t *scale_shoup, void *stream);
/* nwt_2d_radix8_forward_modup_fuse (include/ntt.cuh:199-201, src/ntt/ntt_keyswitch_old.cu:10-265): out[limb] = NTT
 * modulo q_{modulus_index} of in[limb], limbs [start, start + coeff_modulus_size) -- how the reference lifts a
 * plaintext modulo t into RNS limb modulus_index (src/evaluate.cu:1152,1210,1321).  Out of place. */
int pha_nwt_2d_radix8_forward_modup_fuse(pha_context_t ctx, uint64_t *out, const uint64_t *in, size_t modulus_index,
                                         size_t coeff_modulus_size, size_t start_modulus_idx, void *stream);
/* fnwt_1d / fnwt_1d_opt / inwt_1d / inwt_1d_opt (include/ntt.cuh:157-171, src/ntt/ntt_1d.cu:17-292): single-workgroup
 * transforms for dim <= 2048 over caller-built tables (the reference's NTT test and benchmark use them:
 * test/ntt_test.cu:9-69, benchmark/ntt_bench.cu:8-79).  twiddles[limb * dim + k] / twiddles_shoup likewise; modulus is
 * an array of {value, const_ratio[0], const_ratio[1]} triples (DModulus); the inverse multiplies the FIRST half of
 * its outputs by scalar[limb] (the second half gets N^-1 through slot 1 of the inverse table, src/host/ntt.cu:53-55).
 * fnwt_1d_opt ignores start_modulus_idx, as the reference's kernel does (ntt_1d.cu:92-93).  No context needed. */
int pha_fnwt_1d(uint64_t *inout, const uint64_t *twiddles, const uint64_t *twiddles_shoup, const uint64_t *modulus,
                size_t dim, size_t coeff_modulus_size, size_t start_modulus_idx, void *stream);
int pha_fnwt_1d_opt(uint64_t *inout, const uint64_t *twiddles, const uint64_t *twiddles_shoup, const uint64_t *modulus,
                    size_t dim, size_t coeff_modulus_size, size_t start_modulus_idx, void *stream);
int pha_inwt_1d(uint64_t *inout, const uint64_t *itwiddles, const uint64_t *itwiddles_shoup, const uint64_t *modulus,
                const uint64_t *scalar, const uint64_t *scalar_shoup, size_t dim, size_t coeff_modulus_size,
                size_t start_modulus_idx, void *stream);
int pha_inwt_1d_opt(uint64_t *inout, const uint64_t *itwiddles, const uint64_t *itwiddles_shoup, const uint64_t *modulus,
                    const uint64_t *scalar, const uint64_t *scalar_shoup, size_t dim, size_t coeff_modulus_size,
                    size_t start_modulus_idx, void *stream);
/* Extension (no reference counterpart): the same limbs [start, start+size) of `batch` polynomials that
 * lie `poly_stride` elements apart (e.g. the polynomials of a ciphertext) in ONE launch. */
int pha_nwt_2d_radix8_forward_inplace_batched(pha_context_t ctx, uint64_t *inout, size_t coeff_modulus_size,
                                              size_t start_modulus_idx, size_t batch, size_t poly_stride,
                                              void *stream);
int pha_nwt_2d_radix8_backward_inplace_batched(pha_context_t ctx, uint64_t *inout, size_t coeff_modulus_size,
                                               size_t start_modulus_idx, size_t batch, size_t poly_stride,
                                               void *stream);

/* ---- dyadic kernels (include/polymath.cuh:6-307, launched <<<N*L/128,128>>> by evaluate.cu).
 *      The reference passes `const DModulus *modulus` (a row of the QP table); here that is
 *      (ctx, mod_start_idx).  Buffers hold coeff_mod_size limbs. ---- */
int pha_add_rns_poly(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *result,
                     size_t coeff_mod_size, size_t mod_start_idx, void *stream);
int pha_sub_rns_poly(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *result,
                     size_t coeff_mod_size, size_t mod_start_idx, void *stream);
int pha_negate_rns_poly(pha_context_t ctx, const uint64_t *op, uint64_t *result, size_t coeff_mod_size,
                        size_t mod_start_idx, void *stream);
int pha_multiply_rns_poly(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *result,
                          size_t coeff_mod_size, size_t mod_start_idx, void *stream);
int pha_multiply_and_add_rns_poly(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2,
                                  const uint64_t *op3, uint64_t *result, size_t coeff_mod_size,
                                  size_t mod_start_idx, void *stream);
/* Shoup overload polymath.cuh:97-103: scalar / scalar_shoup are device arrays, one entry per limb */
int pha_multiply_scalar_rns_poly(pha_context_t ctx, const uint64_t *op, const uint64_t *scalar,
                                 const uint64_t *scalar_shoup, uint64_t *result, size_t coeff_mod_size,
                                 size_t mod_start_idx, void *stream);
/* tensor_prod_2x2_rns_poly / tensor_square_2x2_rns_poly: operands [2][L][N], result [3][L][N];
 * result may alias operand1 (evaluate.cu:377-383 calls it in place). */
int pha_tensor_prod_2x2_rns_poly(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2,
                                 uint64_t *result, size_t coeff_mod_size, void *stream);
int pha_tensor_square_2x2_rns_poly(pha_context_t ctx, const uint64_t *operand, uint64_t *result,
                                   size_t coeff_mod_size, void *stream);
/* the same two kernels with the reference's `modulus` pointer argument as a first table row (polymath.cu:463-529 take
 * `const DModulus *modulus`; bfv_multiply_behz / _hps run them over base Bsk and base R: src/evaluate.cu:489-497, :763-777):
 * limb i uses row mod_start + i, which may be an auxiliary row (pha_context_prime_info lists them).  pha_add / sub / multiply /
 * multiply_and_add / multiply_scalar_rns_poly accept auxiliary rows through their mod_start in the same way. */
int pha_tensor_prod_2x2_rns_poly_at(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *res, size_t cms,
                                    size_t mod_start, void *stream);
int pha_tensor_square_2x2_rns_poly_at(pha_context_t ctx, const uint64_t *op, uint64_t *res, size_t cms, size_t mod_start,
                                      void *stream);
/* add_to_ct_kernel (src/rns_bconv.cu:763-769) */
int pha_add_to_ct(pha_context_t ctx, uint64_t *ct, const uint64_t *cx, size_t size_Ql, void *stream);

/* ---- the rest of include/polymath.cuh:6-307 (src/polymath.cu): residue-wise kernels the reference's encryption,
 *      decryption and plaintext layers launch around the hot path.  Same conventions: [limb][coeff] buffers,
 *      table rows [mod_start, mod_start + coeff_mod_size) where a mod_start is given, canonical outputs. ---- */
/* add_std_cipher :56-73 -- both polynomials of two size-2 ciphertexts */
int pha_add_std_cipher(pha_context_t ctx, const uint64_t *cipher1, const uint64_t *cipher2, uint64_t *result,
                       size_t coeff_mod_size, void *stream);
/* add_and_negate_rns_poly :82-98 -- -(a + b) */
int pha_add_and_negate_rns_poly(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2, uint64_t *result,
                                size_t coeff_mod_size, size_t mod_start_idx, void *stream);
/* add_many_rns_poly :126-147 -- result[poly_index] = sum of operands[e][poly_index]; operands is a HOST array of
 * add_size DEVICE pointers (the reference takes the same table on the device) */
int pha_add_many_rns_poly(pha_context_t ctx, const uint64_t *const *operands, size_t add_size, uint64_t *result,
                          size_t poly_index, size_t coeff_mod_size, void *stream);
/* multiply_scalar_rns_poly, the overload with ONE scalar for every limb :181-196 (Barrett) */
int pha_multiply_uniform_scalar_rns_poly(pha_context_t ctx, const uint64_t *operand, uint64_t scale, uint64_t *result,
                                         size_t coeff_mod_size, size_t mod_start_idx, void *stream);
/* multiply_scalar_and_add_rns_poly :246-264 -- operand1 + operand2 * scalar; _and_sub :266-283 -- operand1 - operand2 * scalar */
int pha_multiply_scalar_and_add_rns_poly(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2,
                                         uint64_t scalar, uint64_t *result, size_t coeff_mod_size, size_t mod_start_idx,
                                         void *stream);
int pha_multiply_scalar_and_sub_rns_poly(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2,
                                         uint64_t scalar, uint64_t *result, size_t coeff_mod_size, size_t mod_start_idx,
                                         void *stream);
/* multiply_and_scale_add_rns_poly :294-315 -- operand1 * operand2 + operand3 * scale */
int pha_multiply_and_scale_add_rns_poly(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2,
                                        const uint64_t *operand3, uint64_t scale, uint64_t *result,
                                        size_t coeff_mod_size, size_t mod_start_idx, void *stream);
/* multiply_and_add_negate_rns_poly :350-371 -- -(operand1 * operand2 + operand3) (the b half of an RLWE sample) */
int pha_multiply_and_add_negate_rns_poly(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2,
                                         const uint64_t *operand3, uint64_t *result, size_t coeff_mod_size,
                                         size_t mod_start_idx, void *stream);
/* sub_and_scale_rns_poly :392-411 -- (operand1 - operand2) * scale[limb]; _single_mod_poly :374-390 -- one limb, explicit modulus */
int pha_sub_and_scale_rns_poly(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2,
                               const uint64_t *scale, const uint64_t *scale_shoup, uint64_t *result,
                               size_t coeff_mod_size, size_t mod_start_idx, void *stream);
int pha_sub_and_scale_single_mod_poly(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2,
                                      uint64_t scale, uint64_t scale_shoup, uint64_t modulus, uint64_t *result,
                                      void *stream);
/* bfv_add_timesQ_overt_kernel / bfv_sub_timesQ_overt_kernel :413-461 -- ct[limb] +- (pt * (-Ql mod t) mod t) * t^-1 mod q_limb,
 * pt a single limb of N coefficients below t */
int pha_bfv_add_timesQ_overt(pha_context_t ctx, uint64_t *ct, const uint64_t *pt, uint64_t negQl_mod_t,
                             uint64_t negQl_mod_t_shoup, const uint64_t *tInv_mod_q, const uint64_t *tInv_mod_q_shoup,
                             uint64_t t, size_t size_Ql, void *stream);
int pha_bfv_sub_timesQ_overt(pha_context_t ctx, uint64_t *ct, const uint64_t *pt, uint64_t negQl_mod_t,
                             uint64_t negQl_mod_t_shoup, const uint64_t *tInv_mod_q, const uint64_t *tInv_mod_q_shoup,
                             uint64_t t, size_t size_Ql, void *stream);
/* abs_plain_rns_poly :645-664 -- result[limb][i] = operand[i] (+ increment[limb] when operand[i] >= threshold) */
int pha_abs_plain_rns_poly(pha_context_t ctx, const uint64_t *operand, uint64_t plain_upper_half_threshold,
                           const uint64_t *plain_upper_half_increment, uint64_t *result, size_t coeff_mod_size,
                           void *stream);
/* tensor_prod_mxn_rns_poly :546-592 -- ciphertext product of sizes m x n (1..8 polynomials each; the operands sit in
 * registers instead of the reference's per-thread device new[]) */
int pha_tensor_prod_mxn_rns_poly(pha_context_t ctx, const uint64_t *operand1, size_t op1_size, const uint64_t *operand2,
                                 size_t op2_size, uint64_t *result, size_t res_size, size_t coeff_mod_size,
                                 void *stream);
/* multiply_and_negated_add_rns_poly :606-634 -- BEHZ FastBconvSK fix-up: operand3 - alpha_sk * prod(B) with alpha_sk
 * (one limb, modulo m_sk) taken centred */
int pha_multiply_and_negated_add_rns_poly(pha_context_t ctx, const uint64_t *alpha_sk, uint64_t m_sk,
                                          const uint64_t *prod_B_mod_q, const uint64_t *operand3, uint64_t *result,
                                          size_t coeff_mod_size, void *stream);

/* ---- RNS tool at level size_Ql (DRNSTool of context_data(chain) with size_Ql data limbs) ---- */
/* DBaseConverter (include/rns_bconv.cuh:13-87) between two bases given as rows of the context's prime table
 * (0 .. size_QP-1 = the Q primes then the P primes; the auxiliary BFV bases follow once a plain modulus is set).
 * bConv_BEHZ (src/rns_bconv.cu:212-229): dst[j] = sum_i (x_i * qhat_i^-1 mod q_i) * (qhat_i mod p_j) mod p_j, the
 * approximate conversion of the hot path.  bConv_HPS (:248-372): the exact conversion of the HPS multiply (overflow
 * count from a double-precision sum, fused multiply-adds as nvcc builds it).  src [ibase][N] -> dst [obase][N]. */
typedef struct pha_base_converter *pha_base_converter_t;
int pha_base_converter_create(pha_context_t ctx, const uint32_t *ibase, size_t ibase_size, const uint32_t *obase,
                              size_t obase_size, pha_base_converter_t *out);
void pha_base_converter_destroy(pha_base_converter_t conv);
int pha_bConv_BEHZ(pha_base_converter_t conv, uint64_t *dst, const uint64_t *src, void *stream);
int pha_bConv_HPS(pha_base_converter_t conv, uint64_t *dst, const uint64_t *src, void *stream);
/* DBaseConverter::bConv_BEHZ_var1 (include/rns_bconv.cuh:64, src/rns_bconv.cu:231-246; constants src/host/rns.cu:469-496): the
 * quotient-style conversion dst[j] = sum_i (x_i * (-P qhat_i^-1) mod q_i) * (q_i^-1 mod p_j) mod p_j with P = prod(obase); callers
 * src/evaluate.cu:747-749, :911-913.  The var1 constants are built on first use. */
int pha_bConv_BEHZ_var1(pha_base_converter_t conv, uint64_t *dst, const uint64_t *src, void *stream);
/* DBaseConverter::exact_convert_array (include/rns_bconv.cuh:68, src/rns_bconv.cu:374-431): src [ibase][N] -> dst [N] modulo the
 * converter's ONE output modulus (status -1 "out base in exact_convert_array must be one." otherwise, as :423-425), exactly:
 * inner product minus round(sum_i y_i / q_i) * (Q mod t).  The reference's only user converts to the plain modulus t, which is no
 * row of the prime table: pha_base_converter_create_modulus makes a converter from table rows to ONE raw modulus (2 .. 2^61 - 1);
 * such a converter serves exact_convert_array only. */
int pha_base_converter_create_modulus(pha_context_t ctx, const uint32_t *ibase, size_t ibase_size, uint64_t out_modulus,
                                      pha_base_converter_t *out);
int pha_exact_convert_array(pha_base_converter_t conv, uint64_t *dst, const uint64_t *src, void *stream);
/* DBaseConverter::bConv_BEHZ for base_P_to_Ql_conv (rns_bconv.cu:212-229): src [P][N] -> dst [Ql][N] */
int pha_bconv_P_to_Ql(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
/* DRNSTool::modup (rns_bconv.cu:530-627): cks [Ql][N] -> dst [beta][Ql+P][N] */
int pha_modup(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *cks, int scheme, void *stream);
/* phantom::key_switch_inner_prod (eval_key_switch.cu:71-92): rlk = DEVICE array of beta device
 * pointers, each key [2][size_QP][N]; p_cx [2][Ql+P][N] */
int pha_key_switch_inner_prod(pha_context_t ctx, size_t size_Ql, uint64_t *p_cx, const uint64_t *p_t_mod_up,
                              const uint64_t *const *rlk, void *stream);
/* DRNSTool::moddown_from_NTT (rns_bconv.cu:776-828): cx_i [Ql+P][N] (ckks: P limbs clobbered; bfv / bgv:
 * every limb left in coefficient form and the first P limb overwritten -- scratch, exactly as in the
 * reference) -> ct_i [Ql][N]; ct_i may alias cx_i.  bgv needs pha_context_set_plain_modulus. */
int pha_moddown_from_NTT(pha_context_t ctx, size_t size_Ql, uint64_t *ct_i, uint64_t *cx_i, int scheme,
                         void *stream);
/* phantom::keyswitch_inplace (eval_key_switch.cu:95-182) on raw buffers: ct [2][Ql][N] += KS(c2) */
/* DRNSTool::moddown (include/rns.cuh:159-160, src/rns_bconv.cu:712-761): cx_i [Ql + alpha][N] -> ct_i [Ql][N], the mod-down whose
 * BFV input is ALREADY in coefficient form (moddown_from_NTT transforms it first); ckks / bgv inputs in NTT form as there.  cx_i
 * is scratch afterwards (its P limbs are left in coefficient form, scaled for ckks with alpha > 1). */
int pha_moddown(pha_context_t ctx, size_t size_Ql, uint64_t *ct_i, uint64_t *cx_i, int scheme, void *stream);
int pha_keyswitch_inplace(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint64_t *c2,
                          const uint64_t *const *rlk, int scheme, void *stream);
/* Extension (the reference loops over ciphertexts): `batch` independent ciphertexts through ONE set of launches.
 * ct [batch][2][Ql][N] += KS(c2[b]) with c2 [batch][Ql][N]; the key limbs are read once per launch, the NTT and
 * base-conversion launches are batch times larger (the throughput regime of the kernels). */
int pha_keyswitch_inplace_batched(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint64_t *c2, size_t batch,
                                  const uint64_t *const *rlk, int scheme, void *stream);

/* Build-defined fusion (no reference launcher): key switch followed by the CKKS rescale, i.e. the relinearize -> rescale_to_next
 * pair of src/evaluate.cu:1029-1075,1376-1427 (keyswitch_inplace eval_key_switch.cu:95-182 then divide_and_round_q_last_ntt
 * rns.cu:1160-1184) as ONE call: dst [2][Ql-1][N] = rescale(ct + keyswitch(c2)), bit-identical to the two calls.  ct [2][Ql][N]
 * (NTT form) and c2 [Ql][N] are only read; dst must not overlap them.  The mod-down's forward transform over 2 x Ql limbs and
 * the rescale's own last-limb inverse disappear (NTT is linear: both subtractions ride on one forward transform).  ckks only. */
int pha_keyswitch_rescale(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, const uint64_t *c2,
                          const uint64_t *const *rlk, uint64_t *dst, void *stream);
/* the same for `batch` ciphertexts ct [batch][2][Ql][N], c2 [batch][Ql][N] -> dst [batch][2][Ql-1][N] against one key */
int pha_keyswitch_rescale_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, const uint64_t *c2, size_t batch,
                                  const uint64_t *const *rlk, uint64_t *dst, void *stream);
/* Build-defined fusion (no reference launcher), the bgv counterpart: key switch followed by mod_switch_to_next, i.e. the
 * relinearize -> mod_switch_to_next pair of src/evaluate.cu:1028-1077,1376-1427 (keyswitch_inplace eval_key_switch.cu:95-182 then
 * mod_t_and_divide_q_last_ntt rns.cu:1186-1236) as ONE call: dst [2][Ql-1][N] = mod_switch(ct + keyswitch(c2)), bit-identical to
 * pha_keyswitch_inplace(..., PHA_SCHEME_BGV) followed by pha_mod_t_and_divide_q_last_ntt(..., 2, ...) for every tool shape.  ct
 * [2][Ql][N] (NTT form) and c2 [Ql][N] are only read; dst must not overlap them.  Both steps divide in coefficient form, so the
 * forward transform of 2 x Ql limbs, the add to ct and the inverse transform of the same limbs between them cancel: 4 Ql + 2 alpha - 2
 * limb transforms after the key inner product instead of 8 Ql + 2 alpha - 2, and no copy of ct.  Needs
 * pha_context_set_plain_modulus and size_Ql >= 2.  The caller multiplies the correction factor by q_last^-1 mod t, as after
 * mod_switch_to_next. */
int pha_keyswitch_mod_switch(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, const uint64_t *c2,
                             const uint64_t *const *rlk, uint64_t *dst, void *stream);
/* the same for `batch` ciphertexts ct [batch][2][Ql][N], c2 [batch][Ql][N] -> dst [batch][2][Ql-1][N] against one key */
int pha_keyswitch_mod_switch_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, const uint64_t *c2, size_t batch,
                                     const uint64_t *const *rlk, uint64_t *dst, void *stream);
/* tensor_prod_2x2_rns_poly for `batch` ciphertext pairs in the layout above: operands [batch][2][L][N],
 * res01 [batch][2][L][N] receives (c0, c1), res2 [batch][L][N] receives c2; res01 may alias operand1 */
int pha_tensor_prod_2x2_batched(pha_context_t ctx, const uint64_t *operand1, const uint64_t *operand2, uint64_t *res01,
                                uint64_t *res2, size_t coeff_mod_size, size_t batch, void *stream);
/* Extension (no reference launcher; the reference composes tensor_prod_2x2_rns_poly src/polymath.cu:463-496 with
 * add_rns_poly :41-56): for every g < batch
 *   (res01[g][0], res01[g][1], res2[g]) = sum over k < terms of tensor_prod_2x2(op1[g][k], op2[g][k])
 * operand ciphertext (g, k) of opX starts at opX + g * opX_batch_stride + k * opX_term_stride (64-bit words) and is
 * [2][L][N], NTT form, canonical; res01 [batch][2][L][N], res2 [batch][L][N] (the layout of pha_tensor_prod_2x2_batched).
 * One launch; the sums stay in registers and every output word is the canonical residue of the sum, so the result is word for
 * word tensor_prod_2x2 followed by add in any order, and terms == 1 gives the words of pha_tensor_prod_2x2_batched.  A batch
 * stride of 0 shares that operand between all groups (rows of a matrix against one vector).  Refused (status -1, nothing
 * launched): terms == 0, coeff_mod_size out of range, an odd stride (16-byte loads), a term stride below 2 * L * N with
 * terms > 1, an output that overlaps an operand ciphertext.  batch == 0 does nothing. */
int pha_tensor_prod_2x2_sum_batched(pha_context_t ctx, const uint64_t *op1, const uint64_t *op2, uint64_t *res01, uint64_t *res2,
                                    size_t coeff_mod_size, size_t terms, size_t batch,
                                    size_t op1_term_stride, size_t op1_batch_stride,
                                    size_t op2_term_stride, size_t op2_batch_stride, void *stream);
/* Encrypted inner products with ONE key switch per sum (lazy relinearization), operands and strides as above with L = size_Ql.
 * ckks: dst [batch][2][Ql-1][N] = rescale( S01[g] + keyswitch(S2[g]) ), S = the sum above; bit-identical to
 * pha_tensor_prod_2x2_sum_batched followed by pha_keyswitch_rescale_batched.  `chunk` groups go through one set of launches
 * (0: the library's default, 8); the working buffers are sized by the chunk and every chunk size gives the same bits.  The
 * operands are only read; dst must not overlap them. */
int pha_inner_product_relin_rescale_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *op1, const uint64_t *op2,
                                            size_t terms, size_t batch, size_t op1_term_stride, size_t op1_batch_stride,
                                            size_t op2_term_stride, size_t op2_batch_stride, const uint64_t *const *rlk,
                                            uint64_t *dst, size_t chunk, void *stream);
/* ckks / bgv, no rescale: dst [batch][2][Ql][N] = S01[g] + keyswitch(S2[g]) (pha_keyswitch_inplace_batched on dst, into which
 * (c0, c1) of the sums are written directly).  bfv is refused: a bfv product is not an NTT-form tensor product. */
int pha_inner_product_relin_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *op1, const uint64_t *op2, size_t terms,
                                    size_t batch, size_t op1_term_stride, size_t op1_batch_stride, size_t op2_term_stride,
                                    size_t op2_batch_stride, const uint64_t *const *rlk, int scheme, uint64_t *dst,
                                    size_t chunk, void *stream);
/* Extension (no reference launcher; the reference composes multiply_rns_poly src/polymath.cu:156-172 with add_rns_poly :41-56 /
 * multiply_and_add_rns_poly :225-244, then rescale_to_next / mod_switch_to_next): plaintext-weighted sums of ciphertexts, for
 * every g < batch and both polynomials p
 *   res[g][p] = acc[g][p] + sum over k < terms of plain[g][k] (.) ct[g][k][p]          (acc == NULL: no addend)
 * operand (g, k) starts at base + g * batch_stride + k * term_stride (64-bit words); plain (g, k) is [L][N], ct (g, k) and
 * acc (g) are [2][L][N], NTT form, canonical; res [batch][2][L][N].  One launch; the sums stay in registers and every output
 * word is the canonical residue of the sum, so the result is word for word multiply followed by add in any order, and terms == 1
 * without acc gives the words of pha_multiply_rns_poly applied to each polynomial.  A batch stride of 0 shares that operand
 * between all groups (shared ct: rows of a matrix against one vector; shared plain: one layer applied to a batch of inputs).
 * res may be exactly acc when acc_batch_stride == 2 * L * N (accumulate in place); no other overlap of an output with an
 * operand is allowed.  Refused (status -1, nothing launched): a null required pointer, terms == 0, coeff_mod_size out of
 * range, an odd stride (16-byte loads), a plain term stride below L * N or a ct term stride below 2 * L * N with terms > 1, a
 * forbidden overlap.  batch == 0 does nothing. */
int pha_multiply_plain_sum_batched(pha_context_t ctx, const uint64_t *plain, const uint64_t *ct, const uint64_t *acc,
                                   uint64_t *res, size_t coeff_mod_size, size_t terms, size_t batch,
                                   size_t plain_term_stride, size_t plain_batch_stride,
                                   size_t ct_term_stride, size_t ct_batch_stride, size_t acc_batch_stride, void *stream);
/* The sum above with L = size_Ql followed by ONE level drop per sum: dst [batch][2][Ql-1][N] = rescale(S[g]) for ckks
 * (pha_divide_and_round_q_last_ntt) or mod_switch(S[g]) for bgv (pha_mod_t_and_divide_q_last_ntt); bit-identical to
 * pha_multiply_plain_sum_batched followed by that entry with cipher_size = 2 * batch.  `chunk` groups go through one set of
 * launches (0: the library's default, 8); the work buffer is sized by the chunk, nothing is copied, and every chunk size gives
 * the same bits.  The operands are only read; dst must not overlap them.  Also refused: size_Ql < 2, bgv without a plain
 * modulus, and bfv, whose plaintext product is not an NTT-form product of stored operands. */
int pha_plain_inner_product_rescale_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *plain, const uint64_t *ct,
                                            const uint64_t *acc, size_t terms, size_t batch,
                                            size_t plain_term_stride, size_t plain_batch_stride,
                                            size_t ct_term_stride, size_t ct_batch_stride, size_t acc_batch_stride,
                                            int scheme, uint64_t *dst, size_t chunk, void *stream);
/* bgv with the level drop: dst [batch][2][Ql-1][N] = mod_switch( S01[g] + keyswitch(S2[g]) ); bit-identical to
 * pha_tensor_prod_2x2_sum_batched followed by pha_keyswitch_mod_switch_batched, operands, strides and `chunk` as
 * pha_inner_product_relin_rescale_batched, its ckks counterpart (declared after the plaintext sums: existing declarations keep
 * their neighbours). */
int pha_inner_product_relin_mod_switch_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *op1, const uint64_t *op2,
                                               size_t terms, size_t batch, size_t op1_term_stride, size_t op1_batch_stride,
                                               size_t op2_term_stride, size_t op2_batch_stride, const uint64_t *const *rlk,
                                               uint64_t *dst, size_t chunk, void *stream);
/* phantom::hoisting_inplace (include/evaluate.cuh:233-241, src/evaluate.cu:1670-1866) on raw buffers:
 * ct [2][Ql][N] <- sum over the n_elts Galois elements of rotate(ct).  galois_elts is a HOST array;
 * glk is a HOST array of n_elts DEVICE pointer tables (PhantomRelinKey::public_keys_ptr() of each
 * element's key).  One mod-up, one fused gather + inner-product kernel, one pair of mod-downs. */
int pha_hoisting(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint32_t *galois_elts, size_t n_elts,
                 const uint64_t *const *const *glk, int scheme, void *stream);
/* Weighted hoisted rotations -- BUILD-DEFINED (BASELINE config 5 "encrypted matmul"; the reference has no such
 * entry point: its building blocks are hoisting_inplace src/evaluate.cu:1670-1866, multiply_plain_inplace :1297-1340
 * and add_inplace :116-198):  ct [2][Ql][N] (NTT form, ckks / bgv) <- sum_e w_e (.) rotate_e(ct), i.e. the
 * diagonal form of a plaintext-matrix x encrypted-vector product.  The weights are multiplied in before the one
 * shared mod-down, so weights[e] (HOST array of DEVICE pointers) is the plaintext over [Q_l || P], NTT form,
 * [Ql + size_P][N].  Galois element 1 (main diagonal) takes no key: glk[e] may be NULL there. */
int pha_hoisting_weighted(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint32_t *galois_elts, size_t n_elts,
                          const uint64_t *const *const *glk, const uint64_t *const *weights, int scheme, void *stream);

/* Baby-step / giant-step form of the same sum (build-defined, BASELINE config 5): with d = n_giant * n_baby diagonals
 *     ct <- sum_i rot_{giant_elts[i]}( sum_j weights[i * n_baby + j] (.) rot_{baby_elts[j]}(ct) )
 * from n_baby - 1 + n_giant - 1 Galois keys instead of d - 1 (element 1 = no rotation, no key; a null weight = no such term).
 * The baby rotations share one mod-up and stay in the extended base ("double hoisting"): giant step i is exactly
 * pha_hoisting_weighted(ct, baby_elts, baby_glk, weights[i * n_baby ..]) -- B_i, one mod-down each, all in one batched launch set --
 * and the giant rotations share ONE mod-down of the sum of their key-switch inner products:
 *     ct <- (sum_i perm_i(B_i0), sum_{identity i} B_i1) + moddown( sum_{keyed i} <modup(perm_i(B_i1)), giant_glk[i]> ).
 * weights[.] are device buffers [Ql + P][N] (NTT form) like pha_hoisting_weighted's, the tables are HOST arrays. ckks / bgv.
 * At most 63 keyed baby steps and 63 / beta keyed giant steps per call. */
int pha_hoisting_weighted_bsgs(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint32_t *baby_elts, size_t n_baby,
                               const uint64_t *const *const *baby_glk, const uint32_t *giant_elts, size_t n_giant,
                               const uint64_t *const *const *giant_glk, const uint64_t *const *weights, int scheme, void *stream);
/* the same for a BATCH of ciphertexts that share every Galois key and weight (one encrypted layer applied to `batch` encrypted
 * inputs): ct and out are [batch][2][Ql][N]; the elements, key tables and weights [n_giant][n_baby] are exactly what
 * pha_hoisting_weighted_bsgs takes and serve every ciphertext.  out[b] is word for word what pha_hoisting_weighted_bsgs writes into
 * a copy of ct[b], for every `chunk`; ckks / bgv; every refusal of that entry applies, before the first launch.  ct is only read;
 * out may be exactly ct (in place), any other overlap is refused.  `chunk` ciphertexts go through one set of launches -- one mod-up
 * of chunk polynomials, the fused baby-step kernel, which reads each baby key limb, permutation entry and weight once per group of
 * up to 4 ciphertexts, one mod-down of 2 * n_giant * chunk polynomials, the giant steps batched over the ciphertexts -- and size the
 * scratch: with nk keyed giant steps, chunk * (4 n_giant |Ql| + (beta + 2 n_giant + nk beta + 2) |Ql + P| + nk |Ql|) * N words
 * (2.2 GB per ciphertext at the C3 set, level 45, with 16 x 8 steps).  0 = 4; capped by batch and by the grid limits
 * (2 * n_giant * chunk, chunk * nk * beta <= 65535).  A chunk of one ciphertext runs the launches of the single entry.
 * batch = 0 does nothing. */
int pha_hoisting_weighted_bsgs_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t batch,
                                       const uint32_t *baby_elts, size_t n_baby, const uint64_t *const *const *baby_glk,
                                       const uint32_t *giant_elts, size_t n_giant, const uint64_t *const *const *giant_glk,
                                       const uint64_t *const *weights, int scheme, uint64_t *out, size_t chunk, void *stream);
/* the same for n_blocks row blocks that share the input ciphertext and every Galois key (the rows of a matrix-vector product):
 * weights [n_blocks][n_giant][n_baby], out [n_blocks][2][Ql][N] (must not overlap ct, which is only read).  The fused baby-step
 * kernel serves the (block, giant step) pairs eight at a time, so the baby keys are streamed once per eight of them; each block's
 * result is bit-identical to a one-block call. */
int pha_hoisting_weighted_bsgs_blocks(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t n_blocks, const uint32_t *baby_elts,
                                      size_t n_baby, const uint64_t *const *const *baby_glk, const uint32_t *giant_elts, size_t n_giant,
                                      const uint64_t *const *const *giant_glk, const uint64_t *const *weights, uint64_t *out, int scheme,
                                      void *stream);
/* Hoisted rotations of a BATCH of ciphertexts that share the Galois keys (and, in the weighted form, the plaintext weights): one
 * encrypted layer or matrix block applied to `batch` encrypted inputs.  ct and out are [batch][2][Ql][N]; galois_elts, glk and
 * weights are what pha_hoisting / pha_hoisting_weighted take (HOST arrays of device tables and buffers) and serve every ciphertext.
 * out[b] is word for word what the single entry writes into a copy of ct[b]: sum_e rotate_e(ct[b]), resp.
 * sum_e w_e (.) rotate_e(ct[b]).  Schemes as the single entries (plain: ckks / bgv / bfv; weighted: ckks / bgv).
 * ct is only read; out may be exactly ct (in place), any other overlap is refused.  `chunk` ciphertexts go through one set of
 * launches -- one mod-up of beta * chunk digits, the gather + inner-product launches, which read each key limb (permutation entry,
 * weight) once per group of up to 4 ciphertexts, one mod-down of 2 * chunk polynomials -- and size the scratch; 0 = 8; capped by
 * batch and by the grid limits (beta * chunk, 2 * chunk <= 65535).  Every chunk size gives the same words; a chunk of one
 * ciphertext runs the launches of the single entry.  batch = 0 does nothing. */
int pha_hoisting_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t batch, const uint32_t *galois_elts, size_t n_elts,
                         const uint64_t *const *const *glk, int scheme, uint64_t *out, size_t chunk, void *stream);
int pha_hoisting_weighted_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t batch, const uint32_t *galois_elts,
                                  size_t n_elts, const uint64_t *const *const *glk, const uint64_t *const *weights, int scheme,
                                  uint64_t *out, size_t chunk, void *stream);
/* PhantomSecretKey::generate_one_kswitch_key (src/secretkey.cu:297-341 with encrypt_zero_symmetric :232-295),
 * arithmetic part on caller-supplied randomness (pha_generate_kswitch_keys_seeded samples a and e on the device with
 * sample_uniform_poly / sample_error_poly, src/prng.cu, and builds all keys of a set at once).  All buffers on the device:
 *   sk_ntt [QP][N] secret key, NTT form;  new_key_ntt [Q][N] key to switch from (s^2 or galois(s)), NTT form;
 *   a [dnum][QP][N] uniform residues (used as the NTT-form c1, as the reference samples it);
 *   e [dnum][QP][N] noise residues in COEFFICIENT form -- clobbered (scaled by t for bgv, then NTT in place);
 *   evk: device array of dnum device pointers, key d receives [2][QP][N] = (-(a_d s + e_d) + P new_key on the
 *   digit's limbs, a_d), the layout key_switch_inner_prod consumes. */
int pha_generate_one_kswitch_key(pha_context_t ctx, const uint64_t *sk_ntt, const uint64_t *new_key_ntt,
                                 const uint64_t *a, uint64_t *e, uint64_t *const *evk, int scheme, void *stream);
/* bfv_multiply_behz (src/evaluate.cu:447-548), the 2 x 2 case at the top data level: ct1, ct2 [2][Q][N] in
 * coefficient form -> dst [3][Q][N] in coefficient form (ct1 == ct2 takes the squaring kernels, like the
 * reference).  Needs pha_context_set_plain_modulus; the auxiliary base Bsk u {m_tilde} (src/rns.cu:392-560) and
 * its NTT tables are built on first use.  The plain modulus need NOT be below the data primes: the scale by t of step 6 is kept
 * per limb as t mod q_i with its Shoup quotient (the reference keeps t itself, whose quotient floor(t 2^64 / q_i) does not fit 64
 * bits once t >= q_i, and returns noise there); for t < every q_i the words are the reference's.
 * ALL the BFV multiply entries, single-pair and batched: the inputs are only read; every pha_bfv_multiply_* entry refuses a dst
 * that overlaps an input (status -1); in strict mode they and pha_bfv_mul_relin_hps_overq_leveled check both operands, named
 * "<entry> ct1" / "<entry> ct2" with the entry's own name (without the pha_ prefix).  A single-pair entry is its batched
 * pipeline at batch = 1. */
int pha_bfv_multiply_behz(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst, void *stream);
/* bfv_multiply_hps with mul_tech_type::hps (src/evaluate.cu:674-818; bConv_HPS src/rns_bconv.cu:248-372;
 * scaleAndRound_HPS_QR_R src/rns.cu:1700-1746): same shapes as pha_bfv_multiply_behz.  The base R (|Q| + 1 primes
 * below the smallest q_i, src/rns.cu:687-693) and its tables are built on first use.  The double-precision
 * sums are fused multiply-add chains, as nvcc builds the reference's kernels by default.
 * Domain.  (1) No base R: when fewer than |Q| + 1 primes = 1 (mod 2N) lie between 2^(bits - 1) and the
 * smallest q_i, the entry (and the hps_overq ones, which need |Q|) fails with logic_error "failed to find enough qualifying
 * primes 2" (PHA_ERR_LOGIC), writes nothing and leaves the context usable.  (2) Room in R: the scaled tensor t d / Q must stay
 * inside (-R / 2, R / 2); with uniform ciphertext words that holds when t sqrt(2N) 4/3 < R / Q (eight standard deviations), i.e.
 * about t < q_min / (110 sqrt(N / 4096)) for equal-sized data primes and never for chains that mix sizes (R is taken below the
 * SMALLEST q_i).  Outside it the entry still returns 0 and the reference's words, which decrypt to noise: use behz or hps_overq
 * there.  (3) The carry of scaleAndRound_HPS_QR_R is reduced modulo r_0 once and then modulo each r_j from that value; the
 * reference chains the reductions (rns.cu:1733), which makes about N (r_0 - r_|Q|) / r_0 coefficients per polynomial noise
 * (one per product at 30-bit primes).  Wherever the reference's words are consistent across the R limbs these are the same. */
int pha_bfv_multiply_hps(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst, void *stream);
/* bfv_multiply_hps with mul_tech_type::hps_overq, no levels dropped (src/evaluate.cu:674-818, overq branches :745-751,
 * :790-792; bConv_BEHZ_var1 src/rns_bconv.cu:231-246; scaleAndRound_HPS_QlRl_Ql src/rns.cu:1748-1796).  Same shapes as
 * pha_bfv_multiply_hps.  ct1 == ct2 (the same pointer) takes the reference's squaring shortcut, whose result is Q / Rl
 * times the product of two separate objects -- kept as the reference has it. */
int pha_bfv_multiply_hps_overq(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst, void *stream);
/* hps_overq_leveled with size_Q - size_Ql levels dropped (mul_tech_type::hps_overq_leveled; constants src/rns.cu:897-975).
 * How many levels to drop is host arithmetic (FindLevelsToDrop, src/evaluate.cu:551-647; phantom::detail in the host
 * mirror).  All ciphertext buffers stay over the FULL base Q ([.][Q][N]); size_Ql = size_Q is plain hps_overq.
 *   pha_bfv_multiply_hps_overq_leveled -- bfv_multiply_hps, leveled branches src/evaluate.cu:709-711, :747-748, :794-795
 *   pha_scaleAndRound_HPS_Q_Ql         -- DRNSTool::scaleAndRound_HPS_Q_Ql src/rns.cu:1798-1808: [Q][N] -> [Ql][N]
 *   pha_ExpandCRTBasis_Ql_Q            -- DRNSTool::ExpandCRTBasis_Ql_Q src/rns.cu:1810-1836: [Ql][N] -> [Q][N] (in place allowed)
 *   pha_keyswitch_inplace_bfv_leveled  -- keyswitch_inplace, leveled branches src/eval_key_switch.cu:142-147, :170-175 */
int pha_bfv_multiply_hps_overq_leveled(pha_context_t ctx, size_t size_Ql, const uint64_t *ct1, const uint64_t *ct2,
                                       uint64_t *dst, void *stream);
/* bfv_mul_relin_hps with levels dropped (src/evaluate.cu:822-1027): multiply + relinearize in one call; the product's c2
 * never leaves level l, so the result differs (in its noise) from multiply followed by the leveled key switch. dst [2][Q][N] */
int pha_bfv_mul_relin_hps_overq_leveled(pha_context_t ctx, size_t size_Ql, const uint64_t *ct1, const uint64_t *ct2,
                                        const uint64_t *const *rlk, uint64_t *dst, void *stream);
/* Extension (the reference loops over ciphertexts): the BFV multiplies over a batch of independent ciphertext pairs.
 * ct1, ct2 [batch][2][Q][N] -> dst [batch][3][Q][N] (the ct3 layout of pha_relinearize_rotate_batched), coefficient form over
 * the full base Q, canonical.  Ciphertext b of dst is bit-identical to what the matching single-pair entry returns for pair b
 * (the same pipeline at batch = 1).
 * `chunk` pairs (0 = the library's default, 8) go through one set of launches whose count does not depend on chunk, with no
 * device-to-device copies; the scratch is sized by chunk, not by batch, and every chunk gives the same bits.  ct1 == ct2 (the
 * same pointer) takes the squaring path for the whole batch (for hps_overq: the reference's squaring shortcut, as the single
 * entry keeps it).  Refused (status -1), besides what all the multiply entries refuse: null pointers, a missing plain modulus and
 * size_Ql outside [1, |Q|]; batch == 0 does nothing.  More than 32 limbs in a conversion's input base: those conversions run per
 * polynomial (bConv_HPS's second branch), everything else stays batched.
 *   pha_bfv_multiply_hps_overq_batched: size_Ql == |Q| is hps_overq, size_Ql < |Q| is hps_overq_leveled with |Q| - size_Ql
 *   levels dropped (pha_bfv_multiply_hps_overq_leveled). */
int pha_bfv_multiply_behz_batched(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst, size_t batch,
                                  size_t chunk, void *stream);
int pha_bfv_multiply_hps_batched(pha_context_t ctx, const uint64_t *ct1, const uint64_t *ct2, uint64_t *dst, size_t batch,
                                 size_t chunk, void *stream);
int pha_bfv_multiply_hps_overq_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct1, const uint64_t *ct2,
                                       uint64_t *dst, size_t batch, size_t chunk, void *stream);
int pha_scaleAndRound_HPS_Q_Ql(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
int pha_ExpandCRTBasis_Ql_Q(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
int pha_keyswitch_inplace_bfv_leveled(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint64_t *c2,
                                      const uint64_t *const *rlk, void *stream);
/* ---- the DRNSTool steps of the BFV multiplies, ONE polynomial per call (include/rns.cuh:167-200; callers bfv_multiply_behz
 *      src/evaluate.cu:447-548, bfv_multiply_hps :674-818, bfv_mul_relin_hps :822-1027), so that code written against the
 *      reference's DRNSTool links step by step.  All buffers in coefficient form, limb-major, canonical.  size_Ql names the
 *      level's tool as everywhere else; the BEHZ base Bsk and the HPS base R exist at the top data level only (size_Ql = |Q|,
 *      status -1 otherwise), the hps_overq base Rl at every level.  pha_tool_aux_sizes reports |Bsk|, |R|, |Rl| (0 where the
 *      base does not exist at that level); each pointer may be NULL.
 *   pha_fastbconv_m_tilde             rns.cu:1249-1278  src [Q][N]        -> dst [Bsk + 1][N]  (last limb modulo m_tilde = 2^32)
 *   pha_sm_mrq                        rns.cu:1290-1338  src [Bsk + 1][N]  -> dst [Bsk][N]
 *   pha_fast_floor                    rns.cu:1343-1419  (input_base_q [Q][N], input_base_Bsk [Bsk][N]) -> out_base_Bsk [Bsk][N]
 *   pha_fastbconv_sk                  rns.cu:1421-1510  input_base_Bsk [Bsk][N] -> out_base_q [Q][N]
 *   pha_scaleAndRound_HPS_QR_R        rns.cu:1700-1746  src [Q + R][N]    -> dst [R][N]
 *   pha_scaleAndRound_HPS_QlRl_Ql     rns.cu:1748-1796  src [Ql + Rl][N]  -> dst [Ql][N]
 *   pha_ExpandCRTBasis_Ql_Q_add_to_ct rns.cu:1838-1858  dst [Ql limbs] += src [Ql][N] * prod(dropped primes); size_Ql < |Q| */
int pha_tool_aux_sizes(pha_context_t ctx, size_t size_Ql, uint32_t *size_Bsk, uint32_t *size_R, uint32_t *size_Rl);
int pha_fastbconv_m_tilde(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
int pha_sm_mrq(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
int pha_fast_floor(pha_context_t ctx, size_t size_Ql, const uint64_t *input_base_q, const uint64_t *input_base_Bsk,
                   uint64_t *out_base_Bsk, void *stream);
int pha_fastbconv_sk(pha_context_t ctx, size_t size_Ql, const uint64_t *input_base_Bsk, uint64_t *out_base_q, void *stream);
int pha_scaleAndRound_HPS_QR_R(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
int pha_scaleAndRound_HPS_QlRl_Ql(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
int pha_ExpandCRTBasis_Ql_Q_add_to_ct(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
/* Batched modular GEMM (benchmark/matmul_bench.cu:215-541): for z in [0, batch): C[z] = A[z] * B[z] mod q, q = the
 * context prime mod_start_idx + z; row-major A [batch][m][lda], B [batch][k][ldb], C [batch][m][ldc], inputs
 * canonical (below q; q <= 60 bits).  Exact (the reference's benchmark kernels lose the carries of the low product word,
 * :231-232).  Runs on the matrix cores (i8 digit planes, csrc/pha_gemm.hip).  Limits: k <= 16384, batch <= 65535, leading
 * dimensions below 2^23; moduli above 2^50 anywhere in the batch take the 8-digit path for all of it (k in runs of 128,
 * one launch per run). */
int pha_batched_modular_gemm(pha_context_t ctx, uint64_t *C, size_t ldc, const uint64_t *A, size_t lda, const uint64_t *B,
                             size_t ldb, size_t m, size_t n, size_t k, size_t batch, size_t mod_start_idx, void *stream);
/* DRNSTool::mod_t_and_divide_q_last_ntt (rns.cu:1210-1236), the BGV modulus switch: src [cipher][Ql][N]
 * in NTT form (left in coefficient form, as in the reference) -> dst [cipher][Ql-1][N] in NTT form */
int pha_mod_t_and_divide_q_last_ntt(pha_context_t ctx, size_t size_Ql, uint64_t *src, size_t cipher_size,
                                    uint64_t *dst, void *stream);
/* DRNSTool::divide_and_round_q_last_ntt (rns.cu:1160-1184): src [cipher][Ql][N] (last limb is
 * clobbered, as in the reference) -> dst [cipher][Ql-1][N] */
int pha_divide_and_round_q_last_ntt(pha_context_t ctx, size_t size_Ql, uint64_t *src, size_t cipher_size,
                                    uint64_t *dst, void *stream);
/* DRNSTool::divide_and_round_q_last (rns.cu:1113-1126), BFV coefficient-domain mod switch */
int pha_divide_and_round_q_last(pha_context_t ctx, size_t size_Ql, const uint64_t *src, size_t cipher_size,
                                uint64_t *dst, void *stream);

/* ---- ciphertext (+|-|*) plaintext (src/evaluate.cu:1105-1340): the device work of add_plain_inplace,
 *      sub_plain_inplace and multiply_plain_inplace, with DRNSTool's per-level constants (src/rns.cu:292-324) kept by
 *      the context (pha_context_set_plain_modulus).  CKKS needs nothing beyond pha_add/sub/multiply_rns_poly. ---- */
/* multiply_add_plain_with_scaling_variant / multiply_sub_plain_with_scaling_variant (src/scalingvariant.cu:10-60):
 * ct[0] (coefficient form, [Ql][N]) +- round-free (Ql / t) * plain, plain = N coefficients below t */
int pha_bfv_add_plain(pha_context_t ctx, size_t size_Ql, uint64_t *ct, const uint64_t *plain, int subtract, void *stream);
/* multiply_plain_normal (src/evaluate.cu:1256-1300): every polynomial of ct [cipher_size][Ql][N] (coefficient form)
 * times the centred lift of plain, through the NTT */
int pha_bfv_multiply_plain(pha_context_t ctx, size_t size_Ql, uint64_t *ct, size_t cipher_size, const uint64_t *plain,
                           void *stream);
/* BGV: out [Ql][N] = NTT of plain modulo every q_i -- the nwt_2d_radix8_forward_modup_fuse loop of
 * src/evaluate.cu:1150-1154, 1208-1212, 1319-1323 as one launch; the caller then applies
 * multiply_scalar_and_add/sub (correction factor) or multiply_rns_poly */
int pha_bgv_lift_plain(pha_context_t ctx, size_t size_Ql, const uint64_t *plain, uint64_t *out, void *stream);
/* Extension (no reference launcher; the reference runs multiply_plain_normal, src/evaluate.cu:1256-1300, once per product and
 * add_inplace per term): BFV plaintext-weighted sums of ciphertexts with ONE forward transform per term and ONE inverse per sum
 * (DESIGN.md section 4.8d).  All buffers are device memory, strides are 64-bit words, L = size_Ql.  Shared by the three entries:
 * refused (status -1, nothing launched) are a null required pointer, size_Ql outside 1..|Q|, a context without a plain modulus,
 * a plain modulus t that is not below every q_i of the level, an odd stride and buffers that are not 16-byte aligned.
 *
 * The lift: out (i) [L][N] at out + i * out_stride = NTT form of the centred lift of plain (i) ([N] words below t at plain +
 * i * plain_stride; w >= (t + 1) / 2 becomes w + q_j - t in limb j) -- word for word pha_abs_plain_rns_poly followed by
 * pha_nwt_2d_radix8_forward_inplace, but the lift is the load prologue of the transform's first pass: `count` plaintexts x L limbs
 * go through one pair of launches and the lifted coefficient form never reaches memory.  Also refused: out_stride below L * N
 * with count > 1, out overlapping plain.  count == 0 does nothing; counts beyond a launch's grid are cut into pieces. */
int pha_bfv_lift_plain_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *plain, size_t count, size_t plain_stride,
                               uint64_t *out, size_t out_stride, void *stream);
/* For every g < batch, in the ring: res[g] = acc[g] + sum over k < terms of plain[g][k] * ct[g][k]   (acc == NULL: no addend).
 * ct (g, k) at ct + g * ct_batch_stride + k * ct_term_stride, acc (g) and res (g) are [2][L][N] in COEFFICIENT form (bfv's
 * form), canonical; plain (g, k) at plain_ntt + g * plain_batch_stride + k * plain_term_stride is [L][N] as
 * pha_bfv_lift_plain_batched writes it; res is dense [batch][2][L][N].  A batch stride of 0 shares that operand between the
 * groups.  Per `slab` terms (0: the default, 4) the slab's ciphertexts are transformed forward out of place into a work buffer
 * ([chunk][slab][2][L][N] words; [slab][2][L][N], transformed once for all groups, when ct is shared), the one-launch sum of
 * pha_multiply_plain_sum_batched adds the slab to the NTT-form partial sums kept in res, and after the last slab ONE inverse
 * transform per `chunk` groups (0: the default, 8) runs in place in res and adds acc in its final store.  The operands are only
 * read, nothing is copied, every chunk and slab size gives the same bits, and the call can be captured into a graph once the
 * work buffer has its size (first call).  Word for word the loop of pha_bfv_multiply_plain (cipher_size 2, on copies) and
 * pha_add_rns_poly in any order; terms == 1 without acc gives the words of pha_bfv_multiply_plain.  Also refused: terms == 0, a
 * plain term stride below L * N or a ct term stride below 2 * L * N with terms > 1, res overlapping any operand (acc included).
 * batch == 0 does nothing. */
int pha_bfv_multiply_plain_sum_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *plain_ntt, const uint64_t *ct,
                                       const uint64_t *acc, uint64_t *res, size_t terms, size_t batch,
                                       size_t plain_term_stride, size_t plain_batch_stride, size_t ct_term_stride,
                                       size_t ct_batch_stride, size_t acc_batch_stride, size_t chunk, size_t slab, void *stream);
/* The same with RAW plaintexts: plain (g, k) is [N] words below t (what a bfv PhantomPlaintext holds; plain term stride at least N
 * with terms > 1).  Each slab's plaintexts are lifted and transformed into the work buffer (another [chunk][slab][L][N] words;
 * [slab][L][N], lifted once for all groups, when plain is shared).  Bit-identical to pha_bfv_lift_plain_batched followed by
 * pha_bfv_multiply_plain_sum_batched. */
int pha_bfv_plain_inner_product_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *plain, const uint64_t *ct,
                                        const uint64_t *acc, uint64_t *res, size_t terms, size_t batch,
                                        size_t plain_term_stride, size_t plain_batch_stride, size_t ct_term_stride,
                                        size_t ct_batch_stride, size_t acc_batch_stride, size_t chunk, size_t slab, void *stream);

/* ---- Galois (include/galois.cuh:98-130, src/galois.cu:11-39,67-102) ---- */
int pha_apply_galois_ntt(pha_context_t ctx, const uint64_t *src, uint64_t *dst, uint32_t galois_elt,
                         size_t coeff_mod_size, void *stream);
int pha_apply_galois(pha_context_t ctx, const uint64_t *src, uint64_t *dst, uint32_t galois_elt,
                     size_t coeff_mod_size, size_t mod_start_idx, void *stream);
/* the same permutation on `polys` polynomials [polys][coeff_mod_size][N] in one launch (ntt_form != 0: the NTT-domain
 * table permutation, else the coefficient-domain one with its sign) */
int pha_apply_galois_batched(pha_context_t ctx, const uint64_t *src, uint64_t *dst, uint32_t galois_elt,
                             size_t coeff_mod_size, size_t polys, int ntt_form, void *stream);
/* Build-defined helper for rotate on batches (BASELINE config 4): the automorphism of `batch` size-2 ciphertexts
   src [batch][2][Ql][N], written in the layout the key switch that follows needs (rotate_internal / apply_galois_inplace,
   src/evaluate.cu:1567-1624): dst_ct [batch][2][Ql][N] receives (galois(c0), 0), dst_c2 [batch][Ql][N] receives galois(c1).
   ntt_form != 0: NTT-domain permutation (ckks / bgv); 0: coefficient-domain with sign (bfv). */
int pha_apply_galois_for_keyswitch(pha_context_t ctx, const uint64_t *src, uint64_t *dst_ct, uint64_t *dst_c2,
                                   uint32_t galois_elt, size_t size_Ql, size_t batch, int ntt_form, void *stream);

/* BASELINE config 4 as one call (build-defined composition of relinearize_inplace src/evaluate.cu:1028-1077 and
 * apply_galois_inplace :1567-1624 over a batch, no reference launcher): out [batch][2][Ql][N] =
 * rotate_{galois_elt}(relinearize(ct3 [batch][3][Ql][N])), i.e. per ciphertext keyswitch_inplace with rlk, the automorphism, and
 * keyswitch_inplace with glk -- bit-identical to those calls.  ct3 is only read (out must not overlap it); the batch runs
 * `chunk` ciphertexts per set of launches (0 = sized so that a set's mod-up digits stay within the 256 MiB MALL, and the sets
 * alternate between two streams the context owns, forked from and joined back into `stream` with events: warm the call up once
 * before capturing it into a graph); no copies. */
int pha_relinearize_rotate_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct3, size_t batch,
                                   const uint64_t *const *rlk, const uint64_t *const *glk, uint32_t galois_elt, int scheme,
                                   uint64_t *out, size_t chunk, void *stream);

/* ---- multi-GPU (the reference has none): one-time RCCL broadcast of evaluation / Galois keys.  keys[i] (HOST array
 *      of n_keys DEVICE buffers, words_per_key uint64 words each -- for a PhantomRelinKey the dnum buffers of 2 * #QP * N words,
 *      include/secretkey.h:102-165) are sent from rank `root` of `nccl_comm` (an ncclComm_t the caller created for its ranks, one
 *      per GPU) to every other rank, in place, as one RCCL group on `stream`.  No collective exists on the data path: after this
 *      call every rank key-switches its own ciphertexts.  RCCL is resolved with dlopen at first use (no link-time dependency). ---- */
int pha_broadcast_keys(pha_context_t ctx, uint64_t *const *keys, size_t n_keys, size_t words_per_key, int root, void *nccl_comm,
                       void *stream);

/* ---- CKKS encoder (PhantomCKKSEncoder, src/ckks.cu; special FFT src/fft.cu; decompose / compose src/rns_base.cu:49-253;
 *      csrc/pha_ckks.hip, arithmetic in csrc/pha_ckks_fft.h).  N = the context's degree, n = N / 2 slots,
 *      M = 2 N.  All data buffers are DEVICE memory; complex numbers are interleaved (re, im) doubles.  "Bit-exact" for these
 *      entries: a complex product is (ar*br - ai*bi, ar*bi + ai*br), every operation rounded on its own, in the radix-2 butterfly
 *      graph of the reference; the reference's own bits on its hardware depend on its compiler's contraction and are not pinned.
 *      Only canonical words are written: a coefficient that rounds to -0.0 gives 0 where the reference writes q.
 * pha_ckks_encoder_create: the tables of PhantomCKKSEncoder's constructor (roots[i] = e^{2 pi i * i / M}, i < M, from polar() over
 *   an eighth of the circle plus the 8-fold symmetry; group[i] = 5^i mod M, i < n / 2) for ctx, which must outlive the encoder.
 *   _tables copies them to HOST arrays (roots_host: 2 M doubles, group_host: n / 2 words; either may be null).
 * pha_special_fft_backward / _forward (special_fft_backward / special_fft_forward, src/fft.cu:348-422): in place on ONE array of
 *   2^log_n complex numbers, log_n <= log2 n, no bit reversal; backward multiplies the result by `scalar` unless it is 0.
 * pha_decompose_array (DRNSBase::decompose_array): dst [size_Ql][N] <- round(coefficient j) mod q_i, coefficient j = Re src[j]
 *   for j < n, Im src[j - n] above; src n complex numbers.  max_coeff_bit_count picks the kernel (<= 64: the coefficient fits a
 *   word; above: mantissa and exponent), both exact.
 * pha_compose_array (DRNSBase::compose_array): src [size_Ql][N] in coefficient form -> dst n complex numbers, coefficient j =
 *   (centred CRT value) * inv_scale accumulated word by word from the low word up as the reference kernel does.  The level's
 *   big-integer tables are built on the host on its first use.
 * Extension (no reference launcher: the reference encodes one message per call, one launch per FFT stage above 2048 points, and
 *   copies the coefficients to the host for their maximum) pha_ckks_encode_batched: message k = values_size complex numbers at
 *   values + 2 * k * values_stride doubles (values_stride counts complex numbers), k < count <= 65535; plaintext k, in NTT form,
 *   at dst + k * dst_stride: [size_Ql][N], or with_special != 0 [size_Ql + size_P][N] over the limbs [0, size_Ql) u P (the layout
 *   the hoisting entries take; equal to those rows of the key-level encoding).  At most two passes over the message for the FFT at
 *   every N; coefficients that fit a word (max_coeff_bit_count <= 64) are rounded and reduced in the load of the forward
 *   transform's first pass, every limb reading the same [N] doubles, so the decomposed form [L][N] is never written; wider ones go
 *   through the decompose kernel and the plain transform (same words).  Refusals as encode_internal
 *   (status -1): "Input vector is empty", "Input vector exceeds max slots", "scale out of bounds" (scale <= 0 or
 *   (int) log2(scale) + 1 >= the bit count of q_0 .. q_{size_Ql - 1}), "encoded values are too large" (max_coeff_bit_count =
 *   ceil(log2(max(max |coefficient|, 1))) + 1, taken from the bit pattern, >= that bit count; Inf / NaN inputs end here).
 *   bit_counts_host_or_null: HOST array of `count` ints that receives max_coeff_bit_count per message.  The call SYNCHRONISES the
 *   stream once, reading back `count` words: the refusal and the choice of the decompose kernel need the maxima -- so it cannot be
 *   captured into a graph.  dst: 16-byte aligned, dst_stride even and >= the plaintext's size when count > 1.
 * Extension pha_ckks_decode_batched: plaintext k [size_Ql][N] (NTT form, only read) at plain + k * plain_stride -> n complex
 *   numbers at values_out + 2 * k * values_stride doubles; scale as PhantomPlaintext::scale() ("scale out of bounds" when <= 0
 *   or (int) log2(scale) >= the level's bit count).  Strict mode checks plain.
 * Scratch comes from the context's arenas. ---- */
typedef struct pha_ckks_encoder *pha_ckks_encoder_t;
int pha_ckks_encoder_create(pha_context_t ctx, pha_ckks_encoder_t *enc);
void pha_ckks_encoder_destroy(pha_ckks_encoder_t enc);
int pha_ckks_encoder_tables(pha_ckks_encoder_t enc, double *roots_host, uint32_t *group_host);
int pha_special_fft_backward(pha_ckks_encoder_t enc, double *inout, size_t log_n, double scalar, void *stream);
int pha_special_fft_forward(pha_ckks_encoder_t enc, double *inout, size_t log_n, void *stream);
int pha_decompose_array(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const double *src, uint32_t max_coeff_bit_count,
                        void *stream);
int pha_compose_array(pha_context_t ctx, size_t size_Ql, double *dst, const uint64_t *src, double inv_scale, void *stream);
int pha_ckks_encode_batched(pha_ckks_encoder_t enc, size_t size_Ql, int with_special, const double *values, size_t values_size,
                            size_t count, size_t values_stride, double scale, uint64_t *dst, size_t dst_stride,
                            int *bit_counts_host_or_null, void *stream);
int pha_ckks_decode_batched(pha_ckks_encoder_t enc, size_t size_Ql, const uint64_t *plain, size_t count, size_t plain_stride,
                            double scale, double *values_out, size_t values_stride, void *stream);

/* ---- decryption (PhantomSecretKey::ckks_decrypt / bgv_decrypt / bfv_decrypt, src/secretkey.cu:533-691; DRNSTool::
 *      hps_decrypt_scale_and_round src/rns.cu:1519-1689 and decrypt_mod_t; csrc/pha_decrypt.hip, arithmetic and bounds in
 *      csrc/pha_decrypt.h).  All data buffers are DEVICE memory, strides are 64-bit words, L = size_Ql,
 *      N = the context's degree.  The secret key enters as the array pha_generate_one_kswitch_key takes; encryption and public keys
 *      are the next section; sampling (the PRNG of src/prng.cu) is the last section, from seeds: managing them is not part of this library.
 * pha_secret_key_powers (compute_secret_key_array, src/secretkey.cu:196-230): out [max_power][size_QP][N] = s, s^2, ... in NTT form
 *   over all QP rows, the reference's secret_key_array layout, from sk_ntt [size_QP][N]: power 1 is a copy (out may be sk_ntt's own
 *   buffer, then nothing is copied), every further power one pha_multiply_rns_poly.
 * Extension (no reference launcher: the reference decrypts one ciphertext per call with a device copy of c0 and one
 *   multiply_and_add_rns_poly launch per further polynomial) pha_decrypt_phase_batched: ciphertext b < batch, in NTT form,
 *   [cipher_size][L][N] at ct + b * ct_stride; dst (b) [L][N] at dst + b * dst_stride = c0 + sum_{i >= 1} c_i (.) s^i, every word the
 *   canonical residue -- word for word that copy and those launches: ckks_decrypt, and the first half of bgv_decrypt.  sk_powers as
 *   pha_secret_key_powers writes it (n_powers powers; rows [0, L) of the first cipher_size - 1 are read).  ONE launch: a thread
 *   keeps the words of s^i in registers across a group of up to 4 ciphertexts.  dst may be ct itself (result b takes c0 (b)'s place;
 *   dst_stride == ct_stride then), as a caller who is done with the ciphertexts would want.
 * Extension pha_bgv_decrypt_batched: the same ciphertexts -> dst (b) [N] words below t (bgv_decrypt): per `chunk` ciphertexts
 *   (0: the default, 8) the phase kernel into a work buffer ([chunk][L][N] words), ONE batched inverse transform in place, and the
 *   exact conversion to t (exact_convert_array) over the chunk, which multiplies by the inverse of correction_factors[b] mod t in its
 *   store -- the words of decrypt_mod_t followed by multiply_scalar_rns_poly.  correction_factors: HOST array of `batch` words, NULL
 *   = all 1 (a factor of 1 multiplies nothing); a factor that is not invertible mod t returns status -2 "invalid correction factor"
 *   before anything is launched.
 * Extension pha_bfv_decrypt_batched: ciphertext b in COEFFICIENT form (bfv's form), size_Ql <= |Q| (the leveled ciphertexts of
 *   hps_overq_leveled included) -> dst (b) [N] = round(t x / Q_l) mod t of the phase x (bfv_decrypt with the HPS scale-and-round).
 *   Per chunk: c_1 .. c_{k-1} are transformed forward OUT OF PLACE into the work buffer ([chunk][cipher_size - 1][L][N] words; no
 *   copy, no memset), the phase kernel runs without c0, ONE batched inverse transform adds c0 in its final store, and the
 *   scale-and-round writes the plaintexts.  The ciphertexts are only read.  One form of the scale-and-round for every width (the
 *   reference picks one of four kernels by bit counts): differs from the exact rounding only where t x / Q is within L * 2^-14 of a
 *   half-integer.  Deviation: where the reference stores llround of a value in [0, t) and can write t itself (a plaintext 0 with
 *   slightly negative noise), this library writes 0 -- only canonical words are written.
 * Shared by the three batched entries.  Refused (status -1, nothing launched): a null pointer; size_Ql outside 1..|Q|;
 *   cipher_size < 2 or n_powers < cipher_size - 1; with batch > 1 a ct stride below cipher_size * L * N or a dst stride below the
 *   size of a result; an odd stride; buffers that are not 16-byte aligned; dst overlapping sk_powers or ct (except dst == ct of the
 *   phase entry); for the bgv / bfv entries a context without a plain modulus or a level of more than 64 limbs (the scale-and-round's error bound is derived up to there).  batch == 0 does nothing.  No entry synchronises; once
 *   the work buffer has its size and the level's tables exist (first call) a call can be captured into a graph.  Every `chunk` gives
 *   the same bits.  Strict mode (pha_set_strict) checks ct and sk_powers, named "<entry> ct" and "<entry> sk_powers" with <entry> =
 *   decrypt_phase, bgv_decrypt, bfv_decrypt.
 * pha_hps_decrypt_scale_and_round / pha_decrypt_mod_t: the two DRNSTool launchers on ONE polynomial, src [L][N] in coefficient form,
 *   canonical -> dst [N]: round(t x / Q_l) mod t, and the exact conversion of x from Q_l to t of exact_convert_array (no correction
 *   factor).  The words of the batched entries' last step; also refused: dst overlapping src. ---- */
int pha_secret_key_powers(pha_context_t ctx, const uint64_t *sk_ntt, size_t max_power, uint64_t *out, void *stream);
int pha_decrypt_phase_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t cipher_size, size_t batch, size_t ct_stride,
                              const uint64_t *sk_powers, size_t n_powers, uint64_t *dst, size_t dst_stride, void *stream);
int pha_bgv_decrypt_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t cipher_size, size_t batch, size_t ct_stride,
                            const uint64_t *sk_powers, size_t n_powers, const uint64_t *correction_factors, uint64_t *dst,
                            size_t dst_stride, size_t chunk, void *stream);
int pha_bfv_decrypt_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t cipher_size, size_t batch, size_t ct_stride,
                            const uint64_t *sk_powers, size_t n_powers, uint64_t *dst, size_t dst_stride, size_t chunk, void *stream);
int pha_hps_decrypt_scale_and_round(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);
int pha_decrypt_mod_t(pha_context_t ctx, size_t size_Ql, uint64_t *dst, const uint64_t *src, void *stream);

/* ---- noise (PhantomSecretKey::invariant_noise_budget, src/secretkey.cu:752-840, with compose_array and
 *      poly_infinity_norm_coeffmod; csrc/pha_noise.hip, arithmetic and bounds in csrc/pha_noise.h).  The
 *      reference copies the phase to the host, composes it with multi-precision integers and takes the norm on the CPU, one
 *      ciphertext per call behind a stream synchronise; here the norm is a device-side quantity of a BATCH.  All data buffers are
 *      DEVICE memory, strides are 64-bit words, L = size_Ql <= 64, N = the context's degree.  Exact integer arithmetic throughout: no
 *      floating point, no atomics, no dependence on launch order.
 * Extension pha_poly_infty_norm_batched: polynomial c < count, [L][N] in coefficient form with canonical residues at src +
 *   c * src_stride.  With v_j in [0, Q_l) the CRT composition of [scalar * x_{i,j}]_{q_i} (scalar: any 64-bit word, reduced modulo
 *   every q_i on the host), the polynomial's norm is max_j min(v_j, Q_l - v_j): norm [count][L] receives it as L little-endian 64-bit
 *   words (NULL: not written), bits [count] its significant bit count (0 for a zero norm).  Two launches: mixed-radix (Garner)
 *   digits per coefficient and one candidate per workgroup, then the maximum, its conversion to binary and the stores.
 * Extension pha_invariant_noise_budget_batched: ciphertexts and sk_powers as the decrypt entries take them; PHA_SCHEME_BFV:
 *   COEFFICIENT form, the phase of pha_bfv_decrypt_batched (forward transforms of c_1 .. out of place, the phase kernel, one batched
 *   inverse that adds c0), norm taken with scalar = t; PHA_SCHEME_BGV / PHA_SCHEME_CKKS: NTT form, the phase of
 *   pha_bgv_decrypt_batched up to its inverse transform, scalar = 1 (the reference multiplies by t under bfv only; under ckks the
 *   result is the headroom above scale * message).  budget [batch] (int32) = max(0, bitcount(Q_l) - bits - 1); norm [batch][L] may
 *   be NULL.  chunk as in the decrypt entries (0: the default, 8; work buffer [chunk][L][N] words, bfv [chunk][cipher_size - 1][L][N],
 *   plus the candidates).  Every `chunk` gives the same words.  The ciphertexts are only read.
 * Refused (status -1, nothing launched, nothing written): what the decrypt entries refuse (a null ct / sk_powers / src / budget /
 *   bits; size_Ql outside 1..|Q| or above 64; cipher_size < 2 or n_powers < cipher_size - 1; with batch > 1 a ct (src) stride below
 *   the size of an element; an odd ct stride; ct or sk_powers not 16-byte aligned); an unknown scheme; PHA_SCHEME_BFV or
 *   PHA_SCHEME_BGV on a context without a plain modulus; norm / budget / bits overlapping an input or each other.  batch == 0
 *   (count == 0) does nothing.  No entry synchronises; once the work buffer has its size and the tables exist (first call) a call
 *   can be captured into a graph.  Strict mode (pha_set_strict) checks ct, sk_powers and src, named "noise_budget ct",
 *   "noise_budget sk_powers" and "poly_infty_norm src". ---- */
int pha_poly_infty_norm_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *src, size_t count, size_t src_stride,
                                uint64_t scalar, uint64_t *norm, uint32_t *bits, void *stream);
int pha_invariant_noise_budget_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *ct, size_t cipher_size, size_t batch,
                                       size_t ct_stride, const uint64_t *sk_powers, size_t n_powers, int scheme, int32_t *budget,
                                       uint64_t *norm, size_t chunk, void *stream);

/* ---- encryption (PhantomSecretKey::encrypt_zero_symmetric / gen_publickey / encrypt_symmetric, PhantomPublicKey::
 *      encrypt_zero_asymmetric / encrypt_asymmetric, src/secretkey.cu:11-192, 232-295, 382-395, 463-531; csrc/pha_encrypt.hip,
 *      arithmetic and bounds in csrc/pha_encrypt.h) for BATCHES of ciphertexts.  All data buffers are DEVICE
 *      memory, strides are 64-bit words, l = size_Ql, N = the context's degree, k = t for bgv and 1 otherwise.  Randomness is the
 *      caller's, as pha_generate_one_kswitch_key takes it; the seeded samplers (src/prng.cu) that make such operands on the device are
 *      the last section.
 * Samples: a sampled polynomial (the noise e, the ternary u) is [N] SIGNED 64-bit words in two's complement, |v| <= 2^16 (the
 *   reference's samplers give |v| <= 21), ONE polynomial shared by every limb: each limb lifts it modulo its own prime as it is
 *   loaded, the [L][N] residue form is never written.  The entries refuse a context that has a prime below 2^17 among the rows used.
 * The uniform a: canonical words [rows][N] ALREADY in c1's place in the output buffer, taken as NTT-form as the reference samples it
 *   (c1 is its own input; no copy).
 * pha_encrypt_zero_symmetric_batched: ct (b) at ct + b * ct_stride is [2][rows][N], rows = [0, l), or [0, l) u P with with_special
 *   (the encoder's row convention); sk_ntt [size_QP][N]; e (b) [N] at e + b * e_stride.  On exit, ntt_form != 0: (c0, c1) =
 *   (-(a (.) s + NTT(k e)), a), c1 untouched -- ONE forward transform per ciphertext whose load lifts the samples and whose store
 *   forms the product and the sum; ntt_form == 0: (-(iNTT(a (.) s) + e), iNTT(a)), c1 replaced by its inverse transform (bfv's form).
 * pha_public_key_generate (gen_publickey): the same at size_Ql = |Q|, with_special = 1, ntt_form = 1, count = 1: pk [2][size_QP][N]
 *   holds a in its second half on entry.
 * pha_encrypt_symmetric_batched (encrypt_symmetric): ckks: plain (b) [l][N] in NTT form (what pha_ckks_encode_batched writes), added
 *   in the same store; bgv: plain (b) [N] words below t, c0 += NTT(m mod q_i); bfv: plain (b) [N] words below t, coefficient form,
 *   then multiply_add_plain_with_scaling_variant.  plain_stride 0 shares one plaintext.  Extension: the reference encrypts bgv / bfv
 *   at the first data level only; any size_Ql in 1..|Q| is accepted here (the per-level constants of pha_bfv_add_plain).
 * pha_encrypt_asymmetric_batched (encrypt_asymmetric): pk [2][size_QP][N] in NTT form, u (b) [N] at u + b * u_stride, e (b) [2][N] at
 *   e + b * e_stride; over rows [0, l) u P: NTT form c_j = pk_j (.) NTT(u) + NTT(k e_j), bfv c_j = iNTT(pk_j (.) NTT(u)) + e_j; then
 *   DRNSTool::moddown of tool (ctx, size_Ql) on each polynomial and the plaintext step above: ct (b) [2][l][N].  At the top data
 *   level this is word for word the reference.  Extension: below it the reference cannot be followed (src/secretkey.cu:106-121 indexes
 *   a level that has dropped one data prime and no special primes and runs the first level's mod-down on it: "use it with caution when
 *   chain_index != 0"); lower levels are defined here by the same construction over Q_l u P.  `chunk` ciphertexts run per set of
 *   launches (0: the default, 8); the work buffer ([chunk] (5 l + 3 |P|) N words, and chunk * l * N more under bgv) comes from the
 *   context's arena.  Every `chunk` gives the same bits.
 * Shared.  Refused (status -1, nothing launched): a null pointer; size_Ql outside 1..|Q|; a prime below 2^17; with_special or the
 *   asymmetric entry on a context without special primes; an unknown scheme; bgv / bfv on a context without a plain modulus;
 *   count > 65535; with count > 1 a ct stride below the size of a ciphertext or a sample / plaintext stride below the size of an
 *   element (a plain_stride of 0 excepted); an odd stride; buffers that are not 16-byte aligned; ct overlapping an input.
 *   count == 0 does nothing.  No entry synchronises; once the work buffer has its size and the level's tables exist (first call) a call
 *   can be captured into a graph.  Strict mode (pha_set_strict) checks the key, the words of a found in ct, the plaintext and the
 *   sample range, named "<entry> sk", "<entry> pk", "<entry> a", "<entry> plain" and "<entry> samples" with <entry> =
 *   encrypt_zero_symmetric (pha_public_key_generate too), encrypt_symmetric, encrypt_asymmetric. ---- */
int pha_encrypt_zero_symmetric_batched(pha_context_t ctx, size_t size_Ql, int with_special, const uint64_t *sk_ntt, const uint64_t *e,
                                       size_t e_stride, uint64_t *ct, size_t ct_stride, size_t count, int scheme, int ntt_form,
                                       void *stream);
int pha_public_key_generate(pha_context_t ctx, const uint64_t *sk_ntt, const uint64_t *e, uint64_t *pk, int scheme, void *stream);
int pha_encrypt_symmetric_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *sk_ntt, const uint64_t *e, size_t e_stride,
                                  const uint64_t *plain, size_t plain_stride, uint64_t *ct, size_t ct_stride, size_t count, int scheme,
                                  void *stream);
int pha_encrypt_asymmetric_batched(pha_context_t ctx, size_t size_Ql, const uint64_t *pk, const uint64_t *u, size_t u_stride,
                                   const uint64_t *e, size_t e_stride, const uint64_t *plain, size_t plain_stride, uint64_t *ct,
                                   size_t ct_stride, size_t count, int scheme, size_t chunk, void *stream);

/* ---- BFV / BGV batch encoder (PhantomBatchEncoder, src/batchencoder.cu:7-118: constructor and populate_matrix_reps_index_map :7-49,
 *      encode_gpu and encode :51-89, decode_gpu and decode :91-118; csrc/pha_batch.hip, arithmetic and index math in csrc/pha_batch.h,
 *      DESIGN.md section 4.13) for BATCHES of messages.  All data buffers are DEVICE memory except where a name ends in _host, strides
 *      are 64-bit words, N = the context's degree = the slot count, t = the context's plain modulus.  A message is up to N words, the
 *      slots in matrix order (two rows of N / 2); a plaintext is [N] words below t in coefficient form -- what
 *      pha_encrypt_symmetric_batched, pha_encrypt_asymmetric_batched, pha_bfv_plain_inner_product_batched, pha_bfv_lift_plain_batched
 *      and pha_bgv_lift_plain take and pha_bfv_decrypt_batched / pha_bgv_decrypt_batched write.
 * pha_batch_encoder_create: the tables of the constructor and of gpu_plain_tables() for ctx, built on the host: the forward and
 *   inverse twiddles of t in bit-reversed order with Shoup quotients (psi = the minimal primitive 2N-th root), N^-1,
 *   matrix_reps_index_map and its inverse permutation.  The encoder owns them: the context's prime table gains no row.  Needs
 *   pha_context_set_plain_modulus.  Refused (status -1): a context without a plain modulus; a t that is not a prime with t = 1
 *   (mod 2N): "encryption parameters are not valid for batching".  The encoder snapshots t: every later call returns -1 if the
 *   context's plain modulus has changed since.  The context must outlive the encoder.
 * pha_batch_encoder_index_map: matrix_reps_index_map, N words, to a HOST array.
 * pha_plain_nwt_forward_inplace_batched / _backward_ (nwt_2d_radix8_forward_inplace / nwt_2d_radix8_backward_inplace(data,
 *   context.gpu_plain_tables(), 1, 0, s), src/batchencoder.cu:88 and :107): the negacyclic transform modulo t, in place, of `count`
 *   polynomials of [N] words below t, `stride` words apart; the backward one includes N^-1.  Canonical words out.  The same kernels
 *   as encode and decode, with no permutation.
 * Extension (no reference launcher: the reference encodes ONE message per call through a staging buffer, with the permutation as a
 *   launch of its own) pha_batch_encode_batched: message k = values_size words at values + k * values_stride, k < count <= 65535;
 *   plaintext k at dst + k * dst_stride = the inverse transform of buf[index_map[i]] = v_i, where v_i = values[i] for i <
 *   values_size and 0 above, and a word with bit 63 set gets + t (the sign rule of encode_gpu: -x in two's complement encodes
 *   t - x).  values_stride == 0 shares one message; values_size == 0 encodes zeros (values may then be null).  The permutation is
 *   the gather of the first pass's load, N^-1 and the canonical reduction are in the last store; a message crosses global memory
 *   at most twice (N <= 2^14: once).  From 2^20 words per call on, a two-pass transform (N > 2^14) takes the permutation as a
 *   streaming kernel of its own instead, in front of the transform (decode: behind it), where that measured faster (DESIGN.md
 *   section 4.13); the words are the same.
 * Extension pha_batch_decode_batched: plaintext k (only read) at plain + k * plain_stride -> N words at values_out + k *
 *   values_stride: out[i] = ntt[index_map[i]] of the forward transform.
 * Shared.  Refused: a null encoder (status -1, "null encoder"); a changed plain modulus (-1); values_size > N (status -2, "values_matrix
 *   size is too large": the reference throws logic_error there); a null pointer; count > 65535; with count > 1 a dst / plain /
 *   values_out stride below N or a non-zero values stride below values_size; an output overlapping an input.  count == 0 is a no-op
 *   that returns PHA_OK.  Every gather / scatter index comes from the encoder's own tables: no caller-supplied word becomes an
 *   address.  Only canonical words are written: outputs are below t.  No entry synchronises; once the scratch of a two-pass
 *   transform (N > 2^14: count * N words from the context's arena) has its size and the kernels have run once (first call) a call can
 *   be captured into a graph.  PRECONDITION: after the sign rule every value word is below t, and every plaintext word is below t.
 *   Strict mode (pha_set_strict) counts the offenders first and fails with "PHA_STRICT: <entry> values holds k word(s) ..." /
 *   "... <entry> plain ..." with <entry> = batch_encode, batch_decode, plain_nwt_forward, plain_nwt_backward. ---- */
typedef struct pha_batch_encoder *pha_batch_encoder_t;
int pha_batch_encoder_create(pha_context_t ctx, pha_batch_encoder_t *enc);
void pha_batch_encoder_destroy(pha_batch_encoder_t enc);
int pha_batch_encoder_index_map(pha_batch_encoder_t enc, uint64_t *index_map_host);
int pha_plain_nwt_forward_inplace_batched(pha_batch_encoder_t enc, uint64_t *inout, size_t count, size_t stride, void *stream);
int pha_plain_nwt_backward_inplace_batched(pha_batch_encoder_t enc, uint64_t *inout, size_t count, size_t stride, void *stream);
int pha_batch_encode_batched(pha_batch_encoder_t enc, const uint64_t *values, size_t values_size, size_t count, size_t values_stride,
                             uint64_t *dst, size_t dst_stride, void *stream);
int pha_batch_decode_batched(pha_batch_encoder_t enc, const uint64_t *plain, size_t count, size_t plain_stride, uint64_t *values_out,
                             size_t values_stride, void *stream);

/* ---- seeded samplers and key generation (src/prng.cu: salsa20_gpu, sample_ternary_poly, sample_error_poly, sample_uniform_poly,
 *      random_bytes; the call sequences of src/secretkey.cu:297-460: gen_secretkey, generate_one_kswitch_key, gen_relinkey,
 *      create_galois_keys; csrc/pha_prng.hip, arithmetic in csrc/pha_prng.h).  All data buffers are DEVICE
 *      memory, strides are 64-bit words, N = the context's degree.  A seed is 64 bytes of DEVICE memory (bytes 56..63 are never
 *      read, as in the reference); a `seeds` argument holds `count` of them back to back, seed b at seeds + 64 * b.  The caller
 *      supplies every seed: only pha_random_bytes draws entropy.  Everything else is deterministic, seed in and words out.
 * The generator block: 16 32-bit input words = seed bytes 0..31, the 64-bit nonce (low, high), seed bytes 32..55; 10 double rounds of
 *   the Salsa20 quarter-round, plus the input: the Salsa20 core WITHOUT constants on the reference's own layout (published Salsa20
 *   stream vectors do not apply).
 * Reference layout (the launch sites a port keeps; rows [mod_start_idx, mod_start_idx + coeff_mod_size) of the QP table):
 *   pha_sample_ternary_poly: out [cms][N], coefficient i of every limb = [byte0 % 3 - 1] mod q from the block of nonce i.
 *   pha_sample_error_poly:   out [cms][N], the centred binomial value (|v| <= 21) of the block of nonce i, modulo every limb.
 *     Both compute ONE block per coefficient and write it to every limb (the reference recomputes it per limb: the same words).
 *   pha_sample_uniform_poly: out [cms][N]; group g = limb position * (N / 8) + j gives words 8 j .. 8 j + 7 of its limb from the
 *     block of nonce g; a word above (2^64 - 1) - ((2^64 - 1) mod q) - 1 is replaced by the same word of a new block of nonce
 *     g + tries * N * cms (tries = blocks this group has drawn), later words read the newest block; stored modulo q.
 * The forms this library consumes:
 *   pha_sample_ternary_signed_batched / pha_sample_error_signed_batched: out (b) at out + b * out_stride = [N] SIGNED 64-bit words
 *     from seed b -- exactly the u / e operands of pha_encrypt_*_batched; the [L][N] residue form is never written.  (The asymmetric
 *     entry's e [count][2][N] is a batch of 2 * count with stride N.)
 *   pha_sample_uniform_batched: out (b) [rows][N], rows = [0, size_Ql), or [0, size_Ql) u P with with_special (the encoder's row
 *     convention); the nonce uses the row's POSITION, the modulus is the row's prime.  At size_Ql = |Q| with_special this is
 *     pha_sample_uniform_poly over QP.  `out` is meant to be c1's place of a ciphertext buffer or the second half of a key, out_stride
 *     the ciphertext stride: a is never copied.
 * Key generation, composed on the device:
 *   pha_secret_key_generate (gen_secretkey): sk_ntt [size_QP][N] = the forward transform of the ternary sample over all QP limbs --
 *     the array every other entry takes.
 *   pha_generate_kswitch_keys_seeded: n_keys keys of dnum = |Q| / |P| components each.  Component b = key * dnum + digit is
 *     [2][size_QP][N] at evk + b * evk_stride (the tables of device pointers the key switch takes are the caller's, over this
 *     storage: the batched zero encryption addresses ciphertext b as base + b * stride, so the components of one call share one
 *     stride); seeds [n_keys][dnum][2][64]: the uniform seed, then the noise seed; new_keys_ntt: key k [size_Q][N] in NTT form at
 *     new_keys_ntt + k * new_key_stride (s^2: gen_relinkey; galois(s): create_galois_keys).  Three launches and one transform for all
 *     components: a sampled straight into every second half, the noise as [N] signed words (count * N words from the context's
 *     arena), ONE pha_encrypt_zero_symmetric_batched at the key level, P * new_key added on each digit's own limbs.  Word for word
 *     pha_generate_one_kswitch_key per key on the same a and the same noise expanded to residues.
 * pha_random_bytes (random_bytes): `count` bytes of std::random_device into a HOST buffer.
 * Shared.  Refused (status -1, nothing launched): a null pointer; rows outside the context; with_special or key generation on a
 *   context without special primes; |Q| not a multiple of |P|; an unknown scheme, bgv without a plain modulus; count (n_keys * dnum)
 *   above 65535; an odd stride; with count > 1 a stride below the size of an element; buffers (seeds included) that are not 16-byte
 *   aligned; evk overlapping an input; a degree below 8; for the noise in residue form a prime that is not above 21.  count == 0
 *   does nothing.  No entry synchronises; once the arena has its size (first call) a call can be captured into a graph.
 *   Deviation from the reference's public-key encryption, which samples both noise polynomials from ONE seed
 *   (src/secretkey.cu:46-55, 80-81: e_0 = e_1): here every polynomial has its own seed; equal seeds reproduce the reference. ---- */
int pha_random_bytes(unsigned char *host_buf, size_t count);
int pha_sample_ternary_poly(pha_context_t ctx, uint64_t *out, const uint8_t *seed, size_t coeff_mod_size, size_t mod_start_idx,
                            void *stream);
int pha_sample_error_poly(pha_context_t ctx, uint64_t *out, const uint8_t *seed, size_t coeff_mod_size, size_t mod_start_idx,
                          void *stream);
int pha_sample_uniform_poly(pha_context_t ctx, uint64_t *out, const uint8_t *seed, size_t coeff_mod_size, size_t mod_start_idx,
                            void *stream);
int pha_sample_ternary_signed_batched(pha_context_t ctx, const uint8_t *seeds, size_t count, uint64_t *out, size_t out_stride,
                                      void *stream);
int pha_sample_error_signed_batched(pha_context_t ctx, const uint8_t *seeds, size_t count, uint64_t *out, size_t out_stride,
                                    void *stream);
int pha_sample_uniform_batched(pha_context_t ctx, size_t size_Ql, int with_special, const uint8_t *seeds, size_t count, uint64_t *out,
                               size_t out_stride, void *stream);
int pha_secret_key_generate(pha_context_t ctx, const uint8_t *seed, uint64_t *sk_ntt, void *stream);
int pha_generate_kswitch_keys_seeded(pha_context_t ctx, const uint64_t *sk_ntt, const uint64_t *new_keys_ntt, size_t n_keys,
                                     size_t new_key_stride, const uint8_t *seeds, uint64_t *evk, size_t evk_stride, int scheme,
                                     void *stream);

#ifdef __cplusplus
}
#endif
#endif
